"""Inputs of the temporal-alignment-error scorer's large test case (case D of tests/golden/tae_metrics.npz), too large to commit,
and the fixture as the tests read it. Case D is generated from the counter-based integer hash of _eval_inputs.py and IEEE add /
multiply / divide only, so every platform produces the same bits. tools/gen_tae_golden.py scores exactly these arrays with the
reference's eval_TAE and records their checksum; the tests rebuild them and check the checksum before use."""
import hashlib
import os

import numpy as np

from _eval_inputs import REL_TOL, _hash24

CASE_D = dict(N=6, H=120, W=160, max_depth=10.0)
SEED = 30                    # hash stream: chosen so that the fixture tool's rounding guards hold (a seed that violates one is replaced)


def case_d_inputs():
    """(pred float32 [6,120,160], gt float32, K float64 [6,3,3], poses float64 [6,4,4]): a slanted surface 1.9 .. 3.7 m with 10 %
    per-pixel relief, about 10 % of gt zeroed, pred = 1.4 * disparity + 0.1 with 2 % noise; the camera drifts and yaws a little more
    from frame to frame (a few pixels of image motion, so neighbouring sources collide and leave holes)."""
    f = np.float32
    N, H, W = CASE_D["N"], CASE_D["H"], CASE_D["W"]
    idx = np.arange(N * H * W, dtype=np.uint64)
    inv = f(1.0 / (1 << 24))
    u, v, w = _hash24(idx, SEED) * inv, _hash24(idx, (SEED + 1) << 32) * inv, _hash24(idx, (SEED + 2) << 32) * inv      # [0, 1)
    pix = idx % np.uint64(H * W)
    x = (pix % np.uint64(W)).astype(np.float32) / f(W)
    y = (pix // np.uint64(W)).astype(np.float32) / f(H)
    depth = (f(2.0) + x + y * f(0.5)) * (f(0.95) + u * f(0.1))
    disp = f(1.0) / depth
    pred = (f(1.4) * disp + f(0.1)) * (f(0.98) + v * f(0.04))
    gt = np.where(w < f(0.1), f(0.0), depth).astype(np.float32)
    K = np.zeros((N, 3, 3))
    poses = np.zeros((N, 4, 4))
    for i in range(N):
        K[i] = [[150.0 + i, 0.0, 80.5 - 0.25 * i], [0.0, 148.0 - i, 59.25 + 0.5 * i], [0.0, 0.0, 1.0]]
        s = 0.01 * i
        c = 1.0 - s * s / 2.0
        poses[i] = [[c, 0.0, s, 0.03 * i], [0.0, 1.0, 0.0, -0.01 * i], [-s, 0.0, c, 0.05 * i], [0.0, 0.0, 0.0, 1.0]]
    return np.ascontiguousarray(pred.reshape(N, H, W)), np.ascontiguousarray(gt.reshape(N, H, W)), K, poses


def checksum(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------ the fixture as the tests read it
CASES = ("A", "B", "C", "D")
_loaded = {}


def load_case(golden_dir, name):
    """(pred, gt, K, poses, mask or None, max_depth, expected dict) of case A / B / C / D: gt already divided by its factor (numpy's
    own promotion) and cropped, as the scorer takes it. Loaded once and shared; the arrays are read-only."""
    if name in _loaded:
        return _loaded[name]
    fix = np.load(os.path.join(golden_dir, "tae_metrics.npz"))
    a, b, c, d, max_depth, factor = fix[f"{name}_settings"]
    if name == "D":
        pred, raw, K, poses = case_d_inputs()
        assert checksum(pred, raw, K, poses) == str(fix["D_sha256"]), "case D's generated inputs are not the ones the reference scored"
    else:
        pred, raw, K, poses = (fix[f"{name}_{k}"] for k in ("pred", "gt_raw", "K", "poses"))
    gt = np.ascontiguousarray((raw / float(factor))[:, int(a):int(b), int(c):int(d)])
    mask = fix[f"{name}_mask"] if f"{name}_mask" in fix.files else None
    exp = {"tae": float(fix[f"{name}_tae"]), "scale": float(fix[f"{name}_scale_shift"][0]), "shift": float(fix[f"{name}_scale_shift"][1]),
           "pair_errors": fix[f"{name}_pair_errors"], "pair_counts": fix[f"{name}_pair_counts"], "margins": fix[f"{name}_margins"]}
    for arr in (pred, gt, K, poses, mask):
        if arr is not None:
            arr.setflags(write=False)
    _loaded[name] = (pred, gt, K, poses, mask, float(max_depth), exp)
    return _loaded[name]


def assert_matches(got, exp, what=""):
    """The bounds of the issue: TAE, the per-direction errors, scale and shift to REL_TOL (1e-12, the scorer's bound) relative, the
    per-direction counts exact. A direction whose expected error is exactly 0 (no use) must be exactly 0. Prints every figure first."""
    bad = []
    for k in ("tae", "scale", "shift"):
        err = abs(got[k] - exp[k]) / abs(exp[k])
        print(f"{what} {k}: got {got[k]!r} want {exp[k]!r} rel {err:.3e}")
        if not err <= REL_TOL:
            bad.append((k, err))
    ge, ee = np.asarray(got["pair_errors"]), np.asarray(exp["pair_errors"])
    assert ge.shape == ee.shape and ge.dtype == np.float64, (ge.shape, ee.shape, ge.dtype)
    rel = np.where(ee != 0, np.abs(ge - ee) / np.where(ee != 0, np.abs(ee), 1.0), np.where(ge == 0, 0.0, np.inf))
    print(f"{what} pair_errors: worst rel {rel.max():.3e} at {np.unravel_index(rel.argmax(), rel.shape)}")
    if not (rel <= REL_TOL).all():
        bad.append(("pair_errors", rel.max()))
    gc, ec = np.asarray(got["pair_counts"]), np.asarray(exp["pair_counts"])
    print(f"{what} pair_counts: got {gc.ravel().tolist()} want {ec.ravel().tolist()}")
    if gc.shape != ec.shape or not (gc == ec).all():
        bad.append(("pair_counts", gc.ravel().tolist()))
    assert not bad, f"{what}: {bad}"
