"""Inputs of the scorer's large test case (case D of tests/golden/eval_metrics.npz), too large to commit: generated from a
counter-based integer hash in uint64 numpy and IEEE float32 add / multiply / divide only, so every platform produces the same
bits. tools/gen_eval_golden.py scores exactly these arrays with the reference and records their checksum; the tests rebuild
them and check the checksum before use."""
import hashlib

import numpy as np

CASE_D = dict(N=2, H=436, W=1024, max_depth=70.0)


def _hash24(idx, stream):
    """splitmix64 of (index, stream), top 24 bits: exact in float32."""
    z = (idx + np.uint64(stream)) * np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float32)


def case_d_inputs():
    """(pred float32 [2,436,1024], gt float32 [2,436,1024]): depth 0.4 .. 75.4 (some beyond max_depth 70), about 10 % zeros,
    pred = 1.7 * disparity + 0.05 + noise."""
    f = np.float32
    N, H, W = CASE_D["N"], CASE_D["H"], CASE_D["W"]
    idx = np.arange(N * H * W, dtype=np.uint64)
    inv = f(1.0 / (1 << 24))
    u, v, w = _hash24(idx, 1) * inv, _hash24(idx, 2 << 32) * inv, _hash24(idx, 3 << 32) * inv      # [0, 1)
    gt = f(0.4) + u * f(75.0)
    disp = f(1.0) / gt
    pred = f(1.7) * disp + f(0.05) + (v - f(0.5)) * f(2.0) * disp
    gt = np.where(w < f(0.1), f(0.0), gt).astype(np.float32)
    return np.ascontiguousarray(pred.reshape(N, H, W)), np.ascontiguousarray(gt.reshape(N, H, W))


def checksum(pred, gt):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(pred).tobytes())
    h.update(np.ascontiguousarray(gt).tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------ the fixture as the tests read it
SUM_METRICS = ("abs_relative_difference", "squared_relative_difference", "rmse_linear")
DELTA_METRICS = ("delta1_acc", "delta2_acc", "delta3_acc")
# Bounds against the reference (the scorer's section). Sum-based metrics, scale and shift: a reordered fp64 sum of
# n <= 9e5 same-signed terms moves by at most n * 2^-53 ~ 1e-10 relative, in practice ~sqrt(n) * 2^-53; 1e-12 holds on every case.
# Deltas: the reference rounds count / n to float32 (2^-24 = 6e-8 relative of a value <= 1) and averages in float32.
REL_TOL = 1e-12
DELTA_TOL = 1e-7


def load_case(golden_dir, name):
    """(pred, gt, max_depth, max_eval_len, expected dict) of case A / B / C / D: gt already divided by its factor (numpy's own
    promotion) and cropped, as the scorer takes it."""
    import os
    fix = np.load(os.path.join(golden_dir, "eval_metrics.npz"))
    a, b, c, d, max_depth, max_eval_len, factor = fix[f"{name}_settings"]
    if name == "D":
        pred, raw = case_d_inputs()
        assert checksum(pred, raw) == str(fix["D_sha256"]), "case D's generated inputs are not the ones the reference scored"
    else:
        pred, raw = fix[f"{name}_pred"], fix[f"{name}_gt_raw"]
    gt = (raw / float(factor))[:, int(a):int(b), int(c):int(d)]
    exp = dict(zip([str(m) for m in fix["metrics"]], fix[f"{name}_ref"]))
    exp["scale"], exp["shift"] = fix[f"{name}_scale_shift"]
    exp["n_valid"], exp["n_frames_used"] = (int(v) for v in fix[f"{name}_counts"])
    assert fix[f"{name}_margins"][0] > fix["guard"] and fix[f"{name}_margins"][1] > fix["guard"] and fix[f"{name}_margins"][2] != 0.0
    return pred, gt, float(max_depth), int(max_eval_len), exp


def assert_matches(got, exp, what=""):
    """The bounds of the issue: scale, shift and the sum-based metrics to REL_TOL relative, deltas to DELTA_TOL absolute, counts exact.
    Prints every figure before asserting."""
    bad = []
    for k in ("scale", "shift") + SUM_METRICS:
        err = abs(got[k] - exp[k]) / abs(exp[k])
        print(f"{what} {k}: got {got[k]!r} want {exp[k]!r} rel {err:.3e}")
        if not err <= REL_TOL:
            bad.append((k, err))
    for k in DELTA_METRICS:
        err = abs(got[k] - exp[k])
        print(f"{what} {k}: got {got[k]!r} want {exp[k]!r} abs {err:.3e}")
        if not err <= DELTA_TOL:
            bad.append((k, err))
    for k in ("n_valid", "n_frames_used"):
        print(f"{what} {k}: got {got[k]} want {exp[k]}")
        if got[k] != exp[k]:
            bad.append((k, got[k]))
    assert not bad, f"{what}: {bad}"
