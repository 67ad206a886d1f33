"""The loss tests' view of tests/golden/loss_metrics.npz (written by tools/gen_loss_golden.py from the reference's own modules), and
the inputs of its case D, which are too large to commit: generated from the counter-based integer hash of _eval_inputs.py and IEEE
float32 add / multiply only, so every platform produces the same bits; the fixture records their checksum."""
import hashlib
import os

import numpy as np

from _eval_inputs import _hash24

CASES = ("A", "B", "C", "D", "E")
VARIANTS = ("lsq", "mad")
CASE_D = dict(B=1, N=4, H=130, W=257)

# Bounds against the reference's float64 run. SSI: every term is fp64 and the sums are reordered fp64 sums of at most
# 33 410 terms; 1e-12 relative holds with room. TGM: the reference accumulates the pairs into a float32 scalar whatever the input
# dtype (torch.zeros(()) with +=): at most N + 2 float32 roundings of non-negative running sums, and the final division makes N + 3.
SSI_TOL = 1e-12
F32_SANITY_TOL = 1e-5


def tgm_tol(N):
    return (N + 3) * 2.0 ** -24


def case_d_inputs():
    """(pred, y) float32 [1,4,130,257]: y walks by less than 0.1 per frame and never lands within 1e-3 of the 0.05 threshold."""
    f = np.float32
    N, H, W = CASE_D["N"], CASE_D["H"], CASE_D["W"]
    px = H * W
    idx = np.arange(N * px, dtype=np.uint64)
    inv = f(1.0 / (1 << 24))
    u, v, w = (_hash24(idx, s) * inv for s in (5 << 32, 6 << 32, 7 << 32))                  # [0, 1)
    u, v, w = u.reshape(N, px), v.reshape(N, px), w.reshape(N, px)
    y = np.empty((N, px), dtype=np.float32)
    y[0] = f(0.5) + u[0] * f(3.0)
    for i in range(1, N):
        step = (v[i] - f(0.5)) * f(0.2)
        step = np.where(np.abs(np.abs(step) - f(0.05)) < f(1e-3), f(0.02), step).astype(np.float32)
        y[i] = y[i - 1] + step
    pred = (y - f(0.3)) * f(0.6) + (w - f(0.5)) * f(0.2)
    return np.ascontiguousarray(pred.reshape(1, N, H, W)), np.ascontiguousarray(y.reshape(1, N, H, W))


def checksum(pred, y):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(pred).tobytes())
    h.update(np.ascontiguousarray(y).tobytes())
    return h.hexdigest()


_cache = {}


def load_case(golden_dir, name):
    """(pred, y, mask or None, expected dict) of one case, loaded once and read-only. expected: 'ref64' / 'ref32' = {lsq, mad, tgm} of
    the reference's float64 / float32 run, 'n_static' [B,N-1]."""
    if name not in _cache:
        fix = np.load(os.path.join(golden_dir, "loss_metrics.npz"))
        if name == "D":
            pred, y = case_d_inputs()
            assert checksum(pred, y) == str(fix["D_sha256"]), "case D's generated inputs are not the ones the reference scored"
        else:
            pred, y = fix[f"{name}_pred"], fix[f"{name}_y"]
        mask = fix[f"{name}_mask"] if f"{name}_mask" in fix.files else None
        for a in (pred, y) + (() if mask is None else (mask,)):
            a.setflags(write=False)
        assert fix[f"{name}_conditions"][0] > fix["static_guard"] and fix[f"{name}_conditions"][1] > fix["loss_guard"]
        names = [str(k) for k in fix["outputs"]]
        exp = {"ref64": dict(zip(names, fix[f"{name}_ref64"])), "ref32": dict(zip(names, fix[f"{name}_ref32"])),
               "n_static": fix[f"{name}_n_static"]}
        _cache[name] = (pred, y, mask, exp)
    return _cache[name]


def rel(got, want):
    """|got - want| / |want|; 0 when both are the same number (a loss of exactly 0 is exactly 0 in every implementation)."""
    got, want = float(got), float(want)
    if got == want:
        return 0.0
    return abs(got - want) / abs(want) if want != 0.0 else float("inf")


def assert_within(got, want, tol, what):
    err = rel(got, want)
    print(f"{what}: got {got!r} want {want!r} rel {err:.3e} (bound {tol:.3e})")
    assert err <= tol, (what, got, want, err, tol)
