#!/usr/bin/env python
"""Write tests/golden/loss_metrics.npz: what the REFERENCE's loss modules (utils/loss_MiDas.py: Loss_ssi, Loss_tgm, the ones its
train.py imports; utils/loss.py: the Depth-Anything form of Loss_ssi) compute on the five test cases of the device losses
(video_depth_anything_amd/losses.py).

    python tools/gen_loss_golden.py --reference <reference checkout> [--check]

The reference's two files are imported at run time by path from that checkout; nothing of them is copied. Their prints are
silenced. Every case is fed twice: as float32, and as the same values widened to float64 - the second run is the reference's own
arithmetic without its float32 rounding, which is what the tests hold the fp64 device path against.

Cases (seeded, each the smallest shape at which a kernel can still go wrong):
    A  2x5x37x53   H*W = 1961 is odd (misaligned planes); ~60 % mask, frame (0,2) fully masked, frame (1,1) with whole rows masked
    B  1x2x1x3     one valid pixel per frame (den = 0, sc = eps)
    C  1x3x64x64   all valid, values quantised to 1/16 with many ties, negatives and both zeros (key mapping, lower median of an
                   even count)
    D  1x4x130x257 mask=None, more values than one sweep of a 1024-thread block; inputs from tests/_loss_inputs.py, only their
                   checksum is stored (130 * 257 = 33 410 values per plane: an even count)
    E  2x4x16x20   pair (0; 0,1) without a commonly valid pixel, pair (1; 1,2) without a static pixel

Conditions on the INPUTS, checked here and recorded per case so that no pixel may be excused - not tolerances:
    no |y[i+1] - y[i]| (fp64 difference of the float32 values, any pixel) lies within 1e-6 of 0.05: the float32 and float64 runs of
        the reference then count the same static pixels, and n_static is exact
    every frame with at least two valid pixels has an lsq loss above 1e-6 x the mean of its valid y^2: that bounds how much the
        residual's cancellation can amplify rounding (a frame with one valid pixel is fitted exactly: its loss is exactly 0)
--check regenerates everything and compares it with the committed file bit for bit. No test imports the reference.
"""
import argparse
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from _loss_inputs import case_d_inputs, checksum  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "loss_metrics.npz")
OUTPUTS = ["lsq", "mad", "tgm"]
STATIC_GUARD = 1e-6
LOSS_GUARD = 1e-6


def import_reference(root):
    mods = []
    for name in ("loss_MiDas", "loss"):
        spec = importlib.util.spec_from_file_location(f"_reference_{name}", os.path.join(os.path.abspath(root), "utils", f"{name}.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mods.append(mod)
    return mods


# ------------------------------------------------------------------ the cases: (pred, y, mask or None)
def _walk(rng, shape, lo=0.5, hi=3.5):
    """y [B,N,H,W] float32: a random first frame, then steps below 0.1 that stay 1e-3 clear of the 0.05 threshold."""
    B, N, H, W = shape
    y = np.empty(shape, dtype=np.float32)
    y[:, 0] = rng.uniform(lo, hi, (B, H, W)).astype(np.float32)
    for i in range(1, N):
        step = rng.uniform(-0.1, 0.1, (B, H, W)).astype(np.float32)
        step[np.abs(np.abs(step) - 0.05) < 1e-3] = np.float32(0.02)
        y[:, i] = y[:, i - 1] + step
    return y


def _pred_of(rng, y, noise=0.05):
    return ((y - 0.3) * 0.6 + noise * rng.standard_normal(y.shape)).astype(np.float32)


def case_a():
    rng = np.random.default_rng(10)
    shape = (2, 5, 37, 53)
    y = _walk(rng, shape)
    pred = _pred_of(rng, y)
    mask = rng.random(shape) < 0.6
    mask[0, 2] = False
    mask[1, 1, 5:12, :] = False
    mask[1, 3, 36, :] = False
    return pred, y, mask.astype(np.uint8)


def case_b():
    y = np.array([[[[0.7, 1.25, 2.0]], [[0.9, 1.26, 1.5]]]], dtype=np.float32)
    pred = np.array([[[[0.3, 0.55, 0.1]], [[0.2, 0.6, 0.8]]]], dtype=np.float32)
    mask = np.array([[[[0, 1, 0]], [[0, 1, 0]]]], dtype=np.uint8)
    return pred, y, mask


def case_c():
    rng = np.random.default_rng(12)
    shape = (1, 3, 64, 64)
    q = np.float32(1.0 / 16.0)
    y = rng.integers(-32, 33, shape).astype(np.float32) * q
    pred = rng.integers(-24, 25, shape).astype(np.float32) * q
    y[0, 1] = y[0, 0]                                            # a wholly static pair; many exact ties everywhere
    y[0, 1, :8] += q                                             # ... except eight rows that move by 1/16 > 0.05
    # frame 1 of pred: 40 % negative, 20 % zeros of both signs, 40 % positive, so that the lower median lands among the zeros
    u = rng.random((64, 64))
    f1 = np.where(u < 0.4, -rng.integers(1, 25, (64, 64)), np.where(u < 0.6, 0, rng.integers(1, 25, (64, 64)))).astype(np.float32) * q
    f1[(u >= 0.4) & (u < 0.5)] = np.float32(-0.0)
    pred[0, 1] = f1
    y[0, 2, 0, :5] = np.float32(-0.0)
    return pred, y, np.ones(shape, dtype=np.uint8)


def case_d():
    pred, y = case_d_inputs()
    return pred, y, None


def case_e():
    rng = np.random.default_rng(14)
    shape = (2, 4, 16, 20)
    y = _walk(rng, shape)
    step = y[1, 3] - y[1, 2]
    y[1, 2] = y[1, 1] + np.float32(0.5)                          # clip 1, pair (1, 2): nothing is static
    y[1, 3] = y[1, 2] + step
    pred = _pred_of(rng, y)
    mask = rng.random(shape) < 0.8
    mask[0, 0, :, 10:] = False                                   # clip 0, pair (0, 1): no commonly valid pixel
    mask[0, 1, :, :10] = False
    return pred, y, mask.astype(np.uint8)


CASES = (("A", case_a), ("B", case_b), ("C", case_c), ("D", case_d), ("E", case_e))


# ------------------------------------------------------------------ scoring
def run_reference(mods, pred, y, mask, dtype):
    """[lsq, mad, tgm] of the reference on the inputs as `dtype`, as float64 numbers (its results are 0-dim tensors)."""
    midas, da = mods
    p, g = torch.from_numpy(pred.astype(dtype)), torch.from_numpy(y.astype(dtype))
    m = torch.from_numpy(np.ones(pred.shape, dtype=bool) if mask is None else mask != 0)
    with contextlib.redirect_stdout(io.StringIO()), torch.no_grad():
        lsq = midas.Loss_ssi()(p.clone(), g.clone(), m.clone())
        mad = da.Loss_ssi()(p.clone(), g.clone(), m.clone())
        tgm = midas.Loss_tgm()(p.clone(), g.clone(), m.clone())
        tgm_da = da.Loss_tgm()(p.clone(), g.clone(), m.clone())
    assert tgm.dtype == torch.float32, "the reference accumulates Loss_tgm in a float32 scalar whatever the input dtype"
    assert tgm.numpy().tobytes() == tgm_da.numpy().tobytes(), "the two files' Loss_tgm differ"
    return np.array([float(lsq), float(mad), float(tgm)], dtype=np.float64)


def conditions(pred, y, mask):
    """([margin of |dy| to 0.05, smallest lsq loss / mean valid y^2 over the frames with >= 2 valid pixels], n_static [B,N-1]):
    this tool's own fp64 reading of the inputs."""
    B, N, H, W = y.shape
    g, d = y.astype(np.float64), pred.astype(np.float64)
    m = np.ones(y.shape, dtype=bool) if mask is None else mask != 0
    gy = np.abs(g[:, 1:] - g[:, :-1])
    margin = np.abs(gy - 0.05).min()
    n_static = ((gy < 0.05) & m[:, 1:] & m[:, :-1]).sum((2, 3)).astype(np.int64)
    ratio = np.inf
    for b in range(B):
        for i in range(N):
            v = m[b, i]
            if v.sum() < 2:
                continue
            dv, gv = d[b, i][v], g[b, i][v]
            dd, dg = dv - dv.mean(), gv - gv.mean()
            s = (dd * dg).sum() / ((dd * dd).sum() + 1e-8)
            t = gv.mean() - s * dv.mean()
            ratio = min(ratio, ((s * dv + t - gv) ** 2).mean() / (gv * gv).mean())
    return np.array([margin, ratio], dtype=np.float64), n_static


def generate(mods):
    out = {"outputs": np.array(OUTPUTS), "static_guard": np.float64(STATIC_GUARD), "loss_guard": np.float64(LOSS_GUARD)}
    for name, make in CASES:
        pred, y, mask = make()
        assert pred.dtype == np.float32 and y.dtype == np.float32 and np.isfinite(pred).all() and np.isfinite(y).all()
        ref64 = run_reference(mods, pred, y, mask, np.float64)
        ref32 = run_reference(mods, pred, y, mask, np.float32)
        cond, n_static = conditions(pred, y, mask)
        assert cond[0] > STATIC_GUARD, f"case {name}: a |dy| within {STATIC_GUARD} of 0.05 ({cond[0]}): change the seed"
        assert cond[1] > LOSS_GUARD, f"case {name}: an lsq frame loss below {LOSS_GUARD} x mean y^2 ({cond[1]}): change the seed"
        m = np.ones(y.shape, dtype=bool) if mask is None else mask != 0
        if name == "A":
            assert not m[0, 2].any() and not m[1, 1, 5:12].any() and m[1, 1].any() and 0.5 < m.mean() < 0.65
        if name == "B":
            assert (m.sum((2, 3)) == 1).all() and ref64[0] == 0.0
        if name == "C":
            assert m.all() and (np.signbit(pred[0, 1]) & (pred[0, 1] == 0)).any() and (~np.signbit(pred[0, 1]) & (pred[0, 1] == 0)).any()
            assert np.sort(pred[0, 1].ravel())[(64 * 64 - 1) // 2] == 0.0
        if name == "E":
            assert not (m[0, 0] & m[0, 1]).any() and n_static[1, 1] == 0 and (m[1, 1] & m[1, 2]).any()
            assert (np.delete(n_static.ravel(), [0, 4]) > 0).all()
        out[f"{name}_ref64"], out[f"{name}_ref32"] = ref64, ref32
        out[f"{name}_n_static"], out[f"{name}_conditions"] = n_static, cond
        if name == "D":
            out["D_sha256"] = np.array(checksum(pred, y))
        else:
            out[f"{name}_pred"], out[f"{name}_y"] = pred, y
        if mask is not None:
            out[f"{name}_mask"] = mask
        print(f"case {name} {y.shape}: float64 run " + ", ".join(f"{k}={v!r}" for k, v in zip(OUTPUTS, ref64)))
        print("    float32 run " + ", ".join(f"{k}={v!r}" for k, v in zip(OUTPUTS, ref32)))
        print(f"    |dy| margin to 0.05: {cond[0]:.3e}; smallest lsq loss / mean y^2: {cond[1]:.3e}; n_static {n_static.tolist()}")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference project (its utils/loss_MiDas.py and utils/loss.py are imported)")
    ap.add_argument("--check", action="store_true", help="compare with the committed fixture bit for bit instead of writing it")
    args = ap.parse_args()
    new = generate(import_reference(args.reference))
    if args.check:
        old = np.load(OUT)
        assert sorted(old.files) == sorted(new), f"keys differ: {sorted(set(old.files) ^ set(new))}"
        bad = [k for k in new if np.asarray(new[k]).dtype != old[k].dtype or np.asarray(new[k]).tobytes() != old[k].tobytes()]
        if bad:
            sys.exit(f"fixture differs in {bad}")
        print(f"{OUT}: reproduced bit for bit")
    else:
        np.savez(OUT, **new)
        print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
