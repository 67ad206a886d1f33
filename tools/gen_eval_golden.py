#!/usr/bin/env python
"""Write tests/golden/eval_metrics.npz: what the REFERENCE's scorer (benchmark/eval/eval.py eval_depthcrafter, metric.py)
computes on the four test cases of the device scorer (video_depth_anything_amd/evaluate.py).

    python tools/gen_eval_golden.py --reference <reference checkout> [--check]

The reference's modules are imported at run time from that checkout; nothing of them is copied. Three things stand between
its eval.py and a result on a machine without cv2 or a GPU, all arranged from outside the module: a stand-in `cv2` in sys.modules
when cv2 is not importable (the .npy route never calls it), `device = 'cpu'`, and the `metric` global that eval_depthcrafter reads
but the module never binds. `eval_metrics` is set to the six names this project reports. The scale and shift are the ones the
reference's own np.linalg.lstsq call returns (recorded while it runs).

Per case the fixture holds the six metrics, scale / shift, the exact counts, the inputs (cases A-C; case D's come from
tests/_eval_inputs.py and only their checksum is stored) and the guard margins. The guards are conditions on the INPUTS under
which the counts are exact and no pixel may be left out of a comparison - not tolerances; a seed that violates one is replaced:
    no valid pixel has max(p/g, g/p) within 1e-9 of 1.25, 1.25^2 or 1.25^3
    no gt lies within 1e-9 relative of 1e-3 or of max_depth
    at least two valid pixels, and a nonzero determinant of the normal equations
--check regenerates everything and compares it with the committed file bit for bit. No test imports this tool or the reference.
"""
import argparse
import importlib
import os
import sys
import tempfile
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from _eval_inputs import CASE_D, case_d_inputs, checksum  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "eval_metrics.npz")
METRICS = ["abs_relative_difference", "squared_relative_difference", "rmse_linear", "delta1_acc", "delta2_acc", "delta3_acc"]
GUARD = 1e-9


def import_reference(root):
    for name in ("cv2", "matplotlib", "matplotlib.pyplot", "scipy", "scipy.ndimage", "tqdm"):
        try:
            importlib.import_module(name)
        except ImportError:
            stub = types.ModuleType(name)
            stub.map_coordinates = None
            stub.tqdm = lambda it: it
            sys.modules[name] = stub
    sys.path.insert(0, os.path.abspath(root))
    ev = importlib.import_module("benchmark.eval.eval")
    met = importlib.import_module("benchmark.eval.metric")
    ev.device = "cpu"
    ev.metric = met
    ev.eval_metrics = list(METRICS)
    return ev


# ------------------------------------------------------------------ the cases: (pred at the cropped size, raw gt, settings)
def case_a():
    """N=5, 37x53 cropped to 34x50, float32 gt: zeros, a frame without a valid pixel, depth beyond max_depth, pred below the clip."""
    rng = np.random.default_rng(0)
    N, H, W = 5, 37, 53
    gt = rng.uniform(0.3, 12.0, (N, H, W)).astype(np.float32)
    gt[rng.random((N, H, W)) < 0.15] = 0
    gt[3] = 0
    gt[4, :, :20] = 50.0
    disp = np.where(gt > 0, 1 / np.maximum(gt, 1e-3), 0.5)
    pred = (2.5 * disp + 0.4 + 0.15 * rng.standard_normal((N, H, W)) * disp).astype(np.float32)
    pred[0, :3] = -0.2
    pred[1, 5:9, :] = 1e-4
    crop = (2, -1, 3, W)
    return np.ascontiguousarray(pred[:, crop[0]:crop[1], crop[2]:crop[3]]), gt, dict(crop=crop, factor=1.0, max_depth=10.0, max_eval_len=110)


def case_b():
    """N=3, 64x64, uint16 gt with factor 1000 (the float64 path), max_eval_len=2. disparity = 0.5 * pred + 0.3, so the fitted shift is
    far above 1e-3 and pred < 1e-3 wherever gt > 3.33 m: clipping pred before the fit and before the alignment changes the result."""
    rng = np.random.default_rng(1)
    N, H, W = 3, 64, 64
    raw = rng.integers(500, 12000, (N, H, W)).astype(np.uint16)
    raw[raw == 10000] = 10001                                    # gt == max_depth exactly would sit on the validity boundary
    raw[rng.random((N, H, W)) < 0.1] = 0
    disp = 1.0 / np.maximum(raw / 1000.0, 0.1)
    pred = ((disp - 0.3) * 2.0 * (1 + 0.05 * rng.standard_normal((N, H, W)))).astype(np.float32)
    pred[2] = rng.uniform(0.0, 3.0, (H, W)).astype(np.float32)   # unrelated to gt: must be cut off by max_eval_len
    return pred, raw, dict(crop=(0, H, 0, W), factor=1000.0, max_depth=10.0, max_eval_len=2)


def case_c():
    """N=1, 1x301 with 7 valid pixels, all past the first 256: a tail, a block without a valid pixel, the fewest points of a sane fit."""
    rng = np.random.default_rng(2)
    gt = np.zeros((1, 1, 301), np.float32)
    at = np.array([257, 263, 270, 281, 288, 295, 300])
    gt[0, 0, at] = rng.uniform(0.5, 8.0, at.size).astype(np.float32)
    pred = rng.uniform(0.05, 2.0, (1, 1, 301)).astype(np.float32)
    pred[0, 0, at] = (1.3 / gt[0, 0, at] + 0.1 + 0.02 * rng.standard_normal(at.size)).astype(np.float32)
    return pred, gt, dict(crop=(0, 1, 0, 301), factor=1.0, max_depth=10.0, max_eval_len=110)


def case_d():
    pred, gt = case_d_inputs()
    return pred, gt, dict(crop=(0, CASE_D["H"], 0, CASE_D["W"]), factor=1.0, max_depth=CASE_D["max_depth"], max_eval_len=100)


# ------------------------------------------------------------------ scoring
def run_reference(ev, pred, raw_gt, cfg):
    """eval_depthcrafter on .npy files of the case; returns (six metrics, (scale, shift) of its own lstsq)."""
    a, b, c, d = cfg["crop"]
    args = types.SimpleNamespace(a=a, b=b, c=c, d=d, max_eval_len=cfg["max_eval_len"], max_depth_eval=cfg["max_depth"])
    seen = []
    real = np.linalg.lstsq

    def recording(*p, **k):
        out = real(*p, **k)
        seen.append(np.array(out[0], dtype=np.float64).ravel())
        return out

    with tempfile.TemporaryDirectory() as tmp:
        ip, gp = [], []
        for i in range(pred.shape[0]):
            ip.append(os.path.join(tmp, f"inf_{i:03d}.npy"))
            gp.append(os.path.join(tmp, f"gt_{i:03d}.npy"))
            np.save(ip[-1], pred[i])
            np.save(gp[-1], raw_gt[i])
        np.linalg.lstsq = recording
        try:
            res = ev.eval_depthcrafter(ip, gp, [cfg["factor"]] * pred.shape[0], args)
        finally:
            np.linalg.lstsq = real
    assert len(seen) == 1 and seen[0].size == 2
    return np.array(res, dtype=np.float64), seen[0]


def guards(pred, raw_gt, cfg, scale, shift, clip_pred=True):
    """The conditions on the inputs (module docstring), evaluated with the reference's scale / shift. Returns
    ([ratio margin, gt margin, determinant], n_valid, frames used, abs_rel of this restatement)."""
    a, b, c, d = cfg["crop"]
    L = cfg["max_eval_len"]
    gt = (raw_gt / cfg["factor"])[:L, a:b, c:d]
    x32 = pred[:L]
    valid = (gt > 1e-3) & (gt < cfg["max_depth"])
    xc = np.clip(x32, 1e-3, None) if clip_pred else x32
    g = gt.astype(np.float64)[valid]
    x = xc[valid].astype(np.float64)
    if not clip_pred:                                            # the variant the reference does NOT compute: refit without the clip
        y = 1.0 / (g + 1e-8)
        n = x.size
        det = n * (x * x).sum() - x.sum() ** 2
        scale = (n * (x * y).sum() - x.sum() * y.sum()) / det
        shift = ((x * x).sum() * y.sum() - x.sum() * (x * y).sum()) / det
    p = np.clip(1.0 / np.clip(scale * x + shift, 1e-3, None), 1e-3, cfg["max_depth"])
    r = np.maximum(p / g, g / p)
    ratio_margin = min(np.abs(r - t).min() for t in (1.25, 1.25 ** 2, 1.25 ** 3))
    allg = gt.astype(np.float64).ravel()
    gt_margin = min(np.abs(allg / 1e-3 - 1).min(), np.abs(allg / cfg["max_depth"] - 1).min())
    n = x.size
    det = n * (x * x).sum() - x.sum() ** 2
    nf = valid.sum((1, 2))
    fidx = np.nonzero(valid)[0]                                  # frame of every valid pixel
    per_frame = np.bincount(fidx, weights=np.abs(p - g) / g, minlength=len(nf))[nf > 0] / nf[nf > 0]
    return np.array([ratio_margin, gt_margin, det]), int(n), int((nf > 0).sum()), float(per_frame.mean())


def generate(ev):
    out = {"metrics": np.array(METRICS), "guard": np.float64(GUARD)}
    for name, make in (("A", case_a), ("B", case_b), ("C", case_c), ("D", case_d)):
        pred, raw_gt, cfg = make()
        ref, ss = run_reference(ev, pred, raw_gt, cfg)
        margins, n_valid, n_used, abs_rel = guards(pred, raw_gt, cfg, ss[0], ss[1])
        assert margins[0] > GUARD, f"case {name}: a ratio within {GUARD} of a delta threshold ({margins[0]}): change the seed"
        assert margins[1] > GUARD, f"case {name}: a gt within {GUARD} relative of 1e-3 or max_depth ({margins[1]}): change the seed"
        assert n_valid >= 2 and margins[2] != 0.0, f"case {name}: degenerate fit"
        assert abs(abs_rel - ref[0]) <= 1e-9 * abs(ref[0]), f"case {name}: this tool's reading of the inputs disagrees with the reference"
        if name == "A":
            assert n_used == 4, "case A: frame 3 has no valid pixel and must be dropped"
        if name == "B":
            assert ss[1] > 1e-3 and (pred[:2] < 1e-3).any()
            unclipped = guards(pred, raw_gt, cfg, ss[0], ss[1], clip_pred=False)[3]
            assert abs(unclipped - ref[0]) > 1e-6, "case B: clipping pred must change the result"
        if name == "C":
            assert n_valid == 7
        out[f"{name}_ref"] = ref
        out[f"{name}_scale_shift"] = ss
        out[f"{name}_counts"] = np.array([n_valid, n_used], dtype=np.int64)
        out[f"{name}_margins"] = margins
        out[f"{name}_settings"] = np.array(list(cfg["crop"]) + [cfg["max_depth"], cfg["max_eval_len"], cfg["factor"]], dtype=np.float64)
        if name == "D":
            out["D_sha256"] = np.array(checksum(pred, raw_gt))
        else:
            out[f"{name}_pred"], out[f"{name}_gt_raw"] = pred, raw_gt
        print(f"case {name}: n_valid={n_valid} frames used={n_used} scale={ss[0]!r} shift={ss[1]!r}")
        print("   ", ", ".join(f"{m}={v!r}" for m, v in zip(METRICS, ref)))
        print(f"    margins: ratio {margins[0]:.3e}, gt {margins[1]:.3e}, det {margins[2]:.6e}")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference project (its benchmark/eval is imported)")
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
