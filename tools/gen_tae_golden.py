#!/usr/bin/env python
"""Write tests/golden/tae_metrics.npz: what the REFERENCE's temporal-alignment-error scorer (benchmark/eval/eval_tae.py, eval_TAE
and tae_torch) computes on the four test cases of the device scorer (video_depth_anything_amd/evaluate.py, evaluate_tae).

    python tools/gen_tae_golden.py --reference <reference checkout> [--check]

The reference's module is imported at run time from that checkout; nothing of it is copied. What stands between eval_tae.py and a
result on a machine without cv2 or a GPU is arranged from outside the module, as in tools/gen_eval_golden.py: stand-in modules in
sys.modules for the imports that are missing, `device = cpu` (and torch.set_num_threads(1)), and a `cv2` attribute whose imread
reads the .npy masks this tool writes. eval_TAE runs on .npy files in a temporary directory. While it runs, np.linalg.lstsq is
recorded (its scale / shift) and tae_torch is wrapped from outside: every call's arguments and return value are kept.

The tool then REPLAYS every recorded tae_torch call: the same torch operations up to the rounding, then a sequential splat of its
own (source pixels in row-major order, the last one stays), then the same mean. It asserts that this reproduces every value the
reference returned, and the TAE, BIT FOR BIT: on the CPU the reference's index assignment with duplicate indices means last-wins.
The replay also yields what the reference does not return - the per-direction counts, the guard margins, the collision
statistics - and the variants the reference does NOT compute (first-wins, nearest-wins, K[i+1], swapped masks), which the cases
are built to tell apart.

Guards are conditions on the INPUTS under which the winners, and so every count, are exact - not tolerances; a seed that violates
one is replaced:
    every pre-rounding u, v of every source pixel is at least 1e-6 from a half-integer and below 1e6 in magnitude; every |Qz| > 1e-6
    no gt lies within 1e-9 relative of 1e-3 or of max_depth; at least two valid pixels and a nonzero determinant
    fewer than a quarter of a case's aligned depths sit on a clip bound (1e-3 or max_depth)
margins stored per case: [min distance of u, v from a half-integer, max |u|, |v|, min |Qz|, gt margin, determinant, clipped share].
--check regenerates everything and compares it with the committed file bit for bit. No test imports this tool or the reference.
"""
import argparse
import importlib
import os
import sys
import tempfile
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from _tae_inputs import CASE_D, case_d_inputs, checksum  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "tae_metrics.npz")
HALF_GUARD, MAG_GUARD, QZ_GUARD, GT_GUARD = 1e-6, 1e6, 1e-6, 1e-9


class _Cv2Shim:
    """cv2 as eval_tae.py uses it on the .npy route: imread of a mask. Anything else goes to the real module, if there is one."""

    def __init__(self, real):
        self._real = real

    def imread(self, path, flag=None):
        if path.endswith(".npy"):
            return np.load(path)
        return self._real.imread(path, flag)

    def __getattr__(self, name):
        return getattr(self._real, name)


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
    ev = importlib.import_module("benchmark.eval.eval_tae")
    ev.device = torch.device("cpu")
    ev.cv2 = _Cv2Shim(ev.cv2)
    torch.set_num_threads(1)
    return ev


# ------------------------------------------------------------------ the cases
def rot_y(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def pose(R=None, t=(0, 0, 0)):
    T = np.eye(4)
    if R is not None:
        T[:3, :3] = R
    T[:3, 3] = t
    return T


def surface(rng, N, H, W, lo, hi, relief):
    """A smooth surface lo .. hi metres that changes a little from frame to frame, with per-pixel relief."""
    y, x = np.mgrid[0:H, 0:W]
    out = []
    for i in range(N):
        s = 0.5 + 0.25 * np.sin(x / 9.0 + 0.3 * i) + 0.25 * np.cos(y / 7.0 - 0.2 * i)
        out.append((lo + (hi - lo) * s) * (1 + relief * rng.standard_normal((H, W))))
    return np.stack(out)


def pred_of(rng, depth, scale, shift, noise):
    return ((1.0 / depth - shift) / scale * (1 + noise * rng.standard_normal(depth.shape))).astype(np.float32)


def case_a():
    """N=4, 39x57 cropped to 37x53, float32 gt. Pairs 0 and 1 move gently; pair 2 yaws by 90 degrees, so no source pixel lands in the
    image in either direction: tae_torch's first early return of 0, still counted in the denominator. K differs per frame."""
    rng = np.random.default_rng(10)
    N, H, W = 4, 39, 57
    depth = surface(rng, N, H, W, 1.5, 3.5, 0.02)
    gt = depth.astype(np.float32)
    gt[rng.random((N, H, W)) < 0.1] = 0
    crop = (1, -1, 2, -2)
    pred = np.ascontiguousarray(pred_of(rng, depth, 0.8, 0.05, 0.02)[:, 1:-1, 2:-2])
    K = np.stack([np.array([[40.0 + 2 * i, 0, 26.0 + 0.3 * i], [0, 42.0 - 1.5 * i, 18.0 - 0.2 * i], [0, 0, 1]]) for i in range(N)])
    poses = np.stack([pose(), pose(rot_y(1.5), (0.06, 0.02, 0.03)), pose(rot_y(-1.0), (0.10, -0.03, 0.12)), pose(rot_y(89.0), (0.1, 0.0, 0.1))])
    return pred, gt, K, poses, None, dict(crop=crop, factor=1.0, max_depth=10.0)


def case_b():
    """N=3, 48x64, uint16 gt with factor 1000. Pair 0: the camera backs away by 0.9 m, the image shrinks and sources collide. Pair 1:
    it moves forward by 1.4 m past the near bottom rows (0.6 .. 0.9 m), whose points end up BEHIND it and project mirrored into the
    upper rows, later in row-major order than the visible sources there."""
    rng = np.random.default_rng(21)
    N, H, W = 3, 48, 64
    depth = surface(rng, N, H, W, 2.0, 3.5, 0.03)
    depth[:, 38:, :] = 0.6 + 0.3 * rng.random((N, 10, W))
    raw = np.round(depth * 1000).astype(np.uint16)
    depth = raw / 1000.0
    raw[rng.random((N, H, W)) < 0.1] = 0
    pred = pred_of(rng, depth, 1.7, 0.02, 0.03)
    K = np.stack([np.array([[50.0, 0, 31.7], [0, 50.0, 23.6], [0, 0, 1]])] * N)
    poses = np.stack([pose(), pose(rot_y(0.5), (0.02, 0.01, -0.9)), pose(rot_y(-0.5), (0.0, 0.02, 0.5))])
    return pred, raw, K, poses, None, dict(crop=(0, H, 0, W), factor=1000.0, max_depth=10.0)


def case_c():
    """N=3, 3x301 (a tail in every row of blocks, 903 pixels), with masks: frame 1's is all zero, so the two directions that target
    frame 1 are tae_torch's second early return of 0; frames 0 and 2 have different partial masks."""
    rng = np.random.default_rng(32)
    N, H, W = 3, 3, 301
    depth = surface(rng, N, H, W, 1.0, 4.0, 0.02)
    gt = depth.astype(np.float32)
    gt[rng.random((N, H, W)) < 0.1] = 0
    pred = pred_of(rng, depth, 1.2, 0.1, 0.02)
    K = np.stack([np.array([[280.0, 0, 150.2], [0, 290.0, 1.1], [0, 0, 1]])] * N)
    poses = np.stack([pose(), pose(rot_y(0.3), (0.05, 0.0, 0.02)), pose(rot_y(0.8), (0.11, 0.001, 0.05))])
    mask = np.zeros((N, H, W), np.uint8)
    mask[0] = (rng.random((H, W)) < 0.7) * 255
    mask[2] = (rng.random((H, W)) < 0.4) * 255
    return pred, gt, K, poses, mask, dict(crop=(0, H, 0, W), factor=1.0, max_depth=10.0)


def case_d():
    pred, gt, K, poses = case_d_inputs()
    return pred, gt, K, poses, None, dict(crop=(0, CASE_D["H"], 0, CASE_D["W"]), factor=1.0, max_depth=CASE_D["max_depth"])


# ------------------------------------------------------------------ the reference, recorded
def run_reference(ev, pred, raw_gt, K, poses, mask, cfg):
    """eval_TAE on .npy files of the case. Returns (tae, (scale, shift) of its own lstsq, the recorded tae_torch calls)."""
    a, b, c, d = cfg["crop"]
    args = types.SimpleNamespace(a=a, b=b, c=c, d=d, max_depth_eval=cfg["max_depth"], mask=mask is not None, hard_crop=False)
    fits, calls = [], []
    real_lstsq, real_tae = np.linalg.lstsq, ev.tae_torch

    def lstsq(*p, **k):
        out = real_lstsq(*p, **k)
        fits.append(np.array(out[0], dtype=np.float64).ravel())
        return out

    def tae(depth1, depth2, R, T, Kc, m):
        out = real_tae(depth1, depth2, R, T, Kc, m)
        calls.append((depth1.clone(), depth2.clone(), R.clone(), T.clone(), np.array(Kc, dtype=np.float64), m.clone(), out))
        return out

    with tempfile.TemporaryDirectory() as tmp:
        ip, gp, mp = [], [], []
        for i in range(pred.shape[0]):
            for lst, stem, arr in ((ip, "inf", pred), (gp, "gt", raw_gt), (mp, "mask", mask)):
                if arr is not None:
                    lst.append(os.path.join(tmp, f"{stem}_{i:03d}.npy"))
                    np.save(lst[-1], arr[i])
        np.linalg.lstsq, ev.tae_torch = lstsq, tae
        try:
            res = ev.eval_TAE(ip, gp, [cfg["factor"]] * pred.shape[0], mp, list(K), list(poses), args)
        finally:
            np.linalg.lstsq, ev.tae_torch = real_lstsq, real_tae
    assert len(fits) == 1 and fits[0].size == 2 and len(calls) == 2 * (pred.shape[0] - 1)
    return float(res), fits[0], calls


def replay(depth1, depth2, R, T, Kc, m, mode="last"):
    """One tae_torch call again: torch's own operations up to the rounding (so the operands are the reference's, bit for bit), a
    sequential splat in `mode`, torch's mean. Returns (error as the reference returns it, count, stats dict)."""
    H, W = depth1.shape
    fx, fy, cx, cy = Kc[0, 0], Kc[1, 1], Kc[0, 2], Kc[1, 2]
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    xx, yy = xx.to(depth1.dtype), yy.to(depth1.dtype)
    X, Y = (xx - cx) * depth1 / fx, (yy - cy) * depth1 / fy
    p = torch.stack((X.flatten(), Y.flatten(), depth1.flatten()), dim=1)
    q = torch.matmul(p, R.T) + T.to(depth1.dtype)
    up, vp, qz = ((q[:, 0] * fx) / q[:, 2] + cx).numpy(), ((q[:, 1] * fy) / q[:, 2] + cy).numpy(), q[:, 2].numpy()
    u, v = np.rint(up).astype(np.int64), np.rint(vp).astype(np.int64)
    inside = (u >= 0) & (u < W) & (v >= 0) & (v < H)
    half = min(np.abs(up - np.floor(up) - 0.5).min(), np.abs(vp - np.floor(vp) - 0.5).min())
    stats = dict(half=half, mag=max(np.abs(up).max(), np.abs(vp).max()), qz=np.abs(qz).min(), landed=int(inside.sum()))
    proj = np.zeros(H * W)
    hits = np.zeros(H * W, dtype=np.int64)
    seen_pos = np.zeros(H * W, dtype=bool)                             # a source in front of the camera has landed here
    for s in np.nonzero(inside)[0]:                                  # row-major order of the SOURCE pixels
        t = v[s] * W + u[s]
        if mode == "last":
            proj[t] = qz[s]
        elif mode == "first":
            if hits[t] == 0:
                proj[t] = qz[s]
        elif mode == "nearest":                                      # a z-buffer: the smallest positive depth stays
            if qz[s] > 0 and (proj[t] <= 0 or qz[s] < proj[t]):
                proj[t] = qz[s]
        hits[t] += 1
        seen_pos[t] |= qz[s] > 0
    stats["hit_targets"], stats["multi_targets"] = int((hits > 0).sum()), int((hits > 1).sum())
    stats["neg_winner_over_pos"] = int(((proj < 0) & seen_pos).sum())  # (last-wins) the winner is behind the camera, a loser was visible
    if not inside.any():
        return 0, 0, stats
    projt = torch.from_numpy(proj.reshape(H, W))
    use = (projt > 0) & (depth2 > 0) & m
    n = int(use.sum())
    if n == 0:
        return 0, 0, stats
    return torch.mean(torch.abs(depth2[use] - projt[use]) / depth2[use]), n, stats


def bits(x):
    return np.float64(float(x)).tobytes()


def total(errors, npairs):
    s = 0.
    for e in errors:
        s += e
    return float(s / (2 * npairs) * 100)


def generate(ev):
    out = {"guards": np.array([HALF_GUARD, MAG_GUARD, QZ_GUARD, GT_GUARD])}
    for name, make in (("A", case_a), ("B", case_b), ("C", case_c), ("D", case_d)):
        pred, raw_gt, K, poses, mask, cfg = make()
        N = pred.shape[0]
        tae, ss, calls = run_reference(ev, pred, raw_gt, K, poses, mask, cfg)
        last = [replay(*c[:6]) for c in calls]
        for c, r in zip(calls, last):
            assert bits(c[6]) == bits(r[0]), f"case {name}: a sequential last-wins splat does not reproduce the reference ({float(c[6])!r} / {float(r[0])!r})"
        assert bits(total([r[0] for r in last], N - 1)) == bits(tae), f"case {name}: the replayed total differs from eval_TAE's"
        st = [r[2] for r in last]
        # guards
        a, b, c_, d = cfg["crop"]
        gt = (raw_gt / cfg["factor"])[:, a:b, c_:d]
        allg = gt.astype(np.float64).ravel()
        gt_margin = min(np.abs(allg / 1e-3 - 1).min(), np.abs(allg / cfg["max_depth"] - 1).min())
        valid = (gt > 1e-3) & (gt < cfg["max_depth"])
        x = np.clip(pred, 1e-3, None)[valid].astype(np.float64)
        det = x.size * (x * x).sum() - x.sum() ** 2
        depths = torch.stack([calls[0][0]] + [c[1] for c in calls[0::2]]).numpy()          # d[0], then d[i+1] of every forward call
        clipped = float(((depths == 1e-3) | (depths == cfg["max_depth"])).mean())
        margins = np.array([min(s["half"] for s in st), max(s["mag"] for s in st), min(s["qz"] for s in st), gt_margin, det, clipped])
        assert margins[0] > HALF_GUARD and margins[1] < MAG_GUARD and margins[2] > QZ_GUARD, f"case {name}: rounding guards {margins[:3]}: change the seed"
        assert margins[3] > GT_GUARD and x.size >= 2 and det != 0.0, f"case {name}: gt margin / degenerate fit"
        assert clipped < 0.25, f"case {name}: {clipped:.2f} of the aligned depths sit on a clip bound"
        errors = np.array([float(r[0]) for r in last]).reshape(N - 1, 2)
        counts = np.array([r[1] for r in last], dtype=np.int64).reshape(N - 1, 2)
        landed = np.array([s["landed"] for s in st]).reshape(N - 1, 2)
        variants = {}
        if name == "A":
            assert (landed[2] == 0).all() and (errors[2] == 0).all() and (landed[:2] > 0).all() and (counts[:2] > 0).all(), "case A: pair 2 must land nowhere"
            assert not np.array_equal(K[0], K[1])
            other = [replay(c[0], c[1], c[2], c[3], K[min(i // 2 + 1, N - 1)], c[5]) for i, c in enumerate(calls)]
            variants["k_next"] = total([r[0] for r in other], N - 1)
            assert abs(variants["k_next"] - tae) > 1e-6 * tae, "case A: reading K[i+1] must change the result"
        if name == "B":
            assert raw_gt.dtype == np.uint16
            multi = sum(s["multi_targets"] for s in st) / sum(s["hit_targets"] for s in st)
            assert multi >= 0.2, f"case B: only {multi:.2f} of the hit targets have two or more sources"
            for mode in ("first", "nearest"):
                variants[mode] = total([replay(*c[:6], mode=mode)[0] for c in calls], N - 1)
                assert abs(variants[mode] - tae) > 1e-6 * tae, f"case B: {mode}-wins must change the result"
            assert sum(s["neg_winner_over_pos"] for s in st) >= 1, "case B: no target whose winner is behind the camera over a visible loser"
            print(f"    collisions: {multi:.3f} of hit targets; negative winners over a visible loser: {sum(s['neg_winner_over_pos'] for s in st)}")
        if name == "C":
            assert (counts[0, 0] == 0) and (counts[1, 1] == 0) and landed[0, 0] > 0 and landed[1, 1] > 0, "case C: frame 1 as a target must be blanked"
            assert counts[0, 1] > 0 and counts[1, 0] > 0
            sw = [replay(c[0], c[1], c[2], c[3], c[4], calls[i ^ 1][5]) for i, c in enumerate(calls)]      # mask[i] <-> mask[i+1]
            variants["masks_swapped"] = total([r[0] for r in sw], N - 1)
            assert abs(variants["masks_swapped"] - tae) > 1e-6 * tae, "case C: swapping the two masks of a pair must change the result"
        out[f"{name}_tae"] = np.float64(tae)
        out[f"{name}_scale_shift"] = ss
        out[f"{name}_pair_errors"], out[f"{name}_pair_counts"], out[f"{name}_landed"] = errors, counts, landed
        out[f"{name}_margins"] = margins
        out[f"{name}_settings"] = np.array(list(cfg["crop"]) + [cfg["max_depth"], cfg["factor"]], dtype=np.float64)
        for k, v in variants.items():
            out[f"{name}_variant_{k}"] = np.float64(v)
        if name == "D":
            out["D_sha256"] = np.array(checksum(pred, raw_gt, K, poses))
        else:
            out[f"{name}_pred"], out[f"{name}_gt_raw"], out[f"{name}_K"], out[f"{name}_poses"] = pred, raw_gt, K, poses
            if mask is not None:
                out[f"{name}_mask"] = mask
        print(f"case {name}: tae={tae!r} scale={ss[0]!r} shift={ss[1]!r}")
        print(f"    errors {errors.ravel().tolist()}\n    counts {counts.ravel().tolist()} landed {landed.ravel().tolist()}")
        print(f"    margins: half-integer {margins[0]:.3e}, max |u|,|v| {margins[1]:.3e}, min |Qz| {margins[2]:.3e}, gt {margins[3]:.3e}, "
              f"det {margins[4]:.6e}, clipped {margins[5]:.4f}; variants {variants}")
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
