#!/usr/bin/env python
"""Time the TAE scorer's passes on a device-resident scene (a record for DESIGN.md, no threshold): default 180 x 464 x 618, one
scannet scene after the crop. Synthetic inputs: a slanted surface, a camera that drifts a few centimetres per frame. Per pass:
device events around `--repeats` back-to-back launches after a warm-up, the bytes the pass must move computed from the shapes, and
the rate they give; then evaluate_tae end to end (host clock around calls that end in the result copy). Needs a GPU; no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_depth_anything_amd import evaluate as E  # noqa: E402
from video_depth_anything_amd import ops  # noqa: E402


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeats):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / repeats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[180, 464, 618])
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tae_bench needs a GPU"
    N, H, W = args.shape
    P, px = N - 1, H * W
    g = torch.Generator().manual_seed(0)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32) / H, torch.arange(W, dtype=torch.float32) / W, indexing="ij")
    depth = (2.0 + x + 0.5 * y)[None] * (0.95 + 0.1 * torch.rand(N, H, W, generator=g))
    gt = depth.clone()
    gt[torch.rand(N, H, W, generator=g) < 0.1] = 0
    pred = (1.4 / depth + 0.1) * (0.98 + 0.04 * torch.rand(N, H, W, generator=g))
    K = np.array([[577.0, 0, W / 2 - 0.3], [0, 577.0, H / 2 + 0.2], [0, 0, 1]])
    poses = np.stack([np.eye(4)] * N)
    for i in range(N):
        s = 0.002 * i
        poses[i, :3, :3] = [[1 - s * s / 2, 0, s], [0, 1, 0], [-s, 0, 1 - s * s / 2]]
        poses[i, :3, 3] = [0.01 * i, -0.002 * i, 0.015 * i]
    dp, dg = pred.cuda(), gt.cuda()
    for _ in range(2):
        res = E.evaluate_tae(dp, dg, K, poses, 10.0)
    end_to_end = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        E.evaluate_tae(dp, dg, K, poses, 10.0)
        end_to_end.append(1e3 * (time.perf_counter() - t0))

    # the passes on their own, all pairs at once, on the state evaluate_tae builds
    dev = dp.device
    cam = torch.from_numpy(E._tae_cameras(np.broadcast_to(K, (N, 3, 3)), poses)).to(dev)
    fit = torch.tensor([res["scale"], res["shift"], float(res["n_valid"])], dtype=torch.float64, device=dev)
    bpp = min(E.TAE_MAX_BLOCKS, -(-px // E.TAE_PX_PER_BLOCK))
    winner = torch.empty((2 * P, H, W), dtype=torch.int32, device=dev)
    work = torch.empty(4 * P * bpp, dtype=torch.float64, device=dev)
    out = torch.empty(1 + 4 * P, dtype=torch.float64, device=dev)
    t_clear = timed(lambda: winner.zero_(), args.repeats)
    t_splat = timed(lambda: ops.tae_splat(dp, 10.0, fit, cam, winner), args.repeats)            # includes its clear
    t_compare = timed(lambda: ops.tae_compare(dp, None, 10.0, fit, cam, winner, work, 0, bpp), args.repeats)
    t_finish = timed(lambda: ops.tae_finish(work, P, bpp, out), args.repeats)
    landed = int((winner != 0).sum())
    planes = 2 * P * px
    # splat: clear the planes (4 B written per target), read every source once (4 B), one 4-byte atomic per source that lands (an
    # upper bound: every source). compare: winner plane (4 B) + target pred (4 B) per target, + 4 B gathered per hit target.
    b_splat = planes * (4 + 4 + 4)
    b_compare = planes * 8 + landed * 4
    print(json.dumps({"shape": [N, H, W], "pairs": P, "blocks_per_plane": bpp, "tae": res["tae"], "hit_targets": landed, "targets": planes,
                      "end_to_end_ms": end_to_end, "fit_ms_note": "end_to_end includes the fit's two launches per 8 frames",
                      "clear_ms": t_clear, "splat_ms_with_clear": t_splat, "compare_ms": t_compare, "finish_ms": t_finish,
                      "splat_bytes": b_splat, "compare_bytes": b_compare,
                      "splat_GBps": b_splat / t_splat / 1e6, "compare_GBps": b_compare / t_compare / 1e6}))


if __name__ == "__main__":
    main()
