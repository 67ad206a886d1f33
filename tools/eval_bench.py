#!/usr/bin/env python
"""Time evaluate_depth on a device-resident video against evaluate_depth_numpy on the same host (a record for DESIGN.md, no
threshold): default 110 x 480 x 640, Bonn's scene size. Device time = host clock around calls that end in the result's
device-to-host copy (a synchronise), after warm-up; median and spread of the repeats. `--resize h w` also times the resize of a
synthetic N x h x w prediction to the scene's H x W (vda_resize_linear_f32): device events around 20 back-to-back launches after
a warm-up, ms per launch and GB/s against the 4 (N H W) + 4 (N h w) bytes it must move. Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_depth_anything_amd.evaluate import evaluate_depth, evaluate_depth_numpy  # noqa: E402

RESIZE_LAUNCHES = 20


def time_resize(N, h, w, H, W):
    """One JSON-ready dict: the resize of a device-resident [N,h,w] to [N,H,W], timed with device events."""
    from video_depth_anything_amd import ops
    x = torch.rand(N, h, w, generator=torch.Generator().manual_seed(1)).mul_(19.9).add_(0.1).cuda()
    out = torch.empty(N, H, W, dtype=torch.float32, device="cuda")
    for _ in range(3):
        ops.resize_linear(x, out)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(RESIZE_LAUNCHES):
        ops.resize_linear(x, out)
    stop.record()
    stop.synchronize()
    ms = start.elapsed_time(stop) / RESIZE_LAUNCHES
    nbytes = 4 * N * H * W + 4 * N * h * w
    return {"resize": [N, h, w, H, W], "resize_launches": RESIZE_LAUNCHES, "resize_ms": ms, "resize_bytes": nbytes, "resize_GBps": nbytes / ms * 1e-6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[110, 480, 640])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--numpy_repeats", type=int, default=2)
    ap.add_argument("--resize", type=int, nargs=2, metavar=("h", "w"), help="also time the resize of an N x h x w prediction to the scene's size")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "eval_bench needs a GPU"
    N, H, W = args.shape
    if args.resize:
        print(json.dumps(time_resize(N, args.resize[0], args.resize[1], H, W)))
    g = torch.Generator().manual_seed(0)
    gt = torch.rand(N, H, W, generator=g) * 11.0 + 0.3
    gt[torch.rand(N, H, W, generator=g) < 0.15] = 0
    pred = 2.5 / gt.clamp_min(0.1) + 0.4 + 0.1 * torch.randn(N, H, W, generator=g)
    dp, dg = pred.cuda(), gt.cuda()
    for _ in range(3):
        dev = evaluate_depth(dp, dg, 10.0)
    times = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        evaluate_depth(dp, dg, 10.0)
        times.append(time.perf_counter() - t0)
    host_times = []
    for _ in range(args.numpy_repeats):
        t0 = time.perf_counter()
        host = evaluate_depth_numpy(pred.numpy(), gt.numpy(), 10.0)
        host_times.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    evaluate_depth(pred.numpy(), gt.numpy(), 10.0)
    from_host = time.perf_counter() - t0
    rel = max(abs(dev[k] - host[k]) / abs(host[k]) for k in ("scale", "shift", "abs_relative_difference", "squared_relative_difference", "rmse_linear"))
    print(json.dumps({"shape": [N, H, W], "bytes_read_per_pass": 8 * N * H * W,
                      "device_ms_median": 1e3 * float(np.median(times)), "device_ms_min": 1e3 * min(times), "device_ms_max": 1e3 * max(times),
                      "device_from_host_arrays_ms": 1e3 * from_host, "numpy_ms": [1e3 * t for t in host_times],
                      "max_rel_diff_device_vs_numpy": rel, "n_valid": dev["n_valid"] == host["n_valid"] and dev["n_valid"]}))


if __name__ == "__main__":
    main()
