#!/usr/bin/env python
"""Time the validation losses (csrc/losses.hip, video_depth_anything_amd/losses.py) on one validation batch, device-resident:
1 x 32 x 518 x 518 by default, ~70 % mask. A record for DESIGN.md 6g, no threshold. One JSON line:

  lsq / mad   validation_loss(variant=...) end to end on device tensors (ssi + tgm, launches, the one device-to-host copy), host
              clock around each of `--runs` calls after a warm-up: median / min / max in ms
  memcpy      the yardstick, in the same process: a device-to-device hipMemcpyAsync of the bytes one pass over the batch reads
              (pred + y + mask = 9 bytes per pixel), device events around `--runs` back-to-back copies
  numpy       the host twin validation_loss_numpy on the same batch, host clock, one run per variant (skipped with --no-host)

Needs a GPU; no fallback."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_depth_anything_amd.losses import validation_loss, validation_loss_numpy  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=4, default=[1, 32, 518, 518], help="B N H W")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy twin")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "loss_bench needs a GPU"
    B, N, H, W = args.shape
    rng = np.random.default_rng(0)
    y_h = rng.uniform(0.5, 3.5, (B, 1, H, W)).astype(np.float32) + np.cumsum(rng.uniform(-0.1, 0.1, (B, N, H, W)), axis=1).astype(np.float32)
    pred_h = ((y_h - 0.3) * 0.6 + 0.05 * rng.standard_normal(y_h.shape)).astype(np.float32)
    mask_h = (rng.random(y_h.shape) < 0.7).astype(np.uint8)
    pred, y, mask = (torch.from_numpy(a).cuda() for a in (pred_h, y_h, mask_h))
    row = {"shape": [B, N, H, W], "runs": args.runs, "device": torch.cuda.get_device_name(0)}
    for variant in ("lsq", "mad"):
        got = validation_loss(pred, y, mask, variant=variant)                     # warm-up
        ms = []
        for _ in range(args.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            validation_loss(pred, y, mask, variant=variant)
            ms.append(1e3 * (time.perf_counter() - t0))
        row[f"{variant}_ms"] = {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}
        row[f"{variant}_loss"] = got["loss"]
        if not args.no_host:
            t0 = time.perf_counter()
            want = validation_loss_numpy(pred_h, y_h, mask_h, variant=variant)
            row[f"{variant}_numpy_ms"] = 1e3 * (time.perf_counter() - t0)
            assert abs(got["loss"] - want["loss"]) <= 1e-12 * abs(want["loss"]), "the timed result is not the twin's"
    nbytes = pred_h.nbytes + y_h.nbytes + mask_h.nbytes
    hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def copy():
        rc = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, stream)     # 3 = device to device
        assert rc == 0, rc

    copy()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.runs):
        copy()
    b.record()
    torch.cuda.synchronize()
    row["memcpy_bytes"] = nbytes
    row["memcpy_ms"] = a.elapsed_time(b) / args.runs
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
