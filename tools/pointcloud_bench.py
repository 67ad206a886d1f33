#!/usr/bin/env python
"""Time the point-cloud kernels (csrc/pointcloud.hip) on a device-resident block (a record for DESIGN.md 6e, no threshold): default
32 x 720 x 1280, both record types, keeping every pixel and with max_depth (about half the pixels kept). Per variant: device events
around `--repeats` back-to-back calls of ops.pointcloud (all of its launches) after a warm-up, the bytes the call must move computed
from the shapes and the counts, and the rate they give. Two yardsticks measured in the same process, neither assumed:

  memcpy   a device-to-device hipMemcpyAsync that moves the same number of bytes (half of them read, half written), timed the same way
  numpy    unproject_numpy on the host for the same block, host clock, one run

Bytes of a call: keeping every pixel, 4 (depth) + 3 (colour) read and one record written per pixel; with max_depth the count pass
reads the depth once more (4), the write pass reads every depth (4) and the colour of kept pixels (3) and writes their records. The
factor tables and tile counts (kilobytes) are left out. One JSON line per variant. Needs a GPU; no fallback."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_depth_anything_amd import ops  # noqa: E402
from video_depth_anything_amd.pointcloud import RECORD_SIZE, unproject_numpy  # noqa: E402

FX, FY = 470.4, 470.4


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
    ap.add_argument("--shape", type=int, nargs=3, default=[32, 720, 1280])
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--max-depth", type=float, default=10.0)
    ap.add_argument("--no-numpy", action="store_true", help="skip the host yardstick")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pointcloud_bench needs a GPU"
    n, h, w = args.shape
    px = n * h * w
    rng = np.random.default_rng(0)
    depth_h = rng.uniform(0.1, 20.0, size=(n, h, w)).astype(np.float32)          # about half of it within max_depth = 10
    rgb_h = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    depth, rgb = torch.from_numpy(depth_h).cuda(), torch.from_numpy(rgb_h).cuda()
    hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    DEVICE_TO_DEVICE = 3
    counts = torch.empty(n, dtype=torch.int32, device="cuda")
    workspace = torch.empty(ops.pointcloud_workspace_bytes(n, h, w), dtype=torch.uint8, device="cuda")
    for dtype in ("float64", "float32"):
        rs, f32 = RECORD_SIZE[dtype], dtype == "float32"
        records = torch.empty(n * ops.pointcloud_frame_stride(h, w, f32), dtype=torch.uint8, device="cuda")
        for max_depth in (None, args.max_depth):
            call = lambda: ops.pointcloud(depth, rgb, records, counts, workspace, FX, FY, w / 2.0, h / 2.0, max_depth, f32)
            ms = timed(call, args.repeats)
            kept = int(counts.sum())
            moved = px * (7 + rs) if max_depth is None else px * 8 + kept * (3 + rs)
            half = moved // 2
            src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

            def copy():
                rc = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), half, DEVICE_TO_DEVICE, stream)
                assert rc == 0, rc
            copy_ms = timed(copy, args.repeats)
            del src, dst
            row = {"shape": [n, h, w], "dtype": dtype, "max_depth": max_depth, "kept": kept, "pixels": px, "repeats": args.repeats,
                   "call_ms": ms, "bytes_moved": moved, "call_GBps": moved / ms / 1e6,
                   "memcpy_ms": copy_ms, "memcpy_bytes_moved": 2 * half, "memcpy_GBps": 2 * half / copy_ms / 1e6,
                   "call_over_memcpy": ms / copy_ms}
            if not args.no_numpy:
                t0 = time.perf_counter()
                unproject_numpy(depth_h, rgb_h, FX, FY, max_depth=max_depth, dtype=dtype)
                row["numpy_ms"] = 1e3 * (time.perf_counter() - t0)
                row["numpy_over_call"] = row["numpy_ms"] / ms
            print(json.dumps(row), flush=True)
        del records


if __name__ == "__main__":
    main()
