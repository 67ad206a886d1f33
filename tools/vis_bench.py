#!/usr/bin/env python
"""Time the depth visualisation (csrc/visualize.hip, video_depth_anything_amd/visualize.py) on blocks a user would map (a record for
DESIGN.md 6f, no threshold): default 32 x 720 x 1280 and 32 x 518 x 518, colour and gray. Per variant, one JSON line:

  kernel   device events around `--repeats` back-to-back calls of ops.depth_vis on a device-resident block after a warm-up; the bytes
           it must move, 4 read and 3 (colour) or 1 (gray) written per pixel, and the rate they give
  memcpy   the yardstick, measured in the same process and timed the same way: a device-to-device hipMemcpyAsync that moves the same
           7 or 5 bytes per pixel (half of them read, half written)
  colorize numpy array in, numpy array out (visualize.colorize): the host's min / max pass, upload, kernel, download; host clock, best of three
  numpy    the host twin visualize.colorize_numpy on the same block, host clock, one run
  poly     the mapping save_video makes by default (global min / max, float32 normalisation, the degree-6 polynomial
           utils.dc_utils._inferno, or the bare normalisation for gray), host clock, one run

Needs a GPU; no fallback."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from utils import dc_utils  # noqa: E402
from video_depth_anything_amd import ops  # noqa: E402
from video_depth_anything_amd.visualize import colorize, colorize_numpy, inferno_table  # noqa: E402


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


def polynomial_path(depth, grayscale):
    """save_video's default mapping of one block, as utils/dc_utils.py has it."""
    d_min, d_max = depth.min(), depth.max()
    span = max(float(d_max - d_min), 1e-12)
    norm = ((depth - d_min) / span * 255).astype(np.uint8)
    return norm if grayscale else dc_utils._inferno(norm)


def host_ms(fn, runs=1):
    best = float("inf")
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        best = min(best, 1e3 * (time.perf_counter() - t0))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, nargs="+", default=[32, 720, 1280, 32, 518, 518], help="triples n h w")
    ap.add_argument("--repeats", type=int, default=2000)
    ap.add_argument("--no-host", action="store_true", help="skip the host yardsticks (numpy, poly)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "vis_bench needs a GPU"
    assert len(args.shapes) % 3 == 0
    hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    DEVICE_TO_DEVICE = 3
    lut = torch.from_numpy(np.array(inferno_table())).cuda()
    for i in range(0, len(args.shapes), 3):
        n, h, w = args.shapes[i:i + 3]
        px = n * h * w
        depth_h = np.random.default_rng(0).uniform(0.3, 7.3, size=(n, h, w)).astype(np.float32)
        depth = torch.from_numpy(depth_h).cuda()
        minmax = torch.tensor([depth_h.min(), depth_h.max()], dtype=torch.float32, device="cuda")
        for grayscale in (False, True):
            ch = 1 if grayscale else 3
            out = torch.empty(px * ch, dtype=torch.uint8, device="cuda")
            ms = timed(lambda: ops.depth_vis(depth, minmax, None if grayscale else lut, out), args.repeats)
            want = colorize_numpy(depth_h[:1], depth_h.min(), depth_h.max(), grayscale)
            assert np.array_equal(out[:h * w * ch].cpu().numpy(), want.reshape(-1)), "the timed kernel's bytes are not the twin's"
            moved = px * (4 + ch)
            half = moved // 2
            src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

            def copy():
                rc = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), half, DEVICE_TO_DEVICE, stream)
                assert rc == 0, rc
            copy_ms = timed(copy, args.repeats)
            del src, dst, out
            row = {"shape": [n, h, w], "grayscale": grayscale, "pixels": px, "repeats": args.repeats,
                   "kernel_ms": ms, "bytes_moved": moved, "kernel_GBps": moved / ms / 1e6,
                   "memcpy_ms": copy_ms, "memcpy_bytes_moved": 2 * half, "memcpy_GBps": 2 * half / copy_ms / 1e6,
                   "kernel_fraction_of_memcpy_rate": (moved / ms) / (2 * half / copy_ms)}
            colorize(depth_h, grayscale=grayscale)                                     # warm-up: pinned staging buffers
            row["colorize_numpy_to_numpy_ms"] = host_ms(lambda: colorize(depth_h, grayscale=grayscale), runs=3)
            if not args.no_host:
                row["colorize_numpy_ms"] = host_ms(lambda: colorize_numpy(depth_h, grayscale=grayscale))
                row["polynomial_path_ms"] = host_ms(lambda: polynomial_path(depth_h, grayscale))
            print(json.dumps(row), flush=True)
        del depth


if __name__ == "__main__":
    main()
