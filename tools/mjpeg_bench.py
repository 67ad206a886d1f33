#!/usr/bin/env python
"""Time the Motion-JPEG encoder (csrc/mjpeg.hip, video_depth_anything_amd/mjpeg.py) on a block save_video would hand it (a record for
DESIGN.md 6h, no threshold): default 32 x 518 x 518 x 3 frames of a synthetic depth scene mapped through the inferno table, quality
90. One JSON line:

  encode    device events around `--repeats` back-to-back calls of ops.mjpeg_encode (its three kernels: transform, entropy, pack) on a
            device-resident block after a warm-up; the per-kernel split is `rocprofv3 --kernel-trace --stats` of this tool with
            --no-host, a run of its own (profiles/mjpeg/kernel_stats.csv)
  memcpy    the yardstick, measured in the same process and timed the same way: a device-to-device hipMemcpyAsync of the input's bytes
  numpy_to_jpegs   numpy array in, list of JPEG bytes out (mjpeg.encode_jpeg): upload, kernels, download of the compressed bytes and
            the split into frames; host clock, best of three
  pil       PIL's libjpeg encoder on the host, frame by frame, the same tables, 4:4:4; host clock, one run
  twin      mjpeg.encode_jpeg_numpy on the same block; host clock, one run
  sizes     the block as raw bytes, as this encoder's JPEGs (the device's bytes are checked against the twin's on the first frame, and
            on all of them unless --no-host), as PIL's JPEGs, and as the animated GIF save_video falls back to

Needs a GPU; no fallback."""
import argparse
import ctypes
import io
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_depth_anything_amd import mjpeg, ops  # noqa: E402
from video_depth_anything_amd.visualize import colorize_numpy  # noqa: E402


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


def host_ms(fn, runs=1):
    best = float("inf")
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        best = min(best, 1e3 * (time.perf_counter() - t0))
    return best


def scene(n, h, w):
    """float32 [n,h,w]: a floor receding to a horizon, two moving round objects and fine texture - smooth regions, edges and detail."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    rng = np.random.default_rng(0)
    tex = rng.normal(0, 0.02, (h, w)).astype(np.float32)
    out = np.empty((n, h, w), np.float32)
    for i in range(n):
        d = 1.0 + 6.0 * (1.0 - y / h) ** 2 + 0.3 * np.sin(x / 37.0 + 0.1 * i) + tex
        for cx, cy, r, z in ((0.3 * w + 4 * i, 0.6 * h, 0.12 * w, 1.2), (0.7 * w - 3 * i, 0.45 * h, 0.08 * w, 2.0)):
            m = (x - cx) ** 2 + (y - cy) ** 2 < r * r
            d[m] = z + 0.2 * ((x[m] - cx) / r) ** 2
        out[i] = d
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[32, 518, 518], help="n h w")
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--no-host", action="store_true", help="skip the host yardsticks (pil, twin, gif)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mjpeg_bench needs a GPU"
    n, h, w = args.shape
    q = args.quality
    frames_h = colorize_numpy(scene(n, h, w))
    frames = torch.from_numpy(frames_h).cuda()
    qt = np.ascontiguousarray(mjpeg.quant_tables(q), dtype=np.uint16)
    work = torch.empty(ops.mjpeg_workspace_bytes(n, h, w, 3), dtype=torch.uint8, device="cuda")
    out = torch.empty(ops.mjpeg_out_bytes(n, h, w, 3), dtype=torch.uint8, device="cuda")
    lengths = torch.empty(n, dtype=torch.int64, device="cuda")
    ms = timed(lambda: ops.mjpeg_encode(frames, qt, work, out, lengths), args.repeats)
    head = mjpeg.jpeg_header(h, w, 3, q)
    ours = mjpeg.split_payload(head, out, lengths)
    assert ours[:1] == mjpeg.encode_jpeg_numpy(frames_h[:1], q), "the timed kernels' bytes are not the twin's"

    hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    DEVICE_TO_DEVICE = 3
    nbytes = frames.numel()
    dst = torch.empty_like(frames)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def copy():
        rc = hip.hipMemcpyAsync(dst.data_ptr(), frames.data_ptr(), nbytes, DEVICE_TO_DEVICE, stream)
        assert rc == 0, rc
    copy_ms = timed(copy, args.repeats)
    row = {"shape": [n, h, w, 3], "quality": q, "repeats": args.repeats, "input_bytes": nbytes,
           "encode_ms": ms, "encode_input_GBps": nbytes / ms / 1e6, "encode_frames_per_s": n / ms * 1e3,
           "memcpy_ms": copy_ms, "memcpy_GBps": 2 * nbytes / copy_ms / 1e6, "encode_over_memcpy": ms / copy_ms,
           "workspace_bytes": work.numel(), "out_capacity_bytes": out.numel(),
           "jpeg_bytes": sum(map(len, ours)), "jpeg_bytes_per_frame": sum(map(len, ours)) / n}
    mjpeg.encode_jpeg(frames_h, q)                                             # warm-up: pinned staging buffers
    row["numpy_to_jpegs_ms"] = host_ms(lambda: mjpeg.encode_jpeg(frames_h, q), runs=3)
    if not args.no_host:
        from PIL import Image
        tabs = [t.tolist() for t in mjpeg.quant_tables(q)]
        theirs = []

        def pil():
            theirs.clear()
            for f in frames_h:
                buf = io.BytesIO()
                Image.fromarray(f).save(buf, "JPEG", qtables=tabs, subsampling=0)
                theirs.append(buf.getvalue())
        row["pil_ms"] = host_ms(pil)
        row["pil_jpeg_bytes"] = sum(map(len, theirs))
        twin = []
        row["twin_ms"] = host_ms(lambda: twin.extend(mjpeg.encode_jpeg_numpy(frames_h, q)))
        assert twin == ours, "the device's bytes are not the twin's"
        dec = lambda js: mjpeg.decode_jpegs(js).astype(np.float64)
        psnr = lambda a: 10 * np.log10(255.0 ** 2 / np.mean((a - frames_h) ** 2))
        row["psnr_db"], row["pil_psnr_db"] = psnr(dec(ours)), psnr(dec(theirs))
        buf = io.BytesIO()
        ims = [Image.fromarray(f) for f in frames_h]
        t0 = time.perf_counter()
        ims[0].save(buf, "GIF", save_all=True, append_images=ims[1:], duration=42, loop=0)
        row["gif_ms"], row["gif_bytes"] = 1e3 * (time.perf_counter() - t0), len(buf.getvalue())
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
