#!/usr/bin/env python
"""Time the Motion-JPEG decoder (csrc/mjpeg_decode.hip, video_depth_anything_amd/mjpeg.py) on a block run.py would hand it (a record
for DESIGN.md 6i, no threshold): default 32 x 518 x 518 frames of a synthetic depth scene mapped through the inferno table, quality
90. One JSON line per stream kind:

  444_rows        the project's own files: 4:4:4, one restart interval per MCU row (coded by csrc/mjpeg.hip)
  420_rows        PIL's encoder, 4:2:0, one restart interval per MCU row
  444_no_restart  PIL's encoder, 4:4:4, no restart markers: one interval per frame, so ONE LANE decodes a frame

and per line:

  call      device events around back-to-back calls of ops.mjpeg_decode (the interval table and the Huffman tables copied in, the
            coefficients zeroed, the three kernels: entropy, IDCT, colour) on device-resident scans after a warm-up, enough calls for a
            window of about a second; the per-kernel split is `rocprofv3 --kernel-trace --stats` of this tool with --no-host, a run
            of its own (profiles/mjpeg/decode_kernel_stats.csv)
  memcpy    the floor, measured in the same process and timed the same way: a device-to-device hipMemcpyAsync of the output's bytes
  bytes_to_numpy   list of JPEG bytes in, numpy array out (mjpeg.decode_jpeg): header parsing, the marker search, upload, kernels,
            download; host clock, best of three
  pil       PIL's libjpeg decoder on one core, frame by frame; host clock, best of three
  twin      mjpeg.decode_jpeg_numpy on the first --twin-frames frames (its entropy decoder is a Python loop), scaled to the block

The device's pixels are checked against PIL's on every frame unless --no-host. Needs a GPU; no fallback."""
import argparse
import ctypes
import io
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mjpeg_bench import host_ms, scene  # noqa: E402
from video_depth_anything_amd import mjpeg, ops  # noqa: E402
from video_depth_anything_amd.visualize import colorize_numpy  # noqa: E402


def timed_for(fn, seconds):
    """ms per call over enough back-to-back calls for a window of about `seconds`, after a warm-up call that also sizes it."""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    repeats = int(max(3, min(1000, seconds / max(time.perf_counter() - t0, 1e-6))))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeats):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / repeats, repeats


def pil_streams(frames, quality, subsampling, rows):
    from PIL import Image
    hs = 2 if subsampling else 1
    out = []
    for f in frames:
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, "JPEG", quality=quality, subsampling=subsampling, restart_marker_blocks=-(-f.shape[1] // (8 * hs)) if rows else 0)
        out.append(buf.getvalue())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[32, 518, 518], help="n h w")
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--seconds", type=float, default=1.0, help="length of each timed window")
    ap.add_argument("--twin-frames", type=int, default=1)
    ap.add_argument("--no-host", action="store_true", help="skip the host yardsticks (pil, twin) and the pixel check")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mjpeg_decode_bench needs a GPU"
    n, h, w = args.shape
    frames = colorize_numpy(scene(n, h, w))
    kinds = [("444_rows", mjpeg.encode_jpeg(frames, args.quality, device="cuda")),
             ("420_rows", pil_streams(frames, args.quality, 2, True)),
             ("444_no_restart", pil_streams(frames, args.quality, 0, False))]
    hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(out)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def copy():
        rc = hip.hipMemcpyAsync(dst.data_ptr(), out.data_ptr(), out.numel(), 3, stream)       # 3 = device to device
        assert rc == 0, rc
    for name, jpegs in kinds:
        info = mjpeg.parse_jpeg(jpegs[0])
        assert all(j.startswith(info.header) for j in jpegs)
        scan, iv, host_status = mjpeg.device_call_inputs(jpegs, info)
        scan_d = torch.from_numpy(scan.copy()).cuda()
        tables = mjpeg.decode_tables(info)
        work = torch.empty(ops.mjpeg_decode_workspace_bytes(n, h, w, 3, info.hs, info.vs, iv.shape[0]), dtype=torch.uint8, device="cuda")
        st = torch.empty(n, dtype=torch.int32, device="cuda")
        ms, repeats = timed_for(lambda: ops.mjpeg_decode(scan_d, iv, tables, info.qtables, info.hs, info.vs, work, out, st), args.seconds)
        assert not st.any() and not host_status.any()
        copy_ms, _ = timed_for(copy, args.seconds / 4)
        row = {"kind": name, "shape": [n, h, w, 3], "quality": args.quality, "sampling": [info.hs, info.vs], "intervals": int(iv.shape[0]),
               "jpeg_bytes": sum(map(len, jpegs)), "output_bytes": out.numel(), "repeats": repeats, "call_ms": ms, "frames_per_s": n / ms * 1e3,
               "output_GBps": out.numel() / ms / 1e6, "memcpy_ms": copy_ms, "call_over_memcpy": ms / copy_ms, "workspace_bytes": work.numel()}
        got = []
        mjpeg.decode_jpeg(jpegs, device="cuda")
        row["bytes_to_numpy_ms"] = host_ms(lambda: got.append(mjpeg.decode_jpeg(jpegs, device="cuda")), runs=3)
        assert np.array_equal(got[-1], out.cpu().numpy())
        if not args.no_host:
            theirs = []
            row["pil_ms"] = host_ms(lambda: theirs.append(mjpeg.decode_jpegs(jpegs)), runs=3)
            assert np.array_equal(got[-1], theirs[-1]), "the device's pixels are not PIL's"
            row["pil_over_bytes_to_numpy"] = row["pil_ms"] / row["bytes_to_numpy_ms"]
            k = min(args.twin_frames, n)
            twin = []
            row["twin_ms"] = host_ms(lambda: twin.append(mjpeg.decode_jpeg_numpy(jpegs[:k]))) * n / k
            assert np.array_equal(twin[-1], got[-1][:k]), "the device's pixels are not the twin's"
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
