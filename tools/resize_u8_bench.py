#!/usr/bin/env python
"""Time the 8-bit resize (csrc/resize_u8.hip, video_depth_anything_amd/scale.py) at the size it is for (a record for DESIGN.md 6j,
no threshold): default 32 frames of 1080 x 1920 x 3 -> 720 x 1280. One JSON line per mode:

  (default)       kernel   device events around `--repeats` back-to-back launches of ops.resize_linear_u8 on a device-resident block
                           after a warm-up; the bytes it must move (every source byte read once, every output byte written) and their rate
                  memcpy   the yardstick of profiles/visualize and profiles/pointcloud, measured in the same process and timed the same
                           way: a device-to-device hipMemcpyAsync that moves the same total (half of it read, half written)
                  staged   numpy array in, numpy array out (scale.resize_frames): upload, kernel, download; host clock, best of three
                  twin     scale.resize_frames_numpy on the host, one run; bilinear = utils.dc_utils._resize_bilinear (what scales
                           frames without a device), one run; and how many bytes of the two differ
  --write-avi P   writes the end-to-end input: `--frames` (64) frames of 1080 x 1920 as a Motion-JPEG .avi, coded on the device
  --read P        read_video_frames(P, -1, -1, 1280, device="cuda"): host clock, best of three after a warm-up, and a checksum
  --stream-rss P  run.py --stream --mjpeg on P (ViT-S, synthetic weights) as a child process; its peak resident set and wall time

`--repo DIR` makes --read and --stream-rss use another checkout's utils/ and run.py (the parent commit's, for the before / after
pair) with this checkout's library. Needs a GPU; no fallback."""
import argparse
import ctypes
import json
import os
import resource
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(HERE, "video_depth_anything_amd", "libvda_hip.so")     # --repo runs another checkout's Python over this library


def timed(fn, repeats):
    import torch
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


def video(n, h, w):
    """uint8 [n,h,w,3]: the false-colour scene of tools/mjpeg_bench.py (smooth regions, edges, fine texture, motion)."""
    sys.path.insert(0, os.path.join(HERE, "tools"))
    from mjpeg_bench import scene
    from video_depth_anything_amd.visualize import colorize_numpy
    return colorize_numpy(scene(n, h, w))


def checkout(args):
    return "this" if args.repo == HERE else os.path.basename(os.path.normpath(args.repo))


def kernel_mode(args):
    import torch
    from utils.dc_utils import _resize_bilinear
    from video_depth_anything_amd import ops
    from video_depth_anything_amd.scale import resize_frames, resize_frames_numpy
    n, h, w, H, W = args.shape
    frames_h = np.random.default_rng(0).integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    frames_h[: min(n, 4)] = video(min(n, 4), h, w)
    frames = torch.from_numpy(frames_h).cuda()
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
    ms = timed(lambda: ops.resize_linear_u8(frames, out), args.repeats)
    want = resize_frames_numpy(frames_h[:1], H, W)
    assert np.array_equal(out[:1].cpu().numpy(), want), "the timed kernel's bytes are not the twin's"
    moved = frames.numel() + out.numel()
    half = moved // 2
    hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def copy():
        rc = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), half, 3, stream)           # 3 = device to device
        assert rc == 0, rc
    copy_ms = timed(copy, args.repeats)
    del src, dst
    row = {"shape": [n, h, w, 3], "to": [H, W], "repeats": args.repeats, "kernel_ms": ms, "bytes_moved": moved, "kernel_GBps": moved / ms / 1e6,
           "memcpy_ms": copy_ms, "memcpy_bytes_moved": 2 * half, "memcpy_GBps": 2 * half / copy_ms / 1e6,
           "kernel_fraction_of_memcpy_rate": (moved / ms) / (2 * half / copy_ms)}
    resize_frames(frames_h, H, W)                                                          # warm-up: pinned staging buffers
    row["staged_numpy_to_numpy_ms"] = host_ms(lambda: resize_frames(frames_h, H, W), runs=3)
    if not args.no_host:
        few = frames_h[:4]
        twin, bil = [], []
        row["twin_ms_per_frame"] = host_ms(lambda: twin.append(resize_frames_numpy(few, H, W))) / len(few)
        row["resize_bilinear_ms_per_frame"] = host_ms(lambda: bil.append(_resize_bilinear(few, H, W))) / len(few)
        d = np.abs(twin[0].astype(np.int16) - bil[0].astype(np.int16))
        row["twin_vs_resize_bilinear"] = {"bytes_that_differ": float((d != 0).mean()), "worst": int(d.max())}
    print(json.dumps(row), flush=True)


def write_avi_mode(args):
    from video_depth_anything_amd import mjpeg
    n, h, w = args.frames, args.shape[1], args.shape[2]
    few = video(8, h, w)

    def jpegs():
        for i in range(0, n, 8):
            yield from mjpeg.encode_jpeg(np.roll(few, 16 * i, axis=2)[: n - i], 90, "cuda")
    mjpeg.write_avi(args.write_avi, jpegs(), 24.0, w, h)
    print(json.dumps({"wrote": os.path.basename(args.write_avi), "frames": n, "size": [h, w], "bytes": os.path.getsize(args.write_avi)}), flush=True)


def read_mode(args):
    import torch
    sys.path.insert(0, args.repo)
    os.environ.setdefault("VDA_LIB_PATH", LIB)
    from utils.dc_utils import read_video_frames
    got = []

    def read():
        got[:] = [read_video_frames(args.read, -1, -1, args.max_res, device="cuda")[0]]
        torch.cuda.synchronize()
    read()
    ms = host_ms(read, runs=3)
    print(json.dumps({"checkout": checkout(args), "read_video_frames_ms": ms, "frames": list(got[0].shape), "max_res": args.max_res,
                      "crc32": zlib.crc32(got[0].tobytes())}), flush=True)


def stream_rss_mode(args):
    out = os.path.join(args.scratch, "out_" + os.path.basename(os.path.normpath(args.repo)))
    env = dict(os.environ, PYTHONPATH=args.repo, VDA_LIB_PATH=os.environ.get("VDA_LIB_PATH", LIB))
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(args.repo, "run.py"), "--input_video", args.stream_rss, "--output_dir", out, "--encoder", "vits",
                        "--checkpoint", "synthetic", "--stream", "--mjpeg", "--max_res", str(args.max_res)], env=env, capture_output=True, text=True)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    print(json.dumps({"checkout": checkout(args), "run_py_stream_peak_rss_MB": resource.getrusage(resource.RUSAGE_CHILDREN).ru_maxrss / 1024,
                      "wall_s": wall, "frames": int(r.stdout.strip().splitlines()[-1].split()[0])}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=5, default=[32, 1080, 1920, 720, 1280], help="n h w H W")
    ap.add_argument("--repeats", type=int, default=500)
    ap.add_argument("--no-host", action="store_true", help="skip the host yardsticks (twin, bilinear)")
    ap.add_argument("--write-avi", type=str, default=None)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--read", type=str, default=None)
    ap.add_argument("--stream-rss", type=str, default=None)
    ap.add_argument("--max_res", type=int, default=1280)
    ap.add_argument("--repo", type=str, default=HERE)
    ap.add_argument("--scratch", type=str, default=tempfile.gettempdir(), help="where --stream-rss lets run.py write")
    args = ap.parse_args()
    args.repo = os.path.abspath(args.repo)
    if args.stream_rss:
        return stream_rss_mode(args)
    if not args.read:
        sys.path.insert(0, HERE)
    import torch
    assert torch.cuda.is_available(), "resize_u8_bench needs a GPU"
    if args.write_avi:
        write_avi_mode(args)
    elif args.read:
        read_mode(args)
    else:
        kernel_mode(args)


if __name__ == "__main__":
    main()
