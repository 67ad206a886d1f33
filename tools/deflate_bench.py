#!/usr/bin/env python
"""Time the deflate encoder (csrc/deflate.hip, video_depth_anything_amd/deflate.py) on what run.py --save_npz hands it (a record for
DESIGN.md 6k, no threshold): 32 x 518 x 518 float32 depth, as a synthetic field (smooth, a little noise, some zeros) and - with
--model - as the depth the synthetic-checkpoint ViT-S forward gives for a generated clip. One JSON line per input, printed and
appended to <out-dir>/deflate_bench.txt:

  kernels   device events around `--repeats` back-to-back calls of ops.deflate (its four launches: encode, crc, offsets, pack) on a
            device-resident array after a warm-up, the median of `--windows` such windows; the per-kernel split is
            `rocprofv3 --kernel-trace --stats` of this tool with --no-host, a run of its own (profiles/deflate/kernel_stats.csv)
  memcpy    the yardstick, measured in the same process and timed the same way: a device-to-device hipMemcpyAsync of the input's bytes
  numpy_to_bytes   deflate.deflate(numpy array): pinned staging, upload, kernels, download of the stream; host clock, median of five
  savez     deflate.savez_compressed(path, device="cuda", depths=array) beside np.savez_compressed(path, depths=array) - what the
            parent commit's run.py called - on the same host, both to the same directory; host clock, median of three each
  sizes     the stream beside zlib's raw deflate at level 6, Z_RLE and Z_HUFFMAN_ONLY, and the fixed header's share of it; the
            device's bytes are inflated by zlib and compared with the input, and compared with the twin's on the first 4 chunks

Needs a GPU; no fallback."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_depth_anything_amd import deflate, ops  # noqa: E402


def window_ms(fn, repeats):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeats):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / repeats


def timed(fn, repeats, windows):
    fn()
    torch.cuda.synchronize()
    return statistics.median(window_ms(fn, repeats) for _ in range(windows))


def host_ms(fn, runs):
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(out)


def synthetic_field(n, h, w):
    """float32 [n,h,w]: a smooth depth field that drifts from frame to frame, a little noise, and a region of exact zeros (sky)."""
    rng = np.random.default_rng(0)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    out = np.empty((n, h, w), np.float32)
    for i in range(n):
        d = 1.0 + 6.0 * (1.0 - y / h) ** 2 + 0.3 * np.sin(x / 37.0 + 0.1 * i) + rng.normal(0, 0.002, (h, w)).astype(np.float32)
        d[: h // 6, w // 3: w // 3 + w // 4 + i] = 0
        out[i] = d
    return out


def model_depth(n, h, w):
    """The synthetic-checkpoint ViT-S forward's depth for a generated clip of moving gradients and texture."""
    from video_depth_anything_amd.config import get_config
    from video_depth_anything_amd.video_depth import VideoDepthAnything
    from video_depth_anything_amd.weights import synthetic_state_dict
    cfg = get_config("vits")
    m = VideoDepthAnything(encoder="vits", features=cfg.features, out_channels=list(cfg.out_channels))
    m.load_state_dict(synthetic_state_dict(cfg, seed=0), strict=True)
    m = m.to("cuda").eval()
    rng = np.random.default_rng(1)
    y, x = np.mgrid[0:h, 0:w]
    tex = rng.integers(0, 40, (h, w, 3))
    frames = np.stack([np.clip(np.stack([(x + 5 * i) % 256, (y + 3 * i) % 256, (x + y) // 4 % 256], -1) // 2 + tex, 0, 255) for i in range(n)]).astype(np.uint8)
    depths, _ = m.infer_video_depth(frames, 24, input_size=518, device="cuda")
    return np.ascontiguousarray(depths[:n], dtype=np.float32)


def zlib_raw(data, strategy):
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, strategy)
    return len(c.compress(data)) + len(c.flush())


def measure(name, arr, args, hip):
    x = torch.from_numpy(arr).cuda().reshape(-1).view(torch.uint8)
    nbytes = x.numel()
    work = torch.empty(ops.deflate_workspace_bytes(nbytes), dtype=torch.uint8, device="cuda")
    out = torch.empty(ops.deflate_out_bytes(nbytes), dtype=torch.uint8, device="cuda")
    length = torch.empty(1, dtype=torch.int64, device="cuda")
    crcs = torch.empty(deflate.n_chunks(nbytes), dtype=torch.int32, device="cuda")
    ms = timed(lambda: ops.deflate(x, True, work, out, length, crcs), args.repeats, args.windows)
    stream = out[:int(length.item())].cpu().numpy().tobytes()
    raw = arr.tobytes()
    assert zlib.decompress(stream, -15) == raw, "zlib does not inflate the device's stream to the input"
    head = 4 * deflate.CHUNK
    assert stream.startswith(deflate.deflate_numpy(raw[:head], final=False)), "the timed kernels' bytes are not the twin's"
    dst = torch.empty_like(x)
    cur = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def copy():
        rc = hip.hipMemcpyAsync(dst.data_ptr(), x.data_ptr(), nbytes, 3, cur)      # 3: device to device
        assert rc == 0, rc
    copy_ms = timed(copy, args.repeats, args.windows)
    info = []
    deflate.deflate_numpy(raw[:64 * deflate.CHUNK], info=info)
    coded = [d for d in info if not d.get("stored", True)]
    row = {"input": name, "shape": list(arr.shape), "input_bytes": nbytes, "chunks": deflate.n_chunks(nbytes), "repeats": args.repeats, "windows": args.windows,
           "kernels_ms": ms, "kernels_input_GBps": nbytes / ms / 1e6, "memcpy_ms": copy_ms, "memcpy_GBps": 2 * nbytes / copy_ms / 1e6,
           "kernels_over_memcpy": ms / copy_ms, "workspace_bytes": work.numel(), "stream_bytes": len(stream), "ratio": len(stream) / nbytes,
           "header_bytes_per_coded_chunk_first_64": (sum(d["header_bits"] for d in coded) / 8 / len(coded)) if coded else None}
    deflate.deflate(arr)                                                           # warm-up: pinned staging buffers
    row["numpy_to_bytes_ms"] = host_ms(lambda: deflate.deflate(arr), 5)
    row["numpy_to_bytes_input_MBps"] = nbytes / row["numpy_to_bytes_ms"] / 1e3
    with tempfile.TemporaryDirectory(dir=args.tmp) as d:
        ours, theirs = os.path.join(d, "ours.npz"), os.path.join(d, "numpy.npz")
        deflate.savez_compressed(ours, device="cuda", depths=arr)
        row["savez_device_ms"] = host_ms(lambda: deflate.savez_compressed(ours, device="cuda", depths=arr), 3)
        row["npz_device_bytes"] = os.path.getsize(ours)
        assert np.load(ours)["depths"].tobytes() == raw
        if not args.no_host:
            row["savez_numpy_ms"] = host_ms(lambda: np.savez_compressed(theirs, depths=arr), 3)
            row["npz_numpy_bytes"] = os.path.getsize(theirs)
            row["savez_speedup"] = row["savez_numpy_ms"] / row["savez_device_ms"]
    if not args.no_host:
        for key, strategy in (("zlib_level6", zlib.Z_DEFAULT_STRATEGY), ("zlib_rle", zlib.Z_RLE), ("zlib_huffman_only", zlib.Z_HUFFMAN_ONLY)):
            row[key + "_ratio"] = zlib_raw(raw, strategy) / nbytes
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[32, 518, 518], help="n h w")
    ap.add_argument("--repeats", type=int, default=100)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--model", action="store_true", help="also the depth of the synthetic-checkpoint ViT-S forward on a generated clip")
    ap.add_argument("--no-host", action="store_true", help="skip the host yardsticks (np.savez_compressed, zlib)")
    ap.add_argument("--out-dir", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "deflate"))
    ap.add_argument("--tmp", default=None, help="directory for the .npz files that are timed (default: the system's)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "deflate_bench needs a GPU"
    n, h, w = args.shape
    hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    inputs = [("synthetic_field", synthetic_field(n, h, w))]
    if args.model:
        inputs.append(("vits_synthetic_forward", model_depth(n, h, w)))
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "deflate_bench.txt"), "a") as f:
        for name, arr in inputs:
            line = json.dumps(measure(name, arr, args, hip))
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
