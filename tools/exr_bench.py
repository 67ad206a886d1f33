#!/usr/bin/env python
"""Time the EXR writer (csrc/exr.hip, video_depth_anything_amd/exr.py) on what run.py --save_exr hands it (a record for DESIGN.md 6l,
no threshold): 32 x 518 x 518 float32 depth, as a synthetic field (smooth, a little noise, some zeros) and - with --model - as the
depth the synthetic-checkpoint ViT-S forward gives for a generated clip. One JSON line per input, printed and appended to
<out-dir>/exr_bench.txt:

  kernels   device events around `--repeats` back-to-back calls of ops.exr_zip (its four launches: encode, blocks, offsets, pack) on a
            device-resident array after a warm-up, the median of `--windows` such windows
  memcpy    the yardstick, measured in the same process and timed the same way: a device-to-device hipMemcpyAsync of the same bytes
  files     array to files, host clock, median of three each, both into the same directory: exr.write_exr_sequence(device="cuda")
            (staging, upload, kernels, download, one file per frame) beside the host writer exr.write_exr_sequence(device=None)
            (zlib.compress at its default level on one core)
  sizes     the device's files beside the host writer's and the pixels; how many blocks the device wrote raw; the device's files
            are read back by read_exr and compared with the input, and the first frame's is compared with the twin's

Needs a GPU; no fallback."""
import argparse
import ctypes
import json
import os
import struct
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_depth_anything_amd import exr, ops  # noqa: E402
from tools.deflate_bench import host_ms, model_depth, synthetic_field, timed  # noqa: E402


def raw_blocks(data, h, w):
    """Blocks of one file whose dataSize is the rows' size."""
    nb = -(-h // 16)
    raw = 0
    for b, pos in enumerate(struct.unpack_from(f"<{nb}Q", data, 277)):
        raw += struct.unpack_from("<i", data, pos + 4)[0] == 4 * w * min(16, h - 16 * b)
    return raw


def measure(name, arr, args, hip):
    n, h, w = arr.shape
    x = torch.from_numpy(arr).cuda()
    nbytes = arr.nbytes
    work = torch.empty(ops.exr_workspace_bytes(n, h, w), dtype=torch.uint8, device="cuda")
    payload = torch.empty(ops.exr_payload_bytes(n, h, w), dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ms = timed(lambda: ops.exr_zip(x, 277, work, payload, offsets), args.repeats, args.windows)
    dst = torch.empty_like(x)
    cur = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def copy():
        rc = hip.hipMemcpyAsync(dst.data_ptr(), x.data_ptr(), nbytes, 3, cur)      # 3: device to device
        assert rc == 0, rc
    copy_ms = timed(copy, args.repeats, args.windows)
    row = {"input": name, "shape": list(arr.shape), "input_bytes": nbytes, "blocks": n * -(-h // 16), "repeats": args.repeats, "windows": args.windows,
           "kernels_ms": ms, "kernels_input_GBps": nbytes / ms / 1e6, "memcpy_ms": copy_ms, "memcpy_GBps": 2 * nbytes / copy_ms / 1e6,
           "kernels_over_memcpy": ms / copy_ms, "workspace_bytes": work.numel()}
    with tempfile.TemporaryDirectory(dir=args.tmp) as d:
        ours, theirs = os.path.join(d, "device"), os.path.join(d, "host")
        paths = exr.write_exr_sequence(arr, ours, device="cuda")                   # warm-up: pinned staging buffers
        row["files_device_ms"] = host_ms(lambda: exr.write_exr_sequence(arr, ours, device="cuda"), 3)
        files = [open(p, "rb").read() for p in paths]
        for f, frame in zip(files, arr):
            assert exr.read_exr(f)["Z"].tobytes() == frame.tobytes(), "read_exr does not give the input back"
        assert files[0] == exr.encode_exr_numpy(arr[0]), "the device's bytes are not the twin's"
        row["files_device_bytes"] = sum(map(len, files))
        row["ratio"] = row["files_device_bytes"] / nbytes
        row["raw_blocks"] = sum(raw_blocks(f, h, w) for f in files)
        if not args.no_host:
            hpaths = exr.write_exr_sequence(arr, theirs, device=None)
            row["files_host_zlib_ms"] = host_ms(lambda: exr.write_exr_sequence(arr, theirs, device=None), 3)
            row["files_host_zlib_bytes"] = sum(os.path.getsize(p) for p in hpaths)
            row["files_speedup"] = row["files_host_zlib_ms"] / row["files_device_ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[32, 518, 518], help="n h w")
    ap.add_argument("--repeats", type=int, default=100)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--model", action="store_true", help="also the depth of the synthetic-checkpoint ViT-S forward on a generated clip")
    ap.add_argument("--no-host", action="store_true", help="skip the host writer")
    ap.add_argument("--out-dir", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "exr"))
    ap.add_argument("--tmp", default=None, help="directory for the files that are timed (default: the system's)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "exr_bench needs a GPU"
    n, h, w = args.shape
    hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    inputs = [("synthetic_field", synthetic_field(n, h, w))]
    if args.model:
        inputs.append(("vits_synthetic_forward", model_depth(n, h, w)))
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "exr_bench.txt"), "a") as f:
        for name, arr in inputs:
            line = json.dumps(measure(name, arr, args, hip))
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
