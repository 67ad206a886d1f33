#!/usr/bin/env python
"""End-to-end infer_video_depth throughput on one GPU (BASELINE.json config 4 shape: N synthetic 518x518 frames,
ViT-L): uint8 frames start in HOST memory, float32 depth ends in host memory (PCIe-inclusive), stitch included.
Reports OUTPUT frames/s; the sliding window computes 32 frames per 22 new ones (1.47x redundancy at N=1024).

  video_bench.py [enc] [N]                       one timed infer_video_depth
  video_bench.py [enc] [N] --stream [--rounds R] [--block M]
                                                 infer_video_depth and infer_video_depth_stream (a generator of M-frame items in, M = 1 by default, every
                                                 piece kept) timed alternately R times in this one process, after a warm-up of both;
                                                 prints both series, the spread of each and whether the results are bit-identical"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_depth_anything_amd.config import get_config
from video_depth_anything_amd.scheduler import plan_windows
from video_depth_anything_amd.video_depth import VideoDepthAnything
from video_depth_anything_amd.weights import state_dict_spec

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
STREAM = "--stream" in sys.argv
ROUNDS = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 4
BLOCK = int(sys.argv[sys.argv.index("--block") + 1]) if "--block" in sys.argv else 1      # frames per item the source yields
for opt in ("--rounds", "--block"):
    if opt in sys.argv:
        argv.remove(sys.argv[sys.argv.index(opt) + 1])
enc = argv[0] if len(argv) > 0 else "vitl"
N = int(argv[1]) if len(argv) > 1 else 1024
cfg = get_config(enc)
g = torch.Generator().manual_seed(0)
sd = {k: (torch.randn(s, generator=g) * (0.02 if len(s) > 1 else 0.1) + (0 if len(s) > 1 else 1)) for k, s in state_dict_spec(cfg).items()}
m = VideoDepthAnything(encoder=enc, features=cfg.features, out_channels=list(cfg.out_channels))
m.load_state_dict(sd); m = m.to("cuda")
frames = np.random.default_rng(0).integers(0, 256, (N, 518, 518, 3), dtype=np.uint8)
m.infer_video_depth(frames[:40], 24)                      # warm-up (allocations, first-touch)
torch.cuda.synchronize()
nw = len(plan_windows(N))
if STREAM:
    def source(v):
        return (f for f in v) if BLOCK == 1 else (v[i:i + BLOCK] for i in range(0, len(v), BLOCK))

    def run_array():
        t0 = time.perf_counter()
        d, _ = m.infer_video_depth(frames, 24)
        return time.perf_counter() - t0, d

    def run_stream():
        t0 = time.perf_counter()
        st = m.infer_video_depth_stream(source(frames), 24)
        pieces = [d for _, d in st]
        return time.perf_counter() - t0, pieces, st

    list(m.infer_video_depth_stream(source(frames[:80]), 24))       # warm-up of the streamed path (ring, pinned buffers)
    run_array(), run_stream()                                            # one untimed round of each at full length
    ta, ts = [], []
    for r in range(ROUNDS):
        dt, d = run_array()
        ta.append(N / dt)
        dt, pieces, st = run_stream()
        ts.append(N / dt)
        print(f"round {r}: array {ta[-1]:.1f}  stream {ts[-1]:.1f} output frames/s", flush=True)
    same = np.array_equal(np.concatenate(pieces), d) and st.depth_min == d.min() and st.depth_max == d.max()
    fmt = lambda v: " ".join(f"{x:.1f}" for x in v)
    print(f"{enc} N={N} windows={nw} rounds={ROUNDS}, source yields {BLOCK} frame(s) per item; output frames/s")
    print(f"infer_video_depth        : {fmt(ta)}   median {np.median(ta):.1f}  spread (max - min) {max(ta) - min(ta):.1f}")
    print(f"infer_video_depth_stream : {fmt(ts)}   median {np.median(ts):.1f}  spread (max - min) {max(ts) - min(ts):.1f}")
    print(f"stream - array (medians) : {np.median(ts) - np.median(ta):+.1f} frames/s ({(np.median(ts) / np.median(ta) - 1) * 100:+.2f} %); bit-identical: {same}")
    print(f"peak device memory allocated: {torch.cuda.max_memory_allocated() / 2**20:.0f} MiB (both paths ran)")
    sys.exit(0 if same else 1)
t0 = time.perf_counter()
d, _ = m.infer_video_depth(frames, 24)
dt = time.perf_counter() - t0
print(f"{enc} N={N} windows={nw}: {dt:.2f} s  -> {N / dt:.1f} output frames/s ({nw * 32 / dt:.1f} computed frames/s, {dt / nw * 1e3:.1f} ms/window); depth {d.shape} {d.dtype}")
