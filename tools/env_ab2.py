#!/usr/bin/env python
"""Whole forward under a GEMM tuning environment switch (gemm.hip: GemmTuning), one process, one model, interleaved - what
option_ab2.py does for a vda_set_option switch: env_ab2.py [vitl|vits] VDA_GEMM_PLAIN_CONV 0,1
The switch is set in the environment and read again by vda_gemm_reload_tuning before each arm's rounds."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_depth_anything_amd import _lib
from video_depth_anything_amd.config import get_config
from video_depth_anything_amd.video_depth import VideoDepthAnything
from video_depth_anything_amd.weights import synthetic_state_dict
enc, key = sys.argv[1], sys.argv[2]
vals = sys.argv[3].split(",")
arms = list(enumerate(vals))            # (position, value): "0,0" is an A/A run with two arms
cfg = get_config(enc)
m = VideoDepthAnything(encoder=enc, features=cfg.features, out_channels=list(cfg.out_channels))
m.load_state_dict(synthetic_state_dict(cfg, seed=0)); m = m.to("cuda")
x = torch.randn(1, 32, 3, 518, 518, generator=torch.Generator().manual_seed(0)).cuda()
ts = {a: [] for a in arms}; outs = {}
for rep in range(7):
    for a in arms:
        os.environ[key] = a[1]
        _lib.lib.vda_gemm_reload_tuning()
        d = m.forward(x, fp32=False)
        if rep == 0: outs[a] = d.clone()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10): m.forward(x, fp32=False)
        e1.record(); torch.cuda.synchronize()
        ts[a].append(e0.elapsed_time(e1) / 10)
for a in arms:
    t = sorted(ts[a])[len(ts[a]) // 2]
    print(f"{enc} {key}={a[1]}: {t:.3f} ms/clip ({32e3 / t:.1f} frames/s)  all: {[round(u, 3) for u in ts[a]]}", flush=True)
every = [u for a in arms for u in ts[a]]
print(f"max - min of the {len(every)} rounds: {max(every) - min(every):.3f} ms")
a, b = outs[arms[0]], outs[arms[-1]]
print(f"rel-L1 between the two: {float((a - b).abs().mean() / a.abs().mean()):.3e}, bits equal: {bool(torch.equal(a, b))}")
