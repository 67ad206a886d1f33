#!/usr/bin/env python
"""Per-shape table of every GEMM / conv launch in one clip forward: time, TFLOP/s and the kernel vda_gemm_plan picks.
  gemm_table.py [vitl|vits]                    time the Python engine's launches on the GPU
  gemm_table.py [vitl|vits] --plan-only [NCU]  no GPU: the plan of every shape of a 1x32x518x518 forward on NCU compute units (256)"""
import os, sys, collections, ctypes
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_depth_anything_amd import _lib
from video_depth_anything_amd.config import get_config
enc = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else "vitl"
cfg = get_config(enc)


def plan_names(M, N, K, epi, ncu=0, m_plan=0, conv=None, lda=None, ldc=None, P=0, convt=None, relu_in=False, tile_rows=0, **_):
    a = _lib.GemmArgs(M=M, N=N, K=K, lda=K if lda is None else lda, ldc=N if ldc is None else ldc, epilogue=epi, P=P, relu_in=int(relu_in), tile_rows=tile_rows)
    if conv is not None:
        a.a_mode, a.lda = _lib.A_CONV3X3, 0
        a.cB, a.cH, a.cW, a.cCin, a.cHo, a.cWo, a.cStride = conv
    if convt is not None:
        a.tK, a.tH, a.tW, a.tCout = convt
    p = _lib.GemmPlan()
    _lib.check(_lib.lib.vda_gemm_plan(ctypes.byref(a), m_plan, ncu, 0, ctypes.byref(p)), "vda_gemm_plan")
    return " + ".join(f"{_lib.launch_name(p.rec[i])} [{p.rec[i].rows} rows]" if p.n > 1 else _lib.launch_name(p.rec[i]) for i in range(p.n))


if "--plan-only" in sys.argv:
    i = sys.argv.index("--plan-only")
    ncu = int(sys.argv[i + 1]) if len(sys.argv) > i + 1 else 256
    E, D, Fe, T, ph = _lib, cfg.embed_dim, cfg.features, 32, 37
    ocp = [(c + 63) // 64 * 64 for c in cfg.out_channels]
    P, rows, Fhp = ph * ph, T * (ph * ph + 1), (Fe // 2 + 63) // 64 * 64
    cv = lambda hw, Cin, Cout, epi, s=1, relu=False: dict(M=T * ((hw - 1) // s + 1) ** 2, N=Cout, K=9 * Cin, epi=epi, relu_in=relu,
                                                            conv=(T, hw, hw, Cin, (hw - 1) // s + 1, (hw - 1) // s + 1, s))
    shapes = [("patch_embed", dict(M=T * P, N=D, K=640, epi=E.EPI_PATCH_F32, P=P))]
    for name, N, K, epi in (("qkv", 3 * D, D, E.EPI_LN_BIAS_F16), ("proj", D, D, E.EPI_SCALE_RES_SPLIT), ("fc1", 4 * D, D, E.EPI_LN_GELU_F16), ("fc2", D, 4 * D, E.EPI_SCALE_RES_SPLIT)):
        shapes += [(name, dict(M=rows, N=N, K=K, epi=epi)), (name + " (enc_split half)", dict(M=rows // 2, N=N, K=K, epi=epi, m_plan=rows))]
    shapes += [(f"proj{i}", dict(M=T * P, N=ocp[i], K=D, epi=E.EPI_BIAS_F16)) for i in range(4)]
    shapes += [(f"resize{i}", dict(M=T * P, N=k * k * ocp[i], K=ocp[i], ldc=ocp[i], epi=E.EPI_CONVT_F16, convt=(k, ph, ph, ocp[i]))) for i, k in ((0, 4), (1, 2))]
    shapes += [("resize3", cv(ph, ocp[3], ocp[3], E.EPI_BIAS_F16, 2))] + [(f"layer{i + 1}_rn", cv(hw, ocp[i], Fe, E.EPI_BIAS_F16)) for i, hw in enumerate((4 * ph, 2 * ph, ph, 19))]
    for tag, hw2, Cc in (("l3", P, ocp[2]), ("l4", 19 * 19, ocp[3]), ("p4", P, Fe), ("p3", 4 * P, Fe)):
        r = T * hw2
        shapes += [(f"temporal {tag} {n}", dict(M=r, N=N, K=K, epi=epi, **kw)) for n, N, K, epi, kw in (
            ("in", Cc, Cc, E.EPI_BIAS_F32, {}), ("qkv", 3 * Cc, Cc, E.EPI_BIAS_F16, {}), ("attn out", Cc, Cc, E.EPI_SCALE_RES_F32, {}),
            ("ff1", 8 * Cc, Cc, E.EPI_GEGLU_F16, dict(ldc=4 * Cc)), ("ff2", Cc, 4 * Cc, E.EPI_SCALE_RES_F32_H, {}), ("out", Cc, Cc, E.EPI_RES_F16, {}))]
    for i, hw in ((4, 19), (3, ph), (2, 2 * ph), (1, 4 * ph)):
        shapes += [(f"refinenet{i} rcu conv1", cv(hw, Fe, Fe, E.EPI_BIAS_RELU_F16, relu=True)), (f"refinenet{i} rcu conv2", cv(hw, Fe, Fe, E.EPI_RES_F16)),
                   (f"refinenet{i} out", dict(M=T * 4 * hw * hw, N=Fe, K=Fe, epi=E.EPI_BIAS_F16))]
    shapes += [("output_conv1", cv(8 * ph, Fe, Fhp, E.EPI_BIAS_F16)), ("output_conv2.0", cv(518, Fhp, 32, E.EPI_BIAS_RELU_F16))]
    for name, kw in shapes:
        print(f"{name:24s} M={kw['M']:8d} N={kw['N']:5d} K={kw['K']:5d} epi={kw['epi']:2d}  {plan_names(ncu=ncu, **kw)}")
    sys.exit(0)

import torch
from video_depth_anything_amd import ops
from video_depth_anything_amd.video_depth import VideoDepthAnything
from video_depth_anything_amd.weights import state_dict_spec
g = torch.Generator().manual_seed(0)
sd = {k: (torch.randn(s, generator=g) * 0.02 if len(s) > 1 else torch.ones(s)) for k, s in state_dict_spec(cfg).items()}
m = VideoDepthAnything(encoder=enc, features=cfg.features, out_channels=list(cfg.out_channels))
m.load_state_dict(sd); m = m.to("cuda")
x = torch.randn(1, 32, 3, 518, 518, generator=g).cuda()
PE = m.python_engine()          # the Python launch sequence goes through ops.gemm (the handle's C++ one does not)
PE.forward(x); torch.cuda.synchronize()
rec = []
orig = ops.gemm
def wrapped(A, W, out, epi, **kw):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); orig(A, W, out, epi, **kw); e1.record()
    rec.append(((kw["M"], kw["N"], kw["K"], epi, "conv" if kw.get("conv") else "dense", plan_names(epi=epi, **kw)), e0, e1))
ops.gemm = wrapped
for _ in range(3): PE.forward(x)
torch.cuda.synchronize()
agg = collections.OrderedDict()
for key, e0, e1 in rec:
    a = agg.setdefault(key, [0, 0.0]); a[0] += 1; a[1] += e0.elapsed_time(e1)
tot = 0
for (M, N, K, epi, mode, kern), (n, ms) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
    us = ms / n * 1e3; tot += ms / 3
    print(f"{mode:5s} M={M:8d} N={N:5d} K={K:5d} epi={epi} x{n//3:3d}  {us:8.1f} us  {2.0*M*N*K/us/1e6:7.0f} TF/s  {ms/3:6.2f} ms/fwd  {kern}")
print("total gemm ms/fwd", tot)
