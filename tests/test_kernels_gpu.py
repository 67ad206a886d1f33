"""Per-kernel parity: every C-ABI entry point against a plain
torch fp32 CPU evaluation of the same op on the same fp16-rounded operands.

Tolerances: operands are fp16 (rel 2^-11 per element), accumulation fp32; outputs are compared
with  max|y - ref| <= atol + rtol*|ref|  where rtol covers the final fp16 rounding of the output
(2^-10) and atol the accumulated operand rounding over K terms."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _exact import BILINEAR_EDGE_CASES, bilinear_id, check_sentinel, sentinel_out

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU; run them with -m gpu on the MI355X box only")
    from video_depth_anything_amd import ops as o
    return o


@pytest.fixture(params=[-1, 0, 1, 2, 3, 4, 5, 7, 9, 8, 5 + 16 * 64, 10, 11], ids=["auto", "tile128", "tile256x256", "tile256x128", "tile256x256_mfma16", "tile256x128_mfma16",
                                                                            "tile256x256_8phase", "conv_lds_where_it_applies", "tile256x128_8phase", "tile192x128_6waves",
                                                                            "tile192x256_8phase_where_built", "tile192x384_12waves_where_built",
                                                                            "tile192x128_two_workgroups_per_cu_where_built"])
def gemm_variant(request, ops):
    """Run every GEMM/conv test under each tile family (the dispatcher normally picks per shape)."""
    from video_depth_anything_amd._lib import lib
    lib.vda_gemm_set_variant(request.param)
    yield request.param
    lib.vda_gemm_set_variant(-1)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def close(y, ref, rtol=2e-3, atol=2e-3, what=""):
    y = y.detach().float().cpu()
    ref = ref.float()
    err = (y - ref).abs()
    bound = atol + rtol * ref.abs()
    bad = err > bound
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} out of tolerance, max err {float(err.max()):.4g} (ref absmax {float(ref.abs().max()):.4g})"


def dev(t, dtype=None):
    t = t.cuda()
    return t.to(dtype) if dtype is not None else t


# ---------------------------------------------------------------- GEMM epilogues
@pytest.mark.parametrize("M,N,K", [(300, 192, 128), (128, 64, 64), (1000, 48, 192), (257, 384, 1536), (4100, 1024, 1024), (20011, 64, 128)])
def test_gemm_bias(ops, gemm_variant, M, N, K):
    from video_depth_anything_amd import _lib
    A = rnd(M, K, seed=1).to(F16)
    W = rnd(N, K, seed=2, scale=K ** -0.5).to(F16)
    b = rnd(N, seed=3)
    out = torch.empty(M, N, dtype=F16, device="cuda")
    ops.gemm(dev(A), dev(W), out, _lib.EPI_BIAS_F16, M=M, N=N, K=K, bias=dev(b))
    ref = A.float() @ W.float().t() + b
    close(out, ref, what=f"gemm {M}x{N}x{K}")


def test_gemm_gelu_relu_f32(ops, gemm_variant):
    from video_depth_anything_amd import _lib
    M, N, K = 515, 256, 320
    A, W, b = rnd(M, K, seed=4).to(F16), rnd(N, K, seed=5, scale=K ** -0.5).to(F16), rnd(N, seed=6)
    base = A.float() @ W.float().t() + b
    for epi, fn, dt in ((_lib.EPI_BIAS_GELU_F16, F.gelu, F16), (_lib.EPI_BIAS_RELU_F16, F.relu, F16), (_lib.EPI_BIAS_F32, lambda x: x, F32)):
        out = torch.empty(M, N, dtype=dt, device="cuda")
        ops.gemm(dev(A), dev(W), out, epi, M=M, N=N, K=K, bias=dev(b))
        close(out, fn(base), what=f"epilogue {epi}")


def test_gemm_scale_residual_inplace(ops, gemm_variant):
    from video_depth_anything_amd import _lib
    M, N, K = 777, 384, 384
    A, W = rnd(M, K, seed=7).to(F16), rnd(N, K, seed=8, scale=K ** -0.5).to(F16)
    b, gamma, res = rnd(N, seed=9), rnd(N, seed=10), rnd(M, N, seed=11, scale=3.0)
    x = dev(res.clone())
    ops.gemm(dev(A), dev(W), x, _lib.EPI_SCALE_RES_F32, M=M, N=N, K=K, bias=dev(b), gamma=dev(gamma), res=x)
    ref = res + gamma * (A.float() @ W.float().t() + b)
    close(x, ref, rtol=1e-5, atol=2e-3, what="scale+residual fp32")


def test_gemm_scale_residual_f16_out(ops, gemm_variant):
    from video_depth_anything_amd import _lib
    M, N, K = 260, 64, 256
    A, W, b = rnd(M, K, seed=51).to(F16), rnd(N, K, seed=52, scale=K ** -0.5).to(F16), rnd(N, seed=53)
    res = rnd(M, N, seed=54, scale=2.0)
    out = torch.empty(M, N, dtype=F16, device="cuda")
    ops.gemm(dev(A), dev(W), out, _lib.EPI_SCALE_RES_F32_H, M=M, N=N, K=K, bias=dev(b), res=dev(res))
    close(out, res + A.float() @ W.float().t() + b, what="fp32 residual -> fp16 out")


def test_gemm_res_f16_two_residuals(ops, gemm_variant):
    from video_depth_anything_amd import _lib
    M, N, K = 300, 64, 128
    A, W, b = rnd(M, K, seed=12).to(F16), rnd(N, K, seed=13, scale=K ** -0.5).to(F16), rnd(N, seed=14)
    r1, r2 = rnd(M, N, seed=15).to(F16), rnd(M, N, seed=16).to(F16)
    out = torch.empty(M, N, dtype=F16, device="cuda")
    ops.gemm(dev(A), dev(W), out, _lib.EPI_RES_F16, M=M, N=N, K=K, bias=dev(b), res=dev(r1), res2=dev(r2))
    close(out, A.float() @ W.float().t() + b + r1.float() + r2.float(), what="res f16 x2")


def test_gemm_geglu(ops, gemm_variant):
    from video_depth_anything_amd import _lib
    M, Cc = 333, 64
    A = rnd(M, Cc, seed=17).to(F16)
    w, b = rnd(8 * Cc, Cc, seed=18, scale=Cc ** -0.5), rnd(8 * Cc, seed=19)
    wi, bi = ops.pack_geglu(w, b)
    out = torch.empty(M, 4 * Cc, dtype=F16, device="cuda")
    ops.gemm(dev(A), dev(wi), out, _lib.EPI_GEGLU_F16, M=M, N=8 * Cc, K=Cc, ldc=4 * Cc, bias=dev(bi))
    p = A.float() @ w.to(F16).float().t() + b
    val, gate = p.chunk(2, dim=-1)
    close(out, val * F.gelu(gate), what="geglu")


def test_gemm_geglu_full_width_regression(ops):
    """Temporal module 1 of ViT-L (M=11552, N=8192, K=1024): the large-tile epilogue once preloaded gate-lane
    bias past the end of the tensor (a page fault when the bias ends a memory segment)."""
    from video_depth_anything_amd import _lib
    M, Cc = 11552, 1024
    A = rnd(M, Cc, seed=60).to(F16)
    w, b = rnd(8 * Cc, Cc, seed=61, scale=Cc ** -0.5), rnd(8 * Cc, seed=62)
    wi, bi = ops.pack_geglu(w, b)
    out = torch.empty(M, 4 * Cc, dtype=F16, device="cuda")
    ops.gemm(dev(A), dev(wi), out, _lib.EPI_GEGLU_F16, M=M, N=8 * Cc, K=Cc, ldc=4 * Cc, bias=dev(bi))
    sel = torch.arange(0, M, 97)
    p = A[sel].float() @ w.to(F16).float().t() + b
    val, gate = p.chunk(2, dim=-1)
    close(out[sel.cuda()], val * F.gelu(gate), what="geglu full width")


def test_gemm_patch_embed(ops, gemm_variant):
    from video_depth_anything_amd import _lib
    B, H, W_, D = 3, 42, 56, 128
    ph, pw = H // 14, W_ // 14
    P = ph * pw
    x = rnd(B, 3, H, W_, seed=20)
    w, b = rnd(D, 3, 14, 14, seed=21, scale=588 ** -0.5), rnd(D, seed=22)
    pos, cls = rnd(P + 1, D, seed=23), rnd(D, seed=24)
    Kp = 640
    a = torch.zeros(B * P, Kp, dtype=F16, device="cuda")
    ops.patchify(dev(x), a, B, H, W_, Kp)
    tok = torch.full((B, P + 1, D), float("nan"), dtype=F32, device="cuda")
    wp = ops.pack_linear(w.reshape(D, 588), k_pad=Kp)
    ops.gemm(a, dev(wp), tok, _lib.EPI_PATCH_F32, M=B * P, N=D, K=Kp, bias=dev(b), pos=dev(pos), P=P)
    ops.cls_rows(tok, dev(cls), dev(pos), B, P, D)
    ref = F.conv2d(x.to(F16).float(), w.to(F16).float(), b, stride=14).flatten(2).transpose(1, 2)
    ref = torch.cat((cls.expand(B, 1, D), ref), dim=1) + pos
    close(tok, ref, what="patch embed tokens")


@pytest.mark.parametrize("k", [2, 4])
def test_gemm_convtranspose(ops, gemm_variant, k):
    from video_depth_anything_amd import _lib
    B, h, w_, Cc = 2, 5, 7, 48
    Cp = 64
    x = rnd(B, Cc, h, w_, seed=25).to(F16)
    wt, b = rnd(Cc, Cc, k, k, seed=26, scale=Cc ** -0.5), rnd(Cc, seed=27)
    xin = torch.zeros(B, h, w_, Cp, dtype=F16)
    xin[..., :Cc] = x.permute(0, 2, 3, 1)
    wp, bp = ops.pack_convt(wt, b, Cp)
    out = torch.empty(B, h * k, w_ * k, Cp, dtype=F16, device="cuda")
    ops.gemm(dev(xin), dev(wp), out, _lib.EPI_CONVT_F16, M=B * h * w_, N=k * k * Cp, K=Cp, ldc=Cp, bias=dev(bp), convt=(k, h, w_, Cp))
    ref = F.conv_transpose2d(x.float(), wt.to(F16).float(), b, stride=k).permute(0, 2, 3, 1)
    close(out[..., :Cc], ref, what=f"convT k={k}")
    assert float(out[..., Cc:].abs().max()) == 0.0, "pad channels must stay zero"


@pytest.mark.parametrize("stride,relu_in,Cin,Cout,H,W_", [(1, False, 64, 64, 9, 11), (1, True, 128, 256, 12, 7), (2, False, 64, 128, 9, 9),
                                                        (1, True, 64, 32, 20, 20), (1, True, 64, 64, 83, 79), (1, False, 128, 64, 77, 80), (1, True, 256, 256, 40, 41),
                                                        (1, False, 192, 64, 37, 37), (1, False, 64, 32, 45, 70)])
def test_conv3x3(ops, gemm_variant, stride, relu_in, Cin, Cout, H, W_):
    from video_depth_anything_amd import _lib
    B = 3
    x = rnd(B, Cin, H, W_, seed=28).to(F16)
    w, b = rnd(Cout, Cin, 3, 3, seed=29, scale=(9 * Cin) ** -0.5), rnd(Cout, seed=30)
    res = rnd(B, (H - 1) // stride + 1, (W_ - 1) // stride + 1, Cout, seed=31).to(F16)
    Ho, Wo = (H + 2 - 3) // stride + 1, (W_ + 2 - 3) // stride + 1
    xin = x.permute(0, 2, 3, 1).contiguous()
    out = torch.empty(B, Ho, Wo, Cout, dtype=F16, device="cuda")
    ops.gemm(dev(xin), dev(ops.pack_conv3x3(w)), out, _lib.EPI_RES_F16, M=B * Ho * Wo, N=Cout, K=9 * Cin, bias=dev(b), res=dev(res),
             relu_in=relu_in, conv=(B, H, W_, Cin, Ho, Wo, stride))
    xi = F.relu(x.float()) if relu_in else x.float()
    ref = F.conv2d(xi, w.to(F16).float(), b, stride=stride, padding=1).permute(0, 2, 3, 1) + res.float()
    close(out, ref, what="conv3x3")


@pytest.mark.parametrize("B,H,W_,Cout,epi,relu_in,two_res", [(3, 9, 11, 64, "res", True, True), (2, 20, 37, 32, "bias", False, False), (1, 83, 79, 64, "relu", True, False),
                                                            (2, 45, 70, 24, "res", False, False), (32, 74, 74, 64, "res", True, True), (8, 148, 148, 64, "relu", True, False)])
def test_conv3x3_c64_persistent_equals_per_pass_kernel(ops, B, H, W_, Cout, epi, relu_in, two_res):
    """The persistent 64-input-channel LDS convolution (resident weights, specialised waves, two patch buffers; the last two cases have more
    tiles than workgroups) against the per-pass kernel it replaces: the same MFMA order per output element, so bit-identical."""
    from video_depth_anything_amd import _lib
    Cin = 64
    x = dev(rnd(B, H, W_, Cin, seed=401).to(F16))
    w, b = dev(ops.pack_conv3x3(rnd(Cout, Cin, 3, 3, seed=402, scale=(9 * Cin) ** -0.5))), dev(rnd(Cout, seed=403))
    res = dev(rnd(B, H, W_, Cout, seed=404).to(F16))
    res2 = dev(rnd(B, H, W_, Cout, seed=405).to(F16))
    e = {"res": _lib.EPI_RES_F16, "bias": _lib.EPI_BIAS_F16, "relu": _lib.EPI_BIAS_RELU_F16}[epi]
    kw = dict(M=B * H * W_, N=Cout, K=9 * Cin, bias=b, relu_in=relu_in, conv=(B, H, W_, Cin, H, W_, 1))
    if epi == "res":
        kw.update(res=res)
        if two_res:
            kw.update(res2=res2)
    outs = []
    try:
        for v in (1, 0):
            _lib.lib.vda_conv_lds_set_variant(v)
            out = torch.full((B, H, W_, Cout), float("nan"), dtype=F16, device="cuda")
            ops.gemm(x, w, out, e, **kw)
            outs.append(out)
    finally:
        _lib.lib.vda_conv_lds_set_variant(0)
    assert torch.isfinite(outs[1].float()).all()
    assert torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------- LayerNorm folded into the GEMMs either side of it
def split_planes(x):
    hi = x.to(F16)
    return hi, (x - hi.float()).to(F16)


@pytest.mark.parametrize("D,rows", [(1024, 37), (384, 50), (128, 9), (64, 130), (192, 20), (256, 30), (2048, 10), (72, 10)])
def test_split_stats_and_layernorm_split(ops, D, rows):
    """fp32 rows -> (hi, lo) planes + (mean, rstd); LayerNorm of the split stream (with the cls-drop compaction)."""
    x = rnd(rows, D, seed=140, scale=3.0) + 0.7
    hi, lo = torch.empty(rows, D, dtype=F16, device="cuda"), torch.empty(rows, D, dtype=F16, device="cuda")
    stat = torch.empty(rows, 2, device="cuda")
    ops.split_stats(dev(x), hi, lo, stat, 1e-6, rows, D)
    rh, rl = split_planes(x)
    assert torch.equal(hi.cpu(), rh) and torch.equal(lo.cpu(), rl)
    assert float(((hi.float() + lo.float()).cpu() - x).abs().max()) <= 2.0 ** -21 * float(x.abs().max())      # 22 significant bits
    mean, var = x.double().mean(1), x.double().var(1, unbiased=False)
    close(stat[:, 0], mean, rtol=1e-5, atol=1e-6, what="mean")
    close(stat[:, 1], (var + 1e-6).rsqrt(), rtol=1e-5, atol=0, what="rstd")
    w, b = rnd(D, seed=141) + 1.0, rnd(D, seed=142)
    out = torch.empty(rows, D, dtype=F16, device="cuda")
    ops.layernorm_split(hi, lo, out, dev(w), dev(b), 1e-6, rows, D)
    close(out, F.layer_norm(x, (D,), w, b, 1e-6), what="layernorm of hi + lo")
    if rows % 10 == 0:
        G = 10
        out = torch.empty(rows - rows // G, D, dtype=F16, device="cuda")
        ops.layernorm_split(hi, lo, out, dev(w), dev(b), 1e-6, rows, D, group=G, skip=1)
        close(out, F.layer_norm(x, (D,), w, b, 1e-6).reshape(-1, G, D)[:, 1:].reshape(-1, D), what="layernorm of hi + lo, cls dropped")

    # the centred entry (the model's): hi + lo = x - mean(x), stat = (0, rstd)
    ops.split_stats(dev(x), hi, lo, stat, 1e-6, rows, D, center=True)
    xc = (x.double() - mean[:, None]).float()
    assert float(((hi.float() + lo.float()).cpu() - xc).abs().max()) <= 2.0 ** -21 * float(x.abs().max())      # 22 significant bits
    assert torch.equal(stat[:, 0].cpu(), torch.zeros(rows))
    close(stat[:, 1], (var + 1e-6).rsqrt(), rtol=1e-5, atol=0, what="rstd of the centred entry")


@pytest.mark.parametrize("M,N,K", [(777, 384, 384), (4100, 1024, 256), (2500, 384, 1536), (300, 64, 128)])
def test_gemm_split_residual_and_stats(ops, gemm_variant, M, N, K):
    """VDA_EPI_SCALE_RES_SPLIT in place over the two planes: x' = (hi + lo) + gamma * (A W^T + b), re-split; the per-64-column
    partial statistics combine (vda_ln_stats_finalize) to the row's mean / rstd."""
    from video_depth_anything_amd import _lib
    A, W = rnd(M, K, seed=143).to(F16), rnd(N, K, seed=144, scale=K ** -0.5).to(F16)
    b, gamma, x = rnd(N, seed=145), rnd(N, seed=146), rnd(M, N, seed=147, scale=3.0) + 0.3
    hi0, lo0 = split_planes(x)
    hi, lo = dev(hi0.clone()), dev(lo0.clone())
    part = torch.full((N // 64, M, 2), float("nan"), device="cuda")
    ops.gemm(dev(A), dev(W), hi, _lib.EPI_SCALE_RES_SPLIT, M=M, N=N, K=K, bias=dev(b), gamma=dev(gamma), res=hi, res2=lo, out2=lo, stats=part)
    ref = (hi0.float() + lo0.float()) + gamma * (A.float() @ W.float().t() + b)
    got = hi.float() + lo.float()
    close(got, ref, rtol=1e-5, atol=2e-3, what="split residual stream")
    assert bool(((hi.float() - got).abs() <= 2.0 ** -11 * got.abs() + 1e-7).all()), "the hi plane is the stream rounded to fp16 (lo at most half an ulp)"
    stat = torch.empty(M, 2, device="cuda")
    ops.ln_stats_finalize(part, stat, 1e-6, M, N // 64)
    g = got.double().cpu()
    close(stat[:, 0], g.mean(1), rtol=1e-5, atol=1e-5, what="mean from the epilogue's partials")
    close(stat[:, 1], (g.var(1, unbiased=False) + 1e-6).rsqrt(), rtol=1e-4, atol=0, what="rstd from the epilogue's partials")


@pytest.mark.parametrize("M,N,K", [(777, 384, 384), (4100, 1024, 256), (300, 64, 128)])
def test_gemm_split_residual_recentred(ops, gemm_variant, M, N, K):
    """VDA_EPI_SCALE_RES_SPLIT with pos = the (mean, rstd) rows of the LayerNorm in front of the branch: the row's mean leaves the
    stream as the update goes in (x' = x - mean + gamma * (A W^T + b)); entry by vda_split_center_stats_f32; rows with a mean of
    ~25 sigma. LayerNorm of the re-centred stream == LayerNorm of the fp32 stream it stands for."""
    from video_depth_anything_amd import _lib
    A, W = rnd(M, K, seed=190).to(F16), rnd(N, K, seed=191, scale=K ** -0.5).to(F16)
    b, gamma = rnd(N, seed=192), rnd(N, seed=193)
    x = rnd(M, N, seed=194) + 25.0 * (1.0 + 0.1 * rnd(M, 1, seed=195))
    hi, lo, stat = torch.empty(M, N, dtype=F16, device="cuda"), torch.empty(M, N, dtype=F16, device="cuda"), torch.empty(M, 2, device="cuda")
    ops.split_stats(dev(x), hi, lo, stat, 1e-6, M, N, center=True)
    mean = x.double().mean(1, keepdim=True)
    xc = (x.double() - mean).float()
    close(hi.float() + lo.float(), xc, rtol=1e-6, atol=2e-5, what="centred planes")      # (the fp32 mean of values ~25 is good to ~3e-6: a per-row shift)
    assert float(hi.float().abs().max()) < 8.0, "the operand plane holds the token relative to its mean"
    close(stat[:, 0], torch.zeros(M), rtol=0, atol=1e-6, what="mean of the centred planes")
    close(stat[:, 1], (x.double().var(1, unbiased=False) + 1e-6).rsqrt(), rtol=1e-5, atol=0, what="rstd")
    # a residual update with a non-zero mean of its own, re-centred by a statistics row that says "the stream's mean is 0.7"
    stat2 = stat.clone()
    stat2[:, 0] = 0.7
    part = torch.full((N // 64, M, 2), float("nan"), device="cuda")
    ref = (hi.float() + lo.float()).cpu() - 0.7 + gamma * (A.float() @ W.float().t() + b)       # from the planes as they are
    ops.gemm(dev(A), dev(W), hi, _lib.EPI_SCALE_RES_SPLIT, M=M, N=N, K=K, bias=dev(b), gamma=dev(gamma), res=hi, res2=lo, out2=lo, stats=part, pos=stat2)
    got = hi.float() + lo.float()
    close(got, ref, rtol=1e-5, atol=2e-3, what="re-centred split residual stream")
    ops.ln_stats_finalize(part, stat, 1e-6, M, N // 64)
    g = got.double().cpu()
    close(stat[:, 0], g.mean(1), rtol=1e-5, atol=1e-5, what="mean (relative to the new centre)")
    close(stat[:, 1], (g.var(1, unbiased=False) + 1e-6).rsqrt(), rtol=1e-4, atol=0, what="rstd")
    # shift invariance is what makes it legal: LayerNorm of the planes == LayerNorm of the stream they stand for
    w_, b_ = rnd(N, seed=196) + 1.0, rnd(N, seed=197)
    out = torch.empty(M, N, dtype=F16, device="cuda")
    ops.layernorm_split(hi, lo, out, dev(w_), dev(b_), 1e-6, M, N)
    full = x + gamma * (A.float() @ W.float().t() + b)
    close(out, F.layer_norm(full, (N,), w_, b_, 1e-6), what="LayerNorm of the re-centred stream")


@pytest.mark.parametrize("M,N,K", [(777, 1152, 384), (4100, 3072, 1024), (2500, 1536, 384), (300, 192, 128)])
def test_gemm_layernorm_folded(ops, gemm_variant, M, N, K):
    """qkv / fc1 with LayerNorm folded in: A = hi plane, W * diag(ln_w) (vda_fold_ln_weight), epilogue rstd * (acc - mean * c1) + c2
    (then GELU) against LayerNorm(x) @ W^T + b evaluated in fp32 - including rows whose mean is far from zero."""
    from video_depth_anything_amd import _lib
    x = rnd(M, K, seed=150, scale=2.0) + rnd(M, 1, seed=151, scale=3.0)
    Wt, b = rnd(N, K, seed=152, scale=K ** -0.5), rnd(N, seed=153)
    lw, lb = rnd(K, seed=154) * 0.3 + 1.0, rnd(K, seed=155) * 0.3
    Wf, c1, c2 = torch.empty(N, K, dtype=F16, device="cuda"), torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
    ops.fold_ln_weight(dev(Wt), dev(b), dev(lw), dev(lb), Wf, c1, c2, N, K)
    assert torch.equal(Wf.cpu(), (Wt * lw).to(F16))
    close(c1, (Wt * lw).to(F16).float().sum(1), rtol=1e-5, atol=1e-5, what="c1")
    close(c2, b + Wt @ lb, rtol=1e-5, atol=1e-5, what="c2")
    hi, lo, stat = torch.empty(M, K, dtype=F16, device="cuda"), torch.empty(M, K, dtype=F16, device="cuda"), torch.empty(M, 2, device="cuda")
    ops.split_stats(dev(x), hi, lo, stat, 1e-6, M, K)
    ref = F.layer_norm(x, (K,), lw, lb, 1e-6) @ Wt.t() + b
    for epi, fn in ((_lib.EPI_LN_BIAS_F16, lambda t: t), (_lib.EPI_LN_GELU_F16, F.gelu)):
        out = torch.full((M, N), float("nan"), dtype=F16, device="cuda")
        ops.gemm(hi, Wf, out, epi, M=M, N=N, K=K, bias=c2, gamma=c1, stats=stat)
        close(out, fn(ref), rtol=3e-3, atol=6e-3, what=f"LayerNorm-folded GEMM epilogue {epi}")


@pytest.mark.parametrize("regime", ["mean_over_sigma_30", "outlier_channels", "both"])
@pytest.mark.parametrize("M,N,K", [(1370, 1152, 384), (2740, 3072, 1024)])
def test_gemm_layernorm_folded_outlier_rows(ops, M, N, K, regime):
    """The regime of trained DINOv2 residual streams (VERDICT r2 missing #2): rows whose mean is ~30 standard deviations
    from zero, a few channels at 100-300x the typical magnitude, and both at once. The folded form (A = the fp16 operand plane of
    the split stream, statistics applied in the epilogue) must stay within 2x the error of the standalone form
    (LayerNorm in fp32 -> fp16 -> plain GEMM) against the fp32 reference, measured as mean |error| over the output."""
    from video_depth_anything_amd import _lib
    x = rnd(M, K, seed=170)
    if regime in ("mean_over_sigma_30", "both"):
        x = x + 30.0 * (1.0 + 0.2 * rnd(M, 1, seed=171))                # every row: mean ~ 30 sigma
    if regime in ("outlier_channels", "both"):
        ch = torch.tensor([5, K // 3, K - 7])
        x[:, ch] = x[:, ch] + torch.tensor([250.0, -120.0, 300.0]) * (1.0 + 0.1 * rnd(M, 3, seed=172))
    Wt, b = rnd(N, K, seed=173, scale=K ** -0.5), rnd(N, seed=174)
    lw, lb = rnd(K, seed=175) * 0.3 + 1.0, rnd(K, seed=176) * 0.3
    ref = (F.layer_norm(x.double(), (K,), lw.double(), lb.double(), 1e-6) @ Wt.double().t() + b.double()).float()
    # standalone: LayerNorm (fp32 statistics) -> fp16 -> GEMM with the plain bias epilogue
    xn = torch.empty(M, K, dtype=F16, device="cuda")
    ops.layernorm(dev(x), xn, dev(lw), dev(lb), 1e-6, M, K)
    out_s = torch.empty(M, N, dtype=F16, device="cuda")
    ops.gemm(xn, dev(Wt.to(F16)), out_s, _lib.EPI_BIAS_F16, M=M, N=N, K=K, bias=dev(b))
    # folded
    Wf, c1, c2 = torch.empty(N, K, dtype=F16, device="cuda"), torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
    ops.fold_ln_weight(dev(Wt), dev(b), dev(lw), dev(lb), Wf, c1, c2, N, K)
    hi, lo, stat = torch.empty(M, K, dtype=F16, device="cuda"), torch.empty(M, K, dtype=F16, device="cuda"), torch.empty(M, 2, device="cuda")
    ops.split_stats(dev(x), hi, lo, stat, 1e-6, M, K, center=True)          # the model's entry: planes relative to the row's mean
    out_f = torch.full((M, N), float("nan"), dtype=F16, device="cuda")
    ops.gemm(hi, Wf, out_f, _lib.EPI_LN_BIAS_F16, M=M, N=N, K=K, bias=c2, gamma=c1, stats=stat)
    assert torch.isfinite(out_f).all()
    es = float((out_s.float().cpu() - ref).abs().mean())
    ef = float((out_f.float().cpu() - ref).abs().mean())
    scale = float(ref.abs().mean())
    print(f"LN fold, {regime} {M}x{N}x{K}: standalone {es / scale:.3e}, folded {ef / scale:.3e} (relative L1)")
    assert ef <= 2.0 * es + 1e-4 * scale, f"folded LayerNorm error {ef / scale:.3e} vs standalone {es / scale:.3e} ({regime})"


def test_gemm_encoder_shapes_on_sampled_rows(ops):
    """The encoder's GEMMs at the BENCHMARKED row count (M = 32 x 1370 = 43 840: 171.25 row tiles, the partial last round and
    the partial last row tile of every launch) against the fp32 reference on sampled rows (every 61st row + the last 300)."""
    from video_depth_anything_amd import _lib
    M = 43840
    sel = torch.cat([torch.arange(0, M, 61), torch.arange(M - 300, M)]).unique()
    for (N, K) in ((3072, 1024), (1024, 4096), (1152, 384), (384, 1536)):
        A = rnd(M, K, seed=180).to(F16)
        W, b = rnd(N, K, seed=181, scale=K ** -0.5).to(F16), rnd(N, seed=182)
        out = torch.full((M, N), float("nan"), dtype=F16, device="cuda")
        ops.gemm(dev(A), dev(W), out, _lib.EPI_BIAS_F16, M=M, N=N, K=K, bias=dev(b))
        assert torch.isfinite(out).all(), f"{N}x{K}: unwritten or non-finite outputs"
        close(out[sel.cuda()], A[sel].float() @ W.float().t() + b, what=f"gemm 43840x{N}x{K} sampled rows")


@pytest.mark.parametrize("epi_name", ["BIAS_F16", "SCALE_RES_F32", "SCALE_RES_SPLIT", "LN_BIAS_F16"])
def test_gemm_row_split_is_bit_identical(ops, epi_name):
    """vda_gemm_plan_split: M = 43 840 rows as whole rounds of 256-row tiles + a remainder launch on 192-row tiles. Every row must
    come out BIT-identical to the single launch on 256-row tiles (a row's K order and epilogue do not depend on its tile), for
    each epilogue the split is built for; the planner must actually split these shapes on a 256-CU device."""
    import ctypes as C
    from video_depth_anything_amd import _lib
    lib = _lib.lib
    epi = getattr(_lib, "EPI_" + epi_name)
    M, N, K = 43840, 1024, 4096                              # fc2's shape: 2.69 rounds of 256-row tiles on 256 CUs
    m1 = lib.vda_gemm_plan_split(M, N, K, epi, _lib.A_DENSE)
    assert 0 < m1 < M and m1 % 256 == 0, m1
    assert lib.vda_gemm_plan_split(M, 3072, 1024, epi, _lib.A_DENSE) == M, "K = 1024: measured slower when split"
    A, W, b = dev(rnd(M, K, seed=200).to(F16)), dev(rnd(N, K, seed=201, scale=K ** -0.5).to(F16)), dev(rnd(N, seed=202))
    gamma = dev(rnd(N, seed=203).abs() + 0.5)

    def run(variant):
        lib.vda_gemm_set_variant(variant)
        try:
            kw = dict(M=M, N=N, K=K, bias=b)
            if epi_name == "BIAS_F16":
                out = torch.full((M, N), float("nan"), dtype=F16, device="cuda")
                ops.gemm(A, W, out, epi, **kw)
                return (out,)
            if epi_name == "SCALE_RES_F32":
                x = dev(rnd(M, N, seed=204))
                ops.gemm(A, W, x, epi, gamma=gamma, res=x, **kw)
                return (x,)
            if epi_name == "SCALE_RES_SPLIT":
                x = rnd(M, N, seed=204, scale=2.0)
                hi, lo = dev(x.to(F16)), dev((x - x.to(F16).float()).to(F16))
                part = torch.full((N // 64, M, 2), float("nan"), device="cuda")
                stat = dev(torch.stack([rnd(M, seed=205) * 0.1, torch.ones(M)], dim=1).contiguous())
                ops.gemm(A, W, hi, epi, gamma=gamma, res=hi, res2=lo, out2=lo, stats=part, pos=stat, **kw)
                return hi, lo, part
            stat = dev(torch.stack([rnd(M, seed=206) * 0.1, 1.0 + rnd(M, seed=207).abs()], dim=1).contiguous())
            out = torch.full((M, N), float("nan"), dtype=F16, device="cuda")
            ops.gemm(A, W, out, epi, gamma=gamma, stats=stat, **kw)
            return (out,)
        finally:
            lib.vda_gemm_set_variant(-1)

    split, single = run(-1), run(5)                          # auto (splits) / one launch of the 8-phase kernel on 256-row tiles
    assert lib.vda_gemm_last_kernel().decode().startswith("gemm8p_kernel<256")
    for t, (x, y) in enumerate(zip(split, single)):
        assert torch.isfinite(x).all() and torch.equal(x, y), f"{epi_name} output {t}: {int((x != y).sum())} elements differ between the split and the single launch"


def test_gemm_split_residual_without_recentring_survives_the_row_split(ops):
    """VDA_EPI_SCALE_RES_SPLIT with pos == NULL at a shape the dispatcher row-splits (fc2's). The first pass points pos at
    the 256-byte zero page with stride 0; the two row-range calls must keep that stride (they used to come back as "pos given",
    stride 2, and read 43 840 rows of (mean, rstd) out of a 256-byte page). Bit-identical to the single 8-phase launch."""
    from video_depth_anything_amd import _lib
    lib = _lib.lib
    M, N, K = 43840, 1024, 4096
    epi = _lib.EPI_SCALE_RES_SPLIT
    assert lib.vda_gemm_plan_split(M, N, K, epi, _lib.A_DENSE) < M
    A, W, b = dev(rnd(M, K, seed=210).to(F16)), dev(rnd(N, K, seed=211, scale=K ** -0.5).to(F16)), dev(rnd(N, seed=212))
    gamma = dev(rnd(N, seed=213).abs() + 0.5)
    x = rnd(M, N, seed=214, scale=2.0)
    guard = torch.full((1 << 20,), 1.0e4, device="cuda")     # whatever lies behind the zero page must not matter either

    def run(variant):
        lib.vda_gemm_set_variant(variant)
        try:
            hi, lo = dev(x.to(F16)), dev((x - x.to(F16).float()).to(F16))
            part = torch.full((N // 64, M, 2), float("nan"), device="cuda")
            ops.gemm(A, W, hi, epi, M=M, N=N, K=K, bias=b, gamma=gamma, res=hi, res2=lo, out2=lo, stats=part)      # no pos
            return hi, lo, part
        finally:
            lib.vda_gemm_set_variant(-1)

    split, single = run(-1), run(5)
    del guard
    for t, (u, v) in enumerate(zip(split, single)):
        assert torch.isfinite(u).all() and torch.equal(u, v), f"output {t}: {int((u != v).sum())} elements differ"
    # and against the definition on sampled rows: x' = x + gamma * (A W^T + b), no re-centring
    sel = torch.arange(0, M, 97)
    ref = x[sel] + gamma.cpu() * (A[sel.cuda()].float().cpu() @ W.float().cpu().t() + b.cpu())
    got = split[0][sel.cuda()].float().cpu() + split[1][sel.cuda()].float().cpu()
    assert (got - ref).abs().max() < 2e-2 and ((got - ref).abs().mean() / ref.abs().mean()) < 5e-4


@pytest.mark.parametrize("variant", [0, 3, 4, 5])
def test_gemm_row_range_statistics_layout_under_every_kernel_family(ops, variant):
    """a row range of a split-residual GEMM (pointers advanced, M = rows of the range, stats_ld = rows of the WHOLE GEMM)
    must write its partial statistics into the [N/64, stats_ld, 2] array whichever kernel family the dispatcher lands on: the
    128-row kernel + split_partials pass (0), the one-barrier 256 x 256 / 256 x 128 kernels (3 / 4) and the 8-phase kernel (5).
    Two ranges of one GEMM == the single launch under the same variant, bit for bit, planes and statistics."""
    import ctypes as C
    from video_depth_anything_amd import _lib
    lib = _lib.lib
    M, N, K = 4608, 512, 256
    m1 = 2560
    epi = _lib.EPI_SCALE_RES_SPLIT
    A, W, b = dev(rnd(M, K, seed=220).to(F16)), dev(rnd(N, K, seed=221, scale=K ** -0.5).to(F16)), dev(rnd(N, seed=222))
    gamma = dev(rnd(N, seed=223).abs() + 0.5)
    x = rnd(M, N, seed=224, scale=2.0)
    stat = dev(torch.stack([rnd(M, seed=225) * 0.1, torch.ones(M)], dim=1).contiguous())

    def planes():
        return dev(x.to(F16)), dev((x - x.to(F16).float()).to(F16)), torch.full((N // 64, M, 2), float("nan"), device="cuda")

    lib.vda_gemm_set_variant(variant)
    try:
        hi, lo, part = planes()
        ops.gemm(A, W, hi, epi, M=M, N=N, K=K, bias=b, gamma=gamma, res=hi, res2=lo, out2=lo, stats=part, pos=stat)
        hi2, lo2, part2 = planes()
        for r0, rows in ((0, m1), (m1, M - m1)):
            ops.gemm(A[r0:], W, hi2[r0:], epi, M=rows, N=N, K=K, bias=b, gamma=gamma, res=hi2[r0:], res2=lo2[r0:], out2=lo2[r0:],
                     stats=part2[0, r0:], pos=stat[r0:], stats_ld=M)
    finally:
        lib.vda_gemm_set_variant(-1)
    assert torch.isfinite(part).all() and torch.isfinite(part2).all(), "unwritten partial statistics"
    for name, u, v in (("hi", hi2, hi), ("lo", lo2, lo), ("partials", part2, part)):
        assert torch.equal(u, v), f"variant {variant} {name}: {int((u != v).sum())} elements differ between two row ranges and one launch"


def test_gemm_dynamic_tile_schedule_is_result_neutral(ops):
    """vda_gemm_args.sched (eight zeroed counters: the 8-phase kernel draws its tiles dynamically) changes which workgroup computes
    which tile, never a result - also when another kernel holds part of the GPU while it runs."""
    from video_depth_anything_amd import _lib
    for (M, N, K, epi) in ((43840, 1024, 1024, _lib.EPI_BIAS_F16), (9000, 3072, 256, _lib.EPI_BIAS_GELU_F16), (700, 256, 128, _lib.EPI_BIAS_F16),
                           (43840, 256, 64, _lib.EPI_BIAS_F16)):
        A, W, b = dev(rnd(M, K, seed=160).to(F16)), dev(rnd(N, K, seed=161, scale=K ** -0.5).to(F16)), dev(rnd(N, seed=162))
        ref = torch.empty(M, N, dtype=F16, device="cuda")
        ops.gemm(A, W, ref, epi, M=M, N=N, K=K, bias=b)
        side = torch.cuda.Stream()
        for hog in (0, 24):
            out = torch.full((M, N), float("nan"), dtype=F16, device="cuda")
            ctr = torch.zeros(8, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            if hog:
                _lib.lib.vda_debug_occupy(hog, 16384, int(2e6), side.cuda_stream)        # ~1 ms on 24 CUs beside the GEMM
            ops.gemm(A, W, out, epi, M=M, N=N, K=K, bias=b, sched=ctr)
            torch.cuda.synchronize()
            assert torch.equal(out, ref), f"M={M} N={N} K={K} hog={hog}: {int((out != ref).sum())} elements differ"
            if M >= 2048 and N >= 192:      # the 8-phase kernel ran: every tile beyond the workgroups' first was drawn from a counter
                tiles = -(-M // 256) * -(-N // 256)
                assert int(ctr.sum()) >= max(0, tiles - 256), (int(ctr.sum()), tiles)


# ---------------------------------------------------------------- norms
@pytest.mark.parametrize("D,rows", [(384, 50), (1024, 37), (128, 9), (64, 130), (192, 21), (256, 10), (2048, 5), (72, 11), (1032, 3)])
def test_layernorm(ops, D, rows):
    x, w, b = rnd(rows, D, seed=32, scale=3.0) + 0.5, rnd(D, seed=33) + 1.0, rnd(D, seed=34)
    out = torch.empty(rows, D, dtype=F16, device="cuda")
    ops.layernorm(dev(x), out, dev(w), dev(b), 1e-6, rows, D)
    close(out, F.layer_norm(x, (D,), w, b, 1e-6), what="layernorm")


def test_layernorm_drop_cls_and_pe(ops):
    D, G, nb = 128, 13, 4
    x, w, b = rnd(nb * G, D, seed=35), rnd(D, seed=36) + 1.0, rnd(D, seed=37)
    out = torch.empty(nb * (G - 1), D, dtype=F16, device="cuda")
    ops.layernorm(dev(x), out, dev(w), dev(b), 1e-6, nb * G, D, group=G, skip=1)
    ref = F.layer_norm(x, (D,), w, b, 1e-6).reshape(nb, G, D)[:, 1:].reshape(-1, D)
    close(out, ref, what="layernorm drop cls")
    T, hw = 4, 6
    x = rnd(T * hw, D, seed=38)
    pe = rnd(T, D, seed=39)
    out = torch.empty(T * hw, D, dtype=F16, device="cuda")
    ops.layernorm(dev(x), out, dev(w), dev(b), 1e-5, T * hw, D, pe=dev(pe), pe_rows_per_step=hw, pe_steps=T)
    ref = F.layer_norm(x, (D,), w, b, 1e-5).reshape(T, hw, D) + pe[:, None]
    close(out, ref.reshape(-1, D), what="layernorm + pe")


@pytest.mark.parametrize("D,G,nb,gamma", [(1024, 13, 5, True), (384, 7, 9, True), (128, 5, 4, False), (256, 5, 3, True)])
def test_layernorm_residual(ops, D, G, nb, gamma):
    """x += gamma * y in place, then LayerNorm(x) (optionally dropping the cls row of every group): both results checked."""
    rows = nb * G
    x, y = rnd(rows, D, seed=90, scale=2.0), rnd(rows, D, seed=91).to(F16)
    g = (rnd(D, seed=92).abs() + 0.5) if gamma else None
    w, b = rnd(D, seed=93) + 1.0, rnd(D, seed=94)
    xs = x + (g if gamma else 1.0) * y.float()
    for group, skip in ((0, 0), (G, 1)):
        xd = dev(x.clone())
        out = torch.full((rows - (nb if group else 0), D), float("nan"), dtype=F16, device="cuda")
        ops.layernorm_residual(xd, dev(y), dev(g) if gamma else None, out, dev(w), dev(b), 1e-6, rows, D, group=group, skip=skip)
        close(xd, xs, rtol=1e-6, atol=1e-6, what="residual stream")
        ref = F.layer_norm(xs, (D,), w, b, 1e-6)
        if group:
            ref = ref.reshape(nb, G, D)[:, 1:].reshape(-1, D)
        close(out, ref, what="layernorm of the updated stream")


@pytest.mark.parametrize("Cc,hw,frames", [(64, 37, 3), (192, 50, 2), (1024, 19, 2), (384, 361, 2)])
def test_groupnorm(ops, Cc, hw, frames):
    x = (rnd(frames, hw, Cc, seed=40, scale=2.0) + 0.7).to(F16)
    w, b = rnd(Cc, seed=41) + 1.0, rnd(Cc, seed=42)
    chunks = min(8, hw)
    part = torch.empty(frames * chunks * 32 * 2, dtype=F32, device="cuda")
    out = torch.empty(frames, hw, Cc, dtype=F16, device="cuda")
    ops.groupnorm(dev(x), out, dev(w), dev(b), 1e-6, frames, hw, Cc, 32, part, chunks)
    ref = F.group_norm(x.float().permute(0, 2, 1), 32, w, b, 1e-6).permute(0, 2, 1)
    close(out, ref, rtol=3e-3, atol=3e-3, what="groupnorm")


# ---------------------------------------------------------------- attention
def attn_ref(qkv, B, N, H):
    q, k, v = qkv.float().reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    a = ((q * 0.125) @ k.transpose(-2, -1)).softmax(dim=-1)
    return (a @ v).transpose(1, 2).reshape(B, N, H * 64)


@pytest.mark.parametrize("variant", [-1, 1, 2, 3, 0, 4, 5, 7, 8, 9, 10, 11])
# (1, 1, 1): one query, three idle waves, every staged row clamped or out of range; (2, 65, 2): the second key tile holds one key;
# (1, 128, 3): exactly one full query block, no tail mask; (3, 129, 1): a second query block with one live query, and six
# workgroups - fewer than the 8 XCDs, so the block remap's remainder branch runs.
@pytest.mark.parametrize("B,N,H", [(2, 13, 2), (1, 64, 1), (2, 200, 3), (1, 1370, 2), (1, 1, 1), (2, 65, 2), (1, 128, 3), (3, 129, 1)])
def test_attention(ops, B, N, H, variant):
    from video_depth_anything_amd._lib import lib
    qkv = rnd(B, N, 3 * H * 64, seed=43, scale=1.5).to(F16)
    out = torch.full((B, N, H * 64), float("nan"), dtype=F16, device="cuda")
    lib.vda_attention_set_variant(variant)
    try:
        ops.attention(dev(qkv), out, B, N, H)
    finally:
        lib.vda_attention_set_variant(-1)
    close(out, attn_ref(qkv, B, N, H), rtol=3e-3, atol=3e-3, what=f"attention variant {variant}")


def test_attention_rejects_unknown_variant(ops):
    """A code the dispatch table does not list is refused - non-zero, vda_last_error() names it - and leaves the variant as it
    was: the next call is bit for bit the default kernel's."""
    from video_depth_anything_amd._lib import lib
    B, N, H = 2, 13, 2
    qkv = dev(rnd(B, N, 3 * H * 64, seed=43, scale=1.5).to(F16))
    ref, out = (torch.full((B, N, H * 64), float("nan"), dtype=F16, device="cuda") for _ in range(2))
    try:
        assert lib.vda_attention_set_variant(-1) == 0
        ops.attention(qkv, ref, B, N, H)
        assert lib.vda_attention_set_variant(6) != 0
        assert b"vda_attention_set_variant: unknown variant 6" in lib.vda_last_error()
        ops.attention(qkv, out, B, N, H)
    finally:
        lib.vda_attention_set_variant(-1)
    assert torch.equal(out, ref)


@pytest.mark.parametrize("H", [16, 6], ids=["vitl", "vits"])
def test_attention_benchmark_grid(ops, H):
    """The encoder attention at the BENCHMARKED grid: 32 frames x 1370 tokens x 16 (ViT-L) / 6 (ViT-S) heads = 512 / 192
    (frame, head) problems, 11 query blocks each; every 7th problem (+ the last) against the fp32 reference, and no output
    element left unwritten."""
    B, N = 32, 1370
    qkv = rnd(B, N, 3 * H * 64, seed=46, scale=1.5).to(F16)
    out = torch.full((B, N, H * 64), float("nan"), dtype=F16, device="cuda")
    ops.attention(dev(qkv), out, B, N, H)
    assert torch.isfinite(out).all()
    o = out.cpu()
    picks = sorted(set(range(0, B * H, 7)) | {B * H - 1})
    q, k, v = qkv.float().reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)      # [B, H, N, 64]
    for t in picks:
        b_, h_ = divmod(t, H)
        a = ((q[b_, h_] * 0.125) @ k[b_, h_].t()).softmax(dim=-1) @ v[b_, h_]
        close(o[b_, :, h_ * 64:(h_ + 1) * 64], a, rtol=3e-3, atol=3e-3, what=f"attention frame {b_} head {h_}")


@pytest.mark.parametrize("variant", [-1, 1, 8, 9, 10, 11])
def test_attention_spiked_scores(ops, variant):
    """Online-softmax rescale path: keys that dominate late in the sequence (guide rule 26), by a lot (far past the lazy
    threshold of the default kernel: 2^6), by a little (inside it: the reference point stays, p grows up to 64) and in
    consecutive tiles (two moves in a row); queries 5 / 40 / 77 sit in different waves, every other query must be untouched."""
    from video_depth_anything_amd._lib import lib
    B, N, H = 1, 300, 1
    qkv = rnd(B, N, 3 * 64, seed=44).to(F16)
    qkv[0, 250, 64:128] = qkv[0, 5, 0:64] * 6.0          # key 250 aligned with query 5: score ~ +48 (log2: +69)
    qkv[0, 130, 64:128] = qkv[0, 40, 0:64] * 0.45        # key 130 with query 40: ~ +3.6 (log2: +5): inside the lazy threshold
    qkv[0, 70, 64:128] = qkv[0, 77, 0:64] * 2.0          # query 77: a move in tile 1 ...
    qkv[0, 140, 64:128] = qkv[0, 77, 0:64] * 4.0         # ... and a bigger one in tile 2
    out = torch.empty(B, N, 64, dtype=F16, device="cuda")
    lib.vda_attention_set_variant(variant)
    try:
        ops.attention(dev(qkv), out, B, N, H)
    finally:
        lib.vda_attention_set_variant(-1)
    close(out, attn_ref(qkv, B, N, H), rtol=3e-3, atol=3e-3, what=f"attention spiked, variant {variant}")


def test_attention_rows_are_position_independent(ops):
    """A query's result may not depend on which wave / lane / workgroup computes it, nor on its neighbours' scores (the lazy
    rescale of the default kernel is decided per lane): the same 137 tokens as frames 0 and 1 of a batch, the second copy
    surrounded by different neighbours in its waves (one extra token in front), must give bit-identical rows."""
    N, H = 137, 2
    a = rnd(N, 3 * H * 64, seed=48, scale=1.5).to(F16)
    qkv = dev(torch.stack([a, a]))
    out = torch.empty(2, N, H * 64, dtype=F16, device="cuda")
    ops.attention(qkv, out, 2, N, H)
    assert torch.equal(out[0], out[1])
    # shift the queries by one row: keys unchanged (same set, rotated), queries land on other lanes
    b = torch.cat([a[-1:], a[:-1]])
    out2 = torch.empty(1, N, H * 64, dtype=F16, device="cuda")
    ops.attention(dev(b[None]), out2, 1, N, H)
    ref = attn_ref(a[None], 1, N, H)[0]
    close(out2[0, 1:], ref[:-1], rtol=3e-3, atol=3e-3, what="rotated sequence")


@pytest.mark.parametrize("variant", [1, 0])
@pytest.mark.parametrize("Cc,T,hw", [(64, 32, 10), (64, 4, 12), (128, 7, 5), (192, 32, 6), (384, 32, 3), (256, 32, 4), (256, 5, 7), (512, 19, 3), (1024, 32, 3),
                                     (1024, 9, 2)])
def test_temporal_attention(ops, Cc, T, hw, variant):
    from video_depth_anything_amd._lib import lib
    heads, d = 8, Cc // 8
    qkv = rnd(T * hw, 3 * Cc, seed=45).to(F16)
    out = torch.full((T * hw, Cc), float("nan"), dtype=F16, device="cuda")
    lib.vda_temporal_attention_set_variant(variant)          # 1: MFMA kernel for d = 32 / 64 / 128, 0: VALU kernel
    try:
        ops.temporal_attention(dev(qkv), out, T, hw, Cc)
    finally:
        lib.vda_temporal_attention_set_variant(1)
    x = qkv.float().reshape(T, hw, 3, heads, d).permute(2, 1, 3, 0, 4)      # [3, hw, heads, T, d]
    a = (x[0] @ x[1].transpose(-1, -2) * d ** -0.5).softmax(dim=-1)
    ref = (a @ x[2]).permute(2, 0, 1, 3).reshape(T * hw, Cc)
    close(out, ref, what="temporal attention")


@pytest.mark.parametrize("Cc,hw", [(1024, 1369), (1024, 361), (256, 1369), (256, 5476), (192, 1369), (384, 361), (64, 1369), (64, 5476)])
def test_temporal_attention_benchmark_grid(ops, Cc, hw):
    """The four motion modules of ViT-L (C = 1024, 1024, 256, 256) and ViT-S (192, 384, 64, 64) at the BENCHMARKED grid: T = 32
    frames, hw = 37^2 / 19^2 / 37^2 / 74^2 pixels (one wave per (pixel, head): up to 43 808 waves), every pixel against the fp32
    reference."""
    T, heads, d = 32, 8, Cc // 8
    qkv = rnd(T * hw, 3 * Cc, seed=47).to(F16)
    out = torch.full((T * hw, Cc), float("nan"), dtype=F16, device="cuda")
    ops.temporal_attention(dev(qkv), out, T, hw, Cc)
    assert torch.isfinite(out).all()
    x = qkv.float().reshape(T, hw, 3, heads, d).permute(2, 1, 3, 0, 4)      # [3, hw, heads, T, d]
    a = (x[0] @ x[1].transpose(-1, -2) * d ** -0.5).softmax(dim=-1)
    ref = (a @ x[2]).permute(2, 0, 1, 3).reshape(T * hw, Cc)
    close(out, ref, what=f"temporal attention C={Cc} hw={hw}")


# ---------------------------------------------------------------- resampling / layout
@pytest.mark.parametrize("h,w_,H,W_", [(19, 19, 37, 37), (5, 7, 10, 14), (8, 6, 8, 6), (3, 4, 42, 56), (10, 14, 5, 7), (11, 9, 5, 4), (7, 8, 3, 8)])
def test_bilinear_nhwc(ops, h, w_, H, W_):
    B, Cc = 2, 64
    x = rnd(B, Cc, h, w_, seed=46).to(F16)
    add = rnd(B, H, W_, Cc, seed=47).to(F16)
    out = torch.empty(B, H, W_, Cc, dtype=F16, device="cuda")
    ops.bilinear_nhwc(dev(x.permute(0, 2, 3, 1).contiguous()), out, B, h, w_, H, W_, Cc, add=dev(add))
    ref = F.interpolate(x.float(), size=(H, W_), mode="bilinear", align_corners=True).permute(0, 2, 3, 1) + add.float()
    close(out, ref, what="bilinear nhwc")


@pytest.mark.parametrize("h,w_,H,W_,B,Cc,with_add", BILINEAR_EDGE_CASES, ids=[bilinear_id(c) for c in BILINEAR_EDGE_CASES])
def test_bilinear_nhwc_edges(ops, h, w_, H, W_, B, Cc, with_add):
    """Mild downsampling (the shared-rows path's third source row), single-row / single-column sources and outputs, channel counts
    whose vectors per pixel do and do not divide the block (C = 192), with and without the `add` operand. One margin pixel behind
    the output must keep its NaN."""
    x = rnd(B, Cc, h, w_, seed=146).to(F16)
    add = rnd(B, H, W_, Cc, seed=147).to(F16) if with_add else None
    out = torch.full((B * H * W_ + 1, Cc), float("nan"), dtype=F16, device="cuda")
    ops.bilinear_nhwc(dev(x.permute(0, 2, 3, 1).contiguous()), out, B, h, w_, H, W_, Cc, add=None if add is None else dev(add))
    assert bool(out[-1].isnan().all()), "wrote past the last output pixel"
    assert bool(torch.isfinite(out[:-1]).all()), "output pixels left unwritten"
    ref = F.interpolate(x.float(), size=(H, W_), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    close(out[:-1].reshape(B, H, W_, Cc), ref + add.float() if with_add else ref, what="bilinear nhwc edges")


@pytest.mark.parametrize("Cc", [32, 192])
def test_bilinear_nhwc_same_size_without_add_is_a_copy(ops, Cc):
    B, h, w_ = 2, 8, 6
    x = rnd(B, h, w_, Cc, seed=148).to(F16)
    out = torch.full((B, h, w_, Cc), float("nan"), dtype=F16, device="cuda")
    ops.bilinear_nhwc(dev(x), out, B, h, w_, h, w_, Cc)
    assert torch.equal(out.cpu(), x), "a same-size resize without add must be exact"


def test_bilinear_plane_and_identity(ops):
    x = rnd(3, 20, 30, seed=48)
    out = torch.empty(3, 45, 50, dtype=F32, device="cuda")
    ops.bilinear_plane(dev(x), out, 3, 20, 30, 45, 50, relu=True)
    ref = F.relu(F.interpolate(x[:, None], size=(45, 50), mode="bilinear", align_corners=True)[:, 0])
    close(out, ref, rtol=1e-5, atol=1e-5, what="bilinear plane")
    out = torch.empty(3, 20, 30, dtype=F32, device="cuda")
    ops.bilinear_plane(dev(x), out, 3, 20, 30, 20, 30)
    assert torch.equal(out.cpu(), x), "identity resize must be exact"


@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
def test_readout_concat(ops, dtype):
    frames, P, D = 3, 7, 128
    tok = rnd(frames * (P + 1), D, seed=95).to(dtype)
    out = torch.full((frames * P, 2 * D), float("nan"), dtype=dtype, device="cuda")
    ops.readout_concat(dev(tok), out, frames, P, D)
    t = tok.reshape(frames, P + 1, D)
    ref = torch.cat((t[:, 1:], t[:, :1].expand(-1, P, -1)), dim=-1).reshape(frames * P, 2 * D)
    assert torch.equal(out.cpu(), ref)


def test_head_out_and_normalize(ops):
    rows, Cp = 1000, 64
    x = rnd(rows, Cp, seed=49).to(F16)
    w = rnd(32, seed=50)
    out = torch.empty(rows, dtype=F32, device="cuda")
    ops.head_out(dev(x), dev(w), 0.3, out, rows, Cp)
    close(out, F.relu(x[:, :32].float() @ w + 0.3), rtol=1e-4, atol=1e-4, what="head out")
    rng = np.random.default_rng(5)
    fr = rng.integers(0, 256, (3, 14, 28, 3), dtype=np.uint8)
    o = torch.empty(3, 3, 14, 28, dtype=F32, device="cuda")
    ops.normalize_u8(torch.from_numpy(fr).cuda(), o, 3, 14, 28)
    ref = ((fr.astype(np.float32) / 255.0 - [0.485, 0.456, 0.406]) / [0.229, 0.224, 0.225]).astype(np.float32).transpose(0, 3, 1, 2)
    np.testing.assert_array_equal(o.cpu().numpy(), ref)


@pytest.mark.parametrize("rows", [1, 63, 1000])
@pytest.mark.parametrize("Cp", [32, 64])
def test_head_out_ignores_pad_channels(ops, Cp, rows):
    """Channels [32, Cpad) hold NaN: only the 32 live ones may reach the result. rows = 1, 63: a partial block of 4-lane groups."""
    x, w = rnd(rows, Cp, seed=149).to(F16), rnd(32, seed=150)
    x[:, 32:] = float("nan")
    out = sentinel_out(rows, 1, 1)
    ops.head_out(dev(x), dev(w), 0.3, out, rows, Cp)
    check_sentinel(out, rows, 1, "head out")
    assert bool(torch.isfinite(out[:rows]).all()), "a pad channel reached the result"
    close(out[:rows, 0], F.relu(x[:, :32].float() @ w + 0.3), rtol=1e-4, atol=1e-4, what="head out")


@pytest.mark.parametrize("Cc,h,w_,H,W_", [(64, 20, 37, 20, 37), (128, 9, 33, 9, 33), (64, 12, 12, 21, 21), (128, 17, 19, 29, 45)])
def test_depth_tail(ops, Cc, h, w_, H, W_):
    """Fused tail vs F.interpolate -> conv3x3 -> relu -> conv1x1 -> relu (same-size = no resize)."""
    B = 2
    x = rnd(B, Cc, h, w_, seed=70).to(F16)
    w2, b2 = rnd(32, Cc, 3, 3, seed=71, scale=(9 * Cc) ** -0.5), rnd(32, seed=72)
    w3, b3 = rnd(32, seed=73, scale=0.3), 0.4
    out = torch.full((B, H, W_), float("nan"), dtype=F32, device="cuda")
    ops.depth_tail(dev(x.permute(0, 2, 3, 1).contiguous()), dev(ops.pack_conv3x3(w2)), dev(b2), dev(w3), b3, out, B, h, w_, H, W_, Cc)
    up = x.float()
    if (h, w_) != (H, W_):
        up = F.interpolate(up, size=(H, W_), mode="bilinear", align_corners=True).to(F16).float()
    y = F.relu(F.conv2d(up, w2.to(F16).float(), b2, padding=1))
    ref = F.relu((y * w3.view(1, 32, 1, 1)).sum(1) + b3)
    close(out, ref, rtol=2e-3, atol=3e-3, what="depth tail")


@pytest.mark.parametrize("Cc,B,h,w_,H,W_", [(32, 2, 12, 12, 21, 21), (64, 3, 40, 50, 70, 88), (128, 2, 17, 19, 29, 45), (128, 8, 92, 92, 161, 161),
                                            (128, 1, 296, 296, 518, 518)])
def test_depth_tail_persistent_equals_v1(ops, Cc, B, h, w_, H, W_):
    """The persistent resizing tail (weights resident in LDS, two patch buffers; more tiles than workgroups in the last two cases)
    against the round-1 kernel: same arithmetic per output pixel, so bit-identical."""
    from video_depth_anything_amd import _lib
    x = dev(rnd(B, h, w_, Cc, seed=74).to(F16))
    w2, b2 = dev(ops.pack_conv3x3(rnd(32, Cc, 3, 3, seed=75, scale=(9 * Cc) ** -0.5))), dev(rnd(32, seed=76))
    w3, b3 = dev(rnd(32, seed=77, scale=0.3)), 0.4
    outs = []
    try:
        for v in (1, 0):
            _lib.lib.vda_depth_tail_set_variant(v)
            out = torch.full((B, H, W_), float("nan"), dtype=F32, device="cuda")
            ops.depth_tail(x, w2, b2, w3, b3, out, B, h, w_, H, W_, Cc)
            outs.append(out)
    finally:
        _lib.lib.vda_depth_tail_set_variant(0)
    assert torch.isfinite(outs[1]).all()
    assert torch.equal(outs[0], outs[1])


def test_gather_normalize_equals_normalize_of_gathered(ops):
    rng = np.random.default_rng(6)
    video = rng.integers(0, 256, (9, 14, 28, 3), dtype=np.uint8)
    idx = [0, 8, 3, 3, 7]
    a = torch.empty(5, 3, 14, 28, dtype=F32, device="cuda")
    ops.gather_normalize_u8(torch.from_numpy(video).cuda(), torch.tensor(idx, dtype=torch.int32, device="cuda"), a, 5, 14, 28)
    b = torch.empty(5, 3, 14, 28, dtype=F32, device="cuda")
    ops.normalize_u8(torch.from_numpy(np.ascontiguousarray(video[idx])).cuda(), b, 5, 14, 28)
    assert torch.equal(a, b)


def test_refusals(ops):
    """Bad geometry is refused with a message, nothing is launched."""
    from video_depth_anything_amd import _lib
    A, W = torch.zeros(8, 96, dtype=F16, device="cuda"), torch.zeros(8, 96, dtype=F16, device="cuda")
    out = torch.zeros(8, 8, dtype=F16, device="cuda")
    with pytest.raises(_lib.VdaError, match="multiple of 64"):
        ops.gemm(A, W, out, _lib.EPI_BIAS_F16, M=8, N=8, K=96)
    with pytest.raises(_lib.VdaError):
        ops.temporal_attention(torch.zeros(40 * 3 * 64, dtype=F16, device="cuda"), torch.zeros(40 * 64, dtype=F16, device="cuda"), 40, 1, 64)


# ---------------------------------------------------------------------------
# device stitcher (video_depth.py:216-254, utils/util.py:40-74) vs the numpy restatement in scheduler.py
# ---------------------------------------------------------------------------
def test_lsq_scale_shift_matches_closed_form():
    from video_depth_anything_amd import ops
    g = torch.Generator(device="cuda").manual_seed(5)
    pred = torch.rand(2, 61, 47, device="cuda", generator=g) * 3 + 0.5
    target = pred * 1.7 - 0.4 + 0.05 * torch.randn(2, 61, 47, device="cuda", generator=g)
    ws = torch.empty(4 * ops.LSQ_BLOCKS, dtype=torch.float64, device="cuda")
    ss = torch.zeros(2, dtype=torch.float32, device="cuda")
    ops.lsq_scale_shift(pred, target, ws, ss)
    p, t = pred.double().cpu().numpy().ravel(), target.double().cpu().numpy().ravel()
    A = np.stack([p, np.ones_like(p)], 1)
    sol = np.linalg.lstsq(A, t, rcond=None)[0]
    np.testing.assert_allclose(ss.cpu().numpy(), sol, rtol=1e-6)
    ss2 = torch.zeros(2, dtype=torch.float32, device="cuda")
    ops.lsq_scale_shift(pred, target, ws, ss2)
    assert torch.equal(ss, ss2), "reduction must be deterministic"
    # degenerate system (constant prediction): det == 0 -> identity, as utils/util.py:56-62
    c = torch.full((2, 8, 8), 2.0, device="cuda")
    ops.lsq_scale_shift(c, c * 3, ws, ss)
    assert ss.cpu().tolist() == [1.0, 0.0]


@pytest.mark.parametrize("n_frames,metric", [(50, False), (50, True), (32, False), (97, False), (23, True)])
def test_device_stitcher_matches_host_stitcher(n_frames, metric):
    from video_depth_anything_amd import scheduler as S
    from video_depth_anything_amd.stitch import stitch_stream
    H0, W0 = 37, 45
    plan = S.plan_windows(n_frames)
    rng = np.random.default_rng(n_frames)
    base = rng.random((H0, W0), dtype=np.float32) * 4 + 1
    wins = []
    for k in range(len(plan)):
        # every window sees the same scene at its own scale/shift plus noise, like real window outputs
        w = base[None] * (1 + 0.1 * rng.standard_normal((32, 1, 1))).astype(np.float32)
        w = (w * (0.6 + 0.3 * k) + 0.2 * k + 0.02 * rng.standard_normal((32, H0, W0))).astype(np.float32)
        wins.append(np.maximum(w, 0))
    ref = S.stitch_windows(wins, n_frames, metric=metric)
    dev = torch.device("cuda")
    got = stitch_stream((torch.from_numpy(w).to(dev) for w in wins), n_frames, H0, W0, dev, metric=metric)
    assert got.shape == ref.shape and got.dtype == np.float32
    if metric:
        assert np.array_equal(got, ref), "metric stitch has no fitted parameters: bit-exact"
    else:
        # scale/shift: fp64 sums on the device vs numpy's fp32 sums in the closed form (its det cancels digits)
        np.testing.assert_allclose(got, ref, rtol=2e-4, atol=2e-4)


# ---------------------------------------------------------------------------
# position independence: a row's result may not depend on which tile / wave / lane / unrolled copy computes it
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("epi_name", ["BIAS_F16", "BIAS_GELU_F16", "SCALE_RES_F32", "SCALE_RES_F32_H"])
def test_gemm_rows_are_position_independent(ops, gemm_variant, epi_name):
    """A = [A1; A1] with 2740 rows per copy (copies sit at different offsets inside the 256-row tiles): both output halves
    must be BIT-identical. Catches per-copy differences in instruction selection (v_fma_mix vs fma + cvt) as well as races."""
    from video_depth_anything_amd import _lib
    epi = getattr(_lib, "EPI_" + epi_name)
    M1, N, K = 2740, 1024, 1024
    A1 = rnd(M1, K, seed=60).to(F16)
    A = dev(torch.cat([A1, A1]).contiguous())
    W = dev(rnd(N, K, seed=61, scale=K ** -0.5).to(F16))
    bias = dev(rnd(N, seed=62))
    kw = dict(M=2 * M1, N=N, K=K, bias=bias)
    if epi_name.startswith("SCALE_RES"):
        r1 = rnd(M1, N, seed=63)
        res = dev(torch.cat([r1, r1]).contiguous())
        kw.update(res=res, gamma=dev(rnd(N, seed=64).abs()))
        out = res if epi_name == "SCALE_RES_F32" else torch.zeros(2 * M1, N, dtype=F16, device="cuda")
    else:
        out = torch.zeros(2 * M1, N, dtype=F16, device="cuda")
    ops.gemm(A, W, out, epi, **kw)
    torch.cuda.synchronize()
    assert torch.equal(out[:M1], out[M1:]), f"{int((out[:M1] != out[M1:]).sum())} elements depend on the row's position"


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("T,hw,C", [(32, 37 * 37, 1024), (32, 19 * 19, 1024), (5, 3 * 4, 64), (32, 37 * 37, 192)])
def test_rope_rotation_of_q_and_k(ops, T, hw, C, dtype):
    """pe='rope' (motion_module/attention.py:403-429): q, k thirds of qkv rotated pairwise by frame * 10000^(-2i/C); v untouched.
    Reference: the complex product in fp64, as precompute_freqs_cis / apply_rotary_emb state it."""
    g = torch.Generator().manual_seed(T * 1000 + C)
    qkv = torch.randn(T * hw, 3 * C, generator=g).to(dtype)
    ref = qkv.double().clone()
    freqs = 1.0 / (10000.0 ** (torch.arange(0, C, 2, dtype=torch.float64)[: C // 2] / C))
    ang = torch.outer(torch.arange(T, dtype=torch.float64), freqs)              # [T, C/2]
    cis = torch.polar(torch.ones_like(ang), ang).repeat_interleave(hw, 0)       # [T*hw, C/2], frame-major rows
    for part in range(2):
        blk = ref[:, part * C:(part + 1) * C].reshape(T * hw, C // 2, 2)
        rot = torch.view_as_real(torch.view_as_complex(blk.contiguous()) * cis).reshape(T * hw, C)
        ref[:, part * C:(part + 1) * C] = rot
    d = qkv.cuda()
    ops.rope_qk(d, T, hw, C)
    out = d.cpu()
    assert torch.equal(out[:, 2 * C:], qkv[:, 2 * C:])
    err = (out.double() - ref).abs().max().item()
    # fp32: sincosf / expf of an angle up to 31 rad; fp16: one rounding of the result (|x| < ~5 -> ulp 4e-3)
    assert err < (3e-5 if dtype == torch.float32 else 2.5e-3), err


@pytest.mark.parametrize("B,h,w,Cin,Cout,ldc", [(2, 9, 11, 64, 32, 32), (1, 20, 37, 128, 64, 64), (2, 21, 19, 256, 128, 128), (1, 5, 3, 64, 24, 32),
                                               (1, 40, 33, 64, 128, 128), (3, 16, 16, 32, 32, 64), (1, 1, 1, 64, 32, 32), (1, 148, 148, 64, 32, 32)])
def test_conv3x3_over_fused_2x_upsample(ops, B, h, w, Cin, Cout, ldc):
    """vda_conv3x3_up2_f16 = output_conv1 over refinenet1's upsample (dpt.py:117, util/blocks.py:156-160) in one kernel:
    (a) against torch: interpolate(scale 2, bilinear, align_corners) in fp32, one rounding to fp16 (what the unfused path stores),
    conv2d in fp32; (b) against the unfused HIP pair vda_bilinear_nhwc_f16 -> vda_gemm_f16(conv3x3) on the same operands: the two
    differ by the fp32 summation order of the conv only."""
    from video_depth_anything_amd import _lib
    x = rnd(B, Cin, h, w, seed=301).to(F16)
    wt, b = rnd(Cout, Cin, 3, 3, seed=302, scale=(9 * Cin) ** -0.5), rnd(Cout, seed=303)
    xin = dev(x.permute(0, 2, 3, 1).contiguous())
    wp = dev(ops.pack_conv3x3(wt))
    H, W_ = 2 * h, 2 * w
    out = torch.full((B, H, W_, ldc), 7.0, dtype=F16, device="cuda")
    ops.conv3x3_up2(xin, wp, dev(b), out, B, h, w, Cin, Cout, ldc)
    up = F.interpolate(x.float(), size=(H, W_), mode="bilinear", align_corners=True).to(F16).float()
    ref = F.conv2d(up, wt.to(F16).float(), b, padding=1).permute(0, 2, 3, 1)
    close(out[..., :Cout], ref, what="conv3x3 over the fused upsample")
    if ldc > Cout:
        assert float((out[..., Cout:].float() - 7.0).abs().max()) == 0.0, "channels past N are not written"
    if (9 * Cin) % 64:
        return                                           # (the implicit GEMM wants K in whole 64-deep tiles)
    upd = torch.empty(B, H, W_, Cin, dtype=F16, device="cuda")
    ops.bilinear_nhwc(xin, upd, B, h, w, H, W_, Cin)
    two = torch.empty(B, H, W_, Cout, dtype=F16, device="cuda")
    ops.gemm(upd, wp, two, _lib.EPI_BIAS_F16, M=B * H * W_, N=Cout, K=9 * Cin, bias=dev(b), conv=(B, H, W_, Cin, H, W_, 1))
    d = (out[..., :Cout].float() - two.float()).abs()
    assert float(d.max()) <= 2.0 ** -9 * max(1.0, float(two.float().abs().max())), float(d.max())      # one fp16 ulp of the largest value
    assert float((d > 0).float().mean()) < 0.12, "the fused and the unfused path agree bit for bit almost everywhere"


def test_conv3x3_fused_upsample_at_the_benchmarked_grid(ops):
    """ViT-L's output_conv1 as the benchmark runs it (32 frames of 148^2 -> 296^2, 256 -> 128 channels: 6080 workgroups, 359 M
    output elements): the fused kernel against the unfused HIP pair at every output (one fp16 ulp; the pair itself is checked
    against torch in test_bilinear_nhwc / test_conv3x3), and against torch's fp32 arithmetic on two sampled frames."""
    from video_depth_anything_amd import _lib
    B, h, C, N = 32, 148, 256, 128
    g = torch.Generator().manual_seed(77)
    x = torch.randn(B, h, h, C, generator=g).to(F16)
    wt, b = torch.randn(N, C, 3, 3, generator=g) * (9 * C) ** -0.5, torch.randn(N, generator=g)
    xin, wp, bd = x.cuda(), dev(ops.pack_conv3x3(wt)), b.cuda()
    H = 2 * h
    out = torch.empty(B, H, H, N, dtype=F16, device="cuda")
    ops.conv3x3_up2(xin, wp, bd, out, B, h, h, C, N, N)
    up = torch.empty(B, H, H, C, dtype=F16, device="cuda")
    ops.bilinear_nhwc(xin, up, B, h, h, H, H, C)
    two = torch.empty(B, H, H, N, dtype=F16, device="cuda")
    ops.gemm(up, wp, two, _lib.EPI_BIAS_F16, M=B * H * H, N=N, K=9 * C, bias=bd, conv=(B, H, H, C, H, H, 1))
    dmax, frac = 0.0, 0.0
    for f in range(B):                                   # frame by frame: the fp32 difference of 359 M elements would be 1.4 GB
        d = (out[f].float() - two[f].float()).abs()
        dmax, frac = max(dmax, float(d.max())), frac + float((d > 0).float().mean()) / B
    assert dmax <= 2.0 ** -9 * max(1.0, float(two.float().abs().max())), dmax
    assert frac < 0.12, frac
    for f in (0, B - 1):
        upf = F.interpolate(x[f:f + 1].permute(0, 3, 1, 2).float(), size=(H, H), mode="bilinear", align_corners=True).to(F16).float()
        ref = F.conv2d(upf, wt.to(F16).float(), b, padding=1).permute(0, 2, 3, 1)
        close(out[f:f + 1], ref, what=f"fused output_conv1, frame {f}")


@pytest.mark.parametrize("M", [43840, 128 * 3 + 37, 50])
def test_mlp_fused_against_the_unfused_pair_and_fp32(ops, M):
    """vda_mlp_fused_f16 (ViT-S widths): x += gamma * (fc2(GELU(fc1(LayerNorm(x)))) + b2) on the split stream in one kernel, hid kept in
    registers (mlp.py:35-41, block.py:105-106). Against (a) the fp32 definition on sampled rows and (b) the unfused pair of GEMM
    launches it replaces (VDA_EPI_LN_GELU_F16 then VDA_EPI_SCALE_RES_SPLIT) on every row: planes to fp16-GEMM accuracy, partial
    statistics consistent with the planes it wrote. M = 43 840 is the benchmarked clip (256 full workgroups + 173 half ones), the small
    sizes have a ragged last workgroup / fewer rows than one workgroup."""
    from video_depth_anything_amd import _lib
    lib = _lib.lib
    D, H = 384, 1536
    assert lib.vda_mlp_fused_supported(D, H) == 1 and lib.vda_mlp_fused_supported(1024, 4096) == 0
    x = rnd(M, D, seed=300, scale=1.5) + rnd(M, 1, seed=301) * 3.0                       # rows with their own offsets
    mean = x.mean(1, keepdim=True)
    xc = x - mean * 0.9                                                                   # the stream is kept NEAR each row's mean, not on it
    hi0, lo0 = xc.to(F16), (xc - xc.to(F16).float()).to(F16)
    s = hi0.float() + lo0.float()
    mu, var = s.mean(1), s.var(1, unbiased=False)
    stats = torch.stack([mu, (var + 1e-6).rsqrt()], 1).contiguous()
    W1, b1 = rnd(H, D, seed=302, scale=D ** -0.5), rnd(H, seed=303, scale=0.1)
    lnw, lnb = 1.0 + rnd(D, seed=304, scale=0.1), rnd(D, seed=305, scale=0.1)
    W2, b2 = rnd(D, H, seed=306, scale=H ** -0.5), rnd(D, seed=307, scale=0.1)
    gamma = rnd(D, seed=308).abs() + 0.5
    Wf, c1, c2 = torch.empty(H, D, dtype=F16, device="cuda"), torch.empty(H, device="cuda"), torch.empty(H, device="cuda")
    ops.fold_ln_weight(dev(W1), dev(b1), dev(lnw), dev(lnb), Wf, c1, c2, H, D)
    W2h = dev(W2.to(F16))
    W2p = torch.empty_like(W2h)
    ops.mlp_permute_w2(W2h, W2p, D, H)
    # (the permutation is what the header says: inside every 32 hidden units, position 8 g + t holds unit 16 (t >> 2) + 4 g + (t & 3))
    k = torch.arange(H)
    src = (k // 32) * 32 + 16 * ((k % 8) // 4) + 4 * ((k // 8) % 4) + (k % 4)
    assert torch.equal(W2p.cpu(), W2h.cpu()[:, src])

    def planes():
        return dev(hi0), dev(lo0), torch.full((D // 64, M, 2), float("nan"), device="cuda")

    hi, lo, part = planes()
    ops.mlp_fused(hi, dev(stats), Wf, c1, c2, W2p, dev(b2), dev(gamma), hi, lo, part, M, D, H)
    hi2, lo2, part2 = planes()
    hid = torch.empty(M, H, dtype=F16, device="cuda")
    ops.gemm(hi2, Wf, hid, _lib.EPI_LN_GELU_F16, M=M, N=H, K=D, bias=c2, gamma=c1, stats=dev(stats))
    ops.gemm(hid, W2h, hi2, _lib.EPI_SCALE_RES_SPLIT, M=M, N=D, K=H, bias=dev(b2), gamma=dev(gamma), res=hi2, res2=lo2, out2=lo2, stats=part2, pos=dev(stats))
    got, two = hi.float() + lo.float(), hi2.float() + lo2.float()
    assert torch.isfinite(got).all() and torch.isfinite(part).all()
    # (a) fp32 definition on sampled rows
    sel = torch.arange(0, M, max(1, M // 300))
    xs = s[sel]
    ln = (xs - xs.mean(1, keepdim=True)) * (xs.var(1, unbiased=False, keepdim=True) + 1e-6).rsqrt() * lnw + lnb
    ref = xs - mu[sel, None] + gamma * (torch.nn.functional.gelu(ln @ W1.t() + b1) @ W2.t() + b2)
    e_f = float((got[sel.cuda()].cpu() - ref).abs().mean() / ref.abs().mean())
    e_u = float((two[sel.cuda()].cpu() - ref).abs().mean() / ref.abs().mean())
    assert e_f < 1.5e-3 and e_f < 1.3 * e_u + 1e-4, (e_f, e_u)
    # (b) every row against the unfused pair (same operands, different summation order)
    assert float((got - two).abs().max()) < 3e-2 and float((got - two).abs().mean() / two.abs().mean()) < 4e-4
    # partial statistics describe the planes the kernel wrote
    blocks = got.view(M, D // 64, 64)
    assert torch.allclose(part[..., 0].t(), blocks.sum(2), rtol=1e-4, atol=2e-3)
    assert torch.allclose(part[..., 1].t(), ((blocks - blocks.mean(2, keepdim=True)) ** 2).sum(2), rtol=2e-3, atol=2e-3)
    # deterministic, and a row's result does not depend on where it sits (rows 0.. of a second call shifted by 16 rows)
    hi3, lo3, part3 = planes()
    ops.mlp_fused(hi3, dev(stats), Wf, c1, c2, W2p, dev(b2), dev(gamma), hi3, lo3, part3, M, D, H)
    assert torch.equal(hi3, hi) and torch.equal(lo3, lo) and torch.equal(part3, part)
    if M > 200:
        sh = 144
        hi4, lo4 = dev(hi0[sh:]), dev(lo0[sh:])
        part4 = torch.empty(D // 64, M - sh, 2, device="cuda")
        ops.mlp_fused(hi4, dev(stats[sh:]), Wf, c1, c2, W2p, dev(b2), dev(gamma), hi4, lo4, part4, M - sh, D, H)
        assert torch.equal(hi4, hi[sh:]) and torch.equal(lo4, lo[sh:])
