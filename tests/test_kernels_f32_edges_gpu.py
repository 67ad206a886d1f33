"""The fp32-operand GEMM and attention kernels at their tile edges.

Everything that is LINEAR in the fp32 GEMM (dense A, conv3x3, ConvTranspose, patch embed, the bias / ReLU / residual / LayerScale
epilogues) is checked with small integer operands against an fp64 reference by torch.equal: while every partial sum stays below
2**24 (tests/_exact.py: assert_exact_safe, asserted for every case here and shown to be sufficient - and the equalities shown to
be able to fail - on the CPU in tests/test_exact_inputs.py) an exact-fp32 MFMA chain must reproduce it bit for bit in any order, so a
wrong row, tap, pad, scatter column or tile is an inequality, not a judgement about a tolerance. Every output is a buffer filled
with one NaN bit pattern, with a margin of rows behind and, where ldc > N, of columns beside the region the kernel owns: nothing
outside may change and nothing inside may be left (check_sentinel).

The rest (GELU, GEGLU, softmax) is real-valued: fp64 reference, rtol = atol = 2e-5 as in tests/test_kernels_f32_gpu.py."""
import functools
import re

import pytest
import torch
import torch.nn.functional as F

import _exact as E
from _exact import check_sentinel, ints, sentinel_out
from test_kernels_f32_gpu import attn_ref, rnd

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU; run them with -m gpu on the MI355X box only")
    from video_depth_anything_amd import ops as o
    return o


def close64(y, ref, rtol=2e-5, atol=2e-5, what=""):
    """|y - ref| <= atol + rtol |ref| against an fp64 reference; a NaN (an element the kernel left, or a pad that leaked) fails."""
    y = y.detach().cpu().double()
    assert y.shape == ref.shape, f"{what}: shape {tuple(y.shape)} vs {tuple(ref.shape)}"
    assert bool(torch.isfinite(y).all()), f"{what}: {int((~torch.isfinite(y)).sum())} non-finite outputs"
    err = (y - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} out of tolerance, max err {float(err.max()):.4g} (ref absmax {float(ref.abs().max()):.4g})"


def exact(y, ref, what):
    y = y.detach().cpu()
    assert y.dtype == F32 and ref.dtype == F64 and y.shape == ref.shape, what
    if not torch.equal(y.double(), ref):
        bad = (y.double() != ref) | y.isnan()
        first = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} elements differ from the exact result, first at {first}: "
                             f"{float(y[tuple(first)])} != {float(ref[tuple(first)])}")


def padded(t, ld, fill=NAN):
    """[rows, n] -> device [rows, ld] with `fill` in the columns [n, ld)."""
    rows, n = t.shape
    o = torch.full((rows, ld), fill, dtype=F32)
    o[:, :n] = t
    return o.cuda()


# ---------------------------------------------------------------- dense A, exact
@functools.lru_cache(maxsize=None)
def dense_data(case):
    M, N, K, lda, ldc = case
    inp = E.dense_inputs(case)
    E.assert_exact_safe(*E.dense_bounds(inp, K))
    d = {k: v.double() for k, v in inp.items()}
    g = {k: v.cuda() for k, v in inp.items()}
    g["res_ld"], g["res2_ld"] = padded(inp["res"], ldc), padded(inp["res2"], ldc)
    return d, g, E.dense_lin(d["A"], d["W"], d["bias"], K)


DENSE_EPIS = ["bias_f32", "bias_f32_no_bias", "bias_f16", "bias_relu", "scale_res_in_place_gamma", "scale_res_h_separate_out", "res",
              "res_res2"]


@pytest.mark.parametrize("epi", DENSE_EPIS)
@pytest.mark.parametrize("case", E.DENSE_CASES, ids=E.dense_id)
def test_gemm_f32_dense_exact(ops, case, epi):
    from video_depth_anything_amd import _lib
    M, N, K, lda, ldc = case
    d, g, lin = dense_data(case)
    kw = dict(M=M, N=N, K=K, lda=lda, ldc=ldc)
    out = sentinel_out(M, N, ldc)
    if epi == "bias_f32":
        ops.gemm(g["A"], g["W"], out, _lib.EPI_BIAS_F32, bias=g["bias"], **kw)
        ref = lin
    elif epi == "bias_f32_no_bias":
        ops.gemm(g["A"], g["W"], out, _lib.EPI_BIAS_F32, **kw)
        ref = lin - d["bias"]
    elif epi == "bias_f16":
        ops.gemm(g["A"], g["W"], out, _lib.EPI_BIAS_F16, bias=g["bias"], **kw)
        ref = lin
    elif epi == "bias_relu":
        ops.gemm(g["A"], g["W"], out, _lib.EPI_BIAS_RELU_F16, bias=g["bias"], **kw)
        ref = F.relu(lin)
    elif epi == "scale_res_in_place_gamma":
        out[:M, :N] = g["res"]
        ops.gemm(g["A"], g["W"], out, _lib.EPI_SCALE_RES_F32, bias=g["bias"], gamma=g["gamma"], res=out, **kw)
        ref = d["res"] + d["gamma"] * lin
    elif epi == "scale_res_h_separate_out":
        ops.gemm(g["A"], g["W"], out, _lib.EPI_SCALE_RES_F32_H, bias=g["bias"], res=g["res_ld"], **kw)
        ref = d["res"] + lin
    elif epi == "res":
        ops.gemm(g["A"], g["W"], out, _lib.EPI_RES_F16, bias=g["bias"], res=g["res_ld"], **kw)
        ref = lin + d["res"]
    else:
        ops.gemm(g["A"], g["W"], out, _lib.EPI_RES_F16, bias=g["bias"], res=g["res_ld"], res2=g["res2_ld"], **kw)
        ref = lin + d["res"] + d["res2"]
    what = f"gemm_f32 {E.dense_id(case)} {epi}"
    check_sentinel(out, M, N, what)
    exact(out[:M, :N], ref, what)


# ---------------------------------------------------------------- dense A, real-valued epilogues
@functools.lru_cache(maxsize=None)
def real_dense(M, N, K, lda, seed):
    A = torch.full((M, lda), NAN, dtype=F32)
    A[:, :K] = rnd(M, K, seed=seed)
    return A, rnd(N, K, seed=seed + 1, scale=K ** -0.5), rnd(N, seed=seed + 2)


@pytest.mark.parametrize("case", E.DENSE_CASES, ids=E.dense_id)
def test_gemm_f32_dense_gelu(ops, case):
    from video_depth_anything_amd import _lib
    M, N, K, lda, ldc = case
    A, W, b = real_dense(M, N, K, lda, 300)
    out = sentinel_out(M, N, ldc)
    ops.gemm(A.cuda(), W.cuda(), out, _lib.EPI_BIAS_GELU_F16, M=M, N=N, K=K, lda=lda, ldc=ldc, bias=b.cuda())
    check_sentinel(out, M, N, "gelu")
    close64(out[:M, :N], F.gelu(A[:, :K].double() @ W.double().t() + b.double()), what=f"gemm_f32 gelu {E.dense_id(case)}")


@pytest.mark.parametrize("M,Cc", [(33, 16), (257, 48)])
def test_gemm_f32_geglu_edges(ops, M, Cc):
    """N = 8 Cc, K = Cc, ldc = 4 Cc: the output region is N / 2 columns wide. Cc = 16: one K step, one column tile; Cc = 48: three
    column tiles of 128 whose value / gate pairs land 64 output columns apart."""
    from video_depth_anything_amd import _lib
    A = rnd(M, Cc, seed=310)
    w, b = rnd(8 * Cc, Cc, seed=311, scale=Cc ** -0.5), rnd(8 * Cc, seed=312)
    wi, bi = ops.pack_geglu(w, b, dtype=F32)
    out = sentinel_out(M, 4 * Cc, 4 * Cc)
    ops.gemm(A.cuda(), wi.cuda(), out, _lib.EPI_GEGLU_F16, M=M, N=8 * Cc, K=Cc, ldc=4 * Cc, bias=bi.cuda())
    check_sentinel(out, M, 4 * Cc, "geglu")
    val, gate = (A.double() @ w.double().t() + b.double()).chunk(2, dim=-1)
    close64(out[:M], val * F.gelu(gate), what=f"geglu Cc={Cc}")


@pytest.mark.parametrize("N", [32, 64, 256], ids=["tile256x32", "tile128x64", "tile128x128"])
def test_gemm_f32_rows_are_position_independent(ops, N):
    """A = [A1; A1], 137 rows per copy: row r and row 137 + r sit in different lanes, waves and (for the 128-row tiles) workgroups,
    and must come out bit-identical - a row's result depends on its operands only."""
    from video_depth_anything_amd import _lib
    R, K = 137, 48
    A1, W, b, res1 = rnd(R, K, seed=320), rnd(N, K, seed=321, scale=K ** -0.5), rnd(N, seed=322), rnd(R, N, seed=323)
    A, res = torch.cat((A1, A1)).cuda(), torch.cat((res1, res1)).cuda()
    for epi, kw in ((_lib.EPI_BIAS_GELU_F16, {}), (_lib.EPI_SCALE_RES_F32_H, dict(res=res))):
        out = sentinel_out(2 * R, N, N)
        ops.gemm(A, W.cuda(), out, epi, M=2 * R, N=N, K=K, bias=b.cuda(), **kw)
        check_sentinel(out, 2 * R, N, f"epilogue {epi}")
        assert torch.equal(out[:R].view(torch.int32), out[R:2 * R].view(torch.int32)), f"epilogue {epi}: the two copies differ"


def test_gemm_f32_refuses_bad_geometry(ops):
    """Every refusal is decided before the launch: the message names the cause and the output is untouched."""
    from video_depth_anything_amd import _lib
    A, W = torch.zeros(8, 32, dtype=F32, device="cuda"), torch.zeros(64, 16, dtype=F32, device="cuda")
    out = sentinel_out(8, 64, 64)
    res = torch.zeros(16, 64, dtype=F32, device="cuda")
    bad = [
        ("lda=12 must be >= K", dict(epi=_lib.EPI_BIAS_F32, N=8, lda=12)),
        ("lda=18 must be >= K and a multiple of 4", dict(epi=_lib.EPI_BIAS_F32, N=8, lda=18)),
        ("N=6 and ldc=8 must be multiples of 4", dict(epi=_lib.EPI_BIAS_F32, N=6, ldc=8)),
        ("relu_in is only built for the conv A operand", dict(epi=_lib.EPI_BIAS_F32, N=8, relu_in=True)),
        ("residual epilogue needs res", dict(epi=_lib.EPI_SCALE_RES_F32, N=8)),
        ("residual epilogue needs res", dict(epi=_lib.EPI_SCALE_RES_F32_H, N=8)),
        ("residual epilogue needs res", dict(epi=_lib.EPI_RES_F16, N=8)),
        ("GEGLU needs N%32==0", dict(epi=_lib.EPI_GEGLU_F16, N=48, ldc=24)),
    ]
    for msg, kw in bad:
        epi = kw.pop("epi")
        with pytest.raises(_lib.VdaError, match=re.escape(msg)):
            ops.gemm(A, W, out, epi, M=8, K=16, **kw)
    torch.cuda.synchronize()
    assert bool((out.view(torch.int32) == E.SENTINEL_BITS).all()), "a refused call wrote to its output"
    ops.gemm(A, W, out, _lib.EPI_RES_F16, M=8, N=64, K=16, lda=32, res=res)      # the same operands, in order: accepted
    check_sentinel(out, 8, 64, "accepted call")


# ---------------------------------------------------------------- conv3x3, exact
@functools.lru_cache(maxsize=None)
def conv_data(case):
    B, H, W, Cin, Cout, stride, relu_in = case
    inp = E.conv_inputs(case)
    a = {k: v.double().abs() for k, v in inp.items()}
    E.assert_exact_safe(E.conv_ref(a["x"], a["w"], a["bias"], stride, False) + a["res"])
    d = {k: v.double() for k, v in inp.items()}
    return inp, d, E.conv_ref(d["x"], d["w"], None, stride, relu_in)


@pytest.mark.parametrize("epi", ["bias_f32", "no_bias", "bias_relu", "res"])
@pytest.mark.parametrize("case", E.CONV_CASES, ids=E.conv_id)
def test_conv3x3_f32_exact(ops, case, epi):
    """ldc = Cout + 4: the margin columns beside every output row must survive too."""
    from video_depth_anything_amd import _lib
    B, H, W, Cin, Cout, stride, relu_in = case
    inp, d, lin = conv_data(case)
    Ho, Wo = E.conv_out_size(H, W, stride)
    M, ldc = B * Ho * Wo, Cout + 4
    x = inp["x"].permute(0, 2, 3, 1).contiguous().cuda()
    w = ops.pack_conv3x3(inp["w"], dtype=F32).cuda()
    kw = dict(M=M, N=Cout, K=9 * Cin, ldc=ldc, relu_in=relu_in, conv=(B, H, W, Cin, Ho, Wo, stride))
    out = sentinel_out(M, Cout, ldc)
    if epi == "bias_f32":
        ops.gemm(x, w, out, _lib.EPI_BIAS_F32, bias=inp["bias"].cuda(), **kw)
        ref = lin + d["bias"]
    elif epi == "no_bias":
        ops.gemm(x, w, out, _lib.EPI_BIAS_F32, **kw)
        ref = lin
    elif epi == "bias_relu":
        ops.gemm(x, w, out, _lib.EPI_BIAS_RELU_F16, bias=inp["bias"].cuda(), **kw)
        ref = F.relu(lin + d["bias"])
    else:
        ops.gemm(x, w, out, _lib.EPI_RES_F16, bias=inp["bias"].cuda(), res=padded(inp["res"].reshape(M, Cout), ldc), **kw)
        ref = lin + d["bias"] + d["res"]
    what = f"conv3x3_f32 {E.conv_id(case)} {epi}"
    check_sentinel(out, M, Cout, what)
    exact(out[:M, :Cout], ref.reshape(M, Cout), what)


# ---------------------------------------------------------------- ConvTranspose, exact
@pytest.mark.parametrize("k", E.CONVT_K)
@pytest.mark.parametrize("case", E.CONVT_CASES, ids=lambda c: "B%d-%dx%d-C%d-Cp%d" % c)
def test_convtranspose_f32_exact(ops, case, k):
    from video_depth_anything_amd import _lib
    B, h, w_, C, Cp = case
    inp = E.convt_inputs(case, k)
    a = {n: v.double().abs() for n, v in inp.items()}
    E.assert_exact_safe(E.convt_ref(a["x"], a["w"], a["bias"], k))
    xin = torch.zeros(B, h, w_, Cp)
    xin[..., :C] = inp["x"].permute(0, 2, 3, 1)
    wp, bp = ops.pack_convt(inp["w"], inp["bias"], Cp, dtype=F32)
    rows = B * h * k * w_ * k
    out = sentinel_out(rows, Cp, Cp)
    ops.gemm(xin.cuda(), wp.cuda(), out, _lib.EPI_CONVT_F16, M=B * h * w_, N=k * k * Cp, K=Cp, ldc=Cp, bias=bp.cuda(), convt=(k, h, w_, Cp))
    what = f"convT k={k} {case}"
    check_sentinel(out, rows, Cp, what)
    y = out[:rows].reshape(B, h * k, w_ * k, Cp)
    exact(y[..., :C], E.convt_ref(inp["x"].double(), inp["w"].double(), inp["bias"].double(), k), what)
    assert bool((y[..., C:] == 0).all()), "pad channels must be exactly 0"


# ---------------------------------------------------------------- patch embed, exact
@pytest.mark.parametrize("case", E.PATCH_CASES, ids=lambda c: "B%d-%dx%d-D%d" % c)
def test_patch_embed_f32_exact(ops, case):
    from video_depth_anything_amd import _lib
    B, H, W, D = case
    P, Kp = (H // 14) * (W // 14), E.PATCH_KPAD
    inp = E.patch_inputs(case)
    a = {n: v.double().abs() for n, v in inp.items()}
    E.assert_exact_safe(E.patch_ref(a["x"], a["w"], a["bias"], a["pos"], a["cls"]))
    x = inp["x"].cuda()

    # patchify alone: columns [0, 588) are the unfolded image, columns [588, Kpad) are the caller's (still NaN), no row past B*P
    raw = sentinel_out(B * P, 588, Kp)
    ops.patchify(x, raw, B, H, W, Kp)
    check_sentinel(raw, B * P, 588, "patchify")
    exact(raw[:B * P, :588], E.unfold14(inp["x"]).double(), "patchify")

    rows = torch.zeros(B * P, Kp, dtype=F32, device="cuda")          # the GEMM reads the pad columns as the caller left them: zeros
    ops.patchify(x, rows, B, H, W, Kp)
    assert bool((rows[:, 588:] == 0).all())
    tok = sentinel_out(B * (P + 1), D, D)
    pos = inp["pos"].cuda()
    ops.gemm(rows, ops.pack_linear(inp["w"].reshape(D, 588), k_pad=Kp, dtype=F32).cuda(), tok, _lib.EPI_PATCH_F32, M=B * P, N=D, K=Kp,
             bias=inp["bias"].cuda(), pos=pos, P=P)
    bits = tok.view(torch.int32)[:B * (P + 1)].reshape(B, P + 1, D)
    assert bool((bits[:, 0] == E.SENTINEL_BITS).all()), "the GEMM epilogue must leave every frame's cls row alone"
    ops.cls_rows(tok, inp["cls"].cuda(), pos, B, P, D)
    check_sentinel(tok, B * (P + 1), D, "patch tokens")
    d = {n: v.double() for n, v in inp.items()}
    exact(tok[:B * (P + 1)].reshape(B, P + 1, D), E.patch_ref(d["x"], d["w"], d["bias"], d["pos"], d["cls"]), f"patch embed {case}")


# ---------------------------------------------------------------- attention
@pytest.mark.parametrize("B,H", [(3, 1), (1, 3), (2, 2)])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 127, 128, 129, 191])
def test_attention_f32_tile_edges(ops, N, B, H):
    """The single key, the partial last key tile (63, 65, 127, 129, 191), the exact tiles (64, 128) and the 128-query block edge;
    3, 4, 6 or 8 workgroups: both arms of the XCD remap (fewer than 8: only the remainder arm; 8: only the quotient)."""
    qkv = rnd(B, N, 3 * H * 64, seed=400 + N, scale=1.5)
    out = sentinel_out(B * N, H * 64, H * 64)
    ops.attention(qkv.cuda(), out, B, N, H)
    check_sentinel(out, B * N, H * 64, "attention f32")
    close64(out[:B * N].reshape(B, N, H * 64), attn_ref(qkv, B, N, H).double(), what=f"attention f32 B={B} N={N} H={H}")


def uniform_qkv(B, N, H, seed):
    qkv = torch.zeros(B, N, 3, H * 64)
    qkv[:, :, 2] = ints((B, N, H * 64), -8, 8, seed)
    return qkv.reshape(B, N, 3 * H * 64)


@pytest.mark.parametrize("N", [1, 64, 128, 65, 129])
def test_attention_f32_uniform_scores_average_the_values(ops, N):
    """q = k = 0: every score is 0, every weight exp2(0) = 1, the row sum is N and the numerator an integer below 2**24 - both exact.
    N a power of two: 1/N and the product are exact, the output IS the mean. N = 65, 129: two roundings (1/N, the product), each
    half an ulp relative at the most: within 2 ulp of the fp64 mean. A key tile masked wrongly adds a clamped copy of the last key
    or drops one: an error of |v| / N, thousands of ulp."""
    B, H = 2, 2
    qkv = uniform_qkv(B, N, H, 500 + N)
    v = qkv.reshape(B, N, 3, H * 64)[:, :, 2].double()
    E.assert_exact_safe(v.abs().sum(dim=1))
    out = sentinel_out(B * N, H * 64, H * 64)
    ops.attention(qkv.cuda(), out, B, N, H)
    check_sentinel(out, B * N, H * 64, "attention f32 uniform")
    y = out[:B * N].reshape(B, N, H * 64).cpu()
    mean = v.mean(dim=1, keepdim=True).expand(B, N, H * 64)
    if N in (1, 64, 128):
        assert torch.equal(y.double(), mean), f"N={N}: max |y - mean| = {float((y.double() - mean).abs().max()):.3g}"
    else:
        ulp = torch.where(mean == 0, torch.zeros_like(mean), torch.exp2(torch.floor(torch.log2(mean.abs().clamp_min(1e-30))) - 23))
        err = (y.double() - mean).abs()
        worst = float((err / ulp.clamp_min(2.0 ** -149)).max())
        print(f"attention f32 uniform N={N}: worst error {worst:.3f} ulp")
        assert bool((err <= 2 * ulp).all()), f"N={N}: {worst:.3f} ulp from the fp64 mean"


def test_attention_f32_bits_do_not_depend_on_batch_slot_or_launch(ops):
    B, N, H = 2, 129, 2
    one = rnd(1, N, 3 * H * 64, seed=520, scale=1.5)
    qkv = one.expand(B, N, 3 * H * 64).contiguous().cuda()
    out, again = sentinel_out(B * N, H * 64, H * 64), sentinel_out(B * N, H * 64, H * 64)
    ops.attention(qkv, out, B, N, H)
    ops.attention(qkv, again, B, N, H)
    check_sentinel(out, B * N, H * 64, "attention f32")
    bits = out.view(torch.int32)
    assert torch.equal(bits[:N], bits[N:2 * N]), "two batch entries with the same qkv differ"
    assert torch.equal(bits, again.view(torch.int32)), "a second launch gave other bits"
