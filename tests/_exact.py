"""Exact-integer inputs and references for the linear surface of the fp32 and fp16 GEMMs (dense, conv3x3, ConvTranspose, patch embed).

With small integer operands every product and every partial sum of a contraction is an integer; while all of them stay below
2**24 they are exactly representable in fp32, so an fp32 fmaf / MFMA chain reproduces the fp64 result BIT FOR BIT in any
summation order. "Which row, which tap, which pad, which column, which tile" then become equalities without a tolerance.
The condition is checked, not assumed: `assert_exact_safe` takes the reference evaluated with |operand| everywhere, which
bounds every partial sum of every ordering.

The case lists and input builders live here so that tests/test_exact_inputs.py (CPU: the inputs meet the condition and the
equalities can fail) and tests/test_kernels_f32_edges_gpu.py (GPU: the kernels meet them) use the same tensors.

The second half does the same for the fp16 GEMM (fp16 operands, fp32 accumulation, fp16 stores: a second condition, see there)
and tests/test_kernels_f16_edges_gpu.py, and lists that file's launches as shapes (f16_launches) for the planner coverage test
in tests/test_gemm_plan.py. Its "tile seams" part restates the persistent kernels' tile walk (tile_walk) and builds the cases that
give a workgroup three tiles under vda_set_max_wgs.

The last part builds inputs whose SOFTMAX is exact - one key that wins by 52 bits, or every weight 1 - for the fp16 attention
kernels and tests/test_attention_edges_gpu.py, with their preconditions (assert_selector_safe, assert_tattn_selector_safe).

The part after that does it for the fused upsample convolutions (conv_up.hip, tail.hip) and tests/test_upsample_edges_gpu.py: constant
images, selector weights with a derived bound, dyadic resize scales; a plain restatement of resize + convolution (fused_emulate) in the
kernels' own operation orders, with the mistakes of FUSED_MUTATIONS built in; replicas of the kernels' source-window arithmetic."""
import functools

import torch
import torch.nn.functional as F

F16, F32, F64 = torch.float16, torch.float32, torch.float64
EXACT_LIMIT = float(2 ** 24)
FP16_EXACT_LIMIT = 2048.0             # every integer up to 2**11 is an fp16 value (every multiple of 2**-j up to 2**(11 - j))
SENTINEL_BITS = 0x7FC5A5A5            # one fixed quiet-NaN bit pattern: never the result of arithmetic on finite inputs
SENTINEL16_BITS = 0x7E5A              # the same for fp16 buffers
NAN = float("nan")


def ints(shape, lo, hi, seed):
    """float32 tensor of seeded integers in [lo, hi]."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(F32)


def assert_exact_safe(*terms):
    """Each term is an fp64 reference evaluated with the absolute value of every operand: it bounds every partial sum of the
    real evaluation in any order. All must be below 2**24 (and integral, or the bound means nothing)."""
    assert terms, "nothing to check"
    for t in terms:
        assert t.dtype == F64, "the bound is evaluated in fp64"
        assert bool((t == t.round()).all()), "operands are not integers"
        top = float(t.abs().max())
        assert top < EXACT_LIMIT, f"partial sums may reach {top:.0f} >= 2**24: fp32 is not exact here"


def sentinel_out(M, N, ldc, extra_rows=8):
    """Device fp32 [M + extra_rows, ldc] holding SENTINEL_BITS everywhere; the kernel is to write [0:M, 0:N] and nothing else."""
    assert 0 < N <= ldc and M > 0 and extra_rows >= 0
    return torch.full((M + extra_rows, ldc), SENTINEL_BITS, dtype=torch.int32, device="cuda").view(F32)


def sentinel_out_f16(M, N, ldc, extra_rows=8):
    """The fp16 twin: device fp16 [M + extra_rows, ldc] holding SENTINEL16_BITS everywhere."""
    assert 0 < N <= ldc and M > 0 and extra_rows >= 0
    return torch.full((M + extra_rows, ldc), SENTINEL16_BITS, dtype=torch.int16, device="cuda").view(F16)


def check_sentinel(buf, M, N, what=""):
    """fp32 or fp16 buffer of sentinel_out / sentinel_out_f16: the pattern is that of the buffer's dtype."""
    bits, pat = (buf.view(torch.int16).cpu(), SENTINEL16_BITS) if buf.dtype == F16 else (buf.view(torch.int32).cpu(), SENTINEL_BITS)
    assert bool((bits[M:] == pat).all()), f"{what}: wrote past the last row ({int((bits[M:] != pat).sum())} elements)"
    assert bool((bits[:M, N:] == pat).all()), f"{what}: wrote into the columns [N, ldc) ({int((bits[:M, N:] != pat).sum())} elements)"
    left = bits[:M, :N] == pat
    assert not bool(left.any()), f"{what}: {int(left.sum())} elements of the output left unwritten"


# ------------------------------------------------------------------------------------------------ dense A
# (M, N, K, lda, ldc): the branch each case is there for
DENSE_CASES = [
    (1, 4, 16, 16, 4),            # M == 1 (every staged row but one is the clamp min(m, M-1)), one K step: no prefetch; N < one 16-row W piece
    (33, 32, 16, 32, 48),         # 256x32 tile, N == BN; lda > K and ldc > N; one K step
    (255, 36, 48, 48, 36),        # N just past 32 -> 128x64 tile with a 4-column remainder; M one short of two tiles
    (257, 68, 64, 80, 72),        # N just past 64 -> 128x128 tile; M one past two tiles; lda > K, ldc > N
    (129, 132, 32, 32, 132),      # N just past 128 -> second column tile holds 4 live columns; two K steps: one prefetch
    (384, 256, 1536, 1536, 256),  # no partial tile anywhere, the longest K of the model (96 K steps): the double buffer's steady state
    (1100, 260, 16, 16, 260),     # 9 x 3 = 27 tiles: the XCD remap with q = 3, r = 3 takes both arms; partial tile on both axes
]


def dense_id(c):
    return "M%d-N%d-K%d-lda%d-ldc%d" % c


def dense_inputs(case):
    """A [M, lda] with NaN in the columns [K, lda) (they must not reach the output), W [N, K], bias / gamma [N], res / res2 [M, N]."""
    M, N, K, lda, ldc = case
    s = 1000 + 17 * DENSE_CASES.index(case)
    A = torch.full((M, lda), NAN, dtype=F32)
    A[:, :K] = ints((M, K), -3, 3, s)
    return dict(A=A, W=ints((N, K), -6, 6, s + 1), bias=ints((N,), -4, 4, s + 2), gamma=ints((N,), -4, 4, s + 3),
                res=ints((M, N), -4, 4, s + 4), res2=ints((M, N), -4, 4, s + 5))


def dense_lin(A, W, bias, K):
    """A[:, :K] W^T + bias in the dtype of A."""
    return A[:, :K] @ W.t() + bias


def dense_bounds(inp, K):
    """|operand| references for every dense epilogue of the exact list: their maximum bounds every partial sum."""
    d = {k: v.double().abs() for k, v in inp.items()}
    lin = dense_lin(d["A"], d["W"], d["bias"], K)
    return lin, d["res"] + d["gamma"] * lin, lin + d["res"] + d["res2"]


# ------------------------------------------------------------------------------------------------ conv3x3
# (B, H, W, Cin, Cout, stride, relu_in)
CONV_CASES = [
    (1, 1, 1, 16, 4, 1, False),       # M == 1: eight of the nine taps are padding
    (1, 2, 3, 16, 32, 2, False),      # even H at stride 2 (the last window row is one real row + pad), 256x32 tile
    (2, 8, 10, 32, 36, 2, True),      # even H and W at stride 2, relu_in, N just past 32, two frames
    (3, 9, 11, 64, 64, 1, True),      # 128x64 tile, M = 297 = 2 tiles + 41, windows cross frame borders inside a tile
    (1, 5, 5, 16, 132, 1, False),     # N just past 128
    (1, 40, 33, 16, 32, 1, False),    # the fp32 depth tail's conv: 256x32 tile, M = 1320 = 5 tiles + 40 (six tiles)
]


def conv_id(c):
    return "B%d-%dx%d-Cin%d-Cout%d-s%d-relu%d" % (c[:6] + (int(c[6]),))


def conv_out_size(H, W, stride):
    return (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1


def conv_inputs(case):
    """x NCHW in [-3, 3] (negative values make relu_in matter), w [Cout, Cin, 3, 3] in [-2, 2], bias [Cout] and res NHWC in [-4, 4]."""
    B, H, W, Cin, Cout, stride, _ = case
    s = 2000 + 17 * CONV_CASES.index(case)
    Ho, Wo = conv_out_size(H, W, stride)
    return dict(x=ints((B, Cin, H, W), -3, 3, s), w=ints((Cout, Cin, 3, 3), -2, 2, s + 1), bias=ints((Cout,), -4, 4, s + 2),
                res=ints((B, Ho, Wo, Cout), -4, 4, s + 3))


def conv_ref(x, w, bias, stride, relu_in):
    """F.conv2d(padding=1) -> NHWC, in the dtype of x."""
    xi = F.relu(x) if relu_in else x
    return F.conv2d(xi, w, bias, stride=stride, padding=1).permute(0, 2, 3, 1)


def conv_by_taps(x, w, bias, stride, relu_in, shift_tap=None, clamp_pad=False):
    """The same convolution as nine shifted 1x1 products. shift_tap = (ky, kx): that tap reads one pixel to the right of where it
    should; clamp_pad: the border repeats the edge pixel where the convolution pads with zeros."""
    xi = F.relu(x) if relu_in else x
    B, Cin, H, W = xi.shape
    Ho, Wo = conv_out_size(H, W, stride)
    xp = F.pad(xi, (2, 2, 2, 2))
    if clamp_pad:
        xp[:, :, 1:H + 3, 1:W + 3] = F.pad(xi, (1, 1, 1, 1), mode="replicate")
    out = torch.zeros(B, Ho, Wo, w.shape[0], dtype=x.dtype)
    for ky in range(3):
        for kx in range(3):
            dx = 1 if shift_tap == (ky, kx) else 0
            win = xp[:, :, 1 + ky:1 + ky + stride * (Ho - 1) + 1:stride, 1 + kx + dx:1 + kx + dx + stride * (Wo - 1) + 1:stride]
            out += torch.einsum("bchw,oc->bhwo", win, w[:, :, ky, kx])
    return out if bias is None else out + bias


# ------------------------------------------------------------------------------------------------ ConvTranspose (kernel == stride)
# (B, h, w, C, Cp), each with k in CONVT_K
CONVT_CASES = [
    (1, 1, 1, 12, 16),       # M == 1, one K step, pad channels 12..15
    (3, 3, 2, 20, 32),       # three frames: the scatter's frame / row / column decomposition, pad channels 20..31
]
CONVT_K = [2, 4]


def convt_inputs(case, k):
    B, h, w, C, Cp = case
    s = 3000 + 17 * CONVT_CASES.index(case) + k
    return dict(x=ints((B, C, h, w), -3, 3, s), w=ints((C, C, k, k), -2, 2, s + 1), bias=ints((C,), -4, 4, s + 2))


def convt_ref(x, w, bias, k):
    """F.conv_transpose2d(stride=k) -> NHWC [B, h*k, w*k, C]."""
    return F.conv_transpose2d(x, w, bias, stride=k).permute(0, 2, 3, 1)


# ------------------------------------------------------------------------------------------------ patch embed
# (B, H, W, D)
PATCH_CASES = [
    (1, 14, 14, 36),         # P = 1: every GEMM row is a frame of its own, N just past 32
    (2, 28, 42, 132),        # P = 6, two frames: the row -> (frame, patch) split of the epilogue, N just past 128
]
PATCH_KPAD = 640


def patch_inputs(case):
    B, H, W, D = case
    s = 4001 + 17 * PATCH_CASES.index(case)       # (seed 4000 has a zero at pixel (0, 0, 0) of the P = 1 case: a dropped k = 0 went unseen)
    P = (H // 14) * (W // 14)
    return dict(x=ints((B, 3, H, W), -3, 3, s), w=ints((D, 3, 14, 14), -3, 3, s + 1), bias=ints((D,), -3, 3, s + 2),
                pos=ints((P + 1, D), -3, 3, s + 3), cls=ints((D,), -3, 3, s + 4))


def unfold14(x):
    """[B, 3, H, W] -> [B * P, 588], column = c * 196 + ky * 14 + kx: the A matrix of the patch-embed GEMM."""
    return F.unfold(x, kernel_size=14, stride=14).transpose(1, 2).reshape(-1, 588)


def patch_ref(x, w, bias, pos, cls):
    """Tokens [B, P + 1, D]: cls + pos[0] first, then conv(stride 14) + pos[1:]."""
    B, D = x.shape[0], w.shape[0]
    tok = F.conv2d(x, w, bias, stride=14).flatten(2).transpose(1, 2)
    return torch.cat((cls.expand(B, 1, D), tok), dim=1) + pos


# ------------------------------------------------------------------------------------------------ bilinear_nhwc edge geometries
# Shared by the fp16 and fp32 kernel files (real-valued, each file's own tolerance): (h, w, H, W, B, C, with_add).
# C = 192: 256 is no multiple of C / 8, the per-element index path; C = 32: the fp32 depth tail's width; add None: the forward's helper.
BILINEAR_EDGE_CASES = [
    (10, 14, 7, 9, 2, 32, False), (10, 14, 7, 9, 2, 192, True), (10, 14, 7, 9, 2, 128, True),      # scale 1.5: the third source row r2
    (6, 7, 14, 14, 2, 32, True), (6, 7, 14, 14, 2, 192, False), (6, 7, 14, 14, 2, 256, False),     # the tail chain's upsample
    (5, 5, 1, 1, 2, 32, False), (5, 5, 1, 1, 2, 192, True),                                        # H == W == 1: scale 0, one-row block
    (1, 1, 4, 6, 2, 192, False), (1, 1, 4, 6, 2, 128, True), (1, 1, 4, 6, 2, 32, True),            # h == w == 1: every source row is row 0
    (3, 4, 5, 1, 2, 256, True), (3, 4, 5, 1, 2, 32, False), (3, 4, 5, 1, 2, 192, False),           # W == 1, odd H
    (19, 19, 37, 37, 1, 192, True), (19, 19, 37, 37, 1, 32, False), (19, 19, 37, 37, 1, 256, True),  # more (X, vector) pairs than threads
]


def bilinear_id(c):
    return "%dx%d-%dx%d-B%d-C%d-%s" % (c[:6] + ("add" if c[6] else "noadd",))


# ================================================================================================ the fp16 GEMM (gemm.hip and its tile families)
# fp16 operands, fp32 accumulation, most outputs fp16. Two conditions make the fp64 reference the only admissible result:
#   1. every partial sum of every ordering stays below 2**24 (as above: the |operand| reference bounds them), and
#   2. every value a kernel STORES as fp16 or reads back as fp16 (outputs, fp16 residuals, the hi plane of the split epilogue) is a
#      multiple of `step` with |v| <= 2048 * step in the real reference: an fp16 value, so the one final rounding is exact too (and
#      the lo plane of the split epilogue, fp16(x - hi), is exactly 0).
# Operands are small integers (exact in fp16); the LayerNorm-folded epilogue multiplies by rstd in {0.5, 1, 2}: step = 0.5 there.
EPI = dict(BIAS_F16=0, BIAS_GELU_F16=1, BIAS_RELU_F16=2, SCALE_RES_F32=3, RES_F16=4, GEGLU_F16=5, PATCH_F32=6, CONVT_F16=7, BIAS_F32=8,
           SCALE_RES_F32_H=9, SCALE_RES_SPLIT=10, LN_BIAS_F16=11, LN_GELU_F16=12)          # include/vda.h (test_exact_inputs.py holds them to _lib)
# vda_gemm_set_variant values: the parameters of test_kernels_gpu.py's gemm_variant fixture
VARIANTS16 = [-1, 0, 1, 2, 3, 4, 5, 7, 9, 8, 5 + 16 * 64, 10, 11]
NO_LARGE_TILE = (-1, 0, 7)       # variants that force no large tile (7 forces the LDS conv; dense A stays on the 128-row kernel under it)


def assert_exact_safe_f16(bounds, outputs_f16, step=1.0):
    """bounds: |operand| references (fp64) as for assert_exact_safe, in units of `step`; outputs_f16: the REAL references (fp64) of
    everything stored or re-read as fp16: multiples of step, at most 2048 steps from zero."""
    assert_exact_safe(*[b / step for b in bounds])
    assert outputs_f16, "nothing stored as fp16 to check"
    for v in outputs_f16:
        assert v.dtype == F64
        u = v / step
        assert bool((u == u.round()).all()), f"not a multiple of {step}"
        top = float(u.abs().max())
        assert top <= FP16_EXACT_LIMIT, f"|value| reaches {top:.0f} steps of {step} > 2048: its fp16 rounding is not exact"
        assert torch.equal(v.to(F16).double(), v)


def guarded(t, rows_after=8, pad_elems=0):
    """A host tensor as a device view of a larger allocation that holds NaN everywhere else: rows_after rows (elements, for a
    vector) behind it, and at least pad_elems elements on EITHER side (a conv input: (W + 2) * Cin, one padded image row). The
    view starts 16-byte aligned. A clamp or a bound that is off by one then reads a NaN, not a harmless zero or a neighbour."""
    assert t.is_floating_point() and not t.is_cuda
    unit = 16 // t.element_size()
    front = -(-pad_elems // unit) * unit
    back = max(rows_after * (t.shape[-1] if t.dim() >= 2 else 1), pad_elems)
    n = t.numel()
    buf = torch.full((front + n + back,), NAN, dtype=t.dtype, device="cuda")
    buf[front:front + n] = t.reshape(-1).cuda()
    v = buf[front:front + n].view(t.shape)
    assert v.data_ptr() % 16 == 0 and v.is_contiguous()
    return v


def pad_cols(t, ld, dtype):
    """[rows, n] -> host [rows, ld] of dtype with NaN in the columns [n, ld)."""
    rows, n = t.shape
    o = torch.full((rows, ld), NAN, dtype=dtype)
    o[:, :n] = t.to(dtype)
    return o


# ------------------------------------------------------------------------------------------------ dense A
# (M, N, K, lda, ldc): K % 64 == 0, lda % 8 == 0; N % 8 == 0 and ldc % 8 == 0 except in the last case
DENSE16_CASES = [
    (1, 8, 64, 64, 8),               # M == 1 (every staged row but one is the clamp), N below every tile width, one K step: no steady state in any pipeline
    (129, 72, 128, 136, 80),         # M one past a 128-row tile, N one 8-column segment past 64, lda > K, ldc > N
    (191, 128, 192, 192, 128),       # one short of a 192-row tile, three K steps
    (193, 136, 192, 200, 136),       # one past it, N one segment past 128
    (255, 256, 64, 64, 256),         # one short of a 256-row tile
    (257, 264, 320, 320, 272),       # one past it, N one segment past 256, five K steps: the 8-phase kernel's A slots (3) and W slots (2) out of phase
    (385, 384, 448, 448, 384),       # the 192 x 384 tile exactly (variant 10), seven K steps
    (383, 392, 64, 72, 392),         # one segment past it: N % 384 != 0, variant 10 falls through to 256 x 128
    (513, 768, 1536, 1536, 768),     # the model's longest K (24 steps), two column tiles of 384, three of 256
    (130, 36, 64, 64, 36),           # N % 8 != 0: the 128-row kernel's 4-column stores; every forced large tile must refuse it
]


def dense16_inputs(case):
    """Integer operands as fp32 host tensors (each is its own fp16 rounding). A [M, K] in [-3, 3] ({-1, 0, 1} where K >= 448), W in
    [-2, 2]; bias, res, res2 in [-4, 4]; gamma, ln_w, ln_b, mean in [-2, 2]; rstd in {0.5, 1, 2}. (K >= 448: ln_w in {-1, 0, 1} too - with [-2, 2] the LayerNorm-folded
    reference of the K = 1536 case reaches 1475 = 2950 half-steps, past what fp16 holds at a step of 0.5.)
    A seam case (below) is narrowed at every K it has, 320 and 576: it has a million outputs and more where DENSE16_CASES' K = 320 case has 68 000,
    and with A in [-3, 3] and ln_w in [-2, 2] the LayerNorm-folded reference of the first one (M = 4827, N = 256, K = 320) reaches 2124 half-steps - the
    tail of that many sums, which no other seed would cut."""
    M, N, K, lda, ldc = case
    seam = case not in DENSE16_CASES
    s = seam16_seed(case) if seam else 5000 + 17 * DENSE16_CASES.index(case)
    a = 1 if K >= 448 or seam else 3
    rstd = torch.tensor([0.5, 1.0, 2.0])[ints((M,), 0, 2, s + 9).long()]
    return dict(A=ints((M, K), -a, a, s), W=ints((N, K), -2, 2, s + 1), bias=ints((N,), -4, 4, s + 2), gamma=ints((N,), -2, 2, s + 3),
                res=ints((M, N), -4, 4, s + 4), res2=ints((M, N), -4, 4, s + 5), ln_w=ints((K,), -a if a == 1 else -2, a if a == 1 else 2, s + 6), ln_b=ints((K,), -2, 2, s + 7),
                mean=ints((M,), -2, 2, s + 8), rstd=rstd)


def fold_ln(d):
    """vda_fold_ln_weight in the dtype of d: Wf = W * ln_w, c1 = row sums of Wf, c2 = bias + W ln_b."""
    Wf = d["W"] * d["ln_w"]
    return Wf, Wf.sum(1), d["bias"] + d["W"] @ d["ln_b"]


def dense16_refs(d):
    """Every exact dense epilogue's reference in the dtype of d (fp64 from the tests; fp32 to show the two agree)."""
    lin = d["A"] @ d["W"].t() + d["bias"]
    Wf, c1, c2 = fold_ln(d)
    stream = d["res"] + d["res2"] + d["gamma"] * lin            # the split epilogue: (hi + lo) + gamma * (A W^T + b)
    r = dict(bias_f16=lin, bias_f16_no_bias=lin - d["bias"], bias_f32=lin, bias_relu=F.relu(lin), scale_res_in_place_gamma=d["res"] + d["gamma"] * lin,
             scale_res_h_separate_out=d["res"] + lin, res=lin + d["res"], res_res2=lin + d["res"] + d["res2"],
             ln_bias=d["rstd"][:, None] * (d["A"] @ Wf.t() - d["mean"][:, None] * c1) + c2)
    if d["W"].shape[0] % 64 == 0:
        r.update(split=stream, split_pos=stream - d["mean"][:, None])
    return r


DENSE16_F32_OUT = ("bias_f32", "scale_res_in_place_gamma")       # every other exact dense epilogue stores fp16


def dense16_check(inp):
    """Both conditions for every exact epilogue of one case; returns the fp64 references."""
    d = {k: v.double() for k, v in inp.items()}
    a = {k: v.abs() for k, v in d.items()}
    ra, r = dense16_refs(a), dense16_refs(d)
    ln_a, ln = ra.pop("ln_bias"), r["ln_bias"]
    stored = [v for k, v in r.items() if k not in DENSE16_F32_OUT and k != "ln_bias"]
    assert_exact_safe_f16(list(ra.values()), stored + [d["res"], d["res2"]])
    assert_exact_safe_f16([ln_a], [ln], step=0.5)
    return r


# lda == 0, the broadcast row of vda.h: every output row is row 0's result. (M, N, K)
BROADCAST16_CASES = [(300, 136, 128)]


# The persistent kernels' tile order (K = 64: a few milliseconds each). M from the CU count so that 256-row tiles number ncu plus a few:
# one full round and a short last one.  N = 2048: nbn = 8, the L2-blocked walk (it needs a full round); N = 1024: nbn = 4, the last
# partial round dealt by row panel (per_xcd % nbn == 0); N = 768: nbn = 3, the plain mapping with a partial last round.
WALK16_N = [2048, 1024, 768]
# 8 (192 x 128) and 11 (the same, two workgroups per CU): M comes from the CU count in 256-row tiles, so 192-row tiles number more and both have
# more tiles than workgroups too. Not 10: at N = 768 its 192 x 384 tiles number 116 x 2 = 232, fewer than the 256 workgroups, and 384 does not
# divide the other two widths, where it plans variant 4's 256 x 128 tile. (The seam cases below walk the 192 x 384 tile on a capped grid.)
WALK16_VARIANTS = [-1, 3, 4, 5, 9, 5 + 16 * 64, 8, 11]


def walk16_case(ncu, N):
    rt = -(-(ncu + 5) // (N // 256))
    return (256 * rt - 37, N, 64)


def split16_case(ncu):
    """The smallest kind of shape the automatic path row-splits (plan_split in gemm.hip): K = 4096, one round of 256-row tiles over
    nbn = 8 column tiles + 2049 rows on 192-row tiles."""
    return (256 * (ncu // 8) + 2049, 2048, 4096)


def walk16_inputs(case, seed=5900):
    M, N, K = case
    a = 1 if K >= 448 else 3
    return dict(A=ints((M, K), -a, a, seed + N), W=ints((N, K), -2, 2, seed + N + 1), bias=ints((N,), -4, 4, seed + N + 2))


# ------------------------------------------------------------------------------------------------ patch embed / ConvTranspose epilogues (dense A)
# (frames, P, N, K, ldc): M = frames * P rows scatter to frames * (P + 1) token rows, row 0 of each frame left to vda_cls_rows
PATCH16_CASES = [(130, 1, 72, 128, 72), (130, 1, 136, 128, 144), (43, 6, 72, 128, 80), (43, 6, 136, 128, 136)]


def patch16_inputs(case):
    fr, P, N, K, ldc = case
    s = 6000 + 17 * (PATCH16_CASES + SEAM_PATCH16_CASES).index(case)
    return dict(A=ints((fr * P, K), -3, 3, s), W=ints((N, K), -2, 2, s + 1), bias=ints((N,), -4, 4, s + 2), pos=ints((P + 1, N), -4, 4, s + 3))


def patch16_ref(d, P):
    """[frames, P, N]: the rows 1.. of each frame's tokens."""
    N = d["W"].shape[0]
    return (d["A"] @ d["W"].t() + d["bias"]).reshape(-1, P, N) + d["pos"][1:]


# (B, h, w, C, Cp), each with k in CONVT_K: K = Cp must be a multiple of 64 here; channels C..Cp-1 are the pad channels
CONVT16_CASES = [
    (1, 1, 1, 48, 64),       # M == 1
    (3, 3, 2, 40, 64),       # three frames: the scatter's frame / row / column decomposition
]


def convt16_inputs(case, k):
    B, h, w, C, Cp = case
    s = 6501 + 17 * (CONVT16_CASES + SEAM_CONVT16_CASES).index(case) + k          # (seed 6500 has a zero in the last input channel of the 1 x 1 case, k = 4: a dropped k = C - 1 went unseen)
    return dict(x=ints((B, C, h, w), -3, 3, s), w=ints((C, C, k, k), -2, 2, s + 1), bias=ints((C,), -4, 4, s + 2))


# ------------------------------------------------------------------------------------------------ conv3x3
# (B, H, W, Cin, Cout, stride, relu_in, ldc)
CONV16_CASES = [
    (1, 1, 1, 64, 8, 1, False, 8),          # M == 1: eight of the nine taps are padding
    (1, 2, 3, 64, 32, 2, False, 32),        # even H at stride 2: the last window row is one real row + pad
    (2, 8, 10, 64, 72, 2, True, 80),        # even H and W at stride 2, relu_in, N one segment past 64, ldc > N
    (3, 9, 11, 64, 64, 1, True, 64),        # windows cross frame borders inside a tile; the C = 64 persistent LDS kernel's shape
    (1, 5, 5, 128, 136, 1, False, 136),     # N one segment past 128, two K steps per tap
    (1, 17, 33, 64, 24, 1, False, 32),      # the per-pass LDS kernel, Cout no multiple of 32; H = 2 TH + 1, W = TW + 1 (conv_lds.hip: TH = 8, TW = 32)
    (2, 20, 37, 192, 256, 1, True, 256),    # three K steps per tap, a full 256-wide tile
]
CONV16_EPIS = ["bias_f16", "no_bias", "bias_relu", "res", "res_res2"]      # BIAS_F16, BIAS_RELU_F16, RES_F16: what the conv families are built for


def conv16_id(c):
    return "B%d-%dx%d-Cin%d-Cout%d-s%d-relu%d-ldc%d" % (c[:6] + (int(c[6]), c[7]))


def conv16_inputs(case):
    B, H, W, Cin, Cout, stride, _, _ = case
    s = 7000 + 17 * (CONV16_CASES + SEAM_CONV16_CASES).index(case)
    Ho, Wo = conv_out_size(H, W, stride)
    return dict(x=ints((B, Cin, H, W), -3, 3, s), w=ints((Cout, Cin, 3, 3), -2, 2, s + 1), bias=ints((Cout,), -4, 4, s + 2),
                res=ints((B, Ho, Wo, Cout), -4, 4, s + 3), res2=ints((B, Ho, Wo, Cout), -4, 4, s + 4))


def conv16_refs(d, stride, relu_in):
    lin = conv_ref(d["x"], d["w"], None, stride, relu_in)
    b = d["bias"]
    return dict(bias_f16=lin + b, no_bias=lin, bias_relu=F.relu(lin + b), res=lin + b + d["res"], res_res2=lin + b + d["res"] + d["res2"])


def conv16_check(case, inp):
    d = {k: v.double() for k, v in inp.items()}
    a = {k: v.abs() for k, v in d.items()}
    r = conv16_refs(d, case[5], case[6])
    assert_exact_safe_f16([conv16_refs(a, case[5], False)["res_res2"]], list(r.values()) + [d["res"], d["res2"]])
    return r


# ------------------------------------------------------------------------------------------------ depth tail, identity resize (h == H, w == W)
# (B, H, W) x C: conv3x3(C -> 32) + ReLU + conv1x1(32 -> 1) + ReLU; fp32 between the two convolutions and out (tail.hip), so only 2**24 applies
TAIL16_CASES = [(1, 1, 1), (2, 5, 7), (1, 33, 65)]
TAIL16_C = [64, 128]


def tail16_inputs(case, Cc):
    B, H, W = case
    s = 8002 + 17 * TAIL16_CASES.index(case) + Cc          # (seeds 8000 and 8001 leave the 1 x 1 image's only output at 0 after the last ReLU: nothing to see)
    return dict(x=ints((B, Cc, H, W), -3, 3, s), w2=ints((32, Cc, 3, 3), -2, 2, s + 1), b2=ints((32,), -4, 4, s + 2), w3=ints((32,), -2, 2, s + 3),
                b3=float(ints((1,), -4, 4, s + 4)))


def tail16_ref(d, b3):
    y = F.relu(F.conv2d(d["x"], d["w2"], d["b2"], padding=1))
    return F.relu((y * d["w3"].view(1, 32, 1, 1)).sum(1) + b3)


# ------------------------------------------------------------------------------------------------ what the GPU file launches, as shapes
def gemm16_fields(M, N, K, epi, lda=None, ldc=None, conv=None, convt=None, P=0, relu_in=False, tile_rows=0):
    """The shape fields ops.gemm gives vda_gemm_args for these keywords: what vda_gemm_plan reads."""
    f = dict(M=M, N=N, K=K, lda=K if lda is None else lda, ldc=N if ldc is None else ldc, a_mode=0 if conv is None else 1, epilogue=epi,
             relu_in=int(relu_in), P=P, tile_rows=tile_rows)
    if conv is not None:
        f.update(zip(("cB", "cH", "cW", "cCin", "cHo", "cWo", "cStride"), conv))
    if convt is not None:
        f.update(zip(("tK", "tH", "tW", "tCout"), convt))
    return f


def plan16(L, fields, ncu=0, sched=False):
    """(rc, records) of vda_gemm_plan as vda_gemm_f16 itself plans the call (ncu = 0: the current device's)."""
    import ctypes as C
    a = L.GemmArgs(**fields)
    if sched:
        a.sched = 64                 # "set": the planner never follows it
    p = L.GemmPlan()
    rc = L.lib.vda_gemm_plan(C.byref(a), 0, ncu, 0, C.byref(p))
    return rc, ([p.rec[i] for i in range(p.n)] if rc == 0 else [])


DENSE16_EXACT = ["bias_f16", "bias_f16_no_bias", "bias_f32", "bias_relu", "scale_res_in_place_gamma", "scale_res_h_separate_out", "res", "res_res2",
                 "ln_bias", "split", "split_pos"]
DENSE16_REAL = ["gelu", "geglu", "ln_gelu"]
EPI_OF = dict(bias_f16="BIAS_F16", bias_f16_no_bias="BIAS_F16", bias_f32="BIAS_F32", bias_relu="BIAS_RELU_F16", scale_res_in_place_gamma="SCALE_RES_F32",
              scale_res_h_separate_out="SCALE_RES_F32_H", res="RES_F16", res_res2="RES_F16", ln_bias="LN_BIAS_F16", split="SCALE_RES_SPLIT",
              split_pos="SCALE_RES_SPLIT", gelu="BIAS_GELU_F16", geglu="GEGLU_F16", ln_gelu="LN_GELU_F16", no_bias="BIAS_F16")


def dense16_epis(case):
    """The epilogues the GPU file runs on a dense case: split needs N % 64 == 0, GEGLU N % 32 == 0 (its output is N / 2 wide, ldc = N / 2)."""
    N = case[1]
    return [e for e in DENSE16_EXACT + DENSE16_REAL if not (e.startswith("split") and N % 64) and not (e == "geglu" and N % 32)]


def dense16_kw(case, epi):
    M, N, K, lda, ldc = case
    return dict(M=M, N=N, K=K, lda=lda, ldc=N // 2 if epi == "geglu" else ldc)


def conv16_kw(case):
    B, H, W, Cin, Cout, stride, relu_in, ldc = case
    Ho, Wo = conv_out_size(H, W, stride)
    return dict(M=B * Ho * Wo, N=Cout, K=9 * Cin, ldc=ldc, relu_in=relu_in, conv=(B, H, W, Cin, Ho, Wo, stride))


def patch16_kw(case):
    fr, P, N, K, ldc = case
    return dict(M=fr * P, N=N, K=K, ldc=ldc, P=P)


def convt16_kw(case, k):
    B, h, w, C, Cp = case
    return dict(M=B * h * w, N=k * k * Cp, K=Cp, ldc=Cp, convt=(k, h, w, Cp))


ROWPOS16 = dict(M=257, N=264, K=192)        # row position independence: rows 0, 127, 128, 191, 192, 255, 256 of 257 hold the same A row
ROWPOS16_ROWS = [0, 127, 128, 191, 192, 255, 256]


def f16_launches(ncu):
    """Every (variant, sched, fields) that tests/test_kernels_f16_edges_gpu.py hands to vda_gemm_f16, in no particular order: the planner
    coverage test (CPU) walks this list, the GPU file asserts after every launch that the kernel that ran is the one planned.
    (The tile-seam launches run on a capped grid and are planned for it: seam16_launches and pick_cap below, held to the built
    tables in tests/test_exact_inputs.py.)"""
    for v in VARIANTS16:
        for case in DENSE16_CASES:
            for e in dense16_epis(case):
                yield v, False, gemm16_fields(epi=EPI[EPI_OF[e]], **dense16_kw(case, e))
        for M, N, K in BROADCAST16_CASES:
            for e in ("BIAS_F16", "SCALE_RES_F32"):
                yield v, False, gemm16_fields(M, N, K, EPI[e], lda=0)
        for case in PATCH16_CASES:
            yield v, False, gemm16_fields(epi=EPI["PATCH_F32"], **patch16_kw(case))
        for case in CONVT16_CASES:
            for k in CONVT_K:
                yield v, False, gemm16_fields(epi=EPI["CONVT_F16"], **convt16_kw(case, k))
        for e in ("BIAS_F16", "BIAS_GELU_F16"):
            yield v, False, gemm16_fields(epi=EPI[e], **ROWPOS16)
        for case in CONV16_CASES:
            for e in CONV16_EPIS:
                yield v, False, gemm16_fields(epi=EPI[EPI_OF[e]], **conv16_kw(case))
    for v in WALK16_VARIANTS:
        for N in WALK16_N:
            M, N, K = walk16_case(ncu, N)
            yield v, False, gemm16_fields(M, N, K, EPI["BIAS_F16"])
            if v in (-1, 5 + 16 * 64):
                yield v, True, gemm16_fields(M, N, K, EPI["BIAS_F16"])
    M, N, K = split16_case(ncu)
    yield -1, False, gemm16_fields(M, N, K, EPI["BIAS_F16"])


# ------------------------------------------------------------------------------------------------ tile seams: a persistent workgroup's second and third tile
# The cases above give a persistent workgroup at most one tile on a 256-CU device. Under vda_set_max_wgs(8 or 16) a few thousand rows
# are three rounds of the capped grid: what passes from one tile to the next (the prefetched K tile 0, the A slot the epilogue staged
# through, the bias / statistics fragments fetched a tile ahead, the conv row decomposition, the rotated fold walk, the dealt last
# round) is then under the same equalities. The walk model below restates gemm_tile.h's TileWalk so that the CPU file can assert what
# each case's launches do - which workgroup runs which tiles in which order - without a GPU.
FOLD_ROT = 5                          # gemm8p_kernel.h: the folded mode rotates a row panel's columns by FOLD_ROT panels per round


def tile_walk(M, N, bm, bn, nwg, fold=False):
    """gemm_tile.h's TileWalk (plain, dealt, deal_last) for a grid of nwg workgroups, with the FOLD_ROT rotation of gemm8p_kernel.h on
    request: dict(nbn, nbm, ntiles, nwg, per_xcd, full_rounds, rem, deal_last, tiles), tiles[bid] = the tiles workgroup bid runs, in
    order (the kernels' loop ends at the first round whose tile is past the end). The L2-blocked order (32 workgroups per XCD) is not
    modelled: no capped launch takes it."""
    assert nwg > 0 and nwg % 8 == 0, "persistent grids are multiples of the eight XCDs"
    nbn, nbm = -(-N // bn), -(-M // bm)
    ntiles, per_xcd = nbm * nbn, nwg >> 3
    full_rounds, rem = divmod(ntiles, nwg)
    deal_last = rem > 0 and full_rounds > 0 and per_xcd % nbn == 0

    def tile_of(bid, rnd):
        if deal_last and rnd == full_rounds:
            slot = bid >> 3
            j = ((slot // nbn) * 8 + (bid & 7)) * nbn + slot % nbn
            t = rnd * nwg + j if j < rem else ntiles
        else:
            t = rnd * nwg + (bid & 7) * per_xcd + (bid >> 3)
        if fold and t < ntiles:
            i, j = divmod(t, nbn)
            t = i * nbn + (j + (i * nbn // nwg) * FOLD_ROT) % nbn
        return t

    tiles = []
    for bid in range(nwg):
        mine, rnd = [], 0
        while tile_of(bid, rnd) < ntiles:
            mine.append(tile_of(bid, rnd))
            rnd += 1
        tiles.append(mine)
    return dict(M=M, N=N, bm=bm, bn=bn, nbn=nbn, nbm=nbm, ntiles=ntiles, nwg=nwg, per_xcd=per_xcd, full_rounds=full_rounds, rem=rem, deal_last=deal_last, tiles=tiles)


def tile_box(w, t):
    """(r0, r1, c0, c1): the rows and columns of the matrix that tile t of a tile_walk owns."""
    i, j = divmod(t, w["nbn"])
    return i * w["bm"], min((i + 1) * w["bm"], w["M"]), j * w["bn"], min((j + 1) * w["bn"], w["N"])


def seam_pairs(w):
    """[(previous tile, tile)] over every workgroup's tiles of round >= 1: the seams."""
    return [(a, b) for mine in w["tiles"] for a, b in zip(mine, mine[1:])]


def seam16_case(bm, bn, nwg, nbn, K, wide64, pad):
    """(M, N, K, lda, ldc) for bm x bn tiles on nwg workgroups: two full rounds and a partial third (at least three tiles of it), the
    partial row tile in the last round. N: wide64 - a multiple of 64 (split, split_pos and GEGLU apply), the last column tile 64 wide
    where nbn > 1; otherwise one 8-column segment past a tile width (past bn / 2 where nbn == 1). The 192 x 384 tile is forced only
    for N % 384 == 0: whole column tiles, wide64 alone. Asserted through the model by assert_seam16."""
    nbm = -(-(2 * nwg + 3) // nbn)
    M = nbm * bm - 37
    if bn == 384:
        assert wide64
        N = nbn * bn
    elif wide64:
        N = bn if nbn == 1 else (nbn - 1) * bn + 64
    else:
        N = bn // 2 + 8 if nbn == 1 else (nbn - 1) * bn + 8
    return (M, N, K, K + 8 * pad, N + 8 * pad)


def assert_seam16(case, bm, bn, nwg):
    """What a seam case is there for, from the model; returns the walk."""
    M, N, K, lda, ldc = case
    w = tile_walk(M, N, bm, bn, nwg)
    assert sorted(t for mine in w["tiles"] for t in mine) == list(range(w["ntiles"])), "the walk covers every tile once"
    assert w["full_rounds"] == 2 and 0 < w["rem"] < nwg, (case, bm, bn, nwg, w["full_rounds"], w["rem"])
    assert sorted({len(mine) for mine in w["tiles"]}) == [2, 3], "some workgroups run three tiles, the others sit out the last round"
    assert w["deal_last"] == ((nwg >> 3) % w["nbn"] == 0)
    assert M % bm != 0 and N % 8 == 0 and K % 64 == 0 and lda % 8 == 0 and ldc % 8 == 0
    last_panel = range((w["nbm"] - 1) * w["nbn"], w["ntiles"])
    assert all(mine.index(t) >= 1 for mine in w["tiles"] for t in mine if t in last_panel), "the partial row tile falls in a round > 0"
    if w["nbn"] > 1 and N % bn != 0:
        ragged_after_full = [(a, b) for a, b in seam_pairs(w) if b % w["nbn"] == w["nbn"] - 1 and a % w["nbn"] != w["nbn"] - 1]
        # nbn | nwg: plain() and dealt() both keep a workgroup in its column (t and t + nwg are congruent mod nbn, and the dealt slot
        # keeps slot % nbn), so no workgroup can change column tiles at a seam; the modes with nbn = 3 do
        assert bool(ragged_after_full) == (nwg % w["nbn"] != 0), (case, bm, bn, nwg)
    return w


# (bm, bn, workgroups per CU): the large tiles vda_gemm_built lists for dense A
SEAM16_TILES = [(256, 256, 1), (256, 128, 1), (192, 128, 1), (192, 128, 2), (192, 384, 1), (192, 256, 1)]
# (cap, nbn): nbn = 1 on 8 workgroups - the last round dealt (per_xcd % nbn == 0); nbn = 3 - the plain last round; nbn = 2 on 16 - dealt
# with per_xcd = 2. (Two workgroups per CU: 16 workgroups under cap 8 in all three.)
SEAM16_MODES = [(8, 1), (8, 3), (16, 2)]
# what the seam tests force: every variant with a large tile (0 and 7 run the 128-row kernel on dense A)
SEAM16_VARIANTS = [-1, 1, 2, 3, 4, 5, 9, 8, 10, 11, 5 + 16 * 64]


def seam16_specs():
    """[(bm, bn, per_cu, cap, case)]. Every tile in the three modes with N a multiple of 64, and with the one-segment N in the plain mode
    (nbn = 3: the one mode in which a workgroup changes its column tile at a seam, so the one in which a ragged tile follows a full one).
    K steps: 5 (the 8-phase kernel's 3 A slots and 2 W slots out of phase at the seam) and 9; each tile gets both, and lda > K, ldc > N
    with the segment flavour (the 192 x 384 tile, which has none: with nbn = 3)."""
    out = []
    for bm, bn, per_cu in SEAM16_TILES:
        for cap, nbn in SEAM16_MODES:
            cap = 8 if per_cu == 2 else cap
            for wide64 in (True, False):
                if not wide64 and (bn == 384 or nbn != 3):
                    continue
                K = 64 * (9 if nbn == 2 or not wide64 or (bn == 384 and nbn == 3) else 5)
                pad = not wide64 or (bn == 384 and nbn == 3)
                out.append((bm, bn, per_cu, cap, seam16_case(bm, bn, per_cu * cap, nbn, K, wide64, pad)))
    return out


SEAM16_SPECS = seam16_specs()


def seam16_id(spec):
    return "tile%dx%dx%d-cap%d-%s" % (spec[:4] + (dense_id(spec[4]),))


def seam16_seed(case):
    """Seeds of dense16_inputs for a seam case (several tiles may share a shape: the same inputs then)."""
    cases = sorted({s[4] for s in SEAM16_SPECS})
    return 5300 + 31 * cases.index(case)


def seam16_launches(L, spec):
    """[(variant, epilogue name, family, dyn)] that run spec's case on spec's tile under vda_set_max_wgs(cap), from vda_gemm_plan for cap CUs:
    a variant whose family is not built for the epilogue plans another tile, on which this case has other rounds - that launch belongs to
    the spec of that tile, if any. A forced variant that repeats an earlier one's kernel on this tile is left out (8, 10 and 11 fall back
    to variant 4's 256 x 128 tile, 5 + 16 * 64 to variant 5's 256 x 256 one, for the epilogues their own tile is not built for); the
    automatic path stays, its option word differs. dyn: the same launch with sched set draws its tiles (8-phase kernel, default K schedule)."""
    bm, bn, per_cu, cap, case = spec
    out, seen = [], set()
    for v in SEAM16_VARIANTS:
        L.lib.vda_gemm_set_variant(v)
        for e in dense16_epis(case):
            f = gemm16_fields(epi=EPI[EPI_OF[e]], **dense16_kw(case, e))
            rc, recs = plan16(L, f, ncu=cap)
            if rc == 0 and len(recs) == 1 and recs[0].family != L.FAM_128 and (recs[0].bm, recs[0].bn, recs[0].per_cu) == (bm, bn, per_cu):
                if (v < 0, recs[0].family, recs[0].ksched, e) in seen:
                    continue
                seen.add((v < 0, recs[0].family, recs[0].ksched, e))
                rc2, dyn = plan16(L, f, ncu=cap, sched=True)
                out.append((v, e, recs[0].family, bool(rc2 == 0 and len(dyn) == 1 and dyn[0].dyn == 1)))
    L.lib.vda_gemm_set_variant(-1)
    return out


def pick_cap(L, fields, fold=False):
    """(cap, record, walk) for a launch of the conv / patch / ConvTranspose / folded seam cases under the current variant: the first of
    8 and 16 workgroups with at least two full rounds and a partial one on the planned tile, else the first with more than two
    rounds' worth of tiles (N = 16 column tiles can have no partial round on either); None where the plan is the 128-row kernel
    or the tiles are too few on both."""
    found = None
    for cap in (8, 16):
        rc, recs = plan16(L, fields, ncu=cap)
        if rc != 0 or len(recs) != 1 or recs[0].family in (L.FAM_128, L.FAM_CONV_LDS):
            continue
        r = recs[0]
        w = tile_walk(fields["M"], fields["N"], r.bm, r.bn, r.per_cu * cap, fold)
        if w["full_rounds"] >= 2 and w["rem"] > 0:
            return cap, r, w
        if found is None and w["ntiles"] > 2 * w["nwg"]:
            found = (cap, r, w)
    return found


# patch embed (frames, P, N, K, ldc): P = 37 rows per frame, so frame boundaries fall inside 256-row tiles of every round; five K steps
SEAM_PATCH16_CASES = [(131, 37, 136, 320, 144), (131, 37, 264, 320, 264)]
# ConvTranspose (B, h, w, C, Cp), three frames, K = Cp = 128: two K steps. k = 2 (N = 512: 2 or 4 column tiles) on 30 x 30 = 2700 rows = 11 row
# tiles of 256; k = 4 (N = 2048: 8 or 16 column tiles) on 14 x 14 = 588 rows = 3 row tiles, both frame borders inside tiles of later rounds
SEAM_CONVT16_CASES = [(3, 30, 30, 120, 128), (3, 14, 14, 120, 128)]
SEAM_CONVT16 = [(SEAM_CONVT16_CASES[0], 2), (SEAM_CONVT16_CASES[1], 4)]
# conv3x3 (B, H, W, Cin, Cout, stride, relu_in, ldc): 3 x 41 x 41 = 5043 rows = 20 row tiles of 256, frame borders at rows 1681 and 3362
SEAM_CONV16_CASES = [
    (3, 41, 41, 64, 128, 1, True, 128),       # one column tile of either width, the instantiation with the max
    (3, 41, 41, 64, 128, 1, False, 128),      # ... and the plain one
    (3, 41, 41, 128, 136, 1, False, 144),     # two K steps per tap; nbn = 1 of 256 / 2 of 128 with a one-segment last tile; ldc > N
    (3, 41, 41, 64, 264, 1, True, 264),       # nbn = 2 of 256 / 3 of 128; the one shape the automatic path gives a large tile
    (3, 81, 81, 64, 136, 2, False, 136),      # stride 2 from an 81 x 81 source
    (3, 81, 81, 64, 136, 2, True, 136),
    (3, 17, 65, 64, 64, 1, True, 64),         # conv3x3_c64_kernel's: 3 x 3 x 3 = 27 tiles of 8 x 32; on 8 workgroups (one per XCD) the XCD shares are 3 or 4
]
SEAM_C64_CASE = SEAM_CONV16_CASES[-1]
# every variant with a conv family on the large tiles; also what the patch-embed and ConvTranspose epilogues are built on (the 256-row
# tiles alone: 8, 10, 11 and 5 + 16 * 64 would repeat 4 and 5)
SEAM_CONV16_VARIANTS = [-1, 1, 2, 3, 4, 5, 9]
# folded ConvTranspose + conv (k, Cin, Fe, B, H, W): N = k * k * Fe -> nbn = 1, 2 and 4 column tiles of the 8-phase 256 x 256 tile
SEAM_FOLD_CASES = [(2, 64, 64, 2, 47, 50), (2, 64, 128, 2, 30, 40), (4, 64, 64, 2, 24, 25)]
SEAM_C64_EPIS = ["bias_f16", "bias_relu", "res", "res_res2"]
# depth_tail_up_kernel: 3 x 3 x 3 = 27 tiles of 16 x 32 on 8 workgroups
SEAM_TAILUP_CASE = (3, 17, 33, 33, 65)
# the L2-blocked walk (32 workgroups per XCD, uncapped) at five K steps
WALK16_BLOCKED_K = 320
EPI_CONVT_FOLD_F16 = 13               # include/vda.h (test_exact_inputs.py holds it to _lib)


def fold_fields(case):
    k, Cin, Fe, B, H, W = case
    return gemm16_fields(B * H * W, k * k * Fe, 9 * Cin, EPI_CONVT_FOLD_F16, lda=9 * Cin, ldc=Fe, conv=(B, H, W, Cin, H, W, 1), convt=(k, H, W, Fe))


@functools.lru_cache(maxsize=None)
def seam_fold_data(case):
    """(t, Wc, Bc, fp64 reference [B, Fe, k H, k W]) of a folded seam case from tests/_convt_fold_ref.py's integer inputs, with the
    exactness conditions of tests/test_convt_fold_gpu.py: every composed weight, class bias, intermediate and result an fp16 integer."""
    import _convt_fold_ref as R
    k, Cin, Fe, B, H, W = case
    t, wt, bt, wr = R.exact_inputs(k, Cin, Fe, B, H, W, seed=1000 * k + Cin + Fe + 7 * H + W)
    ref = R.unfused(t, wt, bt, wr, k)
    Wc, Bc = R.compose(wt, bt, wr)
    bound = F.conv_transpose2d(t.abs(), wt.abs(), bt.abs(), stride=k) * 27      # (each output sums at most 27 entries of the ConvTranspose's result)
    assert_exact_safe_f16([bound], [F.conv_transpose2d(t, wt, bt, stride=k), R.pack(Wc), R.class_bias(Bc), ref])
    return t, Wc, Bc, ref


def fold_as_gemm(ref, k):
    """[B, Fe, k H, k W] -> the folded GEMM's own [B H W, k k Fe] matrix (column = (py k + px) Fe + co)."""
    B, Fe, kH, kW = ref.shape
    H, W = kH // k, kW // k
    return ref.reshape(B, Fe, H, k, W, k).permute(0, 2, 4, 3, 5, 1).reshape(B * H * W, k * k * Fe)


# ================================================================================================ the fp16 attention kernels (attention.hip, temporal.hip)
# Softmax is not linear, but three families of inputs make its real-arithmetic result an fp16 value that no rounding of a correct
# kernel can move (tests/test_attention_edges_gpu.py; shown sound, and the equalities shown able to fail, in tests/test_exact_inputs.py):
#   selector   every query has ONE key whose score beats every other by >= 51.9 (log2): the result is that key's V row, bit for bit;
#   counting   q = 0: every weight is 1, the result is a count of keys over N;
#   straddle   (real-valued) a whole key tile whose row sum sits below the shipped kernel's fast / slow limit for even queries and
#              above it for odd ones.
ATTN_VARIANTS = [-1, 0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11]           # vda_attention_set_variant; the ablation codes 21 - 25 compute wrong results by design
ATTN_EDGE_N = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 321, 449]      # wave, key-tile and query-block edges; 4, 6, 8 tiles
# (B, N, H): after the (1, N, 1) edges, 6 workgroups twice (the XCD remap's remainder arm only), 8 (the quotient arm only), 18 (both)
ATTN_CASES = [(1, n, 1) for n in ATTN_EDGE_N] + [(3, 129, 1), (1, 129, 3), (2, 65, 4), (3, 193, 3)]
ATTN_BIG_CASE = (1, 1370, 2)            # the workload's N: 22 tiles, 90 live queries in the last block
ATTN_BIG_VARIANTS = [-1, 1]
ATTN_STRADDLE_N = [129, 160, 192, 449]  # 160: a half-full last tile
ATTN_TOL = 3e-3                         # tests/test_kernels_gpu.py's attention bound, rtol = atol
ATTN_SUM_LIMIT = 2048.0                 # SUM_LIMIT of attn_cs_kernel
LOG2E = 1.4426950408889634


def attn_case_id(c):
    return "B%d-N%d-H%d" % c


def attn_seed(case):
    B, N, H = case
    return 9000 + 97 * N + 7 * B + H


def key_codes(j):
    """[len(j), 64]: key j's four base-16 digits (the fourth is the others' sum mod 16, so two keys below 4096 agree in at most
    two), 12.0 at channel 16 s + d_s: each digit fills one 16-channel MFMA k-step."""
    d0, d1, d2 = j % 16, (j // 16) % 16, (j // 256) % 16
    code = torch.zeros(j.numel(), 64)
    for s, d in enumerate((d0, d1, d2, (d0 + d1 + d2) % 16)):
        code[torch.arange(j.numel()), 16 * s + d] = 12.0
    return code


def attn_value_code(B, N, H):
    """V [B, N, H, 64]: integers with |v| <= 1019 that differ between keys, heads and frames."""
    b, j, h, c = torch.meshgrid(torch.arange(B), torch.arange(N), torch.arange(H), torch.arange(64), indexing="ij")
    return ((31 * j + 7 * c + 13 * (b * H + h)) % 2039 - 1019).to(F32)


def attn_selector_inputs(B, N, H, seed):
    """(qkv fp32 [B, N, 3 * H * 64] of fp16 values, pi [B, H, N]): query i of (frame b, head h) carries the code of key pi[b][h][i]."""
    assert 0 < N <= 4096
    g = torch.Generator().manual_seed(seed)
    pi = torch.stack([torch.stack([torch.randperm(N, generator=g) for _ in range(H)]) for _ in range(B)])
    qkv = torch.zeros(B, N, 3, H, 64)
    qkv[:, :, 1] = key_codes(torch.arange(N))[None, :, None, :]
    for b in range(B):
        for h in range(H):
            qkv[b, :, 0, h] = key_codes(pi[b][h])
    qkv[:, :, 2] = attn_value_code(B, N, H)
    return qkv.reshape(B, N, 3 * H * 64), pi


def attn_split(qkv, B, N, H, log2_q=False):
    """q, k, v as fp64 [B, H, N, 64] and the factor that turns q . k into natural-log scores. log2_q: q as q_frag<true> rounds it,
    fp16(fp32(q) * fp32(log2(e) / 8)), the scores then in log2 units."""
    q, k, v = qkv.reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    if log2_q:
        c = torch.tensor(LOG2E, dtype=F32) * 0.125
        return (q.float() * c).to(F16).double(), k.double(), v.double(), 1.0 / LOG2E
    return q.double() * 0.125, k.double(), v.double(), 1.0


def attn_ref64(qkv, B, N, H, log2_q=False):
    """fp64 softmax(q k^T / 8) v -> [B, N, H * 64]."""
    q, k, v, nat = attn_split(qkv, B, N, H, log2_q)
    a = (q @ k.transpose(-1, -2) * nat).softmax(dim=-1)
    return (a @ v).transpose(1, 2).reshape(B, N, H * 64)


def selector_expected(qkv, pi, B, N, H):
    """V[pi] as fp64 [B, N, H * 64]."""
    v = qkv.reshape(B, N, 3, H, 64)[:, :, 2].double()
    out = torch.empty(B, N, H, 64, dtype=F64)
    for b in range(B):
        for h in range(H):
            out[b, :, h] = v[b, pi[b][h], h]
    return out.reshape(B, N, H * 64)


def assert_selector_safe(qkv, pi, B, N, H):
    """The preconditions under which every fp16 attention kernel must return V[pi] bit for bit, in fp64 and under both q scalings
    (q / 8, exact; q * log2(e) / 8 rounded to fp16 as the LOG2 kernels do). A condition on the inputs, not a measurement of a kernel:
      * every winner weight >= 1 - 2**-40: every other weight is <= 2**-40, so against a reference point at the winner's score each
        other p rounds to 0 in fp16 (below 2**-25) and vanishes against 1 in the fp32 row sum; what was accumulated before the winner
        arrived is scaled by as little;
      * sum over the other keys of weight * |v| <= 2**-26: half of half the smallest fp16 subnormal. V holds zeros, and the output next
        to a zero must round to zero (this is tighter than 2**-20, which would do next to |v| >= 1 only);
      * every |v| <= 1019 and integral: an fp16 value, and a relative error of 2e-5 in p (codes 4 and 5 keep the reference point as
        an fp16 pair) moves it by 0.02, far from the quarter unit that could change the final rounding;
      * the largest log2-domain score < 128: exp2 of it is finite in fp32 (the first tile's reference point is 0)."""
    v = qkv.reshape(B, N, 3, H, 64)[:, :, 2].double()
    assert bool((v == v.round()).all()) and float(v.abs().max()) <= 1019, "V: integers up to 1019"
    assert torch.equal(qkv.to(F16).float(), qkv), "every operand is its own fp16 rounding"
    win = pi[:, :, :, None]
    for log2_q in (False, True):
        q, k, vv, nat = attn_split(qkv, B, N, H, log2_q)
        s = q @ k.transpose(-1, -2) * nat                       # natural-log scores [B, H, N, N]
        top = float(s.max()) * LOG2E
        assert top < 128, f"log2 score {top:.1f}: exp2 overflows"
        assert torch.equal(s.argmax(dim=-1), pi), "the winner is not the coded key"
        w = s.softmax(dim=-1)
        others = w.scatter(-1, win, 0.0)
        lose = float(others.sum(-1).max())
        assert lose <= 2.0 ** -40, f"log2_q={log2_q}: a winner's weight is 1 - {lose:.3g} < 1 - 2**-40"
        leak = float((others @ vv.abs()).max())
        assert leak <= 2.0 ** -26, f"log2_q={log2_q}: the other keys contribute up to {leak:.3g} > 2**-26"


def selector_mismatch(y, expect, v_rows=None):
    """None if y [B, N, H * 64] equals expect bit for bit; otherwise a message: how many (row, head) blocks differ and, for the first,
    which key's V row it equals, if any (v_rows: V as [B, N, H, 64])."""
    y = y.double()
    if y.shape == expect.shape and torch.equal(y, expect):
        return None
    B, N, W = expect.shape
    H = W // 64
    bad = ((y != expect) | y.isnan()).reshape(B, N, H, 64).any(-1)
    b, i, h = bad.nonzero()[0].tolist()
    msg = f"{int(bad.sum())}/{bad.numel()} (query, head) rows differ from V[pi] ({int(y.isnan().sum())} NaN); first: frame {b} query {i} head {h}"
    if v_rows is not None:
        row = y.reshape(B, N, H, 64)[b, i, h]
        hit = [(bb, jj) for bb in range(B) for jj in (v_rows[bb, :, h].double() == row).all(-1).nonzero().flatten().tolist()]
        msg += f", which is V of (frame, key) {hit[:3]}" if hit else ", which is no key's V row of that head"
    return msg


def attn_counting_inputs(B, N, H, seed):
    """q = 0, k small integers that must not matter, V[b, j, h, c] = (1 + (b H + h) % 3) * (j % 64 == c): every score 0, every p 1."""
    qkv = torch.zeros(B, N, 3, H, 64)
    qkv[:, :, 1] = ints((B, N, H, 64), -3, 3, seed)
    b, j, h, c = torch.meshgrid(torch.arange(B), torch.arange(N), torch.arange(H), torch.arange(64), indexing="ij")
    qkv[:, :, 2] = ((1 + (b * H + h) % 3) * (j % 64 == c)).to(F32)
    return qkv.reshape(B, N, 3 * H * 64)


def counting_expected(B, N, H):
    """count_c * (1 + (b H + h) % 3) / N as fp64 [B, N, H * 64]: the same row for every query of a (frame, head)."""
    count = torch.bincount(torch.arange(N) % 64, minlength=64).double()
    scale = (1 + torch.arange(B * H) % 3).double().reshape(B, 1, H, 1)
    return (count * scale / N).expand(B, N, H, 64).reshape(B, N, H * 64)


def ulp16(x):
    """Spacing of fp16 at |x| (fp64 in, fp64 out)."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -14)))
    return torch.exp2(e - 10)


def counting_check(y, B, N, H):
    """(ok, worst error in fp16 ulp). The numerator is an integer count times 1, 2 or 3 (exact in fp32), the row sum is N (exact).
    N a power of two: 1/N, the product and the fp16 rounding are all exact - equality. Any other N: two fp32 roundings (1/N, the
    product; 2**-23 relative together, a few times that where 1/N is the hardware's approximate reciprocal) put the fp32 value next
    to the real one, so its fp16 rounding is the real value's fp16 rounding or a neighbour of it: within one fp16 ulp."""
    e = counting_expected(B, N, H)
    r = e.to(F16).double()
    err = (y.double() - r).abs()
    worst = float(torch.nan_to_num(err / ulp16(r), nan=float("inf")).max())
    if N & (N - 1) == 0:
        assert torch.equal(r, e)
        return torch.equal(y.double(), e), worst
    return bool((err <= ulp16(r)).all()), worst


def attn_straddle_inputs(N, seed):
    """B = H = 1. q: channel 0 only, 4.0 (even queries) / 4.5 (odd); k: tile 0 all zero, every later key 6.5 in channel 0; V: positive
    integers. A full later tile's row sum against the reference point 0 the first tile leaves: 64 e^3.25 = 1650 (even) and
    64 e^3.656 = 2478 (odd), either side of attn_cs_kernel's SUM_LIMIT = 2048, interleaved lane by lane in every wave."""
    assert N >= 129
    qkv = torch.zeros(1, N, 3, 64)
    qkv[0, 0::2, 0, 0] = 4.0
    qkv[0, 1::2, 0, 0] = 4.5
    qkv[0, 64:, 1, 0] = 6.5
    qkv[0, :, 2] = ints((N, 64), 1, 1019, seed)
    return qkv.reshape(1, N, 192)


def straddle_tile_sums(qkv, log2_q):
    """(even, odd): row sum of a full later key tile, p relative to the reference point 0."""
    N = qkv.shape[1]
    q, k, _, nat = attn_split(qkv, 1, N, 1, log2_q)
    s = q[0, 0, :2] @ k[0, 0, 64:128].t() * nat
    return tuple(s.exp().sum(-1).tolist())


def tiled_attention(qkv, B, N, H, mutation=None):
    """Plain fp64 restatement of the kernels' tile loop - 64-key tiles, rows past N staged as row N - 1 and masked, running maximum,
    rescale - with one mistake a kernel could make:
      drop_last     the loop runs over N - 1 keys;
      dup_last      the first clamped copy of key N - 1 is left unmasked (needs a partial last tile);
      mask_moved    the last tile's mask boundary sits one key early (the other tiles' code is right);
      stale_v       the last tile multiplies by the V tile before it (a double buffer not yet refilled; needs two tiles);
      heads / frames / queries   results stored to the neighbouring head / frame / query row (needs two of them)."""
    q, k, v, nat = attn_split(qkv, B, N, H)
    Nk = N - 1 if mutation == "drop_last" else N
    nt = -(-Nk // 64)
    m = torch.full((B, H, N, 1), -1e30, dtype=F64)
    l = torch.zeros(B, H, N, 1, dtype=F64)
    acc = torch.zeros(B, H, N, 64, dtype=F64)
    for kt in range(nt):
        rows = torch.arange(kt * 64, kt * 64 + 64)
        staged = rows.clamp_max(N - 1)
        bound = Nk
        if kt == nt - 1:
            bound += {"dup_last": 1 if N % 64 else 0, "mask_moved": -1}.get(mutation, 0)
        s = q @ k[:, :, staged].transpose(-1, -2) * nat
        s[..., rows >= bound] = -1e30
        m_new = torch.maximum(m, s.max(-1, keepdim=True).values)
        alpha = (m - m_new).exp()
        p = (s - m_new).exp()
        vt = v[:, :, (staged - 64) if (mutation == "stale_v" and kt == nt - 1 and kt > 0) else staged]
        acc = acc * alpha + p @ vt
        l = l * alpha + p.sum(-1, keepdim=True)
        m = m_new
    out = acc / l
    if mutation == "heads" and H > 1:
        out = out[:, [1, 0] + list(range(2, H))]
    if mutation == "frames" and B > 1:
        out = out[[1, 0] + list(range(2, B))]
    if mutation == "queries" and N > 1:
        out = out[:, :, [1, 0] + list(range(2, N))]
    return out.transpose(1, 2).reshape(B, N, H * 64)


ATTN_MUTATIONS = ["drop_last", "dup_last", "mask_moved", "stale_v", "heads", "frames", "queries"]


def attn_mutation_applies(mutation, B, N, H):
    """(N == 1: any number of copies of the only key gives the same softmax - only dropping it can show.)"""
    return dict(dup_last=N % 64 != 0 and N > 1, mask_moved=N > 1, stale_v=N > 64, heads=H > 1, frames=B > 1, queries=N > 1).get(mutation, True)


# ------------------------------------------------------------------------------------------------ temporal attention
TATTN_T = [1, 2, 15, 16, 17, 31, 32]                 # 16 / 17: the edge of the VALU kernel's two 16-query halves
TATTN_HW = [1, 3]
TATTN_SELECTOR_GEOM = [(256, 8), (512, 8), (1024, 8), (32, 1), (128, 2), (512, 4)]      # (C, heads): d = 32, 64, 128, 32, 64, 128
TATTN_SMALL_GEOM = [(64, 8), (192, 8), (384, 8)]     # ViT-S: d = 8, 24, 48, which the MFMA kernel does not serve


def tattn_seed(T, hw, C, heads):
    return 9500 + 131 * T + 17 * hw + C + heads


def tattn_selector_inputs(T, hw, C, heads, seed):
    """(qkv fp32 [T * hw, 3 C], rows ordered (frame, pixel), pi [hw, heads, T]). k of frame t: 16.0 at channel t of its head; q of
    frame t: the same code of frame pi[p][h][t]; the winner's score leads by 256 / sqrt(d) >= 22.6.
    V: the spatial integer coding over (frame, pixel, head, channel) with the zero left out - values -1019..-1 and 1..1019. At d = 128
    the other frames' weights (e^-22.6 each) times |v| reach 5e-6: nothing next to |v| >= 1, but next to v = 0 it is a nonzero fp16
    subnormal (the VALU kernel multiplies V by fp32 weights), so with a zero in V the real result would not be V[pi]."""
    d = C // heads
    assert C % heads == 0 and T <= 32 <= d
    g = torch.Generator().manual_seed(seed)
    pi = torch.stack([torch.stack([torch.randperm(T, generator=g) for _ in range(heads)]) for _ in range(hw)])
    qkv = torch.zeros(T, hw, 3, heads, d)
    t = torch.arange(T)
    qkv[t, :, 1, :, t] = 16.0
    for p in range(hw):
        for h in range(heads):
            qkv[t, p, 0, h, pi[p][h]] = 16.0
    f, px, h, c = torch.meshgrid(t, torch.arange(hw), torch.arange(heads), torch.arange(d), indexing="ij")
    m = (31 * f + 7 * c + 13 * (px * heads + h)) % 2038
    qkv[:, :, 2] = torch.where(m < 1019, m - 1019, m - 1018).to(F32)
    return qkv.reshape(T * hw, 3 * C), pi


def tattn_ref64(qkv, T, hw, C, heads):
    """fp64 softmax(q k^T / sqrt(d)) v over the frames of each (pixel, head) -> [T * hw, C]."""
    d = C // heads
    x = qkv.double().reshape(T, hw, 3, heads, d).permute(2, 1, 3, 0, 4)          # [3, hw, heads, T, d]
    a = (x[0] @ x[1].transpose(-1, -2) * d ** -0.5).softmax(dim=-1)
    return (a @ x[2]).permute(2, 0, 1, 3).reshape(T * hw, C)


def tattn_selector_expected(qkv, pi, T, hw, C, heads):
    d = C // heads
    v = qkv.double().reshape(T, hw, 3, heads, d)[:, :, 2]
    out = torch.empty(T, hw, heads, d, dtype=F64)
    for p in range(hw):
        for h in range(heads):
            out[:, p, h] = v[pi[p][h], p, h]
    return out.reshape(T * hw, C)


def assert_tattn_selector_safe(qkv, pi, T, hw, C, heads):
    """The preconditions under which both temporal kernels must return V[pi] bit for bit (fp64; neither kernel rounds q or the scale
    to fp16, so there is one scaling):
      * every v is a nonzero integer with |v| <= 1019: the smallest gap from an output value to a neighbouring fp16 value is 2**-11;
      * every other frame's weight <= 2**-26: the MFMA kernel's fp16 p is exactly 0 (below half the smallest subnormal, 2**-25);
      * the other frames' weights sum to <= 2**-26: the fp32 row sum is 1 in any order (half an ulp of 1 is 2**-24), 1 / sum is 1 and
        the winner's normalised weight is 1;
      * sum over the other frames of weight * |v| <= 2**-13: a quarter of that smallest gap, with room for the VALU kernel's fp32
        accumulation (2**-23 relative per step)."""
    d = C // heads
    x = qkv.double().reshape(T, hw, 3, heads, d).permute(2, 1, 3, 0, 4)
    assert torch.equal(qkv.to(F16).float(), qkv)
    v = x[2]
    assert bool((v == v.round()).all()) and float(v.abs().max()) <= 1019 and float(v.abs().min()) >= 1, "V: nonzero integers up to 1019"
    s = x[0] @ x[1].transpose(-1, -2) * d ** -0.5
    assert torch.equal(s.argmax(dim=-1), pi), "the winner is not the coded frame"
    w = s.softmax(dim=-1)
    others = w.scatter(-1, pi[..., None], 0.0)
    assert float(others.max()) <= 2.0 ** -26 and float(others.sum(-1).max()) <= 2.0 ** -26, f"the other frames weigh up to {float(others.sum(-1).max()):.3g} > 2**-26"
    leak = float((others @ v.abs()).max())
    assert leak <= 2.0 ** -13, f"the other frames contribute up to {leak:.3g} > 2**-13"


# ================================================================================================ the fused upsample convolutions (conv_up.hip, tail.hip)
# A bilinear resize is not linear in small integers: its weights are fractions. Three families of inputs still leave a correct kernel
# no room (tests/test_upsample_edges_gpu.py; shown sound, and shown able to fail, in tests/test_exact_inputs.py):
#   constant   every pixel of a (frame, channel) holds one small integer v: the four weights sum to 1 within a few 2**-24, the fp16
#              rounding of v times that sum is v, and the convolution behind it is the integer convolution of a constant image;
#   selector   every cout has ONE weight 1: the output IS one interpolated patch value, rounded once - a derived bound of ~0.03
#              against errors of tens for a wrong pixel, tap, channel, k-step or cout block;
#   dyadic     scales in {0, 1/4, 1/2, 1, 3/2, 2}: every weight is a multiple of 1/4 per axis, every interpolated value of small
#              integers a multiple of 1/16 - exact in fp16 at every step of any evaluation order.
FUSED_MUTATIONS = ["row_off", "clamp_pad", "halo_zero", "taps_swapped", "stale_kstep", "cout_shift", "frame"]


def ac_coords(n_in, n_out, contracted=False):
    """align_corners=True source positions as the kernels and torch compute them in fp32: scale = fl32((in - 1) / (out - 1)),
    src = fl32(scale * dst), i0 = min(floor(src), in - 1), i1 = min(i0 + 1, in - 1), w = fl32(src - i0) (an exact difference).
    contracted: w = fl32(scale * dst - i0), one rounding - what a compiler that fuses the product into the subtraction computes.
    Returns (i0, i1, w as fp64 [n_out], scale)."""
    one = torch.ones((), dtype=F32)
    scale = (one * (n_in - 1)) / (one * (n_out - 1)) if n_out > 1 else torch.zeros((), dtype=F32)
    dst = torch.arange(n_out, dtype=F32)
    src = scale * dst
    i0 = src.floor().long().clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    w = (scale.double() * dst.double() - i0.double()).float().double() if contracted else (src - i0.float()).double()
    return i0, i1, w, float(scale)


def interp_image(x, H, W, mode="f64", contracted=False, row_off=None):
    """x [B, C, h, w] -> the align_corners bilinear resize [B, C, H, W] as fp64 values, evaluated as `mode` says:
      f64       a00 (1-wx)(1-wy) + a01 wx (1-wy) + a10 (1-wx) wy + a11 wx wy in fp64 on the fp32 coordinates: the definition;
      sum4_f32  conv_up.hip: the four weights as fp32 products, the four-term sum left to right in fp32, one rounding to fp16;
      pk_f16    tail.hip (bilinear8): the four weights rounded to fp16, a product and three fused multiply-adds in fp16;
      lerp_f32  resample.hip: top = a00 (1-wx) + a01 wx, bot likewise, top (1-wy) + bot wy in fp32 (not rounded to fp16 here).
    row_off = Y: output row Y takes its source rows one too low in the image (a mistake to be seen)."""
    B, C, h, w = x.shape
    ya, yb, wy, _ = ac_coords(h, H, contracted)
    xa, xb, wx, _ = ac_coords(w, W, contracted)
    if row_off is not None:
        ya, yb = ya.clone(), yb.clone()
        ya[row_off] = min(int(ya[row_off]) + 1, h - 1)
        yb[row_off] = min(int(ya[row_off]) + 1, h - 1)
    xd = x.double()
    top, bot = xd[:, :, ya], xd[:, :, yb]
    a00, a01, a10, a11 = top[..., xa], top[..., xb], bot[..., xa], bot[..., xb]
    wy, wx = wy.view(1, 1, H, 1), wx.view(1, 1, 1, W)
    if mode == "f64":
        return a00 * ((1 - wx) * (1 - wy)) + a01 * (wx * (1 - wy)) + a10 * ((1 - wx) * wy) + a11 * (wx * wy)
    fx, fy = wx.float(), wy.float()
    ux, uy = 1 - fx, 1 - fy
    if mode == "lerp_f32":
        t, b = a00.float() * ux + a01.float() * fx, a10.float() * ux + a11.float() * fx
        return (t * uy + b * fy).double()
    w00, w01, w10, w11 = ux * uy, fx * uy, ux * fy, fx * fy
    if mode == "sum4_f32":
        return (a00.float() * w00 + a01.float() * w01 + a10.float() * w10 + a11.float() * w11).to(F16).double()
    assert mode == "pk_f16"
    w00, w01, w10, w11 = (t.to(F16).double() for t in (w00, w01, w10, w11))
    o = (a00 * w00).to(F16).double()
    for a, q in ((a01, w01), (a10, w10), (a11, w11)):
        o = (a * q + o).to(F16).double()
    return o


def fused_mutation_applies(m, B, h, H, W, C, N, tile, kc):
    return dict(row_off=h > 1, halo_zero=H > tile[0] or W > tile[1], stale_kstep=C >= 2 * kc, cout_shift=N > 32, frame=B > 1).get(m, True)


def conv_image(p, w, mutation=None, tile=(16, 32), kc=16):
    """p [B, C, H, W] fp64 (the resized image), w [N, C, 3, 3] fp64 -> conv3x3 with zero padding, [B, H, W, N] fp64, no bias.
    With one mistake of a tiled kernel built in:
      clamp_pad     the border repeats the edge pixel;          halo_zero    a tile's first row (column, where there is one tile row)
      taps_swapped  the centre tap and the one right of it;                  reads zeros above (left of) it inside the image;
      stale_kstep   the last kc channels are those of the step before;      cout_shift   cout n holds cout n + 32's result;
      frame         frame b is computed from frame b - 1."""
    B, C, H, W = p.shape
    N = w.shape[0]
    if mutation == "frame":
        p = p[[0] + list(range(B - 1))]
    if mutation == "stale_kstep":
        p = p.clone()
        p[:, C - kc:] = p[:, C - 2 * kc:C - kc]
    if mutation == "taps_swapped":
        w = w.clone()
        w[:, :, 1, 1], w[:, :, 1, 2] = w[:, :, 1, 2].clone(), w[:, :, 1, 1].clone()
    pp = F.pad(p, (1, 1, 1, 1), mode="replicate" if mutation == "clamp_pad" else "constant")
    out = F.conv2d(pp, w).permute(0, 2, 3, 1).contiguous()
    if mutation == "halo_zero":
        wz = torch.zeros_like(w)
        if H > tile[0]:
            wz[:, :, 0] = w[:, :, 0]
            rows = torch.arange(tile[0], H, tile[0])
            out[:, rows] -= F.conv2d(pp, wz).permute(0, 2, 3, 1)[:, rows]
        else:
            wz[:, :, :, 0] = w[:, :, :, 0]
            cols = torch.arange(tile[1], W, tile[1])
            out[:, :, cols] -= F.conv2d(pp, wz).permute(0, 2, 3, 1)[:, :, cols]
    if mutation == "cout_shift":
        out = out[..., [(n + 32) % N for n in range(N)]]
    return out


def fused_emulate(x, w, H, W, mode, mutation=None, tile=(16, 32), kc=16, contracted=False):
    """conv3x3(resize(x)) [B, H, W, N] in fp64 on the resize evaluated as `mode`, with an optional mistake (FUSED_MUTATIONS)."""
    p = interp_image(x, H, W, mode, contracted, row_off=H // 2 if mutation == "row_off" else None)
    return conv_image(p, w.double(), None if mutation == "row_off" else mutation, tile, kc)


def src_window_extent(n_in, n_out, tile):
    """The largest number of source rows (columns) under the halo'd patch of one `tile`-wide output tile, by the kernels' own
    arithmetic: first = min(int(scale * max(o0 - 1, 0)), in - 1), last = the i1 of the patch's last pixel inside the image. Also
    asserts that no source index lies before `first` (the kernels clamp such an index to the window: it would be a wrong pixel)."""
    i0, i1, _, _ = ac_coords(n_in, n_out)
    ext = 1
    for o0 in range(0, n_out, tile):
        lo, hi = max(o0 - 1, 0), min(o0 + tile, n_out - 1)
        first = int(i0[lo])
        assert int(i0[lo:hi + 1].min()) >= first
        ext = max(ext, int(i1[lo:hi + 1].max()) - first + 1)
    return ext


# ------------------------------------------------------------------------------------------------ vda_conv3x3_up2_f16
# (B, h, w, C, N, ldc): out [B, 2h, 2w, N] = conv3x3(bilinear2x(x)) + bias. 16 x 32 output tiles, grid = tiles rounded up to 8,
# 16-channel k-steps, 32-cout blocks (CB = 1, 2, 4), the wide store path where N % 8 == 0 and ldc % 8 == 0 and out is 16-byte aligned.
UP2_TH, UP2_TW, UP2_SH, UP2_SW, UP2_KC = 16, 32, 11, 19, 16
UP2_CASES = [
    (1, 1, 1, 16, 4, 4),             # both scales 0; nk = 1; narrow store; 7 idle workgroups
    (1, 8, 16, 16, 32, 32),          # exactly one full 16 x 32 tile
    (2, 9, 17, 32, 24, 32),          # exactly 8 tiles; the last tiles 2 rows / 2 columns wide; partial cout block in the wide path; nk = 2
    (3, 9, 17, 48, 40, 44),          # 12 tiles in a grid of 16: per_xcd = 2, tile >= ntiles; CB = 2, partial second block; narrow; odd nk
    (1, 17, 33, 64, 128, 128),       # CB = 4; the largest source window: 10 of 11 rows, 18 of 19 columns
    (1, 17, 33, 32, 100, 104),       # CB = 4, partial last block, narrow
    (1, 1, 40, 16, 32, 32),          # a single source row
    (1, 40, 1, 16, 32, 32),          # a single source column
    (1, 148, 2, 16, 32, 32),         # the workload's extent: source rows up to 147
    (1, 2, 148, 16, 32, 32),         # ... and columns
]
UP2_OFFSET_CASES = [UP2_CASES[3], UP2_CASES[2]]      # repeated with out 8 bytes into its allocation: a narrow case, and a wide one made narrow by that alone


def up2_id(c):
    return "B%d-%dx%d-C%d-N%d-ldc%d" % c


def up2_geometry(case):
    """What the launch of one case looks like: tiles, grid, per_xcd, idle workgroups, k-steps, cout blocks, store path, window extents."""
    B, h, w, C, N, ldc = case
    tiles_x, tiles_y = -(-2 * w // UP2_TW), -(-2 * h // UP2_TH)
    ntiles = tiles_x * tiles_y * B
    grid = -(-ntiles // 8) * 8
    return dict(tiles_x=tiles_x, tiles_y=tiles_y, ntiles=ntiles, grid=grid, per_xcd=grid // 8, idle=grid - ntiles, nk=C // UP2_KC,
                CB=1 if N <= 32 else 2 if N <= 64 else 4, wide=N % 8 == 0 and ldc % 8 == 0, partial_block=N % 32 != 0,
                rows=src_window_extent(h, 2 * h, UP2_TH), cols=src_window_extent(w, 2 * w, UP2_TW))


def up2_const_inputs(case):
    """x [B, C, h, w] = v[b, c] in [-3, 3] at every pixel, w [N, C, 3, 3] in [-2, 2], bias [N] in [-4, 4]."""
    B, h, w, C, N, _ = case
    s = 11000 + 17 * (UP2_CASES.index(case) if case in UP2_CASES else 31) + C
    v = ints((B, C), -3, 3, s)
    return dict(x=v[:, :, None, None].expand(B, C, h, w).contiguous(), w=ints((N, C, 3, 3), -2, 2, s + 1), bias=ints((N,), -4, 4, s + 2))


def up2_const_ref(case, inp):
    """The fp64 reference [B, 2h, 2w, N] of the constant family, its preconditions asserted:
      * the four fp32 weights of every output pixel sum to 1 within 2**-22 (each is a product of two fp32 numbers in [0, 1], rounded
        once: 4 x 2**-25, plus what 1 - w loses: nothing, w being a multiple of 2**-24 below 1). v times the weights, summed in fp32
        in any order with or without fused multiply-adds, is then within |v| (2**-22 + 4 x 2**-24) of v, and half an fp16 ulp of an
        integer |v| <= 3 is |v| 2**-12 or more: the patch holds v itself, and exact zeros outside the image;
      * the fp32 evaluation of the kernel's own expression gives exactly that (a check of the argument, not a replacement for it);
      * every partial sum of the convolution stays below 2**24 and every output is an integer of magnitude <= 2048."""
    B, h, w, C, N, _ = case
    H, W = 2 * h, 2 * w
    d = {k: v.double() for k, v in inp.items()}
    assert bool((d["x"] == d["x"][:, :, :1, :1]).all()) and float(d["x"].abs().max()) <= 3
    ones = torch.ones(1, 1, h, w, dtype=F64)
    for contracted in (False, True):
        assert float((interp_image(ones, H, W, "f64", contracted) - 1).abs().max()) <= 2.0 ** -22
    big = d["x"].expand(B, C, h, w)[:, :, :1, :1].expand(B, C, H, W)
    assert torch.equal(interp_image(inp["x"], H, W, "sum4_f32"), big), "the interpolated constant is the constant"
    ref = conv_image(big, d["w"]) + d["bias"]
    assert_exact_safe_f16([conv_image(big.abs(), d["w"].abs()) + d["bias"].abs()], [ref])
    return ref


def up2_selector_x(case):
    """x [B, C, h, w]: integers in [-64, 64]; a step of one frame, row, column or channel changes the value by 29, 37, 11 or 7 mod 129."""
    B, h, w, C, _, _ = case
    b, c, y, x = torch.meshgrid(torch.arange(B), torch.arange(C), torch.arange(h), torch.arange(w), indexing="ij")
    return ((29 * b + 37 * y + 11 * x + 7 * c + 5) % 129 - 64).to(F32)


def up2_selector_sets(case):
    """[(w [N, C, 3, 3] of zeros and one 1 per cout, picks [(tap, channel)] per cout)]: as many sets as it takes for every
    (tap, 16-channel k-step, 8-channel chunk) to be some cout's pick; the channel inside the chunk varies with the cout."""
    _, _, _, C, N, _ = case
    nk = C // UP2_KC
    ncombo = 9 * nk * 2
    sets = []
    for s in range(-(-ncombo // N)):
        w, picks = torch.zeros(N, C, 3, 3), []
        for n in range(N):
            jj = s * N + n
            j = jj % ncombo
            tap, ks, chunk = j % 9, (j // 9) % nk, j // (9 * nk)
            ch = 16 * ks + 8 * chunk + (3 * jj + jj // ncombo) % 8
            w[n, ch, tap // 3, tap % 3] = 1.0
            picks.append((tap, ch))
        sets.append((w, picks))
    return sets


def up2_selector_coverage(case):
    """The (tap, k-step, chunk) triples picked by some cout of some set."""
    return {(tap, ch // 16, (ch // 8) % 2) for _, picks in up2_selector_sets(case) for tap, ch in picks}


def up2_selector_bound(r, h, w, amax):
    """|y - r| <= ulp16(r) / 2 + 2**-22 max(h, w) amax + 2**-22 amax for the fp16 output y of a kernel that evaluates the definition
    r (interp_image "f64": a00 (1-wx)(1-wy) + ... in fp64 on the fp32 coordinates of ac_coords) in fp32, in any order. Derivation,
    with y' the kernel's fp32 value, |y - r| <= |y - y'| + |y' - r|:
      * ulp16(r) / 2 - the one rounding of y' to fp16 (ulp16 floors at the subnormal spacing 2**-24, so the term never vanishes).
      * 2**-22 max(h, w) amax - the coordinate. We take w = src - i0 of src = fl32(scale dst), an exact difference. A compiler
        that contracts scale dst - i0 into one fused operation sees the unrounded product instead: its weight differs by the rounding
        of src, at most half an ulp of a number below max(h, w): 2**-24 max(h, w). The value is bilinear in (wx, wy) with slopes
        |a01 - a00|, |a10 - a00|, ... <= 2 amax, and there are two axes: 2 x 2 amax x 2**-24 max(h, w).
      * 2**-22 amax - the fp32 evaluation on given weights. 1 - w is exact from the second source cell on (w is a multiple of 2**-23
        there); a weight product u v <= 1 is rounded by <= 2**-25, four of them against |a| <= amax: 2**-23 amax; the four products
        a w and the three additions are rounded by <= 2**-24 of partial sums that are convex combinations of the corners,
        |.| <= amax, or not at all where they are fused: <= 2**-23 amax once the products' errors are weighted by the w that sum to 1.
    This is a first-order count: it does not add the cross terms, the first source cell's 1 - w (2**-25 more per axis) or the
    contracted weight's own rounding, which a strict worst case with every error aligned would - one more 2**-22 amax, against
    slack of at least that size in the coordinate term wherever max(h, w) is not just past a power of two. It is therefore CHECKED,
    not trusted: tests/test_exact_inputs.py evaluates two orders (conv_up.hip's four-weight sum; torch's F.interpolate in fp32)
    against the plain and the contracted coordinates for every case and at (17, 33), (148, 5), (5, 148), (148, 148), (1, 7):
    the worst error is 0.98 of the bound, nearly all of it the fp16 rounding. A wrong pixel, tap or channel is an error of 7 or more."""
    return ulp16(r) / 2 + 2.0 ** -22 * max(h, w) * amax + 2.0 ** -22 * amax


# ------------------------------------------------------------------------------------------------ vda_depth_tail_f16 with a resize, dyadic scales
# (B, h, w, H, W) x C: resize h x w -> H x W, conv3x3(C -> 32) + ReLU, conv1x1(32 -> 1) + ReLU, fp32 out
TAILUP_CASES = [
    (1, 1, 1, 5, 7),             # both scales 0
    (2, 9, 17, 17, 33),          # 1/2 in both axes; two tile rows and columns of the 16 x 32 persistent tile, the second one pixel wide
    (1, 5, 9, 17, 33),           # 1/4 in both axes
    (1, 9, 9, 17, 33),           # 1/2 in y, 1/4 in x
    (1, 17, 9, 17, 33),          # rows identical, columns 1/4
    (1, 17, 17, 17, 33),         # rows identical, columns 1/2: the source region exceeds 256 pixels -> depth_tail_kernel<1>
    (1, 33, 65, 17, 33),         # downsampling by 2: the same fallback
    (1, 7, 5, 5, 9),             # 3/2 in y, 1/2 in x
]
TAILUP_C = [32, 64, 128]
TAIL_KERNELS = ("depth_tail_kernel<0>", "depth_tail_kernel<1>", "depth_tail_up_kernel")     # vda_depth_tail_last_kernel: identity, resize, persistent resize
TAIL_SRC_ROWS = 256              # v2::SRC_ROWS of tail.hip


def tailup_many_tiles_case(ncu):
    """More 16 x 32 tiles (9 per frame) than compute units: a persistent workgroup takes a second tile."""
    return (ncu // 9 + 1, 17, 33, 33, 65)


def tailup_id(c):
    return "B%d-%dx%d-to-%dx%d" % c


def tail_src_extent(n_in, n_out, tile):
    """v2::src_extent of tail.hip (halo_lo = -1): the source rows / columns the dispatcher sizes a tile's region with."""
    scale = torch.tensor(ac_coords(n_in, n_out)[3], dtype=F32)
    ext = 1
    for o0 in range(0, n_out, tile):
        lo, hi = max(o0 - 1, 0), min(o0 + tile, n_out - 1)
        a = min(int(scale * torch.tensor(float(lo), dtype=F32)), n_in - 1)
        b = min(int(scale * torch.tensor(float(hi), dtype=F32)) + 1, n_in - 1)
        ext = max(ext, b - a + 1)
    return ext


def tailup_kernel(case, variant=0):
    """The kernel vda_depth_tail_f16 must run for a case under vda_depth_tail_set_variant(variant)."""
    B, h, w, H, W = case
    if h == H and w == W:
        return TAIL_KERNELS[0]
    fits = tail_src_extent(h, H, 16) * tail_src_extent(w, W, 32) <= TAIL_SRC_ROWS
    return TAIL_KERNELS[2] if fits and variant != 1 else TAIL_KERNELS[1]


def assert_dyadic(h, w, H, W):
    """Both align_corners scales are in {0, 1/4, 1/2, 1, 3/2, 2} - exact in fp32, every src = scale * dst exact, every weight a multiple of 1/4."""
    for n_in, n_out in ((h, H), (w, W)):
        s = ac_coords(n_in, n_out)[3]
        assert s in (0.0, 0.25, 0.5, 1.0, 1.5, 2.0), f"scale {s} of {n_in} -> {n_out}"
        assert n_out == 1 or s * (n_out - 1) == n_in - 1, "the fp32 scale is the exact ratio"
        wgt = ac_coords(n_in, n_out)[2] * 4
        assert bool((wgt == wgt.round()).all())


def tailup_inputs(case, Cc):
    """As tail16_inputs, but w3 in [-1, 3] and b3 in [0, 4]: with symmetric ranges the last ReLU leaves half of a small case's
    outputs (all 35 of the 1 x 1 image's, at C = 64) at zero, where nothing can be seen."""
    B, h, w, H, W = case
    s = 12000 + 17 * (TAILUP_CASES.index(case) if case in TAILUP_CASES else 29) + Cc
    return dict(x=ints((B, Cc, h, w), -3, 3, s), w2=ints((32, Cc, 3, 3), -2, 2, s + 1), b2=ints((32,), -4, 4, s + 2), w3=ints((32,), -1, 3, s + 3),
                b3=float(ints((1,), 0, 4, s + 4)))


def dyadic_resize_ref(x, H, W):
    """fp64 resize [B, C, H, W] of integer x with |x| <= 3 at dyadic scales, its exactness asserted: a multiple of 1/16 with |v| <= 3,
    equal to torch's own fp64 F.interpolate. Products a * w (w a multiple of 1/16 <= 1) and every partial sum of the four are then
    multiples of 1/16 below 16: fp16 values, so the packed-fp16 chain of bilinear8, the fp32 four-term sum and the nested fp32
    lerp all give this value without a rounding."""
    assert_dyadic(x.shape[2], x.shape[3], H, W)
    assert bool((x == x.round()).all()) and float(x.abs().max()) <= 3
    up = interp_image(x, H, W, "f64")
    assert bool((up * 16 == (up * 16).round()).all()) and float(up.abs().max()) <= 3
    assert torch.equal(up, F.interpolate(x.double(), size=(H, W), mode="bilinear", align_corners=True))
    return up


def tailup_ref(case, inp, b3):
    """fp64 reference [B, H, W] with its preconditions: the resize is exact (dyadic_resize_ref), and in units of 1/16 every partial
    sum of both convolutions stays below 2**24 - the fp32 MFMA chain and the fp32 epilogue are exact in any order."""
    B, h, w, H, W = case
    d = {k: v.double() for k, v in inp.items()}
    a = {k: v.abs() for k, v in d.items()}
    up, upa = dyadic_resize_ref(d["x"], H, W), dyadic_resize_ref(a["x"], H, W)
    assert bool((upa >= up.abs()).all())
    assert_exact_safe(16 * tail16_ref(dict(a, x=upa), abs(b3)), 16 * F.conv2d(upa, a["w2"], a["b2"], padding=1))
    return tail16_ref(dict(d, x=up), b3)


def tail_epilogue(lin, d, b3):
    """[B, H, W, 32] conv sums -> ReLU(sum_co ReLU(lin + b2) w3 + b3)."""
    return F.relu((F.relu(lin + d["b2"]) * d["w3"]).sum(-1) + b3)


# ------------------------------------------------------------------------------------------------ vda_bilinear_nhwc_f16 / _f32, dyadic scales
BILINEAR_DYADIC_C = [32, 192]


def bilinear_dyadic_inputs(case, Cc):
    B, h, w, H, W = case
    s = 13000 + 17 * TAILUP_CASES.index(case) + Cc
    return dict(x=ints((B, Cc, h, w), -3, 3, s), add=ints((B, Cc, H, W), -4, 4, s + 1))


def bilinear_dyadic_refs(case, inp):
    """(resize, resize + add) as fp64 NHWC [B, H, W, C]: multiples of 1/16 up to 7, fp16 values - the kernel's nested fp32 lerp, the
    addition and the fp16 store are all exact."""
    B, h, w, H, W = case
    up = dyadic_resize_ref(inp["x"].double(), H, W)
    both = up + inp["add"].double()
    assert_exact_safe_f16([16 * (up.abs() + inp["add"].double().abs())], [up, both], step=1.0 / 16)
    return up.permute(0, 2, 3, 1).contiguous(), both.permute(0, 2, 3, 1).contiguous()
