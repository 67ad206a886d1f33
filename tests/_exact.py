"""Exact-integer inputs and references for the fp32 GEMM's linear surface (dense, conv3x3, ConvTranspose, patch embed).

With small integer operands every product and every partial sum of a contraction is an integer; while all of them stay below
2**24 they are exactly representable in fp32, so an fp32 fmaf / MFMA chain reproduces the fp64 result BIT FOR BIT in any
summation order. "Which row, which tap, which pad, which column, which tile" then become equalities without a tolerance.
The condition is checked, not assumed: `assert_exact_safe` takes the reference evaluated with |operand| everywhere, which
bounds every partial sum of every ordering.

The case lists and input builders live here so that tests/test_exact_inputs.py (CPU: the inputs meet the condition and the
equalities can fail) and tests/test_kernels_f32_edges_gpu.py (GPU: the kernels meet them) use the same tensors."""
import torch
import torch.nn.functional as F

F32, F64 = torch.float32, torch.float64
EXACT_LIMIT = float(2 ** 24)
SENTINEL_BITS = 0x7FC5A5A5            # one fixed quiet-NaN bit pattern: never the result of arithmetic on finite inputs
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


def check_sentinel(buf, M, N, what=""):
    bits = buf.view(torch.int32).cpu()
    assert bool((bits[M:] == SENTINEL_BITS).all()), f"{what}: wrote past the last row ({int((bits[M:] != SENTINEL_BITS).sum())} elements)"
    assert bool((bits[:M, N:] == SENTINEL_BITS).all()), f"{what}: wrote into the columns [N, ldc) ({int((bits[:M, N:] != SENTINEL_BITS).sum())} elements)"
    left = bits[:M, :N] == SENTINEL_BITS
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
