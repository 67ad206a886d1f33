"""The fp16 attention kernels (attention.hip: four kernels behind eleven variant codes; temporal.hip: the MFMA and the VALU kernel) at
their wave, key-tile and query-block edges, with inputs whose softmax is exact.

Softmax is not linear, so small integers alone do not make it exact; three input families do (tests/_exact.py, each with its
precondition asserted here for every case; shown sound - and the equalities shown able to fail - on the CPU in
tests/test_exact_inputs.py):
  selector   every query carries the code of one key, whose score leads every other by >= 51.9 (log2). Once a query has seen its
             winner every running-maximum or lazy reference point IS the winner's score (a lead of 26 or more forces the move in codes
             8 - 11 alike), the winner's p is 1 (codes 0 - 3 and 7: 1 +- 3e-6, the rounding of m * log2(e); codes 4 and 5: 1 +- 2e-5,
             the fp16 pair), every other p is 0 in fp16 and nothing against 1 in the fp32 row sum, what was accumulated before is
             scaled by 2^-51: the output is the winner's V row - integers up to 1019 - BIT FOR BIT. One key dropped, a stale V tile, a
             wrong fragment index in one tile, a head, frame or query row in the wrong place: an inequality.
  counting   q = 0: every p is 1, the row sum N, the numerator a count of keys. A key dropped or a clamped copy of key N - 1 left
             unmasked changes a channel by 64 / N of its value (the selector cannot see a key counted twice: softmax normalises it
             away). Equality at N a power of two, one fp16 ulp elsewhere (E.counting_check).
  straddle   (real-valued, the existing 3e-3) a whole key tile whose row sum is 1650 for even queries and 2478 for odd ones: either
             side of the shipped kernel's fast / slow decision (qsum <= 2048), lane by lane in every wave.

qkv is a 16-byte-aligned view into a NaN-filled allocation with eight rows of NaN either side (a masked score gives p = 0, and
0 * NaN = NaN: a read past the input shows only if NaN sits there); the output a buffer of one NaN bit pattern with eight rows
behind it: nothing outside the kernel's region may change, nothing inside may be left, everything inside is finite."""
import functools

import pytest
import torch

import _exact as E
from _exact import check_sentinel, guarded, sentinel_out_f16
from test_kernels_f16_edges_gpu import L  # noqa: F401  (fixture)
from test_kernels_gpu import attn_ref, close, ops, rnd  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

F16, F32, F64 = torch.float16, torch.float32, torch.float64
variants = pytest.mark.parametrize("variant", E.ATTN_VARIANTS)
# every case under every variant; the workload's N once, under the default and the plain running-maximum kernel
CASE_GRID = [(v, c) for v in E.ATTN_VARIANTS for c in E.ATTN_CASES] + [(v, E.ATTN_BIG_CASE) for v in E.ATTN_BIG_VARIANTS]
case_grid = pytest.mark.parametrize("variant,case", CASE_GRID, ids=lambda x: E.attn_case_id(x) if isinstance(x, tuple) else "v%d" % x)


def h16(t):
    assert torch.equal(t.to(F16).to(t.dtype), t), "an operand is not an fp16 value"
    return t.to(F16)


def run_guarded(launch, qkv, rows, width, what):
    """Launch on a guarded fp16 copy of qkv ([..., row length]) into a sentinel buffer of rows x width (+ 8); the owned region on the host."""
    row = qkv.shape[-1]
    x = guarded(h16(qkv), rows_after=8, pad_elems=8 * row)
    out = sentinel_out_f16(rows, width, width)
    launch(x, out)
    torch.cuda.synchronize()
    check_sentinel(out, rows, width, what)
    y = out[:rows].cpu()
    bad = ~torch.isfinite(y.float())
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} non-finite outputs, first at {bad.nonzero()[0].tolist()}"
    return y


def attention(ops, L, qkv, B, N, H, variant, what):
    assert L.lib.vda_attention_set_variant(variant) == 0
    try:
        y = run_guarded(lambda x, out: ops.attention(x, out, B, N, H), qkv, B * N, H * 64, f"{what}, variant {variant}, B={B} N={N} H={H}")
    finally:
        L.lib.vda_attention_set_variant(-1)
    return y.reshape(B, N, H * 64)


@functools.lru_cache(maxsize=None)
def selector_case(case):
    """Inputs, winners and V[pi] of one case, with the preconditions asserted: built once, shared by the variants, never written to."""
    B, N, H = case
    qkv, pi = E.attn_selector_inputs(B, N, H, E.attn_seed(case))
    E.assert_selector_safe(qkv, pi, B, N, H)
    return qkv, E.selector_expected(qkv, pi, B, N, H)


@functools.lru_cache(maxsize=None)
def counting_case(case):
    B, N, H = case
    qkv = E.attn_counting_inputs(B, N, H, E.attn_seed(case))
    v = qkv.reshape(B, N, 3, H, 64)[:, :, 2].double()
    E.assert_exact_safe(v.sum(dim=1))                               # the numerators: integer counts below 2**24
    assert not bool(qkv.reshape(B, N, 3, H * 64)[:, :, 0].any()) and float((E.attn_ref64(qkv, B, N, H) - E.counting_expected(B, N, H)).abs().max()) <= 1e-15
    return qkv


@functools.lru_cache(maxsize=None)
def straddle_case(N):
    qkv = E.attn_straddle_inputs(N, 9900 + N)
    for log2_q in (False, True):
        even, odd = E.straddle_tile_sums(qkv, log2_q)
        assert even <= E.ATTN_SUM_LIMIT * 0.92 and odd >= E.ATTN_SUM_LIMIT * 1.08, (even, odd)
    return qkv, E.attn_ref64(qkv, 1, N, 1)


# ---------------------------------------------------------------- spatial attention
@case_grid
def test_attention_f16_selects_the_coded_key(ops, L, variant, case):
    B, N, H = case
    qkv, expect = selector_case(case)
    y = attention(ops, L, qkv, B, N, H, variant, "selector")
    msg = E.selector_mismatch(y, expect, qkv.reshape(B, N, 3, H, 64)[:, :, 2])
    assert msg is None, f"variant {variant}, B={B} N={N} H={H}: {msg}"


@case_grid
def test_attention_f16_counts_every_key_once(ops, L, variant, case):
    """Equality where N is a power of two (1, 32, 64, 128); elsewhere within one fp16 ulp of the fp64 value rounded to fp16
    (E.counting_check has the derivation). A key dropped or doubled: 64 / N of a channel's value, 4.7 % at N = 1370, against 2**-10."""
    B, N, H = case
    y = attention(ops, L, counting_case(case), B, N, H, variant, "counting")
    ok, worst = E.counting_check(y, B, N, H)
    if N & (N - 1):
        print(f"attention f16 counting, variant {variant}, B={B} N={N} H={H}: worst error {worst:.3f} fp16 ulp")
    assert ok, f"variant {variant}, B={B} N={N} H={H}: {worst:.3f} fp16 ulp from the counts over N ({'equality' if N & (N - 1) == 0 else 'bound: 1'})"


@variants
def test_attention_f16_sum_limit_straddle(ops, L, variant):
    """Even queries below attn_cs_kernel's SUM_LIMIT on key tile 1 (fast path, p ~ 26 in fp16), odd queries above it (slow path: the
    reference point moves by 5.27 and the tile's p is recomputed), in the same wave; N = 129, 192: a last tile of one key / none
    partial; 160: half a tile; 449: six more tiles on the moved reference point. Every kernel must agree on the same inputs: fp64
    reference, the attention bound of tests/test_kernels_gpu.py."""
    for N in E.ATTN_STRADDLE_N:
        qkv, ref = straddle_case(N)
        y = attention(ops, L, qkv, 1, N, 1, variant, "straddle")
        err = (y.double() - ref).abs() / (E.ATTN_TOL + E.ATTN_TOL * ref.abs())
        for par, name in ((0, "even (fast)"), (1, "odd (slow)")):
            print(f"attention f16 straddle, variant {variant}, N={N}, {name} queries: worst error {float(err[0, par::2].max()):.3f} of the bound")
        close(y, ref, rtol=E.ATTN_TOL, atol=E.ATTN_TOL, what=f"attention straddle, variant {variant}, N={N}")


@variants
def test_attention_f16_rows_are_position_independent(ops, L, variant):
    """test_attention_rows_are_position_independent's construction under every variant: the same 137 tokens as frames 0 and 1 of a
    batch give bit-identical rows; rotated by one row (other lanes, other neighbours) they stay within the attention bound."""
    N, H = 137, 2
    a = rnd(N, 3 * H * 64, seed=48, scale=1.5).to(F16)
    y = attention(ops, L, torch.stack([a, a]).float(), 2, N, H, variant, "two copies")
    assert torch.equal(y[0].view(torch.int16), y[1].view(torch.int16)), f"variant {variant}: two frames with the same qkv differ"
    b = torch.cat([a[-1:], a[:-1]])
    y2 = attention(ops, L, b[None].float(), 1, N, H, variant, "rotated")
    ref = attn_ref(a[None], 1, N, H)[0]
    close(y2[0, 1:], ref[:-1], rtol=E.ATTN_TOL, atol=E.ATTN_TOL, what=f"rotated sequence, variant {variant}")
    close(y[0], ref, rtol=E.ATTN_TOL, atol=E.ATTN_TOL, what=f"variant {variant}")


# ---------------------------------------------------------------- temporal attention
def temporal(ops, L, qkv, T, hw, C, heads, variant, what):
    L.lib.vda_temporal_attention_set_variant(variant)              # 1: MFMA kernel for d = 32 / 64 / 128, 0: VALU kernel
    try:
        return run_guarded(lambda x, out: ops.temporal_attention(x, out, T, hw, C, heads), qkv, T * hw, C,
                           f"{what}, variant {variant}, T={T} hw={hw} C={C} heads={heads}")
    finally:
        L.lib.vda_temporal_attention_set_variant(1)


@functools.lru_cache(maxsize=None)
def tattn_selector_case(T, hw, C, heads):
    qkv, pi = E.tattn_selector_inputs(T, hw, C, heads, E.tattn_seed(T, hw, C, heads))
    E.assert_tattn_selector_safe(qkv, pi, T, hw, C, heads)
    return qkv, E.tattn_selector_expected(qkv, pi, T, hw, C, heads)


@pytest.mark.parametrize("variant", [1, 0], ids=["mfma", "valu"])
@pytest.mark.parametrize("C,heads", E.TATTN_SELECTOR_GEOM)
def test_temporal_attention_f16_selects_the_coded_frame(ops, L, C, heads, variant):
    """T = 1 (one key), 15 / 16 / 17 (the VALU kernel's two 16-query halves), 31 / 32; one pixel and three; 1, 2, 4 and 8 heads (waves
    with head >= heads return early in the MFMA kernel; the VALU launcher's head group follows heads). The output is V[pi] bit for bit."""
    for T in E.TATTN_T:
        for hw in E.TATTN_HW:
            qkv, expect = tattn_selector_case(T, hw, C, heads)
            y = temporal(ops, L, qkv, T, hw, C, heads, variant, "temporal selector")
            if not torch.equal(y.double(), expect):
                bad = y.double() != expect
                row, col = bad.nonzero()[0].tolist()
                d = C // heads
                raise AssertionError(f"variant {variant}, T={T} hw={hw} C={C} heads={heads}: {int(bad.sum())}/{bad.numel()} elements differ from V[pi], first at "
                                     f"frame {row // hw} pixel {row % hw} head {col // d} channel {col % d}: {float(y[row, col])} != {float(expect[row, col])}")


@pytest.mark.parametrize("variant", [1, 0], ids=["mfma", "valu"])
@pytest.mark.parametrize("C,heads", E.TATTN_SMALL_GEOM)
def test_temporal_attention_f16_frame_count_edges(ops, L, C, heads, variant):
    """ViT-S's head dims (8, 24, 48: the VALU kernel under either variant) at the same frame counts and pixel counts: Gaussian inputs,
    fp64 reference, test_temporal_attention's bound."""
    for T in E.TATTN_T:
        for hw in E.TATTN_HW:
            qkv = rnd(T * hw, 3 * C, seed=45 + T + hw).to(F16).float()
            y = temporal(ops, L, qkv, T, hw, C, heads, variant, "temporal")
            close(y, E.tattn_ref64(qkv, T, hw, C, heads), what=f"temporal attention variant {variant} T={T} hw={hw} C={C}")
