"""The row-normalisation kernels of csrc/norm.hip - vda_layernorm_f32_f16 / _f32, vda_layernorm_residual_f32_f16, vda_split_stats_f32,
vda_split_center_stats_f32, vda_layernorm_split_f16, vda_ln_stats_finalize, vda_groupnorm_nhwc_f16 / _f32 - at the edges of their
ladder, with inputs of tests/_norm_inputs.py whose statistics are exact (each shown sound, and each assertion shown able to fail, on the
CPU in tests/test_norm_inputs.py):

  1  exact rows      x = m + a * s (+-1 balanced): mean, centred values and variance are exact in any order, the fp16 output IS the integer
                     s * w + b (+ pe) - torch.equal; the fp32 output within 7 * 2**-24 * (|w| + |b| + |pe|) (counted roundings). Both sides
                     of every rung, 1 / R - 1 / R / R + 1 / 2 R + 3 rows around the R rows of a workgroup, group / skip compaction, pe.
  2  bit agreement   real-valued rows: the kernels that share load_row_stats agree to the bit, rows do not depend on their position.
  3  ill-conditioned rows against fp64 within the two-pass forward bound.
  4  vda_ln_stats_finalize: exact partials, real partials within the bound of np Chan updates, the overflow flag.
  5  GroupNorm: exact inputs (identical bits for every `chunks`), geometry around the kernels' blocks, the one-pass bound.
  6  refusals.

Every output is a sentinel buffer with 8 rows behind the result: nothing outside may change, nothing inside may be left. Every
equality is asserted without a tolerance; every tolerance is a formula derived beside it (here or in _norm_inputs.py), none was fitted to
what the kernels return."""
import pytest
import torch

import _norm_inputs as NI
from _exact import SENTINEL16_BITS, SENTINEL_BITS, check_sentinel, sentinel_out, sentinel_out_f16
from _norm_inputs import F16, F32, F64, LnCase, U
from test_kernels_gpu import ops  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def dev(t, dtype=F32):
    return None if t is None else t.to(dtype).contiguous().cuda()


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == F16 else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def untouched(buf):
    torch.cuda.synchronize()
    return bool((bits(buf).cpu() == (SENTINEL16_BITS if buf.dtype == F16 else SENTINEL_BITS)).all())


def out_buffer(rows, D, dtype):
    return sentinel_out_f16(rows, D, D) if dtype == F16 else sentinel_out(rows, D, D)


# ---------------------------------------------------------------- 1. exact-statistics rows
def run_ln(ops, case, inp):
    """One launch of the case's entry into sentinel buffers; the dict NI.ln_mismatch takes, after the sentinel checks."""
    D, rows, e, what = case.D, case.rows, case.entry, NI.ln_case_id(case)
    if e in ("stats", "center_stats"):
        hi, lo, stat = sentinel_out_f16(rows, D, D), sentinel_out_f16(rows, D, D), sentinel_out(rows, 2, 2)
        ops.split_stats(dev(inp["x"]), hi, lo, stat, case.eps, rows, D, center=e == "center_stats")
        torch.cuda.synchronize()
        for buf, n, name in ((hi, D, "hi"), (lo, D, "lo"), (stat, 2, "stat")):
            check_sentinel(buf, rows, n, f"{what} {name}")
        return dict(hi=hi[:rows].cpu(), lo=lo[:rows].cpu(), stat=stat[:rows].cpu())
    rows_out = inp["rows_out"]
    out = out_buffer(rows_out, D, F32 if e == "layernorm_f32" else F16)
    w, b = dev(inp["w"]), dev(inp["b"])
    got = {}
    if e in ("layernorm_f16", "layernorm_f32"):
        ops.layernorm(dev(inp["x"]), out, w, b, case.eps, rows, D, group=case.group, skip=case.skip, pe=dev(inp["pe"]),
                      pe_rows_per_step=case.prs, pe_steps=case.steps)
    elif e == "split":
        ops.layernorm_split(dev(inp["hi"], F16), dev(inp["lo"], F16), out, w, b, case.eps, rows, D, group=case.group, skip=case.skip)
    else:
        stream = sentinel_out(rows, D, D)
        stream[:rows] = dev(inp["x0"])
        ops.layernorm_residual(stream, dev(inp["y"], F16), dev(inp["gamma"]), out, w, b, case.eps, rows, D, group=case.group, skip=case.skip)
        torch.cuda.synchronize()
        check_sentinel(stream, rows, D, f"{what} stream")
        got["stream"] = stream[:rows].cpu()
    torch.cuda.synchronize()
    check_sentinel(out, rows_out, D, f"{what} out")
    got["out"] = out[:rows_out].cpu()
    return got


def check_ln_cases(ops, cases):
    assert cases
    for case in cases:
        inp = NI.ln_inputs(case)                          # (asserts the preconditions)
        bad = NI.ln_mismatch(case, inp, run_ln(ops, case, inp))
        assert bad is None, f"{NI.ln_case_id(case)}: {bad}"


@pytest.mark.parametrize("D", NI.LN_D)
@pytest.mark.parametrize("entry", NI.LN_ENTRIES)
def test_exact_rows_on_both_sides_of_every_rung(ops, entry, D):
    """rows = 1, R - 1, R, R + 1, 2 R + 3 for the rung's R rows per workgroup. fp16 outputs equal the integer n; planes equal fp16(x)
    (or +-a) and 0; stat[:, 0] is m (or 0) exactly and stat[:, 1] within 2 ulp of 1 / sqrt(a**2 + eps) (var + eps rounds once - half an
    ulp after the root - and rsqrtf is within one); the residual entries leave x0 + gamma * y = x in the stream, bit for bit.
    layernorm_f32: |y - ref| <= 7 * 2**-24 * (|w| + |b| + |pe|) against ((x - mean) * rstd) * w + b (+ pe) in fp64 - one rsqrtf ulp and
    the rounding of var + eps (2.5 U on rstd), two multiplies (U each), the add of b (U), the add of pe (U), each relative to a magnitude
    of at most |w| + |b| + |pe|: 6.5 U, fewer than 7 ulps of |w| + |b| + |pe| (NI.ln_f32_ref_and_bound)."""
    check_ln_cases(ops, [c for c in NI.ln_shape_cases(entry) if c.D == D])


@pytest.mark.parametrize("shape", NI.LN_GROUP_SHAPES, ids=lambda s: f"D{s[0]}-r{s[1]}")
@pytest.mark.parametrize("entry", NI.LN_COMPACTING)
def test_exact_rows_group_skip_compaction(ops, entry, shape):
    """(group, skip) in (1, 0), (5, 1), (5, 2), (5, 4), (rows, 1): row r lands at g * (group - skip) + i - skip, the slot of a dropped row
    is not written (the sentinel behind row rows - dropped stays), and the residual entries update the stream of dropped rows too."""
    check_ln_cases(ops, [c for c in NI.ln_group_cases(entry) if (c.D, c.rows) == shape])


@pytest.mark.parametrize("entry", ["layernorm_f16", "layernorm_f32"])
def test_exact_rows_pe_steps_follow_the_input_row(ops, entry):
    """pe_rows_per_step in {1, 6}, pe_steps in {1, 4}, and once under group = 5, skip = 1: out += pe[(r / pe_rows_per_step) % pe_steps]
    with r the INPUT row (include/vda.h)."""
    check_ln_cases(ops, NI.ln_pe_cases(entry))


# ---------------------------------------------------------------- 2. bit agreement between the kernels
def real_case(D, seed=0):
    rows = 2 * NI.ln_rung(D)[2] + 3
    x = NI.real_rows(rows, D, 300 + D + seed)
    w, b = NI.real_affine(D, 400 + D)
    return rows, x, w, b


def ln_out(ops, x, w, b, rows, D, dtype, eps=1e-6):
    out = out_buffer(rows, D, dtype)
    ops.layernorm(x, out, w, b, eps, rows, D)
    torch.cuda.synchronize()
    check_sentinel(out, rows, D, "layernorm")
    return out[:rows].cpu()


BIT_D = NI.LN_RUNG_D + [72]


@pytest.mark.parametrize("D", BIT_D)
def test_layernorm_split_equals_layernorm_of_the_register_image(ops, D):
    """layernorm_split(hi, lo) == layernorm(hi.float() + lo.float()), bit for bit: that fp32 sum is the kernel's own register image."""
    rows, x, w, b = real_case(D)
    hi, lo = NI.split_planes(x)
    img = hi.float() + lo.float()
    out = sentinel_out_f16(rows, D, D)
    ops.layernorm_split(dev(hi, F16), dev(lo, F16), out, dev(w), dev(b), 1e-6, rows, D)
    torch.cuda.synchronize()
    check_sentinel(out, rows, D, "layernorm_split")
    assert same_bits(out[:rows].cpu(), ln_out(ops, dev(img), dev(w), dev(b), rows, D, F16))


@pytest.mark.parametrize("gamma", [True, False], ids=["gamma", "no_gamma"])
@pytest.mark.parametrize("D", BIT_D)
def test_layernorm_residual_equals_layernorm_of_the_stream_it_leaves(ops, D, gamma):
    rows, x, w, b = real_case(D)
    y = NI.real_rows(rows, D, 500 + D).to(F16)
    g = dev(NI.real_affine(D, 600 + D)[0]) if gamma else None
    stream, out = dev(x), sentinel_out_f16(rows, D, D)
    ops.layernorm_residual(stream, dev(y, F16), g, out, dev(w), dev(b), 1e-6, rows, D)
    torch.cuda.synchronize()
    check_sentinel(out, rows, D, "layernorm_residual")
    assert not torch.equal(stream.cpu(), x), "the stream was updated"
    assert same_bits(out[:rows].cpu(), ln_out(ops, stream, dev(w), dev(b), rows, D, F16))


@pytest.mark.parametrize("D", BIT_D)
def test_layernorm_f16_output_is_the_rounded_f32_output(ops, D):
    """Round to nearest even of the fp32 entry's output."""
    rows, x, w, b = real_case(D)
    y32, y16 = (ln_out(ops, dev(x), dev(w), dev(b), rows, D, t) for t in (F32, F16))
    assert same_bits(y16, y32.to(F16))


@pytest.mark.parametrize("D", BIT_D)
def test_split_stats_agree_with_each_other_and_with_layernorm(ops, D):
    """split_stats and split_center_stats give the same rstd bits, and split_stats' (mean, rstd) reproduces layernorm's fp32 output
    through ((x - mean) * rstd) * w + b in fp32 to within 1 ulp - of the larger of the product and the result: the kernel may contract
    the multiply-add, which skips the rounding of the product (half an ulp of it) before the final one (half an ulp of the result)."""
    rows, x, w, b = real_case(D)
    stats = []
    for center in (False, True):
        hi, lo, stat = sentinel_out_f16(rows, D, D), sentinel_out_f16(rows, D, D), sentinel_out(rows, 2, 2)
        ops.split_stats(dev(x), hi, lo, stat, 1e-6, rows, D, center=center)
        torch.cuda.synchronize()
        for buf, n in ((hi, D), (lo, D), (stat, 2)):
            check_sentinel(buf, rows, n, f"split_stats center={center}")
        stats.append(stat[:rows].cpu())
        if not center:
            assert same_bits(hi[:rows].cpu(), x.to(F16)) and same_bits(lo[:rows].cpu(), (x - x.to(F16).float()).to(F16)), "hi = fp16(x), lo = fp16(x - hi)"
    assert same_bits(stats[0][:, 1], stats[1][:, 1]) and bool((stats[1][:, 0] == 0).all())
    mean, rstd = stats[0][:, :1], stats[0][:, 1:]
    prod = (x - mean) * rstd * w
    y = ln_out(ops, dev(x), dev(w), dev(b), rows, D, F32)
    assert bool(((y.double() - (prod + b).double()).abs() <= NI.ulp32(torch.maximum(prod.abs(), y.abs()))).all())


@pytest.mark.parametrize("D", BIT_D)
def test_rows_do_not_depend_on_their_position(ops, D):
    """One row in every row of two workgroups and a ragged tail: all output rows are identical, and equal to a one-row launch's."""
    rows, x, w, b = real_case(D)
    one = x[3:4].contiguous()
    rep = one.expand(rows, D).contiguous()
    for dtype in (F32, F16):
        many, single = ln_out(ops, dev(rep), dev(w), dev(b), rows, D, dtype), ln_out(ops, dev(one), dev(w), dev(b), 1, D, dtype)
        assert same_bits(many, single.expand(rows, D).contiguous()), f"layernorm {dtype}"
    res = []
    for xs, n in ((rep, rows), (one, 1)):
        hi, lo, stat, out = sentinel_out_f16(n, D, D), sentinel_out_f16(n, D, D), sentinel_out(n, 2, 2), sentinel_out_f16(n, D, D)
        ops.split_stats(dev(xs), hi, lo, stat, 1e-6, n, D, center=True)
        ops.layernorm_split(hi[:n], lo[:n], out, dev(w), dev(b), 1e-6, n, D)
        torch.cuda.synchronize()
        check_sentinel(out, n, D, "layernorm_split")
        res.append((stat[:n].cpu(), hi[:n].cpu(), lo[:n].cpu(), out[:n].cpu()))
    for many, single in zip(*res):
        assert same_bits(many, single.expand_as(many).contiguous())


# ---------------------------------------------------------------- 3. ill-conditioned rows against fp64
ILL_ROWS = 9


def ill_reference(x64, w, b, eps):
    mean = x64.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(x64.var(1, unbiased=False, keepdim=True) + NI.f32(eps))
    yhat = (x64 - mean) * rstd
    return mean[:, 0], rstd[:, 0], yhat, yhat * w.double() + b.double()


@pytest.mark.parametrize("regime", [r for r in NI.ILL_REGIMES if r != "constant"])
@pytest.mark.parametrize("D", BIT_D)
def test_ill_conditioned_rows_within_the_two_pass_forward_bound(ops, D, regime):
    """layernorm (fp32 out), split_stats and layernorm_split on rows shifted by +40, with three channels at 400 / -650 / 900, both, and
    |x| ~ 1e4 with sigma ~ 1, against fp64.
    The bound (NI.ln_forward_bound): L = 3 + NCH + log2 LPR is the longest chain of fp32 additions of a row sum on the rung; the
    normalised value yhat is within (L + 4) * 2**-24 * (mean|x| * rstd + |yhat|) - the mean's error L U mean|x| (+ U for the division)
    reaches yhat through rstd, everything relative to yhat itself (the variance's chain halved by the root, the subtraction, the rsqrtf
    ulp, the multiply) is the |yhat| term. That times |w|; then the output's own roundings: 2 U (|yhat w| + |b|) for the multiply and
    the add in fp32, and half an fp16 ulp for the fp16 store. For the statistics: |mean - mean64| <= (L + 4) U mean|x|, and rstd
    relative (L + 4) U (mean|x| * rstd + 1), the same expression at |yhat| = 1.
    (The centred squares are summed along 8 NCH + log2 LPR sequential additions, so on the NCH = 4 rung a strict worst case of the |yhat|
    term would be 23 U, not 17 U: the bound asserted is the tighter one.)"""
    eps = 1e-6
    x = NI.ill_rows(regime, ILL_ROWS, D, 40 + D)
    w, b = NI.real_affine(D, D)
    mean, rstd, yhat, ref = ill_reference(x.double(), w, b, eps)
    fb = NI.ln_forward_bound(x.double(), yhat, D, eps)
    bound = fb * w.double().abs() + 2 * U * ((yhat * w.double()).abs() + b.double().abs())
    y = ln_out(ops, dev(x), dev(w), dev(b), ILL_ROWS, D, F32, eps).double()
    err = (y - ref).abs()
    print(f"layernorm_f32 D={D} {regime}: worst {float((err / bound).max()):.3g} of the bound")
    assert bool((err <= bound).all()), f"layernorm fp32: worst {float((err / bound).max()):.3g} of the bound"

    hi, lo, stat = sentinel_out_f16(ILL_ROWS, D, D), sentinel_out_f16(ILL_ROWS, D, D), sentinel_out(ILL_ROWS, 2, 2)
    ops.split_stats(dev(x), hi, lo, stat, eps, ILL_ROWS, D)
    torch.cuda.synchronize()
    check_sentinel(stat, ILL_ROWS, 2, "split_stats stat")
    st = stat[:ILL_ROWS].cpu().double()
    k = (NI.ln_chain(D) + 4) * U
    mabs = x.double().abs().mean(1)
    print(f"split_stats D={D} {regime}: mean {float(((st[:, 0] - mean).abs() / (k * mabs)).max()):.3g}, rstd {float(((st[:, 1] - rstd).abs() / (rstd * k * (mabs * rstd + 1))).max()):.3g} of the bound")
    assert bool(((st[:, 0] - mean).abs() <= k * mabs).all()), "split_stats mean"
    assert bool(((st[:, 1] - rstd).abs() <= rstd * k * (mabs * rstd + 1)).all()), "split_stats rstd"

    img = hi[:ILL_ROWS].cpu().double() + lo[:ILL_ROWS].cpu().double()             # what layernorm_split normalises (exact in fp64)
    _, _, yhat2, ref2 = ill_reference(img, w, b, eps)
    bound2 = NI.ln_forward_bound(img, yhat2, D, eps) * w.double().abs() + 2 * U * ((yhat2 * w.double()).abs() + b.double().abs())
    bound2 = bound2 + NI.ulp16(ref2.abs() + bound2) / 2
    out = sentinel_out_f16(ILL_ROWS, D, D)
    ops.layernorm_split(hi[:ILL_ROWS], lo[:ILL_ROWS], out, dev(w), dev(b), eps, ILL_ROWS, D)
    torch.cuda.synchronize()
    check_sentinel(out, ILL_ROWS, D, "layernorm_split")
    err2 = (out[:ILL_ROWS].cpu().double() - ref2).abs()
    assert bool((err2 <= bound2).all()), f"layernorm_split: worst {float((err2 / bound2).max()):.3g} of the bound"


@pytest.mark.parametrize("D", NI.LN_RUNG_D + NI.LN_RUNG_D_RAGGED)
def test_a_constant_row_gives_b_exactly(ops, D):
    """Every element c = 3.25: c * D is exact in fp32 (asserted), so the row sum is c * D in any order, the correctly rounded division
    gives the mean c, every centred value is 0 and the variance 0: the output is b bit for bit (fp16(b) from layernorm_split), and
    rstd is within 2 ulp of 1 / sqrt(eps) (rsqrtf's ulp; 0 + eps is exact)."""
    c, rows, eps = NI.ILL_CONSTANT, 5, 1e-6
    assert float(torch.tensor(c, dtype=F32) * D) == c * D and (c * D) % 0.25 == 0 and c * D < 2 ** 22, "c * D (and every partial sum k * c) is exact"
    x = NI.ill_rows("constant", rows, D, 0)
    w, b = NI.real_affine(D, D)
    assert torch.equal(ln_out(ops, dev(x), dev(w), dev(b), rows, D, F32, eps), b.expand(rows, D))
    hi, lo, stat, out = sentinel_out_f16(rows, D, D), sentinel_out_f16(rows, D, D), sentinel_out(rows, 2, 2), sentinel_out_f16(rows, D, D)
    ops.split_stats(dev(x), hi, lo, stat, eps, rows, D)
    ops.layernorm_split(hi[:rows], lo[:rows], out, dev(w), dev(b), eps, rows, D)
    torch.cuda.synchronize()
    check_sentinel(stat, rows, 2, "stat"), check_sentinel(out, rows, D, "out")
    st = stat[:rows].cpu().double()
    ref = torch.tensor(1.0 / NI.f32(eps) ** 0.5, dtype=F64)
    assert bool((st[:, 0] == c).all()) and bool(((st[:, 1] - ref).abs() <= 2 * NI.ulp32(ref)).all())
    assert torch.equal(out[:rows].cpu(), b.to(F16).expand(rows, D))


# ---------------------------------------------------------------- 4. vda_ln_stats_finalize
def run_finalize(ops, partial, eps, overflow=None):
    np_, rows, _ = partial.shape
    stat = sentinel_out(rows, 2, 2)
    ops.ln_stats_finalize(dev(partial), stat, eps, rows, np_, overflow)
    torch.cuda.synchronize()
    check_sentinel(stat, rows, 2, f"ln_stats_finalize rows={rows} np={np_}")
    return stat[:rows].cpu()


@pytest.mark.parametrize("np_", NI.FIN_NP)
def test_finalize_exact_partials(ops, np_):
    """Every block of a row has the same dyadic mean and an integer m2: after the first block delta is 0, so the combined mean is exact and
    m2 the integer total; rstd = rsqrtf(m2 / n + eps) is within 2 ulp of fp64 (the division and the add round once each, half an ulp
    each after the root; rsqrtf one). np around the batch of 8 loads, rows around the 64-row workgroup."""
    for rows in NI.FIN_ROWS:
        partial, mean, m2 = NI.finalize_exact_inputs(rows, np_)
        st = run_finalize(ops, partial, 1e-6).double()
        assert torch.equal(st[:, 0], mean), f"rows={rows}: the combined mean is not exact"
        ref = 1.0 / torch.sqrt(m2 / (64 * np_) + NI.f32(1e-6))
        assert bool(((st[:, 1] - ref).abs() <= 2 * NI.ulp32(ref)).all()), f"rows={rows}: rstd"


@pytest.mark.parametrize("np_", NI.FIN_NP)
def test_finalize_real_partials_within_the_chan_bound(ops, np_):
    """Block means anywhere in +-30 with sigma ~ 1 inside a block, against the pooled fp64 statistics of the same partials; the bound of
    np sequential Chan updates is derived in NI.finalize_pooled."""
    partial = NI.finalize_real_inputs(65, np_)
    mean, rstd, mean_tol, rstd_tol = NI.finalize_pooled(partial, 1e-6)
    st = run_finalize(ops, partial, 1e-6).double()
    assert bool(((st[:, 0] - mean).abs() <= mean_tol).all()), f"mean: worst {float(((st[:, 0] - mean).abs() / mean_tol).max()):.3g} of the bound"
    assert bool(((st[:, 1] - rstd).abs() <= rstd_tol).all()), f"rstd: worst {float(((st[:, 1] - rstd).abs() / rstd_tol).max()):.3g} of the bound"


def test_finalize_overflow_flag(ops):
    """Finite partials leave the flag as it was (0 and 7: the kernel never clears it); +inf, -inf or NaN in the sum or the m2 slot of one
    partial raises it to 1 and changes no other row's statistics; overflow = None is accepted."""
    rows, np_ = 130, 9
    partial = NI.finalize_real_inputs(rows, np_)
    clean = run_finalize(ops, partial, 1e-6)
    for held in (0, 7):
        flag = torch.tensor([-77, held, -77], dtype=torch.int32, device="cuda")
        assert same_bits(run_finalize(ops, partial, 1e-6, flag[1:2]), clean)
        assert flag.tolist() == [-77, held, -77]
    for block, row in NI.finalize_overflow_places(rows, np_):
        for slot in (0, 1):
            for value in NI.FIN_BAD:
                p = partial.clone()
                p[block, row, slot] = value
                flag = torch.tensor([-77, 0, -77], dtype=torch.int32, device="cuda")
                st = run_finalize(ops, p, 1e-6, flag[1:2])
                assert flag.tolist() == [-77, 1, -77], f"{value} at block {block}, row {row}, slot {slot}: flag {flag.tolist()}"
                others = torch.arange(rows) != row
                assert same_bits(st[others], clean[others]), "another row's statistics changed"
                assert same_bits(run_finalize(ops, p, 1e-6, None)[others], clean[others])


# ---------------------------------------------------------------- 5. GroupNorm
def run_groupnorm(ops, x, w, b, eps, groups, chunks, what):
    frames, hw, C = x.shape
    out = out_buffer(frames * hw, C, x.dtype)
    partial = sentinel_out(frames * chunks * groups, 2, 2)            # sized exactly, 8 guard rows behind
    ops.groupnorm(x, out, w, b, eps, frames, hw, C, groups, partial, chunks)
    torch.cuda.synchronize()
    check_sentinel(out, frames * hw, C, f"{what} out")
    check_sentinel(partial, frames * chunks * groups, 2, f"{what} partial")
    return out[:frames * hw].cpu().view(frames, hw, C), partial[:frames * chunks * groups].cpu().view(frames, chunks, groups, 2)


@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
@pytest.mark.parametrize("C,groups", NI.GN_GEOM)
def test_groupnorm_exact_inputs_over_chunks_and_geometry(ops, C, groups, dtype):
    """hw around the apply kernel's 32 rows per block, 1 and 3 frames, chunks in {1, 2, one with empty trailing chunks, hw} (and hw = 10,
    chunks = 7). The one-pass sums are integers below 2**24: every partial is the exact (sum x, sum x**2) of its rows - zeros for an
    empty chunk -, the output has identical bits for every `chunks`, the fp16 output is the integer n, and the fp32 output is within
    3 * 2**-24 * (|w| + |b|) of ((x - mean) * rstd) * w + b in fp64: rstd is the fp64 value rounded once (U), x - mean = +-a and its
    product with rstd are exact, the multiply by w and the add of b round once each (NI.gn_f32_ref_and_bound)."""
    for frames, hw in [(f, hw) for hw in NI.GN_HW for f in NI.GN_FRAMES] + [(1, 10)]:
        d = NI.gn_exact_inputs(frames, hw, C, groups)               # (asserts the preconditions)
        x, w, b = dev(d["x"], dtype), dev(d["w"]), dev(d["b"])
        first = None
        for chunks in NI.gn_chunks(hw) + ([7] if hw == 10 else []):
            what = f"groupnorm C={C} groups={groups} frames={frames} hw={hw} chunks={chunks}"
            y, partial = run_groupnorm(ops, x, w, b, 1e-6, groups, chunks, what)
            rpc = -(-hw // chunks)
            xg = d["x"].view(frames, hw, groups, C // groups)
            want = torch.stack([torch.stack([xg[:, k * rpc:(k + 1) * rpc].sum((1, 3)), (xg[:, k * rpc:(k + 1) * rpc] ** 2).sum((1, 3))], -1) for k in range(chunks)], 1)
            assert torch.equal(partial.double(), want), f"{what}: the partial sums are not the exact integers"
            if dtype == F16:
                assert torch.equal(y.double(), d["n"]), f"{what}: the fp16 output is not the integer result"
            else:
                ref, bound = NI.gn_f32_ref_and_bound(d, 1e-6)
                assert bool(((y.double() - ref).abs() <= bound).all()), f"{what}: beyond 3 * 2**-24 * (|w| + |b|)"
            first = y if first is None else first
            assert same_bits(first, y), f"{what}: the output depends on chunks"


GN_REAL_L = {(C, g, hw, chunks): NI.gn_chain(hw, C, g, chunks) for C, g in NI.GN_GEOM for hw in (33, 65) for chunks in (1, 8, hw)}


@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
@pytest.mark.parametrize("C,groups", NI.GN_GEOM)
def test_groupnorm_one_pass_statistics_at_a_mean_of_30_sigma(ops, C, groups, dtype):
    """Groups whose mean is 30 sigma, and a constant frame (variance clamped at 0), against fp64 F.group_norm of the operand the kernel
    reads. The bound (NI.gn_real_ref_and_bound) comes from the one-pass formula: the relative error of the variance is at most
    (1 + mean**2 / var) * L * 2**-23 with L = rows per thread + rows per pass + channels per group, the longest fp32 addition chain:
        (C, groups)   rows per pass   L at hw = 33: chunks 1 / 8 / 33     L at hw = 65: chunks 1 / 8 / 65
        (64, 32)      32              36 / 35 / 35                        37 / 35 / 35
        (128, 64)     16              21 / 19 / 19                        23 / 19 / 19
        (192, 32)     10              20 / 17 / 17                        23 / 17 / 17
        (1024, 32)    2               51 / 37 / 35                        67 / 39 / 35
        (8, 4)        256             259 / 259 / 259                     259 / 259 / 259
        (72, 1)       28              102 / 101 / 101                     103 / 101 / 101
    (asserted below against NI.gn_chain). The constant frame's output must be b within the same bound, which there is the mean's
    error (L + 1) U |c| times 1 / sqrt(eps) times |w|, plus the affine's roundings."""
    table = {(64, 32): (36, 35, 35, 37, 35, 35), (128, 64): (21, 19, 19, 23, 19, 19), (192, 32): (20, 17, 17, 23, 17, 17),
             (1024, 32): (51, 37, 35, 67, 39, 35), (8, 4): (259,) * 6, (72, 1): (102, 101, 101, 103, 101, 101)}
    assert tuple(GN_REAL_L[(C, groups, hw, ch)] for hw in (33, 65) for ch in (1, 8, hw)) == table[(C, groups)]
    for hw in (33, 65):
        x, w, b = NI.gn_real_inputs(2, hw, C, groups, dtype)
        for chunks in (1, 8, hw):
            ref, bound, L = NI.gn_real_ref_and_bound(x, w, b, 1e-6, groups, chunks)
            assert L == GN_REAL_L[(C, groups, hw, chunks)]
            what = f"groupnorm C={C} groups={groups} hw={hw} chunks={chunks} L={L}"
            y, _ = run_groupnorm(ops, dev(x, dtype), dev(w), dev(b), 1e-6, groups, chunks, what)
            err = (y.double() - ref).abs()
            print(f"{what}: worst {float((err[1] / bound[1]).max()):.3g} of the bound at 30 sigma, {float((err[0] / bound[0]).max()):.3g} on the constant frame")
            assert bool((err <= bound).all()), f"{what}: worst {float((err / bound).max()):.3g} of the bound"
            assert float((ref[0] - b.double()).abs().max()) < 1e-9, "the constant frame's reference is b"


# ---------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_output_untouched(ops):
    """ln_check, the pe check, groupnorm_launch and vda_ln_stats_finalize refuse bad geometry with VdaError; nothing is launched."""
    from video_depth_anything_amd._lib import VdaError
    z32 = lambda *s: torch.zeros(*s, dtype=F32, device="cuda")      # noqa: E731
    z16 = lambda *s: torch.zeros(*s, dtype=F16, device="cuda")      # noqa: E731
    rows = 12

    def ln_entries(D, group=0, skip=0, n=rows):
        """Every LayerNorm-family entry at this geometry, each with its own sentinel outputs."""
        w, b = z32(D), z32(D)
        o16, o32 = sentinel_out_f16(n, D, D), sentinel_out(n, D, D)
        yield "layernorm_f16", [o16], lambda: ops.layernorm(z32(n, D), o16, w, b, 1e-6, n, D, group=group, skip=skip)
        yield "layernorm_f32", [o32], lambda: ops.layernorm(z32(n, D), o32, w, b, 1e-6, n, D, group=group, skip=skip)
        o, s = sentinel_out_f16(n, D, D), sentinel_out(n, D, D)
        yield "layernorm_residual", [o, s], lambda: ops.layernorm_residual(s, z16(n, D), None, o, w, b, 1e-6, n, D, group=group, skip=skip)
        o2 = sentinel_out_f16(n, D, D)
        yield "layernorm_split", [o2], lambda: ops.layernorm_split(z16(n, D), z16(n, D), o2, w, b, 1e-6, n, D, group=group, skip=skip)
        if group == 0:
            for center in (False, True):
                hi, lo, st = sentinel_out_f16(n, D, D), sentinel_out_f16(n, D, D), sentinel_out(n, 2, 2)
                yield f"split_stats center={center}", [hi, lo, st], lambda hi=hi, lo=lo, st=st, center=center: ops.split_stats(z32(n, D), hi, lo, st, 1e-6, n, D, center=center)

    for why, kw in (("D = 12", dict(D=12)), ("D = 2056", dict(D=2056)), ("rows % group != 0", dict(D=64, group=5)), ("skip = group", dict(D=64, group=4, skip=4)),
                    ("skip < 0", dict(D=64, group=4, skip=-1))):
        for name, outs, call in ln_entries(**kw):
            with pytest.raises(VdaError):
                call()
            assert all(untouched(o) for o in outs), f"{name}, {why}: the refused call wrote"

    D = 64
    w, b = z32(D), z32(D)
    out = sentinel_out_f16(rows, D, D)
    off = lambda: z16(rows * D + 4)[4:]                               # noqa: E731  an fp16 view 8 bytes into its allocation
    assert off().data_ptr() % 16 == 8 and off().is_contiguous()
    for name, call in (("layernorm_split hi", lambda: ops.layernorm_split(off(), z16(rows, D), out, w, b, 1e-6, rows, D)),
                       ("layernorm_split lo", lambda: ops.layernorm_split(z16(rows, D), off(), out, w, b, 1e-6, rows, D)),
                       ("layernorm_residual y", lambda: ops.layernorm_residual(z32(rows, D), off(), None, out, w, b, 1e-6, rows, D))):
        with pytest.raises(VdaError):
            call()
        assert untouched(out), f"{name} offset by 8 bytes: the refused call wrote"
    flat = sentinel_out_f16(rows + 1, D, D, extra_rows=0).view(-1)
    with pytest.raises(VdaError):
        ops.layernorm(z32(rows, D), flat[4:4 + rows * D], w, b, 1e-6, rows, D)
    assert untouched(flat), "layernorm out offset by 8 bytes: the refused call wrote"
    with pytest.raises(VdaError):
        ops.layernorm(z32(rows, D), out, w, b, 1e-6, rows, D, pe=z32(4, D), pe_rows_per_step=3, pe_steps=0)
    assert untouched(out), "pe with pe_steps = 0: the refused call wrote"

    hw = 16
    for why, C, groups, chunks in (("groups = 128", 1024, 128, 4), ("C % groups != 0", 72, 32, 4), ("C = 1032", 1032, 8, 4), ("chunks = 0", 64, 32, 0),
                                  ("chunks = hw + 1", 64, 32, hw + 1)):
        for dtype in (F16, F32):
            o, partial = out_buffer(hw, C, dtype), sentinel_out(2 * (hw + 1) * 128, 2, 2)
            with pytest.raises(VdaError):
                ops.groupnorm(torch.zeros(1, hw, C, dtype=dtype, device="cuda"), o, z32(C), z32(C), 1e-6, 1, hw, C, groups, partial, chunks)
            assert untouched(o) and untouched(partial), f"groupnorm {why}: the refused call wrote"

    stat = sentinel_out(rows, 2, 2)
    with pytest.raises(VdaError):
        ops.ln_stats_finalize(z32(1, rows, 2), stat, 1e-6, rows, 0)
    assert untouched(stat), "ln_stats_finalize np = 0: the refused call wrote"
