"""Inputs, case lists and preconditions for the row-normalisation kernels (csrc/norm.hip), shared by tests/test_norm_inputs.py (CPU:
the inputs meet their preconditions and the equalities can fail) and tests/test_norm_edges_gpu.py (GPU: the kernels meet them).

LayerNorm family - rows whose statistics are exact in fp32 under ANY summation order:

    x[r, j] = m_r + a_r * s[r, j]     s = +-1 with exactly D / 2 of each sign, m_r an integer, a_r a power of two

Every partial sum is an integer below 2**24, so the mean is m_r, every centred value +-a_r and the variance a_r**2, bit for bit. With
integer w (nonzero), b and pe (multiples of 8) the result is n = s * w + b (+ pe), a nonzero integer below 2048, and the fp32 value
the kernel holds before it stores lies within about 4e-5 of n (rstd = 1 / sqrt(a**2 + eps), not 1 / a): far inside half an fp16 ulp
(>= 4.9e-4 at |n| >= 1), so the fp16 output IS n. ln_model is a plain restatement of the operation in fp32 on the CPU - the row as
LPR lanes x NCH chunks of 8, as the kernels hold it - with the single mistakes of LN_MUTATIONS built in; ln_mismatch is the assertion
both test files apply (to the model's output there, to the kernel's here).

vda_ln_stats_finalize - partials whose Chan combination is exact (every 64-column block of a row has the same dyadic mean, integer
centred squares), and real-valued ones with their pooled fp64 statistics and the bound of np sequential updates.

GroupNorm - the same +-1 construction per (frame, group): the one-pass sums (sum x, sum x**2) are integers below 2**24, so the result
does not depend on `chunks` and equals the integer n.

The sentinel helpers come from tests/_exact.py."""
import collections
import math

import torch

from _exact import EXACT_LIMIT, FP16_EXACT_LIMIT

F16, F32, F64 = torch.float16, torch.float32, torch.float64
U = 2.0 ** -24                          # unit roundoff of fp32: one rounding is a relative error of at most U
EPS_LIST = (1e-6, 1e-5)                 # the model's two LayerNorm epsilons (encoder, motion modules)


def f32(v):
    """A Python float rounded to fp32 (eps as the kernels receive it)."""
    return float(torch.tensor(v, dtype=F32))


def ulp32(t):
    """Spacing of fp32 at |t| (fp64 in, fp64 out): 2**(floor(log2 |t|) - 23), the smallest normal's for 0."""
    t = t.double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(t)) - 23)


def ulp16(t):
    t = t.double().abs().clamp_min(2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(t)) - 10)


def step_ulps(t, k):
    """Positive fp32 values moved by k ulps."""
    assert t.dtype == F32 and bool((t > 0).all())
    return (t.view(torch.int32) + k).view(F32)


# ------------------------------------------------------------------------------------------------ the ladder
LN_D = [8, 64, 72, 128, 136, 256, 264, 512, 520, 1024, 1032, 2048]       # both sides of every rung of ln_ladder
LN_RUNG_D = [64, 128, 256, 512, 1024, 2048]                             # one D per rung
LN_RUNG_D_RAGGED = [72, 136, 264, 520, 1032, 1544]                      # one per rung, the row not a whole number of lane groups (D = 72 is on the second)


def ln_rung(D):
    """(LPR lanes per row, NCH chunks per lane, R rows per workgroup) of ln_ladder for a row of D elements."""
    assert D > 0 and D % 8 == 0 and D <= 2048
    nchunk = D // 8
    for top, lpr, nch in ((8, 8, 1), (16, 16, 1), (32, 32, 1), (64, 64, 1), (128, 64, 2), (256, 64, 4)):
        if nchunk <= top:
            return lpr, nch, 4 * (64 // lpr)
    raise AssertionError


def ln_rows(D):
    """1, one below, exactly, one above a workgroup, two workgroups and a ragged tail."""
    R = ln_rung(D)[2]
    return [r for r in (1, R - 1, R, R + 1, 2 * R + 3) if r > 0]


def ln_chain(D):
    """The longest chain of fp32 additions a row sum goes through: 3 inside a chunk (pairwise over 8), one per chunk of a lane, log2
    LPR across the lanes."""
    lpr, nch, _ = ln_rung(D)
    return 3 + nch + int(math.log2(lpr))


# ------------------------------------------------------------------------------------------------ exact rows
LN_MAX_ROWS = 80                    # every case takes the first `rows` of the same 80 seeded rows of its D
LnCase = collections.namedtuple("LnCase", "entry D rows group skip prs steps eps")
LN_ENTRIES = ["layernorm_f16", "layernorm_f32", "split", "residual_gamma", "residual", "stats", "center_stats"]
LN_COMPACTING = ["layernorm_f16", "layernorm_f32", "split", "residual_gamma", "residual"]
LN_GROUP_SHAPES = [(512, 15), (64, 70)]     # one lane group per row / 8 rows per wave; rows a multiple of 5, more than one workgroup at D = 64
LN_PE = [(1, 1), (1, 4), (6, 1), (6, 4)]    # (pe_rows_per_step, pe_steps)


def ln_group_skip(rows):
    return [(1, 0), (5, 1), (5, 2), (5, 4), (rows, 1)]


def ln_case_id(c):
    s = f"{c.entry}-D{c.D}-r{c.rows}"
    if c.group:
        s += f"-g{c.group}s{c.skip}"
    if c.steps:
        s += f"-pe{c.prs}x{c.steps}"
    return s


def ln_shape_cases(entry):
    """Every (D, rows) of the ladder for one entry; eps alternates between the model's two."""
    return [LnCase(entry, D, rows, 0, 0, 0, 0, EPS_LIST[i % 2]) for i, D in enumerate(LN_D) for rows in ln_rows(D)]


def ln_group_cases(entry):
    return [LnCase(entry, D, rows, g, s, 0, 0, 1e-6) for D, rows in LN_GROUP_SHAPES for g, s in ln_group_skip(rows)]


def ln_pe_cases(entry):
    out = [LnCase(entry, D, rows, 0, 0, prs, steps, 1e-5) for D, rows in LN_GROUP_SHAPES for prs, steps in LN_PE]
    return out + [LnCase(entry, D, rows, 5, 1, 6, 4, 1e-5) for D, rows in LN_GROUP_SHAPES]      # the step index comes from the INPUT row


def ln_cases():
    out = []
    for e in LN_ENTRIES:
        out += ln_shape_cases(e)
    for e in LN_COMPACTING:
        out += ln_group_cases(e)
    for e in ("layernorm_f16", "layernorm_f32"):
        out += ln_pe_cases(e)
    return out


def balanced_signs(n_sets, n, g):
    """[n_sets, n] of +-1 with exactly n / 2 of each sign per set."""
    assert n % 2 == 0, f"{n} elements cannot hold as many +1 as -1"
    rank = torch.rand(n_sets, n, generator=g, dtype=F64).argsort(1).argsort(1)
    return torch.where(rank < n // 2, 1.0, -1.0).to(F64)


def nonzero_ints(shape, lo, hi, g):
    """Integers of magnitude lo..hi, either sign (fp64)."""
    mag = torch.randint(lo, hi + 1, tuple(shape), generator=g)
    sign = torch.randint(0, 2, tuple(shape), generator=g) * 2 - 1
    return (mag * sign).to(F64)


def ln_rows_data(D):
    """The 80 seeded rows of one D and the operand forms of every entry (fp64 integers; cast where they are used)."""
    g = torch.Generator().manual_seed(7100 + D)
    N = LN_MAX_ROWS
    d = dict(D=D)
    d["s"] = balanced_signs(N, D, g)
    d["m"] = nonzero_ints((N, 1), 64, 512, g)                  # |m| >= 64 > a: a row never looks centred, a wrong divisor never goes unseen
    d["a"] = torch.exp2(torch.randint(0, 6, (N, 1), generator=g).to(F64))
    d["x"] = d["m"] + d["a"] * d["s"]
    d["w"] = nonzero_ints((D,), 1, 7, g)
    d["b"] = torch.randint(-4, 5, (D,), generator=g).to(F64) * 8
    d["pe"] = torch.randint(-8, 9, (4, D), generator=g).to(F64) * 8
    d["t"] = torch.randint(-2, 3, (N, D), generator=g).to(F64)              # split: hi = x - t, lo = t
    d["y"] = torch.randint(-3, 4, (N, D), generator=g).to(F64)              # residual: x0 = x - gamma * y
    d["gamma"] = nonzero_ints((D,), 1, 2, g)
    return d


_rows_cache = {}


def ln_inputs(case):
    """The operands of one case (fp64 holding exactly representable values) and what it must produce."""
    if case.D not in _rows_cache:
        _rows_cache[case.D] = ln_rows_data(case.D)
        assert_ln_rows(_rows_cache[case.D])
    d = _rows_cache[case.D]
    r = case.rows
    inp = {k: (v[:r] if k in ("s", "m", "a", "x", "t", "y") else v) for k, v in d.items()}
    inp["pe"] = d["pe"][:case.steps] if case.steps else None
    if case.entry == "residual":
        inp["gamma"] = None
    g = inp["gamma"] if inp["gamma"] is not None else torch.ones(case.D, dtype=F64)
    inp["x0"] = inp["x"] - g * inp["y"]
    inp["hi"], inp["lo"] = inp["x"] - inp["t"], inp["t"]
    assert float(inp["hi"].abs().max()) <= FP16_EXACT_LIMIT and float(inp["x0"].abs().max()) < EXACT_LIMIT
    n = inp["s"] * inp["w"] + inp["b"]
    if case.steps:
        step = (torch.arange(r) // case.prs) % case.steps
        n = n + inp["pe"][step]
    keep = [row for row in range(r) if ln_out_row(row, case.group, case.skip) >= 0]
    assert [ln_out_row(row, case.group, case.skip) for row in keep] == list(range(len(keep))), "compaction is dense and keeps the order"
    inp["rows_out"] = len(keep)
    inp["n"] = n[keep]
    assert bool((inp["n"] != 0).all()) and float(inp["n"].abs().max()) < FP16_EXACT_LIMIT
    return inp


def ln_out_row(row, group, skip):
    """include/vda.h: row r with r % group < skip is dropped, the rest compacted."""
    if group <= 0:
        return row
    g, i = divmod(row, group)
    return -1 if i < skip else g * (group - skip) + i - skip


def assert_ln_rows(d):
    """The preconditions of the exact rows, asserted (not assumed): balanced signs, integers, every partial sum of x, of the centred
    squares and of |x| in any order below 2**24, n a nonzero integer below 2048."""
    D = d["D"]
    s, m, a, x, w, b = d["s"], d["m"], d["a"], d["x"], d["w"], d["b"]
    assert bool((s.abs() == 1).all()) and bool((s.sum(1) == 0).all()), "signs are not balanced: the row mean would not be m"
    assert bool((m == m.round()).all()) and float(m.abs().max()) <= 512
    assert bool((torch.log2(a) == torch.log2(a).round()).all()) and float(a.min()) >= 1 and float(a.max()) <= 32
    assert bool((x == x.round()).all())
    assert float(x.abs().sum(1).max()) < EXACT_LIMIT, "partial sums of x may reach 2**24: the mean is not exact"
    assert float((a * a * D).max()) < EXACT_LIMIT, "the centred squares may reach 2**24"
    assert bool((s * w + b != 0).all()), "n = 0: an fp16 output could not tell a small error from none"
    assert bool((w != 0).all()) and float(w.abs().max()) <= 7 and bool((w == w.round()).all())
    assert bool((b % 8 == 0).all()) and float(b.abs().max()) <= 32
    if "pe" in d and d["pe"] is not None:
        assert bool((d["pe"] % 8 == 0).all())
        n_top = 7 + 32 + float(d["pe"].abs().max())
    else:
        n_top = 7 + 32
    assert n_top < FP16_EXACT_LIMIT


# ------------------------------------------------------------------------------------------------ the operation, restated
LN_MUTATIONS = ["divisor", "absent_chunks", "neighbour_chunk", "pe_step", "compaction", "lo_ignored"]


def ln_mutation_applies(mutation, case):
    lpr, nch, _ = ln_rung(case.D)
    ragged = case.D // 8 < lpr * nch
    return {"divisor": ragged, "absent_chunks": ragged, "neighbour_chunk": case.D > 8 and case.entry in LN_COMPACTING,
            "pe_step": case.steps > 1 and case.skip > 0, "compaction": case.skip > 0 and case.entry in LN_COMPACTING,
            "lo_ignored": case.entry == "split"}[mutation]


def _lane_sum(v, lpr, nch):
    """fp32 [rows, nch * lpr * 8] in the kernels' order: pairwise inside a chunk, a lane's chunks in turn, a halving tree across lanes."""
    c = v.view(v.shape[0], nch, lpr, 8)
    c = c[..., 0::2] + c[..., 1::2]
    c = c[..., 0::2] + c[..., 1::2]
    c = (c[..., 0] + c[..., 1])
    acc = torch.zeros_like(c[:, 0])
    for k in range(nch):
        acc = acc + c[:, k]
    while acc.shape[1] > 1:
        h = acc.shape[1] // 2
        acc = acc[:, :h] + acc[:, h:]
    return acc[:, 0]


def _seq_sum(v):
    """Left to right, one element at a time."""
    acc = torch.zeros(v.shape[0], dtype=F32)
    for j in range(v.shape[1]):
        acc = acc + v[:, j]
    return acc


def ln_model(case, inp, mutation=None, order="lanes", rstd_ulps=0, fma=False):
    """What the entry of `case` leaves behind, every step in fp32 on the CPU: dict(out=, stream=, stat=, hi=, lo=) with the keys that
    entry has. `out` is [rows_out, D] in the entry's output type, NaN where nothing was stored. mutation: one of LN_MUTATIONS.
    order: "lanes" (the kernels') or "seq"; rstd_ulps moves rstd; fma contracts the affine's multiply-add."""
    assert mutation is None or mutation in LN_MUTATIONS
    D, rows, eps = case.D, case.rows, f32(case.eps)
    lpr, nch, _ = ln_rung(D)
    slots = lpr * nch * 8
    res = {}
    if case.entry == "split":
        img = inp["hi"].to(F16).float()
        if mutation != "lo_ignored":
            img = img + inp["lo"].to(F16).float()
    elif case.entry in ("residual", "residual_gamma"):
        g = inp["gamma"].float() if inp["gamma"] is not None else torch.ones(D)
        img = (g.double() * inp["y"].to(F16).double() + inp["x0"].float().double()).float()          # fmaf: one rounding
        res["stream"] = img.clone()
    else:
        img = inp["x"].float()
    pad = torch.zeros(rows, slots, dtype=F32)
    pad[:, :D] = img
    fsum = (lambda v: _lane_sum(v, lpr, nch)) if order == "lanes" else _seq_sum
    div = float(slots) if mutation == "divisor" else float(D)
    mean = fsum(pad) / div
    present = (torch.arange(slots) < D) | (mutation == "absent_chunks")
    dlt = torch.where(present, pad - mean[:, None], torch.zeros(()))
    rstd = torch.rsqrt(fsum(dlt * dlt) / div + eps)
    if rstd_ulps:
        rstd = step_ulps(rstd, rstd_ulps)
    if case.entry in ("stats", "center_stats"):
        ctr = mean if case.entry == "center_stats" else torch.zeros(rows)
        dd = img - ctr[:, None]
        res["hi"] = dd.to(F16)
        res["lo"] = (dd - res["hi"].float()).to(F16)
        res["stat"] = torch.stack([mean - ctr, rstd], 1)
        return res
    w, b = inp["w"].float(), inp["b"].float()
    if mutation == "neighbour_chunk":
        w, b = torch.roll(w, -8), torch.roll(b, -8)
    t = (img - mean[:, None]) * rstd[:, None]
    v = (t.double() * w.double() + b.double()).float() if fma else t * w + b
    odt = F32 if case.entry == "layernorm_f32" else F16
    out = torch.full((inp["rows_out"] + rows + 1, D), float("nan"), dtype=F32)
    for r in range(rows):
        o = ln_out_row(r, case.group, case.skip)
        if o < 0:
            continue
        if mutation == "compaction":
            o += case.skip
        vr = v[r]
        if case.steps:
            vr = vr + inp["pe"][((o if mutation == "pe_step" else r) // case.prs) % case.steps].float()
        out[o] = vr
    res["out"] = out[:inp["rows_out"]].to(odt)
    return res


def ln_f32_ref_and_bound(case, inp):
    """The fp32-out entry against the formula in fp64, ((x - mean) * rstd) * w + b (+ pe) with rstd = 1 / sqrt(a**2 + eps): the bound
    counts the roundings. x - mean = +-a is exact. rstd: var + eps rounds once (U, halved by the square root) and rsqrtf is within one
    ulp (at most 2 U relative): 2.5 U. Two multiplies, U each - 4.5 U on a term of magnitude at most |w|. The add of b: U of at most
    |w| + |b|. The add of pe: U of at most |w| + |b| + |pe|. In all at most 6.5 U (|w| + |b| + |pe|), and U z < ulp(z): the bound is
    7 * 2**-24 * (|w| + |b| + |pe|), fewer than 7 ulps of |w| + |b| + |pe|. (An fma in place of the last multiply and add only drops a rounding.)"""
    keep = [r for r in range(case.rows) if ln_out_row(r, case.group, case.skip) >= 0]
    rstd = 1.0 / torch.sqrt(inp["a"] * inp["a"] + f32(case.eps))
    ref = (inp["s"] * inp["a"] * rstd) * inp["w"] + inp["b"]
    mag = (inp["w"].abs() + inp["b"].abs()).expand_as(ref).clone()
    if case.steps:
        pe = inp["pe"][(torch.arange(case.rows) // case.prs) % case.steps]
        ref, mag = ref + pe, mag + pe.abs()
    return ref[keep], 7 * U * mag[keep]


def ln_mismatch(case, inp, got):
    """The assertion of the exact-statistics tests: None, or what is wrong with `got` (the dict ln_model returns, or the same from the
    device)."""
    r, D = case.rows, case.D
    if "stream" in got:
        if not torch.equal(got["stream"].double(), inp["x"]):
            bad = (got["stream"].double() != inp["x"]).any(1).nonzero().flatten().tolist()
            return f"the stream differs from x0 + gamma * y in rows {bad[:8]}"
    if case.entry in ("stats", "center_stats"):
        centred = case.entry == "center_stats"
        want0 = torch.zeros(r, dtype=F64) if centred else inp["m"][:, 0]
        if not torch.equal(got["stat"][:, 0].double(), want0):
            return f"stat[:, 0] is not exactly {'0' if centred else 'm'}: max diff {float((got['stat'][:, 0].double() - want0).abs().max()):.3g}"
        ref = 1.0 / torch.sqrt(inp["a"][:, 0] ** 2 + f32(case.eps))
        err = (got["stat"][:, 1].double() - ref).abs() / ulp32(ref)
        if not bool((err <= 2).all()):            # var + eps: half an ulp after the root; rsqrtf: one ulp
            return f"rstd is {float(err.max()):.2f} ulp from 1 / sqrt(a**2 + eps)"
        want_hi = inp["a"] * inp["s"] if centred else inp["x"]
        if not torch.equal(got["hi"].double(), want_hi):
            return "the hi plane is not " + ("+-a" if centred else "fp16(x)")
        if not torch.equal(got["lo"].double(), torch.zeros(r, D, dtype=F64)):
            return "the lo plane is not 0"
        return None
    out = got["out"]
    if tuple(out.shape) != (inp["rows_out"], D):
        return f"out has shape {tuple(out.shape)}"
    if case.entry == "layernorm_f32":
        ref, bound = ln_f32_ref_and_bound(case, inp)
        err = (out.double() - ref).abs()
        if not bool((err <= bound).all()):        # (NaN fails)
            return f"fp32 out: {int((~(err <= bound)).sum())} elements beyond 7 * 2**-24 * (|w| + |b| + |pe|), worst {float(torch.nan_to_num(err / bound, nan=1e30).max()):.3g} of it"
        return None
    if not torch.equal(out.double(), inp["n"]):
        bad = (out.double() != inp["n"]).any(1).nonzero().flatten().tolist()
        return f"fp16 out differs from the integer result in output rows {bad[:8]} ({len(bad)} in all)"
    return None


# ------------------------------------------------------------------------------------------------ real-valued rows
def real_rows(rows, D, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, D, generator=g) * 3 + 0.7).to(F32)


def real_affine(D, seed):
    g = torch.Generator().manual_seed(seed)
    return (1 + 0.5 * torch.randn(D, generator=g)).to(F32), (0.3 * torch.randn(D, generator=g)).to(F32)


def split_planes(x):
    hi = x.to(F16)
    return hi, (x - hi.float()).to(F16)


ILL_REGIMES = ["offset", "channels", "both", "constant", "large"]


def ill_rows(regime, rows, D, seed):
    """Rows in the regimes of tests/_outliers.py (fp32): every element + 40; three channels at 400, -650, 900; both; a constant row;
    |x| ~ 1e4 with sigma ~ 1."""
    from _outliers import OFFSET, OUTLIER_CHANNELS, OUTLIER_VALUES
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, D, generator=g)
    if regime in ("offset", "both"):
        x = x + OFFSET
    if regime in ("channels", "both"):
        for c, v in zip(OUTLIER_CHANNELS, OUTLIER_VALUES):
            x[:, c % D] += v
    if regime == "constant":
        x = torch.full((rows, D), ILL_CONSTANT)
    if regime == "large":
        x = x + 1e4
    return x.to(F32)


ILL_CONSTANT = 3.25         # c * k is exact in fp32 for every k <= 2048 (13 / 4 times an integer below 2**11): the mean is c, every centred value 0


def ln_forward_bound(x64, yhat, D, eps):
    """The two-pass algorithm's forward bound on the normalised value yhat = (x - mean) * rstd:
    (L + 4) * 2**-24 * (mean|x| * rstd + |yhat|), L = ln_chain(D). The row sum's error is at most L U sum|x|, so the mean's L U mean|x|
    (+ U for the division), which reaches yhat multiplied by rstd; the centred squares carry the same chain (relative (L + 2) U on the
    variance, half of it on rstd), the subtraction, the rsqrtf ulp and the multiply are the |yhat| term."""
    mean = x64.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x64 - mean) ** 2).mean(1, keepdim=True) + f32(eps))
    return (ln_chain(D) + 4) * U * (x64.abs().mean(1, keepdim=True) * rstd + yhat.abs())


# ------------------------------------------------------------------------------------------------ vda_ln_stats_finalize
FIN_NP = [1, 2, 6, 7, 8, 9, 16, 17]        # around the kernel's batch of 8 loads
FIN_ROWS = [1, 63, 64, 65, 130]            # around its 64-row workgroup


def finalize_exact_inputs(rows, np_, seed=0):
    """partial [np, rows, 2]: every block of row r has the mean k_r / 4 (sum = 16 k_r) and an integer centred sum of squares. The Chan
    update then has delta = 0 after the first block: mean = k_r / 4 and m2 = the integer total, exactly."""
    g = torch.Generator().manual_seed(8200 + 131 * rows + np_ + seed)
    k = nonzero_ints((rows,), 1, 200, g)
    m2 = torch.randint(1, 4097, (np_, rows), generator=g).to(F64)
    partial = torch.stack([(16 * k).expand(np_, rows), m2], 2)
    assert float(m2.sum(0).max()) < EXACT_LIMIT and float((16 * k).abs().max()) < EXACT_LIMIT
    return partial.to(F32).contiguous(), k / 4, m2.sum(0)


def finalize_model(partial, eps, batch_clamp=True):
    """ln_stats_finalize_kernel in fp32 on the CPU; batch_clamp=False reads a ninth-to-sixteenth slot that is not there as a block of
    zeros (the mistake min(j0 + u, np - 1) and its guard prevent)."""
    np_, rows, _ = partial.shape
    n = torch.zeros(rows)
    mean, m2 = torch.zeros(rows), torch.zeros(rows)
    steps = np_ if batch_clamp else -(-np_ // 8) * 8
    for j in range(steps):
        q = partial[j] if j < np_ else torch.zeros(rows, 2)
        mb = q[:, 0] * (1.0 / 64.0)
        delta = mb - mean
        nn = n + 64.0
        mean = mean + delta * (64.0 / nn)
        m2 = m2 + (q[:, 1] + delta * delta * (n * 64.0 / nn))
        n = nn
    return torch.stack([mean, torch.rsqrt(m2 / n + f32(eps))], 1)


def finalize_real_inputs(rows, np_, seed=0):
    """Block means that differ by many sigma: a block's 64 columns have sigma ~ 1 (m2 ~ 64) and a mean anywhere in +-30."""
    g = torch.Generator().manual_seed(8300 + 131 * rows + np_ + seed)
    mb = (torch.rand(np_, rows, generator=g) * 60 - 30)
    m2 = 64 * (0.5 + torch.rand(np_, rows, generator=g))
    return torch.stack([mb * 64, m2], 2).to(F32).contiguous()


def finalize_pooled(partial, eps):
    """(mean, rstd, mean bound, rstd bound) in fp64 from the same fp32 partials.
    Bound of np sequential Chan updates, A = max |block mean|, R = max - min block mean, per row:
      mean: one step computes delta (U), 64 / nn (U), their product (U) and the add (U) on magnitudes at most 2 A (the 1 / 64 is exact):
            the error grows by at most 7 U A a step (the update itself contracts what it inherits) - E <= 8 np U A.
      m2:   all terms are non-negative, so relative errors carry: delta (U), its square (U more, 2 U from delta), n * 64 / nn (U), the
            product (U), the inner add (U), the running add (U a step): at most (np + 8) U relative; and delta inherits E, which moves
            delta**2 * (<= 64) by at most 64 * 2 R E a step: (np + 8) U + 128 np R E / M2.
      rstd: half the relative error of m2, the division, the add of eps (U each, halved) and the rsqrtf ulp (2 U): + 4 U."""
    p = partial.double()
    np_ = p.shape[0]
    mb = p[..., 0] / 64
    mean = mb.mean(0)
    M2 = p[..., 1].sum(0) + (64 * (mb - mean) ** 2).sum(0)
    rstd = 1.0 / torch.sqrt(M2 / (64 * np_) + f32(eps))
    A = mb.abs().max(0).values
    R = mb.max(0).values - mb.min(0).values
    E = 8 * np_ * U * A
    rel = (np_ + 8) * U + 128 * np_ * R * E / M2
    return mean, rstd, E, rstd * (0.5 * rel + 4 * U)


FIN_BAD = [float("inf"), float("-inf"), float("nan")]


def finalize_overflow_places(rows, np_):
    """(block, row): first block of row 0, last block of the last row, a middle block of a row in the second workgroup."""
    assert rows > 64 and np_ >= 3
    return [(0, 0), (np_ - 1, rows - 1), (np_ // 2, 64 + (rows - 64) // 2)]


# ------------------------------------------------------------------------------------------------ GroupNorm
GN_HW = [1, 31, 32, 33, 65]                 # around the apply kernel's 32 rows per block
GN_FRAMES = [1, 3]
GN_GEOM = [(64, 32), (128, 64), (192, 32), (1024, 32), (8, 4), (72, 1)]     # (C, groups): C / 8 = 24 and 9 do not divide 256; two rows per pass; 64 groups; one group
GN_APPLY_ROWS = 32


def gn_chunks(hw):
    """1, 2, hw and one that leaves trailing chunks empty (ceil(hw / chunks) * (chunks - 1) >= hw), where hw has them."""
    out = [1] + ([2] if hw >= 2 else []) + [hw]
    ragged = [c for c in range(2, hw) if -(-hw // c) * (c - 1) >= hw]
    return sorted(set(out + ragged[:1]))


def gn_has_empty_chunk(hw, chunks):
    return -(-hw // chunks) * (chunks - 1) >= hw


def gn_chain(hw, C, groups, chunks):
    """Longest fp32 addition chain of the partial kernel: rows a thread sums, rows summed across the pass, channels of a group."""
    rows_par = 256 // (C // 8)
    per_thread = -(-(-(-hw // chunks)) // rows_par)
    return per_thread + rows_par + C // groups


def gn_exact_inputs(frames, hw, C, groups, seed=0):
    """x [frames, hw, C] = m[f, g] + a[f, g] * s with the signs balanced over each (frame, group) (fp64 integers), integer w and b."""
    cpg = C // groups
    n = hw * cpg
    g = torch.Generator().manual_seed(9100 + 7 * hw + 1031 * frames + C + groups + seed)
    a = torch.exp2(torch.randint(0, 3, (frames, groups), generator=g).to(F64))
    top = min(40, int(math.isqrt(int(EXACT_LIMIT) // n)) - 5)
    m = nonzero_ints((frames, groups), max(1, top // 2), top, g)
    s = balanced_signs(frames * groups, n, g).view(frames, groups, hw, cpg).permute(0, 2, 1, 3).reshape(frames, hw, C)
    rep = lambda t: t.repeat_interleave(cpg, 1)[:, None, :]      # noqa: E731
    d = dict(s=s, m=m, a=a, x=rep(m) + rep(a) * s, w=nonzero_ints((C,), 1, 7, g), b=torch.randint(-4, 5, (C,), generator=g).to(F64) * 8,
             frames=frames, hw=hw, C=C, groups=groups)
    d["n"] = s * d["w"] + d["b"]
    d["a_full"] = rep(a).expand(frames, hw, C)
    assert_gn_exact(d)
    return d


def assert_gn_exact(d):
    frames, hw, C, groups = d["frames"], d["hw"], d["C"], d["groups"]
    cpg = C // groups
    n = hw * cpg
    assert n % 2 == 0, "hw * C / groups is odd: the signs cannot balance"
    per = d["s"].view(frames, hw, groups, cpg).sum((1, 3))
    assert bool((per == 0).all()), "signs are not balanced over a (frame, group)"
    assert float((n * (d["m"].abs() + d["a"]) ** 2).max()) < EXACT_LIMIT, "the one-pass sums may reach 2**24"
    assert float(d["x"].abs().max()) <= FP16_EXACT_LIMIT and bool((d["x"] == d["x"].round()).all())
    assert bool((d["n"] != 0).all()) and float(d["n"].abs().max()) < FP16_EXACT_LIMIT


def gn_model(d, eps, chunks, dtype=F32, drop_last_chunk=False):
    """The two GroupNorm kernels restated: fp32 one-pass partial sums per chunk (rows in turn, then channels of the group), combined in
    fp64, applied in fp32. drop_last_chunk: the mistake of combining chunks - 1 partials."""
    frames, hw, C, groups = d["frames"], d["hw"], d["C"], d["groups"]
    cpg = C // groups
    x = d["x"].to(dtype).float()
    rpc = -(-hw // chunks)
    a = torch.zeros(frames, groups, dtype=F64)
    q = torch.zeros(frames, groups, dtype=F64)
    for k in range(chunks - (1 if drop_last_chunk else 0)):
        rows = x[:, k * rpc:min(hw, (k + 1) * rpc)]
        sa, sq = torch.zeros(frames, C), torch.zeros(frames, C)
        for r in range(rows.shape[1]):
            sa, sq = sa + rows[:, r], sq + rows[:, r] * rows[:, r]
        ga, gq = torch.zeros(frames, groups), torch.zeros(frames, groups)
        for c in range(cpg):
            ga, gq = ga + sa.view(frames, groups, cpg)[..., c], gq + sq.view(frames, groups, cpg)[..., c]
        a, q = a + ga.double(), q + gq.double()
    n = float(hw * cpg)
    mean = a / n
    var = (q / n - mean * mean).clamp_min(0)
    rstd = (1.0 / torch.sqrt(var + f32(eps))).float()
    rep = lambda t: t.repeat_interleave(cpg, 1)[:, None, :]      # noqa: E731
    return ((x - rep(mean.float())) * rep(rstd) * d["w"].float() + d["b"].float()).to(dtype)


def gn_f32_ref_and_bound(d, eps):
    """fp32 GroupNorm on the exact inputs against ((x - mean) * rstd) * w + b in fp64: the mean m and the variance a**2 come out of
    the fp64 combine exactly, rstd is the fp64 value rounded to fp32 (U), x - mean = +-a and its product with rstd are exact, the
    multiply by w and the add of b round once each: at most U |w| + U |w| + U (|w| + |b|) <= 3 * 2**-24 * (|w| + |b|), fewer than 3
    ulps of |w| + |b|."""
    rstd = 1.0 / torch.sqrt(d["a_full"] ** 2 + f32(eps))
    ref = (d["s"] * d["a_full"] * rstd) * d["w"] + d["b"]
    return ref, (3 * U * (d["w"].abs() + d["b"].abs())).expand_as(ref)


def gn_real_inputs(frames, hw, C, groups, dtype, seed=0):
    """Groups with a mean of 30 sigma (sigma = 1/2, mean = +-15), frame 0 constant (variance clamped at 0)."""
    g = torch.Generator().manual_seed(9500 + hw + C + groups + seed)
    cpg = C // groups
    sign = (torch.randint(0, 2, (frames, 1, groups), generator=g) * 2 - 1).to(F32).repeat_interleave(cpg, 2)
    x = 0.5 * torch.randn(frames, hw, C, generator=g) + 15.0 * sign
    x[0] = GN_CONSTANT
    w, b = real_affine(C, 9600 + C)
    return x.to(dtype), w, b


GN_CONSTANT = 3.3


def gn_real_ref_and_bound(x, w, b, eps, groups, chunks):
    """fp64 F.group_norm of the operand as the kernel reads it, and the one-pass formula's bound.
    sum x and sum x**2 go through chains of L = gn_chain() fp32 additions (the squares one rounding more): relative L * 2**-24 and
    (L + 1) * 2**-24. var = E[x**2] - mean**2 (fp64 from there) then has an absolute error of at most (var + mean**2) (L + 1) U + 2 mean**2
    L U <= (var + mean**2) * L * 2**-23 =: dv for L >= 1 - relative (1 + mean**2 / var) * L * 2**-23. The computed variance lies in
    [max(0, var - dv), var + dv] (the clamp at 0 only moves it towards the truth), so with rho = dv / (var + eps) the computed rstd is the
    true one times a factor in [1 / sqrt(1 + rho), 1 / sqrt(max(eps / (var + eps), 1 - rho))]: no first-order step, it holds where the
    variance is lost (the constant frame: rho >> 1, factor in [.., 1], and yhat = 0). The normalised value yhat = (x - mean) * rstd moves
    by |yhat| times that factor's distance from 1, and by the mean's error - mean|x| (L + 1) U: L U from the sum, U from its rounding
    to fp32 - times the largest rstd. The affine and the store: 3 U (|yhat w| + |b|) in fp32, half an fp16 ulp of the result on top
    for fp16."""
    import torch.nn.functional as Fn
    frames, hw, C = x.shape
    cpg = C // groups
    L = gn_chain(hw, C, groups, chunks)
    x64 = x.double()
    ref = Fn.group_norm(x64.permute(0, 2, 1), groups, w.double(), b.double(), f32(eps)).permute(0, 2, 1)
    xg = x64.view(frames, hw, groups, cpg)
    mean = xg.mean((1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean((1, 3))
    e = f32(eps)
    rho = (var + mean ** 2) * L * 2 * U / (var + e)
    rstd = 1.0 / torch.sqrt(var + e)
    rep = lambda t: t.repeat_interleave(cpg, 1)[:, None, :]      # noqa: E731
    yhat = (x64 - rep(mean)) * rep(rstd)
    up = 1.0 / torch.sqrt(torch.maximum(e / (var + e), 1 - rho))
    down = 1.0 / torch.sqrt(1 + rho)
    err_hat = yhat.abs() * rep(torch.maximum(up - 1, 1 - down)) + rep(xg.abs().mean((1, 3)) * (L + 1) * U * rstd * up)
    bound = err_hat * w.double().abs() + 3 * U * ((yhat * w.double()).abs() + b.double().abs())
    if x.dtype == F16:
        bound = bound + ulp16(ref) / 2 + ulp16(ref.abs() + bound) / 2
    return ref, bound, L
