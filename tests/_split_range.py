"""Inputs at the edge of the split residual stream's range, shared by tests/test_split_range_inputs.py (CPU: the inputs are what they
claim and every comparison can fail) and tests/test_split_range_gpu.py (GPU: the kernels meet them).

The stream is two fp16 planes, x = hi + lo with hi = fp16(x), lo = fp16(x - hi) (include/vda.h, VDA_EPI_SCALE_RES_SPLIT). 65 504 is
the largest fp16; the largest fp32 below 65 520 (NA below) still rounds to it, with lo = 16; 65 520 rounds to inf, and lo is then
fp16(x - inf) = -inf: a SATURATED element, hi + lo = NaN for whoever reads it back.

A case is the operand set of one residual update whose fp32 result X[m, n] is known exactly, whatever the order of the sums:

    X = ((res_hi + res_lo) - pos[m]) + gamma[n] * (A[m, :] . W[n, :] + bias[n])          (one fma on top of exact terms)

A in [-2, 2], W in [-1, 1], bias in [0, 8] are integers, gamma a power of two in {0.5, 1, 2}: gamma * (acc + bias) = u is a multiple of
0.5 with 0 <= |u| <= 272 (K = 64). The target X is placed through the residual planes, r = X - u + pos, a multiple of 0.5 of at most
65 504 - which two fp16 hold exactly (the remainder after hi is at most 16, in steps of 0.5). pos is the row's integer centre: -+300 in
a row that holds +-65 504 (so that r stays below it for every u), -+40 000 in a row that holds a saturating value (r + 40 000 and the
fma's result, up to 1e5, are integers or half-integers far below 2**24). The fused MLP kernel reaches the same X with acc = 0 (fc1 = 0:
GELU(0) = 0), bias = b2 and pos = the LayerNorm mean of its statistics rows.

Row kinds:
  EXACT      every 64-column block is c + a * s, s = +-1 with 32 of each sign (or a constant: +-65 504 in all 64 columns). Block sum 64 c,
             mean c, centred values +-a, centred squares 64 a**2: integers or half-integers below 2**24 in any order - the partial
             statistics of VDA_EPI_SCALE_RES_SPLIT are exact, from the fp32 values and from the stored planes alike (hi + lo = X).
  NEAR       +-NA in all 64 columns of one block, a small constant minus 2**-8 in the others: the fraction rides on pos (= -+300 +-
             2**-8; A's row is 0, so u = gamma * bias >= 0 and (r - pos) stays below 65 536, where fp32 still holds 2**-8). In range, but
             hi + lo = 65 520 is not X: a kernel that takes the statistics from its fp32 values has a block sum of 64 X, one that re-reads
             the planes 64 * 65 520 - both exact in a pairwise or (planes) any order, centred squares 0. The other blocks are 64 equal
             values of at most 18 significant bits: sum exact in any order, centred squares 0.
  SATURATED  one element of one block holds 65 520, -65 520, 65 536 or 1e5; the rest of the row is as in an EXACT row. Its planes are
             +-inf / -+inf there; its statistics depend on where the kernel takes them from and are not compared.

Placements: rows 0, 127, 128, 255, 256, 270, M - 13 and M - 1 (first and last row, either side of every tile height, rows of the last
partial 128-, 192- and 256-row tile), each value in each of them over the eight scenes of a shape, the block moving with the scene."""
import numpy as np

NA = float(np.nextafter(np.float32(65520.0), np.float32(0.0)))          # 65519.99609375 = 65520 - 2**-8: the largest fp32 that stays finite
IN_RANGE = (65504.0, -65504.0, NA, -NA)
SATURATING = (65520.0, -65520.0, 65536.0, 1.0e5)
VALUES = IN_RANGE + SATURATING
SCENES = tuple(range(8))
EXACT, NEAR, SATURATED, IGNORED = 0, 1, 2, 3
ORDINARY_C = (2049.0, 4097.5, -2049.0, -4097.5, 100.0, 0.5, 1023.0, -3.5)      # 2049 and 4097.5 need the lo plane
NEAR_C = (100.0, 0.5, 1023.0, -3.5)                                           # at most 10 bits in front of the 2**-8 fraction
ORDINARY_A = (0.0, 1.0, 2.0, 4.0)
GEMM_SHAPES = ((300, 128, 64), (2, 64, 64))        # (M, N, K)
MLP_SHAPES = ((50, 384), (128 * 3 + 37, 384))      # (M, D); hidden = 4 D
U = 2.0 ** -24
# vda_gemm_set_variant value (the parameters of test_kernels_gpu.py's gemm_variant fixture) -> the family VDA_EPI_SCALE_RES_SPLIT runs in
# at GEMM_SHAPES: 0 = the 128-row kernel (it has no 32x32x16-MFMA large tile: variants 1 and 2 stay there), 2 = 256 / 192-row tiles on
# 16x16x32 MFMA, 3 = the 8-phase kernel. tests/test_split_range_inputs.py holds the table to the planner.
VARIANT_FAMILY = {-1: 0, 0: 0, 1: 0, 2: 0, 7: 0, 3: 2, 4: 2, 8: 2, 10: 2, 11: 2, 5: 3, 9: 3, 5 + 16 * 64: 3}
FORWARD_VARIANTS = (-1, 1, 4, 5, 8)                # what the forward tests run the tiny model under
VITS_FRAMES, VITS_TOKENS = 32, 19 * 19 + 1         # the ViT-S clip of the forward tests: 32 frames of 266 x 266


def special_rows(M):
    rows = []
    for r in (0, 127, 128, 255, 256, 270, M - 13, M - 1):
        if 0 <= r < M and r not in rows:
            rows.append(r)
    return rows


def scene(M, N, k, sat_from=0):
    """[(row, value, block, column in the block)] of scene k: special row i holds VALUES[(k + 3 i) % 8] (3 and 8 are coprime: over the
    eight scenes every row holds every value; a shape with two special rows holds one in-range and one saturating value in scenes
    1, 2, 3, 6 and 7), in block (i + k) % (N / 64). Rows below sat_from take the in-range value of that index instead."""
    nb = N // 64
    out = []
    for i, r in enumerate(special_rows(M)):
        v = VALUES[(k + 3 * i) % 8]
        if r < sat_from:
            v = IN_RANGE[(k + 3 * i) % 4]
        out.append((r, v, (i + k) % nb, (11 * k + 5 * i + 3) % 64))
    return out


def planes_of(X):
    """The definition, in numpy: hi = float16(X), lo = float16(X - float32(hi))."""
    assert X.dtype == np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        hi = X.astype(np.float16)
        lo = (X - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def build(M, N, K, placements, seed, gemm=True):
    """The operands and references of one case (module docstring). gemm = False: no A / W (acc = 0), the fused MLP kernel's form."""
    assert N % 64 == 0 and (not gemm or K % 64 == 0)
    nb = N // 64
    rng = np.random.default_rng([seed, M, N, K])
    c = rng.choice(ORDINARY_C, size=(M, nb))
    a = rng.choice(ORDINARY_A, size=(M, nb))
    s = np.where(rng.permuted(np.tile(np.arange(64), (M * nb, 1)), axis=1) < 32, 1.0, -1.0).reshape(M, nb, 64)
    T = c[:, :, None] + a[:, :, None] * s                      # fp64 [M, nb, 64]
    kind = np.full(M, EXACT)
    frac = np.zeros(M)
    p = rng.integers(-3, 4, size=M).astype(np.float64)
    A = rng.integers(-2, 3, size=(M, K)).astype(np.float64) if gemm else np.zeros((M, 1))
    W = rng.integers(-1, 2, size=(N, K)).astype(np.float64) if gemm else np.zeros((N, 1))
    for r, v, b, col in placements:
        assert kind[r] == EXACT, "one placement per row"
        sign = 1.0 if v > 0 else -1.0
        if abs(v) > NA:
            T[r, b, col] = v
            kind[r], p[r] = SATURATED, -sign * 40000.0
        elif abs(v) == NA:
            T[r] = rng.choice(NEAR_C, size=(nb, 1))
            T[r, b] = sign * 65520.0
            kind[r], p[r], frac[r] = NEAR, -sign * 300.0, sign * 2.0 ** -8
            A[r] = 0.0
        else:
            assert abs(v) == 65504.0
            T[r, b] = v
            p[r] = -sign * 300.0
    Tint = T.reshape(M, N)
    T = Tint - frac[:, None]
    bias = rng.integers(0, 9, size=N).astype(np.float64)
    gamma = rng.choice((0.5, 1.0, 2.0), size=N)
    u = gamma * (A @ W.T + bias)
    r = Tint - u + p[:, None]
    pos = p + frac
    # ---- preconditions: every intermediate of the evaluation is held exactly
    X = T.astype(np.float32)
    assert np.array_equal(X.astype(np.float64), T), "a target is not an fp32 value"
    assert np.array_equal(r * 2, np.round(r * 2)) and np.abs(r).max() <= 65504.0
    res_hi, res_lo = planes_of(r.astype(np.float32))
    assert np.array_equal(res_hi.astype(np.float64) + res_lo.astype(np.float64), r), "the residual planes do not hold r"
    assert np.array_equal(pos.astype(np.float32).astype(np.float64), pos)
    q = r - pos[:, None]                                       # (res_hi + res_lo) - pos: one fp32 subtraction
    assert np.array_equal(q.astype(np.float32).astype(np.float64), q), "(r - pos) rounds in fp32"
    assert np.abs(A @ W.T).max() + 8 < 2 ** 11 and np.abs(u).max() <= 2 * (2 * K + 8)
    assert np.array_equal(q + u, T)                            # the fma: exact terms, a representable result
    hi, lo = planes_of(X)
    sat_elems = ~np.isfinite(hi.astype(np.float32))
    assert np.array_equal(sat_elems.any(1), kind == SATURATED) and np.array_equal(sat_elems, np.abs(T) >= 65520.0)
    # ---- partial statistics of the EXACT rows, [nb, M, 2] as the kernels lay them out
    blocks = T.reshape(M, nb, 64)
    mean = blocks.mean(-1)
    d = blocks - mean[..., None]
    part = np.stack((blocks.sum(-1), (d * d).sum(-1)), axis=-1).transpose(1, 0, 2)
    ex = kind == EXACT
    top = np.abs(d[ex]).max(-1)
    assert np.array_equal(np.abs(d[ex]), np.broadcast_to(top[..., None], d[ex].shape)) and (top <= 4.0).all(), "an EXACT block is not c +- a"
    assert np.array_equal(blocks[ex].sum(-1), 64 * mean[ex]) and (np.abs(blocks[ex]).sum(-1) < 2 ** 24).all()
    assert np.array_equal(part.astype(np.float32).astype(np.float64)[:, ex], part[:, ex])
    near_block = np.zeros((M, nb), dtype=bool)
    for row in np.flatnonzero(kind == NEAR):
        assert np.array_equal(d[row], np.zeros((nb, 64))), "a NEAR row's blocks are constants"
        near_block[row] = np.abs(blocks[row, :, 0]) == NA
        assert near_block[row].sum() == 1
        others = blocks[row, ~near_block[row], 0]
        assert (np.abs(others) < 1024).all() and np.array_equal(others * 256, np.round(others * 256))    # 18 bits: 64 of them sum exactly
    f32 = lambda t: np.ascontiguousarray(t, dtype=np.float32)
    return dict(M=M, N=N, K=K, A=A.astype(np.float16), W=W.astype(np.float16), bias=f32(bias), gamma=f32(gamma),
                pos=f32(np.stack((pos, np.ones(M)), axis=1)), res_hi=res_hi, res_lo=res_lo, X=X, hi=hi, lo=lo, kind=kind,
                sat_rows=np.flatnonzero(kind == SATURATED), part=f32(part), near_block=near_block, placements=list(placements))


def zeroed(case):
    """The same launch with the saturated rows replaced by zeros: A, the residual planes and the centre. Those rows then hold gamma *
    bias; every other row's operands are the same bits."""
    z = dict(case)
    for k in ("A", "res_hi", "res_lo", "pos"):
        z[k] = case[k].copy()
        z[k][case["sat_rows"]] = 0
    z["pos"][:, 1] = 1.0
    X = z["X"].copy()
    X[case["sat_rows"]] = case["gamma"] * case["bias"]
    z["X"] = X
    z["hi"], z["lo"] = planes_of(X)
    z["kind"] = np.where(case["kind"] == SATURATED, IGNORED, case["kind"])    # (gamma * bias is no c +- a block: statistics not compared)
    z["sat_rows"] = np.zeros(0, dtype=np.int64)
    return z


def fp64_result(case):
    """X once more, from the operands as the kernel receives them, in fp64."""
    g = {k: np.asarray(v, dtype=np.float64) for k, v in case.items() if k in ("A", "W", "bias", "gamma", "pos", "res_hi", "res_lo")}
    return (g["res_hi"] + g["res_lo"] - g["pos"][:, :1]) + g["gamma"] * (g["A"] @ g["W"].T + g["bias"])


# ------------------------------------------------------------------------------------------------ the comparisons of the GPU file
def bits16(t):
    return np.ascontiguousarray(t, dtype=np.float16).view(np.uint16)


def bits32(t):
    return np.ascontiguousarray(t, dtype=np.float32).view(np.uint32)


def planes_mismatch(case, hi, lo, rows=None):
    """None, or what differs: both planes bit for bit against the definition (every row, or `rows`)."""
    sel = slice(None) if rows is None else rows
    for name, got, ref in (("hi", hi, case["hi"]), ("lo", lo, case["lo"])):
        bad = bits16(got)[sel] != bits16(ref)[sel]
        if bad.any():
            m, n = np.argwhere(bad)[0]
            return (f"{name} plane: {int(bad.sum())} elements differ, the first at ({m}, {n}) of the compared rows: "
                    f"{np.asarray(got)[sel][m, n]!r}, not {np.asarray(ref)[sel][m, n]!r} (X = {case['X'][sel][m, n]!r})")
    return None


def near_sum_bound(mode):
    """|block sum - 64 NA| of a NEAR row's +-NA block. A pairwise tree over 64 equal values is exact, and so is any order over the planes'
    65 520. `mlp`: vda_mlp_fused_f16 adds 16 of its fp32 values in sequence before it pairs lanes - each of the 15 additions rounds a
    partial sum of at most 16 NA (half an ulp of 2**20: 2**-4) and the two pairings double it: 4 * 15 * 2**-4."""
    return 0.0 if mode == "gemm" else 4 * 15 * 2.0 ** -4


def partials_mismatch(case, part, mode="gemm"):
    """None, or what differs, in the [N / 64, M, 2] partial statistics of the rows that are in range. EXACT rows: equality with the
    builder's (sum, centred squares). NEAR rows: the +-NA block's sum is 64 NA or 64 * 65 520 (within near_sum_bound of the first for the
    fused MLP kernel) and its centred squares are those of a mean that is off by delta / 64 when the sum is off by delta: 64 equal
    centred values of delta / 64 (the subtraction of two fp32 that close is exact), delta**2 / 64 up to the roundings of 64 fused
    multiply-adds - and 0 when delta is 0; the other blocks equal the builder's. Saturated rows are not looked at."""
    part = np.asarray(part, dtype=np.float32)
    ref = case["part"]
    assert part.shape == ref.shape
    ex = case["kind"] == EXACT
    bad = (bits32(part) != bits32(ref))[:, ex].any(-1)
    if bad.any():
        b, i = np.argwhere(bad)[0]
        m = np.flatnonzero(ex)[i]
        return f"partial statistics of row {m}, block {b}: {part[b, m].tolist()}, not {ref[b, m].tolist()} ({int(bad.sum())} blocks differ)"
    for m in np.flatnonzero(case["kind"] == NEAR):
        for b in range(ref.shape[0]):
            got = part[b, m].astype(np.float64)
            if not case["near_block"][m, b]:
                if not np.array_equal(bits32(part[b, m]), bits32(ref[b, m])):
                    return f"NEAR row {m}, constant block {b}: {got.tolist()}, not {ref[b, m].tolist()}"
                continue
            sign = np.sign(case["X"][m, 64 * b])
            from_values, from_planes = sign * 64 * NA, sign * 64 * 65520.0
            delta = min(abs(got[0] - from_values), abs(got[0] - from_planes) if mode == "gemm" else np.inf)
            if not (np.isfinite(got).all() and delta <= near_sum_bound(mode)):
                return f"NEAR row {m}, block {b}: sum {got[0]!r} is neither {from_values!r} nor {from_planes!r}"
            if not 0.0 <= got[1] <= delta * delta / 64 * (1 + 64 * U):
                return f"NEAR row {m}, block {b}: centred squares {got[1]!r} of 64 equal values (sum off by {delta})"
    return None


def nonfinite_rows(part):
    part = np.asarray(part, dtype=np.float32)
    return np.flatnonzero(~np.isfinite(part).all(axis=(0, 2)))


def next_step_mismatch(case, part2, flag, stat, stat_clean):
    """The step AFTER the one that saturated, over planes that hold +-inf / -+inf: part2 = the partials of a second residual GEMM over
    them, flag / stat = what vda_ln_stats_finalize makes of part2, stat_clean = the same chain from the zeroed planes. None, or what is
    wrong: the rows with a non-finite partial are exactly the saturated rows, the flag is 1 exactly when there is one, and every other
    row's (mean, rstd) is the clean chain's, bit for bit."""
    bad_rows = nonfinite_rows(part2)
    if not np.array_equal(bad_rows, case["sat_rows"]):
        return f"rows with a non-finite partial: {bad_rows.tolist()}, saturated rows: {case['sat_rows'].tolist()}"
    want = int(len(case["sat_rows"]) > 0)
    if int(flag) != want:
        return f"overflow flag {int(flag)}, expected {want}"
    keep = np.ones(case["M"], dtype=bool)
    keep[case["sat_rows"]] = False
    diff = (bits32(stat) != bits32(stat_clean))[keep].any(-1)
    if diff.any():
        m = np.flatnonzero(keep)[np.flatnonzero(diff)[0]]
        return f"(mean, rstd) of the in-range row {m}: {np.asarray(stat)[m].tolist()}, clean chain {np.asarray(stat_clean)[m].tolist()}"
    return None


def rows_mismatch(got, ref, rows, what):
    """None, or the first of `rows` in which two arrays of the same dtype differ in a bit."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape
    if len(rows) == 0:
        return None
    view = np.uint16 if got.dtype == np.float16 else np.uint32
    bad = (np.ascontiguousarray(got).view(view) != np.ascontiguousarray(ref).view(view))[rows].reshape(len(rows), -1).any(-1)
    if bad.any():
        return f"{what}: row {int(np.asarray(rows)[np.flatnonzero(bad)[0]])} differs ({int(bad.sum())} rows)"
    return None


# ------------------------------------------------------------------------------------------------ the tap LayerNorm's own cases
LN_ROWS, LN_GROUP, LN_SKIP = 300, 5, 1
LN_D = (128, 384)                                   # 16 lanes per row (tiny) and 64 (ViT-S: the v_readlane rung)
LN_SAT_ROWS = (0, 255, 256, 270, 299)               # % 5 = 0, 0, 1, 0, 4: three that group / skip drops, two that it keeps


def ln_case(D, i, value_shift=0):
    """Planes with ONE saturated row, LN_SAT_ROWS[i], holding SATURATING[(i + value_shift) % 4] in block (i + value_shift) % (D / 64);
    every other special row holds an in-range edge value. (case, row, dropped by LN_GROUP / LN_SKIP)."""
    row = LN_SAT_ROWS[i]
    nb = D // 64
    pl = [(r, IN_RANGE[(j + i) % 4], (j + i) % nb, 0) for j, r in enumerate(special_rows(LN_ROWS)) if r != row]
    pl.append((row, SATURATING[(i + value_shift) % 4], (i + value_shift) % nb, (7 * i + 2 + 29 * value_shift) % 64))
    return build(LN_ROWS, D, 64, pl, seed=50 + i, gemm=False), row, row % LN_GROUP < LN_SKIP


def ln_in_range_case(D, k):
    """No saturated row: +-65 504 and +-NA in every special row (scene k with every value taken from IN_RANGE)."""
    return build(LN_ROWS, D, 64, scene(LN_ROWS, D, k, sat_from=LN_ROWS), seed=70 + k, gemm=False)


def ln_kept(rows, group, skip):
    """(input rows that are normalised, their output rows) under group / skip."""
    r = np.arange(rows)
    if group <= 0:
        return r, r
    keep = r % group >= skip
    return r[keep], (r // group * (group - skip) + r % group - skip)[keep]
