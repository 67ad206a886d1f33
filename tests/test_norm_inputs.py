"""CPU side of tests/test_norm_edges_gpu.py: the inputs of tests/_norm_inputs.py meet the preconditions their equalities rest on
(asserted for every case, nothing assumed), the plain fp32 restatement of each operation meets the very assertion the GPU test
applies to the kernels, and the same restatement with one mistake built in (LN_MUTATIONS and the GroupNorm / finalize twins) fails it
in every listed case the mistake can show in. The derived bounds are checked to hold for the restatement, never fitted to a kernel."""
import pytest
import torch

import _norm_inputs as NI
from _norm_inputs import F16, F32, F64, LnCase, U


def full_case(entry, D, eps, **kw):
    f = dict(entry=entry, D=D, rows=NI.LN_MAX_ROWS, group=0, skip=0, prs=0, steps=0, eps=eps)
    f.update(kw)
    return LnCase(**f)


# ---------------------------------------------------------------- the case lists reach the branches they name
def test_the_case_lists_cover_every_rung_and_every_row_count_around_a_workgroup():
    rungs = [NI.ln_rung(D) for D in NI.LN_D]
    assert sorted(set(rungs)) == sorted({(8, 1, 32), (16, 1, 16), (32, 1, 8), (64, 1, 4), (64, 2, 4), (64, 4, 4)})
    for lo, hi in zip(NI.LN_D[1::2], NI.LN_D[2::2]):
        assert hi == lo + 8 and NI.ln_rung(lo) != NI.ln_rung(hi), "both sides of a rung"
    assert [NI.ln_rung(D)[:2] for D in NI.LN_RUNG_D] == [(8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4)]
    assert [NI.ln_rung(D)[:2] for D in NI.LN_RUNG_D_RAGGED] == [(16, 1), (32, 1), (64, 1), (64, 2), (64, 4), (64, 4)]
    for D in NI.LN_D:
        R = NI.ln_rung(D)[2]
        assert NI.ln_rows(D) == [1, R - 1, R, R + 1, 2 * R + 3] and max(NI.ln_rows(D)) <= NI.LN_MAX_ROWS
    ragged = [D for D in NI.LN_D if D // 8 < NI.ln_rung(D)[0] * NI.ln_rung(D)[1]]
    assert ragged == [8, 72, 136, 264, 520, 1032], "nchunk < LPR * NCH: the `ok` flag of chunk_sq is live on every rung"
    for D, rows in NI.LN_GROUP_SHAPES:
        assert rows % 5 == 0 and rows <= NI.LN_MAX_ROWS and rows > NI.ln_rung(D)[2]
    assert NI.ln_rung(512)[0] == 64 and NI.ln_rung(64)[0] == 8
    ids = [NI.ln_case_id(c) for c in NI.ln_cases()]
    assert len(ids) == len(set(ids))
    assert NI.ln_chain(64) == 3 + 1 + 3 and NI.ln_chain(2048) == 3 + 4 + 6


def test_compaction_places_row_r_at_its_group_offset():
    for group, skip in ((5, 1), (5, 2), (5, 4), (15, 1)):
        for r in range(30):
            g, i = divmod(r, group)
            assert NI.ln_out_row(r, group, skip) == (-1 if i < skip else g * (group - skip) + i - skip)
    assert [NI.ln_out_row(r, 0, 0) for r in range(4)] == [0, 1, 2, 3] == [NI.ln_out_row(r, 1, 0) for r in range(4)]


# ---------------------------------------------------------------- exact rows
@pytest.mark.parametrize("D", NI.LN_D)
def test_exact_rows_meet_their_preconditions_and_fp32_rounds_to_the_integer(D):
    """Sums below 2**24, n a nonzero integer below 2048, and the fp32 evaluation - two summation orders, rstd moved by +-2 ulp, the
    affine contracted to an fma or not, both epsilons, with and without pe - rounds to n in fp16 from within 5e-5 (half an fp16 ulp at
    |n| >= 1 is at least 4.9e-4)."""
    NI.assert_ln_rows(NI.ln_rows_data(D))
    for eps in NI.EPS_LIST:
        for kw in ({}, dict(prs=1, steps=4)):
            case = full_case("layernorm_f32", D, eps, **kw)
            inp = NI.ln_inputs(case)
            outs = []
            for order in ("lanes", "seq"):
                for k in (-2, 0, 2):
                    for fma in (False, True):
                        v = NI.ln_model(case, inp, order=order, rstd_ulps=k, fma=fma)["out"]
                        assert v.dtype == F32
                        assert float((v.double() - inp["n"]).abs().max()) < 5e-5
                        assert torch.equal(v.to(F16).double(), inp["n"]), "the fp32 value does not round to n"
                        outs.append(v)
            assert torch.equal(outs[0], outs[6]), "the summation order changed a result whose sums are exact"


@pytest.mark.parametrize("D", [8, 72, 2048])
def test_exact_row_statistics_are_exact_in_either_order(D):
    case = full_case("stats", D, 1e-6)
    inp = NI.ln_inputs(case)
    for order in ("lanes", "seq"):
        st = NI.ln_model(case, inp, order=order)["stat"]
        assert torch.equal(st[:, 0].double(), inp["m"][:, 0])
        assert torch.equal(st[:, 1], torch.rsqrt((inp["a"][:, 0] ** 2).float() + NI.f32(1e-6)))


def test_the_helpers_refuse_inputs_that_break_a_precondition():
    d = NI.ln_rows_data(64)
    NI.assert_ln_rows(d)
    bad = dict(d, s=d["s"].clone())
    bad["s"][3, 0] = -bad["s"][3, 0]
    with pytest.raises(AssertionError, match="not balanced"):
        NI.assert_ln_rows(bad)
    bad = dict(d, x=d["x"] + 2.0 ** 20)
    with pytest.raises(AssertionError, match="2\\*\\*24"):
        NI.assert_ln_rows(bad)
    bad = dict(d, w=d["w"].clone(), b=d["b"].clone())
    bad["w"][0], bad["b"][0] = 7, 0
    bad["s"] = d["s"].clone()
    NI.assert_ln_rows(bad)
    bad["w"][0], bad["b"][0] = 8, 8                                            # n = +-8 + 8: 0 wherever s = -1
    with pytest.raises(AssertionError, match="n = 0"):
        NI.assert_ln_rows(bad)
    with pytest.raises(AssertionError, match="as many"):
        NI.balanced_signs(2, 7, torch.Generator().manual_seed(0))
    with pytest.raises(AssertionError, match="as many"):
        NI.gn_exact_inputs(1, 1, 8, 8)                                         # hw * C / groups = 1
    g = NI.gn_exact_inputs(1, 33, 64, 32)
    with pytest.raises(AssertionError, match="2\\*\\*24"):
        NI.assert_gn_exact(dict(g, m=g["m"] * 100))
    with pytest.raises(AssertionError, match="not balanced"):
        NI.assert_gn_exact(dict(g, s=g["s"].abs()))


def test_n_is_never_zero_because_w_is_odd_sized_against_multiples_of_8():
    for D in NI.LN_D:
        d = NI.ln_rows_data(D)
        assert bool(((d["w"].abs() >= 1) & (d["w"].abs() <= 7)).all()) and bool((d["b"] % 8 == 0).all()) and bool((d["pe"] % 8 == 0).all())
        assert len({tuple(r.tolist()) for r in d["pe"]}) == 4, "pe steps differ: a wrong step index is seen"
        assert len({tuple(d["w"][k:k + 8].tolist()) for k in range(0, D, 8)}) > 1 or D == 8, "w differs between chunks"


# ---------------------------------------------------------------- the restatement meets the assertion; the mistakes fail it
ALL_CASES = NI.ln_cases()


def test_the_restated_operation_meets_the_assertion_in_every_case():
    for case in ALL_CASES:
        inp = NI.ln_inputs(case)
        assert NI.ln_mismatch(case, inp, NI.ln_model(case, inp)) is None, NI.ln_case_id(case)


@pytest.mark.parametrize("mutation", NI.LN_MUTATIONS)
def test_every_built_in_mistake_fails_wherever_it_applies(mutation):
    hit = [c for c in ALL_CASES if NI.ln_mutation_applies(mutation, c)]
    assert hit, f"{mutation} applies to no listed case"
    for case in hit:
        inp = NI.ln_inputs(case)
        assert NI.ln_mismatch(case, inp, NI.ln_model(case, inp, mutation)) is not None, f"{mutation} goes unnoticed in {NI.ln_case_id(case)}"
    if mutation in ("divisor", "absent_chunks"):
        assert {NI.ln_rung(c.D)[:2] for c in hit} == {(8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4)}, "seen on every rung"
        assert {c.rows for c in hit if c.D == 72} >= {1, 15, 16, 17, 35}
    if mutation == "compaction":
        assert {(c.group, c.skip) for c in hit} == {(5, 1), (5, 2), (5, 4), (15, 1), (70, 1)}


def test_a_single_wrong_element_fails_the_assertion():
    """One output off by one fp16 ulp, one row of the stream off by one, an unwritten (NaN) output: each is seen."""
    case = [c for c in ALL_CASES if c.entry == "residual_gamma" and c.D == 64 and c.group == 5 and c.skip == 2][0]
    inp = NI.ln_inputs(case)
    good = NI.ln_model(case, inp)
    for key, r, bump in (("out", inp["rows_out"] - 1, 2.0 ** -5), ("stream", 5, 1.0), ("out", 0, float("nan"))):
        got = {k: v.clone() for k, v in good.items()}
        got[key][r, -1] += bump
        assert NI.ln_mismatch(case, inp, got) is not None
    case = [c for c in ALL_CASES if c.entry == "layernorm_f32" and c.D == 520][0]
    inp = NI.ln_inputs(case)
    got = NI.ln_model(case, inp)
    ref, bound = NI.ln_f32_ref_and_bound(case, inp)
    assert float(((got["out"].double() - ref).abs() / bound).max()) < 1
    got["out"][0, 3] = NI.step_ulps(got["out"][0, 3].abs()[None], 64)[0] * got["out"][0, 3].sign()
    assert NI.ln_mismatch(case, inp, got) is not None, "64 ulps of an output pass the bound of 7 ulps of |w| + |b|"
    case = [c for c in ALL_CASES if c.entry == "center_stats" and c.D == 136][0]
    inp = NI.ln_inputs(case)
    got = NI.ln_model(case, inp)
    got["stat"][0, 1] = NI.step_ulps(got["stat"][0, 1][None], 4)[0]
    assert NI.ln_mismatch(case, inp, got) is not None


# ---------------------------------------------------------------- ill-conditioned rows: the bound holds for the restatement
@pytest.mark.parametrize("regime", [r for r in NI.ILL_REGIMES if r != "constant"])
@pytest.mark.parametrize("D", NI.LN_RUNG_D_RAGGED[:1] + NI.LN_RUNG_D)
def test_the_two_pass_forward_bound_holds_for_the_fp32_restatement(regime, D):
    x = NI.ill_rows(regime, 9, D, 40 + D)
    w, b = NI.real_affine(D, D)
    case = LnCase("layernorm_f32", D, 9, 0, 0, 0, 0, 1e-6)
    y = NI.ln_model(case, dict(x=x.double(), w=w.double(), b=b.double(), rows_out=9))["out"].double()
    x64 = x.double()
    yhat = (x64 - x64.mean(1, keepdim=True)) / torch.sqrt(x64.var(1, unbiased=False, keepdim=True) + NI.f32(1e-6))
    ref = yhat * w.double() + b.double()
    bound = NI.ln_forward_bound(x64, yhat, D, 1e-6) * w.double().abs() + 2 * U * ((yhat * w.double()).abs() + b.double().abs())
    assert bool(((y - ref).abs() <= bound).all()), f"worst {float(((y - ref).abs() / bound).max()):.3g} of the bound"


def test_a_constant_row_has_zero_variance_and_gives_b():
    for D in NI.LN_RUNG_D + NI.LN_RUNG_D_RAGGED:
        assert float(torch.tensor(NI.ILL_CONSTANT * D, dtype=F64)) == float(torch.tensor(NI.ILL_CONSTANT, dtype=F32) * D), "c * D is exact in fp32"
        x = NI.ill_rows("constant", 3, D, 0)
        w, b = NI.real_affine(D, D)
        case = LnCase("layernorm_f32", D, 3, 0, 0, 0, 0, 1e-6)
        for order in ("lanes", "seq"):
            y = NI.ln_model(case, dict(x=x.double(), w=w.double(), b=b.double(), rows_out=3), order=order)["out"]
            assert torch.equal(y, b.expand(3, D))


# ---------------------------------------------------------------- vda_ln_stats_finalize
def test_finalize_exact_partials_combine_exactly():
    for np_ in NI.FIN_NP:
        for rows in NI.FIN_ROWS:
            partial, mean, m2 = NI.finalize_exact_inputs(rows, np_)
            assert partial.shape == (np_, rows, 2) and torch.equal(partial[..., 0].double() / 64, mean.expand(np_, rows))
            st = NI.finalize_model(partial, 1e-6)
            assert torch.equal(st[:, 0].double(), mean), "the combined mean is exact"
            ref = 1.0 / torch.sqrt(m2 / (64 * np_) + NI.f32(1e-6))
            assert float(((st[:, 1].double() - ref).abs() / NI.ulp32(ref)).max()) <= 2
            if np_ % 8:
                bad = NI.finalize_model(partial, 1e-6, batch_clamp=False)
                assert not torch.equal(bad[:, 0].double(), mean), "a batch slot past np read as a block goes unnoticed"


def test_finalize_real_partials_stay_inside_the_chan_bound():
    for np_ in NI.FIN_NP:
        partial = NI.finalize_real_inputs(65, np_)
        mean, rstd, mean_tol, rstd_tol = NI.finalize_pooled(partial, 1e-6)
        st = NI.finalize_model(partial, 1e-6).double()
        assert bool(((st[:, 0] - mean).abs() <= mean_tol).all()) and bool(((st[:, 1] - rstd).abs() <= rstd_tol).all())
        assert float((rstd_tol / rstd).max()) < 1e-3, "the bound still says something"
        if np_ > 1:
            mb = partial[..., 0].double() / 64
            assert float((mb.max(0).values - mb.min(0).values).median()) > 10, "block means differ by many sigma (sigma ~ 1)"


def test_finalize_overflow_places():
    assert NI.finalize_overflow_places(130, 9) == [(0, 0), (8, 129), (4, 97)]


# ---------------------------------------------------------------- GroupNorm
GN_CASES = [(f, hw, C, g) for C, g in NI.GN_GEOM for hw in NI.GN_HW for f in NI.GN_FRAMES if (hw * (C // g)) % 2 == 0]


def test_groupnorm_case_lists():
    assert len(GN_CASES) == len(NI.GN_GEOM) * len(NI.GN_HW) * len(NI.GN_FRAMES), "every listed geometry has an even group size"
    assert [256 % (C // 8) for C, _ in NI.GN_GEOM] == [0, 0, 16, 0, 0, 4] and 256 // (1024 // 8) == 2
    assert NI.gn_chunks(1) == [1] and NI.gn_chunks(33) == [1, 2, 8, 33] and NI.gn_has_empty_chunk(10, 7) and NI.gn_has_empty_chunk(33, 8)
    assert not NI.gn_has_empty_chunk(33, 2) and not NI.gn_has_empty_chunk(33, 33)
    for hw in NI.GN_HW:
        assert hw == 1 or any(NI.gn_has_empty_chunk(hw, c) for c in NI.gn_chunks(hw))
    assert NI.gn_chain(65, 64, 32, 1) == 3 + 32 + 2 and NI.gn_chain(65, 1024, 32, 1) == 33 + 2 + 32


@pytest.mark.parametrize("C,groups", NI.GN_GEOM)
def test_groupnorm_exact_inputs_do_not_depend_on_chunks(C, groups):
    for frames, hw in ((1, 1), (3, 33), (1, 65), (1, 10)):
        d = NI.gn_exact_inputs(frames, hw, C, groups)               # (asserts the preconditions)
        chunk_list = NI.gn_chunks(hw) + ([7] if hw == 10 else [])
        ref, bound = NI.gn_f32_ref_and_bound(d, 1e-6)
        first = None
        for chunks in chunk_list:
            y32, y16 = NI.gn_model(d, 1e-6, chunks, F32), NI.gn_model(d, 1e-6, chunks, F16)
            assert torch.equal(y16.double(), d["n"]), "the fp16 result is the integer n"
            assert bool(((y32.double() - ref).abs() <= bound).all())
            first = y32 if first is None else first
            assert torch.equal(first, y32), "exact sums: the result cannot depend on chunks"
            if chunks > 1 and not NI.gn_has_empty_chunk(hw, chunks):
                assert not torch.equal(NI.gn_model(d, 1e-6, chunks, F16, drop_last_chunk=True).double(), d["n"]), "a dropped chunk goes unnoticed"


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_groupnorm_one_pass_bound_holds_for_the_restatement(dtype):
    for C, groups in NI.GN_GEOM:
        for hw in (33, 65):
            x, w, b = NI.gn_real_inputs(2, hw, C, groups, dtype)
            for chunks in (1, hw):
                ref, bound, L = NI.gn_real_ref_and_bound(x, w, b, 1e-6, groups, chunks)
                d = dict(x=x.double(), w=w.double(), b=b.double(), frames=2, hw=hw, C=C, groups=groups)
                y = NI.gn_model(d, 1e-6, chunks, dtype).double()
                assert bool(((y - ref).abs() <= bound).all()), f"C={C} hw={hw} chunks={chunks} L={L}: worst {float(((y - ref).abs() / bound).max()):.3g} of the bound"
                assert float((ref[0] - b.double()).abs().max()) < 1e-9, "frame 0 is constant: its reference is b"
                assert float(bound[1].max()) < 0.1, "the bound still says something on the 30-sigma frames"
