"""CPU side of tests/test_split_range_gpu.py: the cases of tests/_split_range.py are what they claim (an fp64 and an fp32 evaluation of
the operands give the target, the planes follow from the definition by two independent fp16 roundings, the partial statistics come out
of plain fp32 restatements of the kernels' three summation orders), every comparison the GPU file applies can fail (one plane bit, one
partial, one flag, one row), and the planner sends the GPU file's shapes where that file says it does."""
import ctypes as C

import numpy as np
import pytest
import torch

import _split_range as SR

F32 = np.float32


def gemm_cases():
    for M, N, K in SR.GEMM_SHAPES:
        for k in SR.SCENES:
            yield SR.build(M, N, K, SR.scene(M, N, k), seed=k)


def mlp_cases():
    for M, D in SR.MLP_SHAPES:
        for k in SR.SCENES:
            yield SR.build(M, D, 64, SR.scene(M, D, k), seed=20 + k, gemm=False)


def all_cases():
    yield from gemm_cases()
    yield from mlp_cases()
    for D in SR.LN_D:
        for i in range(len(SR.LN_SAT_ROWS)):
            yield SR.ln_case(D, i)[0]
        yield SR.ln_in_range_case(D, 1)


# ---------------------------------------------------------------- the edge itself
def test_the_edge_of_fp16_is_where_the_module_says():
    x = np.array([65504.0, SR.NA, 65520.0, 65536.0, 1e5, -SR.NA, -65520.0, 2049.0, 4097.5], dtype=F32)
    hi, lo = SR.planes_of(x)
    assert SR.NA == 65520.0 - 2.0 ** -8 and np.nextafter(F32(SR.NA), F32(1e9)) == F32(65520.0)
    assert hi.tolist() == [65504.0, 65504.0, np.inf, np.inf, np.inf, -65504.0, -np.inf, 2048.0, 4096.0]
    assert lo.tolist() == [0.0, 16.0, -np.inf, -np.inf, -np.inf, -16.0, np.inf, 1.0, 1.5]
    with np.errstate(invalid="ignore"):
        back = hi.astype(F32) + lo.astype(F32)
    assert np.isnan(back[[2, 3, 4, 6]]).all() and back[1] == 65520.0 and back[7] == 2049.0 and back[8] == 4097.5
    # torch rounds the same way (an independent implementation of the conversion)
    t = torch.from_numpy(x)
    th = t.half()
    assert np.array_equal(SR.bits16(th.numpy()), SR.bits16(hi)) and np.array_equal(SR.bits16((t - th.float()).half().numpy()), SR.bits16(lo))


# ---------------------------------------------------------------- the references are what they claim
def test_every_case_evaluates_to_its_target_in_fp64_and_in_fp32():
    n = 0
    for case in all_cases():
        assert np.array_equal(SR.fp64_result(case), case["X"].astype(np.float64))
        f = {k: case[k].astype(F32) for k in ("A", "W", "res_hi", "res_lo")}
        for order in (slice(None), slice(None, None, -1)):            # K summed forwards and backwards: integers, the same
            acc = np.zeros((case["M"], case["N"]), dtype=F32)
            for kk in range(f["A"].shape[1])[order]:
                acc += f["A"][:, kk:kk + 1] * f["W"][:, kk][None, :]
            x32 = ((f["res_hi"] + f["res_lo"]) - case["pos"][:, :1]) + case["gamma"] * (acc + case["bias"])      # (gamma * v is exact: no fma needed)
            assert x32.dtype == F32 and np.array_equal(SR.bits32(x32), SR.bits32(case["X"]))
        t = torch.from_numpy(case["X"])
        assert SR.planes_mismatch(case, t.half().numpy(), (t - t.half().float()).half().numpy()) is None
        sat = ~np.isfinite(case["hi"].astype(F32))
        assert np.array_equal(case["lo"].astype(F32)[sat], -case["hi"].astype(F32)[sat]), "a saturated element is (+-inf, -+inf)"
        inr = case["kind"] == SR.EXACT
        assert np.array_equal(case["hi"][inr].astype(np.float64) + case["lo"][inr].astype(np.float64), case["X"][inr].astype(np.float64))
        n += 1
    assert n == 8 * 4 + 2 * 6


def test_the_scenes_place_every_value_in_every_special_row_and_block():
    for M, N in [(m, n) for m, n, _ in SR.GEMM_SHAPES] + list(SR.MLP_SHAPES):
        rows = SR.special_rows(M)
        assert rows[0] == 0 and rows[-1] == M - 1
        seen = {(r, v) for k in SR.SCENES for r, v, _, _ in SR.scene(M, N, k)}
        assert seen == {(r, v) for r in rows for v in SR.VALUES}
        for r in rows:
            assert {b for k in SR.SCENES for rr, _, b, _ in SR.scene(M, N, k) if rr == r} == set(range(N // 64))
    assert SR.special_rows(300) == [0, 127, 128, 255, 256, 270, 287, 299] and SR.special_rows(2) == [0, 1]
    assert SR.special_rows(421) == [0, 127, 128, 255, 256, 270, 408, 420] and SR.special_rows(50) == [0, 37, 49]
    # the row-range scene: nothing saturates below the split
    case = SR.build(300, 128, 64, SR.scene(300, 128, 0, sat_from=280), seed=0)
    assert case["sat_rows"].tolist() == [299] and (case["kind"][:280] != SR.SATURATED).all()
    kinds = [SR.build(2, 64, 64, SR.scene(2, 64, k), seed=k)["kind"].tolist() for k in SR.SCENES]
    assert [SR.EXACT, SR.SATURATED] in kinds and [SR.SATURATED, SR.EXACT] in kinds and [SR.NEAR, SR.SATURATED] in kinds


# ---------------------------------------------------------------- the kernels' summation orders, restated in fp32
def tree(v):
    """pairwise over the last axis (a power of two long), fp32"""
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def partials_pairwise_from_values(X):
    """finish_row8: eight lanes of eight columns, pairwise in the lane, then a butterfly across the lanes."""
    M, N = X.shape
    b = X.reshape(M, N // 64, 8, 8)
    s = tree(tree(b))
    d = b - (s * F32(1 / 64))[..., None, None]
    sq = np.zeros(b.shape[:3], dtype=F32)
    for e in range(8):
        sq = d[..., e] * d[..., e] + sq
    return np.stack((s, tree(sq)), axis=-1).transpose(1, 0, 2)


def partials_sequential_from_planes(hi, lo):
    """split_partials_kernel: 64 columns in order, from the stored planes."""
    x = (hi.astype(F32) + lo.astype(F32)).reshape(hi.shape[0], -1, 64)
    s = np.zeros(x.shape[:2], dtype=F32)
    for e in range(64):
        s = s + x[..., e]
    d = x - (s * F32(1 / 64))[..., None]
    sq = np.zeros_like(s)
    for e in range(64):
        sq = d[..., e] * d[..., e] + sq
    return np.stack((s, sq), axis=-1).transpose(1, 0, 2)


def partials_mlp_from_values(X):
    """vda_mlp_fused_f16: a lane holds columns 16 j + 4 fh + e (j, e < 4) of the block, adds them in sequence, then pairs the four lanes."""
    M, N = X.shape
    b = X.reshape(M, N // 64, 4, 4, 4).transpose(0, 1, 3, 2, 4).reshape(M, N // 64, 4, 16)       # [.., fh, 4 j + e]
    s = np.zeros(b.shape[:3], dtype=F32)
    for i in range(16):
        s = s + b[..., i]
    s = tree(s)
    d = b - (s * F32(1 / 64))[..., None, None]
    sq = np.zeros(b.shape[:3], dtype=F32)
    for i in range(16):
        sq = d[..., i] * d[..., i] + sq
    return np.stack((s, tree(sq)), axis=-1).transpose(1, 0, 2)


def in_range_only(case, part):
    """Saturated rows' partials are family-dependent and not compared: blank them so that NaN warnings do not hide anything."""
    part = part.copy()
    part[:, case["sat_rows"]] = 0
    return part


def test_the_partial_statistics_are_exact_in_every_order_a_kernel_uses():
    with np.errstate(invalid="ignore", over="ignore"):
        for case in gemm_cases():
            for part in (partials_pairwise_from_values(case["X"]), partials_sequential_from_planes(case["hi"], case["lo"])):
                assert SR.partials_mismatch(case, in_range_only(case, part)) is None
            z = SR.zeroed(case)
            assert SR.partials_mismatch(z, partials_pairwise_from_values(z["X"])) is None
        for case in mlp_cases():
            assert SR.partials_mismatch(case, in_range_only(case, partials_mlp_from_values(case["X"])), mode="mlp") is None
        # the one bound: 3 NA, 5 NA, ... are no fp32 values, so the fused kernel's 16 additions in sequence round on the way (the GEMMs'
        # pairwise tree never does); this restatement lands on 64 NA all the same, well within the bound
        row = np.full((1, 64), SR.NA, dtype=F32)
        assert float(partials_pairwise_from_values(row)[0, 0, 0]) == 64 * SR.NA and float(F32(3) * F32(SR.NA)) != 3 * SR.NA
        off = abs(float(partials_mlp_from_values(row)[0, 0, 0]) - 64 * SR.NA)
        assert off <= SR.near_sum_bound("mlp") and SR.near_sum_bound("gemm") == 0


# ---------------------------------------------------------------- every comparison can fail
def flip(t, idx, bit=0):
    out = np.array(t, copy=True)
    view = out.view(np.uint16 if out.dtype == np.float16 else np.uint32)
    view[idx] ^= 1 << bit
    return out


def test_one_wrong_plane_bit_is_noticed():
    case = SR.build(300, 128, 64, SR.scene(300, 128, 3), seed=3)
    assert SR.planes_mismatch(case, case["hi"], case["lo"]) is None
    sat = np.argwhere(~np.isfinite(case["hi"].astype(F32)))[0]
    for plane in ("hi", "lo"):
        for idx in ((0, 0), (299, 127), (255, 64), (256, 63), tuple(sat)):
            for bit in (0, 15):
                got = {"hi": case["hi"], "lo": case["lo"], plane: flip(case[plane], idx, bit)}
                assert plane in SR.planes_mismatch(case, got["hi"], got["lo"])
    # a saturated element that comes back as the largest finite value, or with a finite lo, is a mismatch
    hi = case["hi"].copy()
    hi[tuple(sat)] = np.float16(65504.0) * np.sign(hi[tuple(sat)])
    assert SR.planes_mismatch(case, hi, case["lo"]) is not None
    assert SR.planes_mismatch(case, case["hi"], np.where(np.isfinite(case["lo"].astype(F32)), case["lo"], np.float16(0))) is not None
    assert SR.planes_mismatch(case, hi, case["lo"], rows=np.array([1, 2, 3])) is None           # (rows: only those are compared)
    # leakage: a neighbour of the saturated row that turned NaN
    near = flip(case["hi"], (int(sat[0]) - 1 if sat[0] else 1, 5), 14)
    assert SR.rows_mismatch(near, case["hi"], np.flatnonzero(case["kind"] != SR.SATURATED), "hi") is not None
    assert SR.rows_mismatch(case["hi"], case["hi"], np.arange(300), "hi") is None
    assert SR.rows_mismatch(near, case["hi"], np.zeros(0, dtype=np.int64), "hi") is None         # (no row in range: the two-row shape)


def test_one_wrong_partial_is_noticed():
    with np.errstate(invalid="ignore", over="ignore"):
        for case, mode, model in ((SR.build(300, 128, 64, SR.scene(300, 128, 2), seed=2), "gemm", partials_pairwise_from_values),
                                  (SR.build(421, 384, 64, SR.scene(421, 384, 2), seed=22, gemm=False), "mlp", partials_mlp_from_values)):
            part = in_range_only(case, model(case["X"]))
            assert SR.partials_mismatch(case, part, mode) is None
            ex, nr = np.flatnonzero(case["kind"] == SR.EXACT), np.flatnonzero(case["kind"] == SR.NEAR)
            assert len(ex) and len(nr)
            for m in (ex[0], ex[-1], nr[0]):
                for b in range(part.shape[0]):
                    for slot in (0, 1):
                        # one ulp - except in the one place with a bound instead of an equality (the fused kernel's +-NA block: the sum
                        # may be 3.75 off, the squares 3.75**2 / 64): there 32 ulps (8.0) of the sum, 2.0 in the squares
                        bit = (5, 30)[slot] if mode == "mlp" and case["near_block"][m, b] else 0
                        assert SR.partials_mismatch(case, flip(part, (b, m, slot), bit), mode) is not None, (mode, m, b, slot)
            bad = part.copy()
            bad[0, ex[0], 1] = np.nan
            assert SR.partials_mismatch(case, bad, mode) is not None
            # a NEAR block whose sum is the planes' (64 * 65 520) passes too (the 128-row kernel re-reads them), with squares of 0 only
            m = nr[0]
            b = int(np.flatnonzero(case["near_block"][m])[0])
            alt = part.copy()
            alt[b, m] = (np.sign(case["X"][m, 64 * b]) * 64 * 65520.0, 0.0)
            assert SR.partials_mismatch(case, alt, mode) is None
            alt[b, m, 1] = 1.0
            assert SR.partials_mismatch(case, alt, mode) is not None
            alt[b, m] = (np.sign(case["X"][m, 64 * b]) * 64 * 65504.0, 0.0)              # (hi alone: the lo plane forgotten)
            assert SR.partials_mismatch(case, alt, mode) is not None


def test_one_wrong_flag_or_statistics_row_of_the_next_step_is_noticed():
    case = SR.build(300, 128, 64, SR.scene(300, 128, 5), seed=5)
    M, nb = 300, 2
    part2 = np.ones((nb, M, 2), dtype=F32)
    for r, v, b, _ in case["placements"]:
        if abs(v) > SR.NA:
            part2[b, r] = np.nan
    stat = np.random.default_rng(0).standard_normal((M, 2)).astype(F32)
    dirty = stat.copy()
    dirty[case["sat_rows"]] = np.nan
    assert SR.next_step_mismatch(case, part2, 1, dirty, stat) is None
    assert "flag" in SR.next_step_mismatch(case, part2, 0, dirty, stat)
    ok = case["kind"] != SR.SATURATED
    leak = part2.copy()
    leak[1, np.flatnonzero(ok)[3], 0] = np.inf
    assert "non-finite" in SR.next_step_mismatch(case, leak, 1, dirty, stat)
    miss = part2.copy()
    miss[:, case["sat_rows"][0]] = 1.0
    assert "non-finite" in SR.next_step_mismatch(case, miss, 1, dirty, stat)
    assert "in-range row" in SR.next_step_mismatch(case, part2, 1, flip(dirty, (int(np.flatnonzero(ok)[-1]), 1)), stat)
    z = SR.zeroed(case)
    assert SR.next_step_mismatch(z, np.ones_like(part2), 0, stat, stat) is None
    assert "flag" in SR.next_step_mismatch(z, np.ones_like(part2), 1, stat, stat)


def test_the_layernorm_cases_hold_one_saturated_row_where_they_say():
    dropped = []
    for D in SR.LN_D:
        for i, row in enumerate(SR.LN_SAT_ROWS):
            case, r, drop = SR.ln_case(D, i)
            assert r == row and case["sat_rows"].tolist() == [row]
            dropped.append(drop)
            kept_in, kept_out = SR.ln_kept(SR.LN_ROWS, SR.LN_GROUP, SR.LN_SKIP)
            assert (row in kept_in) == (not drop) and len(kept_in) == 240 and kept_out.tolist() == list(range(240))
        assert SR.ln_in_range_case(D, 1)["sat_rows"].size == 0
        assert {v for k in SR.SCENES for _, v, _, _ in SR.ln_in_range_case(D, k)["placements"]} == set(SR.IN_RANGE)
    assert dropped.count(True) == 6 and dropped.count(False) == 4
    assert {SR.ln_case(128, i, s)[0]["placements"][-1][1] for i in range(5) for s in range(4)} == set(SR.SATURATING)
    r, o = SR.ln_kept(7, 0, 0)
    assert r.tolist() == o.tolist() == list(range(7))


# ---------------------------------------------------------------- where the planner sends the shapes
MI355X_CUS = 256


def plan(L, M, N, K, ncu=MI355X_CUS, m_plan=0):
    a = L.GemmArgs()
    a.M, a.N, a.K, a.lda, a.ldc, a.a_mode, a.epilogue = M, N, K, K, N, L.A_DENSE, L.EPI_SCALE_RES_SPLIT
    p = L.GemmPlan()
    assert L.lib.vda_gemm_plan(C.byref(a), m_plan, ncu, 0, C.byref(p)) == 0, L.lib.vda_last_error()
    return [p.rec[i] for i in range(p.n)]


@pytest.fixture()
def L():
    from video_depth_anything_amd import _lib
    yield _lib
    _lib.lib.vda_gemm_set_variant(-1)


def test_the_checked_tap_layernorm_is_bound_and_validates_before_any_launch(L):
    """vda_layernorm_split_check_f16 is vda_layernorm_split_f16 with the flag in front of the stream; the ABI version does not move
    (an addition), and bad arguments are refused before any HIP call."""
    plain, checked = L.SIGNATURES["vda_layernorm_split_f16"], L.SIGNATURES["vda_layernorm_split_check_f16"]
    assert checked == (plain[0], plain[1][:-1] + [C.c_void_p, plain[1][-1]]) and L.lib.vda_abi_version() == 8
    buf = (C.c_char * 4096)()
    p = C.cast(C.addressof(buf) + (-C.addressof(buf)) % 16, C.c_void_p)
    assert L.lib.vda_layernorm_split_check_f16(None, None, None, None, None, 1e-6, 4, 128, 0, 0, None, None) != 0
    assert b"vda_layernorm_split_check_f16: null pointer" in L.lib.vda_last_error()
    assert L.lib.vda_layernorm_split_check_f16(p, p, p, p, p, 1e-6, 4, 128, 0, 0, C.c_void_p(p.value + 2), None) != 0
    assert b"4-byte aligned" in L.lib.vda_last_error()
    assert L.lib.vda_layernorm_split_check_f16(p, p, p, p, p, 1e-6, 4, 132, 0, 0, None, None) != 0
    assert b"multiple of 8" in L.lib.vda_last_error()


def test_the_planner_sends_the_shapes_to_the_row_layout_families(L):
    """The statistics of the step that saturates are finite only in the row-layout families (256 / 192-row tiles): the kernel tests
    reach them by forcing a variant, the ViT-S forward by itself; tiny (D = 128 < 192) never does under automatic dispatch."""
    for M, N, K in SR.GEMM_SHAPES:
        for v, fam in SR.VARIANT_FAMILY.items():
            L.lib.vda_gemm_set_variant(v)
            recs = plan(L, M, N, K)
            assert [r.family for r in recs] == [fam], (M, N, K, v, L.launch_name(recs[0]))
    assert {L.FAM_256S, L.FAM_8P} <= set(SR.VARIANT_FAMILY.values()) and SR.VARIANT_FAMILY[-1] == L.FAM_128
    assert {SR.VARIANT_FAMILY[v] for v in SR.FORWARD_VARIANTS} == {L.FAM_128, L.FAM_256S, L.FAM_8P}
    L.lib.vda_gemm_set_variant(-1)
    rows = SR.VITS_FRAMES * SR.VITS_TOKENS
    for m, m_plan in ((rows, 0), (rows // 2, rows)):                   # the whole clip, and a frame half planned for the clip (enc_split)
        recs = plan(L, m, 384, 1536, m_plan=m_plan)
        assert len(recs) == 1 and recs[0].family == L.FAM_256S and (recs[0].bm, recs[0].bn) == (192, 384), L.launch_name(recs[0])
        assert plan(L, m, 384, 384, m_plan=m_plan)[0].family == L.FAM_256S
    for K in (128, 512):                                               # tiny's proj and fc2 at the forward tests' 39 token rows
        assert plan(L, 39, 128, K)[0].family == L.FAM_128
