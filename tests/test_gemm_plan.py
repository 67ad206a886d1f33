"""vda_gemm_plan: what vda_gemm_f16 runs, as a value computed without a GPU.

tests/golden/gemm_dispatch_parent.npz is the dispatch of the commit BEFORE the planner existed, recorded launch by launch
(profiles/r08/README.txt says how): the planner must reproduce every row. It is never regenerated from the planner."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest


@pytest.fixture(scope="module")
def L():
    from video_depth_anything_amd import _lib
    yield _lib
    _lib.lib.vda_gemm_set_variant(-1)
    _lib.lib.vda_gemm_set_debug(0)
    _lib.lib.vda_gemm_reload_tuning()


ARG_FIELDS = ("M", "N", "K", "lda", "ldc", "a_mode", "epilogue", "relu_in", "cB", "cH", "cW", "cCin", "cHo", "cWo", "cStride", "P", "tK", "tH", "tW", "tCout", "tile_rows")


def plan(L, ncu=256, m_plan=0, sched=False, sched_per_launch=0, **fields):
    """(rc, [records]) for a shape with NULL operands"""
    a = L.GemmArgs()
    for k, v in fields.items():
        setattr(a, k, v)
    if sched:
        a.sched = 64                 # "set": the planner never follows it
    p = L.GemmPlan()
    rc = L.lib.vda_gemm_plan(C.byref(a), m_plan, ncu, sched_per_launch, C.byref(p))
    return rc, [p.rec[i] for i in range(p.n)] if rc == 0 else []


def dense(M, N, K, epi, **kw):
    return dict(dict(M=M, N=N, K=K, lda=K, ldc=N, a_mode=0, epilogue=epi), **kw)


def parse_name(name):
    """kernel name -> (family, bm, bn, per_cu, ksched, dyn), the fields of a record it is made of"""
    kern, targs = re.fullmatch(r"(\w+)<(.*)>", name).groups()
    t = [s.strip() for s in targs.split(",")]
    if kern == "gemm_kernel":
        return (0, int(t[0]), int(t[1]), 1, 1, 0)
    if kern == "gemm256_kernel":
        return (1, 256, int(t[0]), 1, 1, 0)
    if kern == "gemm256s_kernel":
        return (2, int(t[3]), int(t[0]), int(t[4]), 1, 0)
    if kern == "gemm8p_kernel":
        return (3, int(t[4]), int(t[0]), 1, int(t[3]), int(t[5] == "true"))
    assert kern == "conv3x3_lds_kernel"
    return (4, 0, 32 * int(t[0]), 1, 1, 0)


def grid_of(r, N, ncu):
    tiles = -(-r.rows // r.bm) * -(-N // r.bn)
    if r.family == 0:
        return tiles
    return (tiles + 7) // 8 * 8 if tiles < r.per_cu * ncu else r.per_cu * ncu       # persistent workgroups


def test_planner_reproduces_the_recorded_dispatch_of_the_parent_commit(L, golden_dir, monkeypatch):
    """Every row of the table - model shapes of ViT-L / ViT-S / tiny forwards (whole clip and enc_split halves) and a sweep across every
    branch, variant and environment switch - gives the same launches: row ranges, kernel (family, tile, name), option word, tile_rows
    and grid. On the way: the records cover [0, M) exactly once in order, and every kernel planned is one its family is built for."""
    z = np.load(os.path.join(golden_dir, "gemm_dispatch_parent.npz"))
    cols = {c: i for i, c in enumerate(z["columns"].tolist())}
    names, envs, tab = z["names"].tolist(), [json.loads(e) for e in z["envs"].tolist()], z["table"].tolist()
    lib, emitted, env_now = L.lib, set(), None
    arg_idx = [cols[f] for f in ARG_FIELDS]
    assert len(tab) > 100000
    for row in tab:
        if row[cols["env"]] != env_now:
            env_now = row[cols["env"]]
            for k in [k for e in envs for k in e]:
                monkeypatch.delenv(k, raising=False)
            for k, v in envs[env_now].items():
                monkeypatch.setenv(k, v)
            lib.vda_gemm_reload_tuning()
        lib.vda_gemm_set_variant(row[cols["variant"]])
        lib.vda_gemm_set_debug(row[cols["debug"]])
        fields = {f: row[i] for f, i in zip(ARG_FIELDS, arg_idx)}
        rc, recs = plan(L, ncu=row[cols["ncu"]], m_plan=row[cols["m_plan"]], sched=bool(row[cols["sched"]]), **fields)
        what = {c: row[i] for c, i in cols.items() if i < cols["rc"]}
        assert (rc != 0) == (row[cols["rc"]] != 0), what
        assert len(recs) == row[cols["n"]], what
        at = 0
        for i, r in enumerate(recs):
            name = L.launch_name(r)
            want = names[row[cols[f"name_{i}"]]]
            assert (r.r0, r.rows, r.options, r.tile_rows, name) == (row[cols[f"r0_{i}"]], row[cols[f"rows_{i}"]], row[cols[f"options_{i}"]],
                                                                    row[cols[f"tile_rows_{i}"]], want), (what, i, name, want)
            assert (r.family, r.bm, r.bn, r.per_cu, r.ksched, r.dyn) == parse_name(want), (what, i)
            assert (r.a_mode, r.epilogue) == (fields["a_mode"], fields["epilogue"])
            if r.family != L.FAM_CONV_LDS:
                assert grid_of(r, fields["N"], row[cols["ncu"]]) == row[cols[f"grid_{i}"]], (what, i)
            assert r.r0 == at and r.rows > 0, what
            at += r.rows
            emitted.add((r.family, r.bm, r.bn, r.per_cu, r.a_mode, r.epilogue))
        assert rc != 0 or at == fields["M"], what
    # built pairs: the planner emitted nothing its family's table does not list, and the table has every family in it
    assert {e[0] for e in emitted} == {L.FAM_128, L.FAM_256, L.FAM_256S, L.FAM_8P, L.FAM_CONV_LDS}
    for e in sorted(emitted):
        assert lib.vda_gemm_built(*e) == 1, e


def test_built_tables(L):
    """The (family, tile, A mode, epilogue) sets as the families' own lists give them (gemm_epilogue.h), enumerated without a launch."""
    built = lambda fam, bm, bn, per_cu, mode: [e for e in range(13) if L.lib.vda_gemm_built(fam, bm, bn, per_cu, mode, e)]
    every, conv = list(range(13)), [L.EPI_BIAS_F16, L.EPI_BIAS_RELU_F16, L.EPI_RES_F16]
    for bn in (128, 256):
        assert built(L.FAM_8P, 256, bn, 1, 0) == every and built(L.FAM_256S, 256, bn, 1, 0) == every
        assert built(L.FAM_256, 256, bn, 1, 0) == list(range(10))
        for fam in (L.FAM_8P, L.FAM_256S, L.FAM_256):
            assert built(fam, 256, bn, 1, 1) == conv
    assert built(L.FAM_128, 128, 64, 1, 0) == every and built(L.FAM_128, 128, 128, 1, 1) == every
    assert built(L.FAM_8P, 192, 256, 1, 0) == [L.EPI_BIAS_F16, L.EPI_SCALE_RES_F32, L.EPI_SCALE_RES_SPLIT, L.EPI_LN_BIAS_F16]
    assert built(L.FAM_8P, 192, 256, 1, 1) == [] and built(L.FAM_8P, 192, 128, 1, 0) == []
    assert built(L.FAM_256S, 192, 128, 1, 0) == [0, 1, 3, 10, 11, 12] and built(L.FAM_256S, 192, 128, 2, 0) == [0, 1, 11, 12]
    assert built(L.FAM_256S, 192, 384, 1, 0) == [0, 3, 10, 11, 12] and built(L.FAM_256S, 192, 384, 1, 1) == []
    assert built(L.FAM_CONV_LDS, 0, 64, 1, 1) == conv and built(L.FAM_CONV_LDS, 0, 64, 1, 0) == []
    assert built(9, 256, 256, 1, 0) == []


@pytest.mark.parametrize("D,T,hw", [(1024, 32, 37 * 37), (1024, 5, 37 * 37), (1024, 32, 20 * 37), (384, 32, 37 * 37), (384, 33, 37 * 37), (384, 5, 20 * 37)])
@pytest.mark.parametrize("ncu", [256, 128, 8])
def test_enc_split_half_is_planned_as_the_whole_clip(L, monkeypatch, D, T, hw, ncu):
    """The bit-identity of enc_split rests on this: a frame half planned for the whole clip's rows (m_plan) gets the kernel, tile,
    workgroups per CU and option word of the whole-clip GEMM (its row split aside: a half is one launch)."""
    monkeypatch.setenv("VDA_GEMM_SPLIT", "0")
    L.lib.vda_gemm_reload_tuning()
    L.lib.vda_gemm_set_variant(-1)
    L.lib.vda_gemm_set_debug(0)
    rows = T * (hw + 1)
    gemms = [(3 * D, D, L.EPI_LN_BIAS_F16), (D, D, L.EPI_SCALE_RES_SPLIT), (4 * D, D, L.EPI_LN_GELU_F16), (D, 4 * D, L.EPI_SCALE_RES_SPLIT)]
    key = lambda r: (r.family, r.bm, r.bn, r.per_cu, r.ksched, r.dyn, r.options)
    whole = []
    for N, K, epi in gemms:
        rc, recs = plan(L, ncu=ncu, **dense(rows, N, K, epi))
        assert rc == 0 and len(recs) == 1
        whole.append(key(recs[0]))
    monkeypatch.delenv("VDA_GEMM_SPLIT")
    L.lib.vda_gemm_reload_tuning()
    for (N, K, epi), want in zip(gemms, whole):
        for nf in {T // 2, T - T // 2}:
            rc, recs = plan(L, ncu=ncu, m_plan=rows, sched_per_launch=1, **dense(nf * (hw + 1), N, K, epi))
            assert rc == 0 and len(recs) == 1, "a half is never row-split"
            assert key(recs[0]) == want, (N, K, epi, nf)


def test_planner_needs_no_operands_and_no_gpu(L):
    """NULL operands plan (the forward's sizing pass plans with them); vda_gemm_f16 still refuses them before any HIP call. Nothing
    here needs a device: ncu is given (ncu = 0 asks the current device and falls back to 8 CUs without one)."""
    L.lib.vda_gemm_set_variant(-1)
    rc, recs = plan(L, ncu=256, **dense(43840, 1024, 4096, L.EPI_SCALE_RES_SPLIT))
    assert rc == 0 and [(r.r0, r.rows, r.bm) for r in recs] == [(0, 31744, 256), (31744, 12096, 192)]
    rc, one = plan(L, ncu=256, sched=True, **dense(43840, 1024, 4096, L.EPI_SCALE_RES_SPLIT))
    assert rc == 0 and len(one) == 1 and one[0].dyn == 1, "one block of sched counters is one launch"
    rc, two = plan(L, ncu=256, sched=True, sched_per_launch=1, **dense(43840, 1024, 4096, L.EPI_SCALE_RES_SPLIT))
    assert rc == 0 and len(two) == 2 and L.launch_name(two[1]) == "gemm8p_kernel<256, 0, 10, 1, 192, true>"
    a = L.GemmArgs()
    assert L.lib.vda_gemm_plan(C.byref(a), 0, 256, 0, C.byref(L.GemmPlan())) != 0 and b"empty problem" in L.lib.vda_last_error()
    assert L.lib.vda_gemm_plan(None, 0, 256, 0, None) != 0
    a = L.GemmArgs(**dense(300, 192, 128, L.EPI_BIAS_F16))
    assert L.lib.vda_gemm_f16(C.byref(a), None) != 0 and b"null operand" in L.lib.vda_last_error()


# ---------------------------------------------------------------- what the exact-integer fp16 edge tests run
# A forced variant whose family has no instantiation for the epilogue (pick fails in plan_one) plans the 128-row kernel instead, silently.
# With dense A: the 32x32x16-MFMA family (variants 1, 2) and the split-residual / LayerNorm-folded epilogues. With conv A: none - every
# large-tile family is built for the three conv epilogues (BIAS_F16, BIAS_RELU_F16, RES_F16), the only ones the edge tests run on conv A.
FALLBACK_128 = {(v, 0, e) for v in (1, 2) for e in (10, 11, 12)}        # (variant, A mode, epilogue)
# Pairs a forced tile shape is not built for, which plan_one moves to ANOTHER large tile (never to the 128-row kernel): variant 8
# (192 x 128) / 10 (192 x 384) / 11 (192 x 128 twice per CU) -> 256 x 128 of the same family, 5 + 16 * 64 (192 x 256) -> 256 x 256 8-phase.
BUILT_192 = {8: (2, 192, 128, 1), 10: (2, 192, 384, 1), 11: (2, 192, 128, 2), 5 + 16 * 64: (3, 192, 256, 1)}


def test_edge_tests_reach_every_built_kernel(L):
    """tests/test_kernels_f16_edges_gpu.py asserts after every launch that the kernel that ran is the one vda_gemm_plan names; this is
    the other half: over the launches of that file (tests/_exact.py: f16_launches, planned for 256 CUs) the planned kernels contain
    EVERY (family, tile, workgroups per CU) that vda_gemm_built lists, for dense and for conv A - no built instantiation is beyond
    vda_gemm_set_variant's reach. Refusals and fall-backs are the tabulated ones and no others."""
    import _exact as E
    lib = L.lib
    lib.vda_gemm_set_debug(0)
    built = {(fam, bm, bn, pc, mode) for fam in range(5) for bm in (0, 128, 192, 256) for bn in (32, 64, 128, 256, 384) for pc in (1, 2) for mode in (0, 1)
             if any(lib.vda_gemm_built(fam, bm, bn, pc, mode, e) for e in range(13))}
    assert len(built) == 22, sorted(built)
    reached, fell_back, n, splits = set(), set(), 0, 0
    for v, sched, f in E.f16_launches(256):
        lib.vda_gemm_set_variant(v)
        rc, recs = E.plan16(L, f, ncu=256, sched=sched)
        n += 1
        odd = f["N"] % 8 != 0 or f["ldc"] % 8 != 0
        if odd and v not in E.NO_LARGE_TILE:                 # a refusal plan_one documents: the large tiles own 8-column row segments
            assert rc != 0 and b"multiples of 8" in lib.vda_last_error(), (v, f)
            continue
        assert rc == 0, (v, f, lib.vda_last_error())
        assert sum(r.rows for r in recs) == f["M"]
        splits += len(recs) == 2
        for r in recs:
            key = (r.family, r.bm, r.bn, r.per_cu, r.a_mode)
            assert lib.vda_gemm_built(*key, r.epilogue) == 1, (v, f)
            reached.add(key)
            if v in (0, 7) and not (v == 7 and r.family == L.FAM_CONV_LDS):
                assert r.family == L.FAM_128
            elif v > 0:
                fb = (v, r.a_mode, r.epilogue) in FALLBACK_128
                assert (r.family == L.FAM_128) == fb, (v, f, L.launch_name(r))
                fell_back.add((v, r.a_mode, r.epilogue)) if fb else None
                if v in BUILT_192 and r.a_mode == 0 and not fb:
                    want = BUILT_192[v]
                    is192 = lib.vda_gemm_built(*want, 0, r.epilogue) == 1 and (v != 10 or f["N"] % 384 == 0)
                    assert (key[:4] == want) == is192, (v, f, L.launch_name(r))
            if r.dyn:
                assert sched and r.family == L.FAM_8P
    lib.vda_gemm_set_variant(-1)
    assert n > 2000 and splits == 1, "the row-split case splits, nothing else does"
    assert fell_back == FALLBACK_128, "every tabulated fall-back is exercised"
    assert reached == built, f"built but never planned: {sorted(built - reached)}; planned but not built: {sorted(reached - built)}"
    for e in range(13):                                       # conv A: the three epilogues of E.CONV16_EPIS are what every conv family is built for
        for fam, bm, bn in ((1, 256, 256), (2, 256, 128), (3, 256, 256), (3, 256, 128), (4, 0, 32), (4, 0, 64)):
            assert lib.vda_gemm_built(fam, bm, bn, 1, 1, e) == (e in {E.EPI[E.EPI_OF[x]] for x in E.CONV16_EPIS})


# ---------------------------------------------------------------- launch obeys plan (GPU)
# (family, bm, bn, A mode, forced variant that names the family, tile_rows)
TARGETS = [(0, 128, 64, 0, 0, 0), (0, 128, 128, 0, 0, 0), (0, 128, 128, 1, 0, 0), (2, 256, 128, 0, 4, 0), (2, 192, 128, 0, 8, 0), (2, 192, 384, 0, 10, 0),
           (2, 256, 128, 1, 4, 0), (3, 256, 256, 0, 5, 0), (3, 192, 256, 0, 5 + 16 * 64, 192), (3, 256, 256, 1, 5, 0), (4, 0, 32, 1, 7, 0), (4, 0, 64, 1, 7, 0)]


@pytest.mark.gpu
def test_launch_obeys_plan():
    """One shape per kernel family and tile the automatic path reaches: vda_gemm_f16 runs the planned kernel (its name is the plan's),
    the result is bit-identical under the forced variant that names that family and agrees with the 128-row kernel within
    test_gemm_bias's tolerance. Shapes: the smallest M (N <= 384, K = 64, or 1024 where 64 cannot reach the family) the planner picks
    the family for on 8 CUs (vda_set_max_wgs(8) keeps the grids and the shapes small), or on the whole device where 8 CUs never pick it."""
    import torch
    from video_depth_anything_amd import _lib as L, ops
    from test_kernels_gpu import close, dev, rnd
    lib = L.lib
    lib.vda_gemm_set_variant(-1)
    try:
        for fam, bm, bn, mode, variant, tile_rows in TARGETS:
            found = None
            lib.vda_gemm_set_variant(-1)               # (the launches of the previous target end under variant 0)
            # (8 CUs first; the whole device for what 8 CUs never pick: 192 x 128 tiles need equal round counts of both tilings)
            for cap, K, M0, N in ((cap, K, M0, N) for cap, Ms in ((8, [1, 100] + list(range(2048, 6145, 64))), (0, range(2048, 45057, 256)))
                                  for K in (64, 1024) for M0 in Ms for N in (32, 64, 128, 192, 256, 384)):
                lib.vda_set_max_wgs(cap)
                if mode == 0:
                    f, geo = dense(M0 + (M0 > 100), N, K, L.EPI_BIAS_F16, tile_rows=tile_rows), None
                else:
                    Cin, B = K if K == 64 else 128, max(1, -(-M0 // 361))
                    geo = (B, 19, 19, Cin, 19, 19, 1)
                    f = dict(M=B * 361, N=N, K=9 * Cin, lda=0, ldc=N, a_mode=1, epilogue=L.EPI_BIAS_F16, cB=B, cH=19, cW=19, cCin=Cin, cHo=19, cWo=19, cStride=1)
                rc, recs = plan(L, ncu=0, **f)
                if rc == 0 and len(recs) == 1 and (recs[0].family, recs[0].bm, recs[0].bn) == (fam, bm, bn):
                    found = (f, geo, recs[0])
                    break
            assert found, f"the planner reaches (family {fam}, {bm} x {bn}, A mode {mode}) for no candidate shape"
            f, geo, rec = found
            M, N, K = f["M"], f["N"], f["K"]
            A = dev((rnd(M, K, seed=1) if geo is None else rnd(geo[0], 19, 19, geo[3], seed=1)).to(torch.float16))
            W, b = dev(rnd(N, K, seed=2, scale=K ** -0.5).to(torch.float16)), dev(rnd(N, seed=3))
            outs = []
            for v in (-1, variant, 0):
                lib.vda_gemm_set_variant(v)
                out = torch.full((M, N), float("nan"), dtype=torch.float16, device="cuda")
                ops.gemm(A, W, out, L.EPI_BIAS_F16, M=M, N=N, K=K, bias=b, conv=geo, tile_rows=tile_rows)
                got = lib.vda_gemm_last_kernel().decode()
                if v != 0:
                    assert (parse_name(got)[:3]) == (fam, bm, bn), (v, got)
                if v == -1:
                    assert got == L.launch_name(rec), "vda_gemm_f16 launched what vda_gemm_plan planned"
                outs.append(out)
            assert torch.equal(outs[0], outs[1]), f"{L.launch_name(rec)}: differs from variant {variant}"
            close(outs[0], outs[2].float().cpu(), what=f"{L.launch_name(rec)} against the 128-row kernel")
    finally:
        lib.vda_gemm_set_variant(-1)
        lib.vda_set_max_wgs(0)
