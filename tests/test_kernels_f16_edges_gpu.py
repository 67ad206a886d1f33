"""The fp16 GEMM's five kernel families at their tile edges.

Everything LINEAR in vda_gemm_f16 (dense and implicit-3x3 A; the bias / ReLU / residual / LayerScale / split-residual / LayerNorm-folded /
patch-embed / ConvTranspose epilogues) is checked with small integer operands against an fp64 reference by torch.equal, under every
vda_gemm_set_variant value. Two conditions make that reference the only admissible result (tests/_exact.py: assert_exact_safe_f16,
asserted for every case here; shown sufficient - and the equalities shown able to fail - on the CPU in tests/test_exact_inputs.py):
every partial sum stays below 2**24, and everything stored or re-read as fp16 is an fp16 value. A wrong row, tap, pad, column, K step
or tile is then an inequality, not a judgement about 2e-3.

Every output is a buffer filled with one NaN bit pattern with a margin of rows behind and, where ldc > N, columns beside the region the
kernel owns (check_sentinel: nothing outside may change, nothing inside may be left). Every input is a view of a larger NaN-filled
allocation (guarded): a clamp or a bound that is off by one puts a NaN into the output. After every launch the kernel that ran
(vda_gemm_last_kernel) must be the one vda_gemm_plan names for the call: tests/test_gemm_plan.py shows on the CPU that these launches
reach every built (family, tile, workgroups per CU), so "under variant v" cannot silently mean a second run of the 128-row kernel.

GELU, GEGLU and LayerNorm+GELU are real-valued: randn operands, fp64 reference, tests/test_kernels_gpu.py's tolerances.

Tile seams (the last part of the file). On a 256-CU device the cases above give a persistent workgroup one tile, and the tile walks
two, at one K step. What a workgroup carries from one tile into the next - K tile 0 issued before the previous epilogue, K tile 1
landing in the A slot that epilogue staged through, the bias and (mean, rstd) fragments fetched a tile ahead, set_sources and
TapCursor::seek under conv A, the rotation of the folded mode, the dealt last round and the stagger of the workgroups that sit it out,
the drawn tile index - is run under vda_set_max_wgs(8) or (16) (capped), where a few thousand rows are two full rounds and a partial
third: every large tile in the walk's three modes at five and nine K steps with every epilogue it is built for, statically and with the
dynamic draw; conv A, the patch-embed and ConvTranspose row maps, the folded mode, the C = 64 LDS convolution; the L2-blocked order
(uncapped) at five K steps. Each such launch asserts from its plan record that the tiles exceed two rounds of the capped grid."""
import contextlib
import functools
import re

import pytest
import torch
import torch.nn.functional as F

import _convt_fold_ref as R
import _exact as E
from _exact import check_sentinel, guarded, pad_cols, sentinel_out, sentinel_out_f16
from test_kernels_gpu import close, gemm_variant, ops, rnd  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

F16, F32, F64 = torch.float16, torch.float32, torch.float64
NAN = float("nan")


@pytest.fixture(scope="module")
def L(ops):
    from video_depth_anything_amd import _lib
    yield _lib
    _lib.lib.vda_gemm_set_variant(-1)
    _lib.lib.vda_conv_lds_set_variant(0)
    _lib.lib.vda_depth_tail_set_variant(0)
    _lib.lib.vda_set_max_wgs(0)


@contextlib.contextmanager
def capped(L, n):
    """vda_set_max_wgs(n) for the block: every persistent grid launched inside is sized as for n CUs (n workgroups, 2 n for the kernel with
    two workgroups per CU) and vda_gemm_plan plans for them; 0 again on every way out."""
    L.lib.vda_set_max_wgs(n)
    try:
        yield
    finally:
        L.lib.vda_set_max_wgs(0)


def assert_seam(L, recs, M, N, cap):
    """From the plan record: a large tile, and more tiles than two rounds of the capped grid - some workgroup runs a third tile."""
    r = recs[0]
    assert len(recs) == 1 and r.family not in (L.FAM_128, L.FAM_CONV_LDS), f"{L.launch_name(r)}: no persistent large-tile kernel, the case covers nothing"
    tiles = -(-M // r.bm) * -(-N // r.bn)
    assert tiles > 2 * r.per_cu * cap, f"{L.launch_name(r)}: {tiles} tiles on {r.per_cu * cap} workgroups are no three rounds, the case covers nothing"
    return r


def exact(y, ref, what):
    y = y.detach().cpu()
    assert ref.dtype == F64 and y.shape == ref.shape, what
    if not torch.equal(y.double(), ref):
        bad = (y.double() != ref) | y.isnan()
        first = bad.nonzero()[0].tolist()
        rows = bad.reshape(bad.shape[0], -1).any(1).nonzero().flatten().tolist()
        cols = bad.reshape(-1, bad.shape[-1]).any(0).nonzero().flatten().tolist()
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} elements differ from the exact result ({int(y.isnan().sum())} NaN), first at {first}: "
                             f"{float(y[tuple(first)])} != {float(ref[tuple(first)])}; leading index {rows[:4]}..{rows[-1]}, last index {cols[:4]}..{cols[-1]}")


def close_finite(y, ref, what, **tol):
    """close() lets a NaN pass (NaN > bound is False): a leaked guard or pad must fail here too."""
    bad = ~torch.isfinite(y.float())
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} non-finite outputs, first at {bad.nonzero()[0].tolist()}"
    close(y, ref, what=what, **tol)


def launch(ops, L, A, W, out, epi, sched=None, **kw):
    """ops.gemm + the assertion that makes the planner's coverage table true on the device: the kernel that ran is the planned one."""
    tensors = {k: kw.pop(k) for k in ("bias", "res", "res2", "gamma", "pos", "out2", "stats") if k in kw}
    rc, recs = E.plan16(L, E.gemm16_fields(epi=epi, **kw), ncu=0, sched=sched is not None)
    assert rc == 0, L.lib.vda_last_error()
    ops.gemm(A, W, out, epi, sched=sched, **tensors, **kw)
    got = L.lib.vda_gemm_last_kernel().decode()
    assert got == L.launch_name(recs[-1]), f"ran {got}, planned {L.launch_name(recs[-1])}"
    return recs


def refused(L, variant, N, ldc):
    return variant not in E.NO_LARGE_TILE and (N % 8 != 0 or ldc % 8 != 0)


def h16(t):
    assert torch.equal(t.to(F16).to(t.dtype), t)
    return t.to(F16)


# ---------------------------------------------------------------- dense A, exact
@functools.lru_cache(maxsize=None)
def dense_data(case):
    """(fp64 references, guarded device operands) of one case, shared by the thirteen variants."""
    M, N, K, lda, ldc = case
    inp = E.dense16_inputs(case)
    ref = E.dense16_check(inp)
    d = {k: v.double() for k, v in inp.items()}
    Wf, c1, c2 = E.fold_ln(d)
    g = dict(A=guarded(pad_cols(inp["A"], lda, F16)), W=guarded(h16(inp["W"])), bias=guarded(inp["bias"]), gamma=guarded(inp["gamma"]),
             res32=guarded(pad_cols(inp["res"], ldc, F32)), res16=guarded(pad_cols(inp["res"], ldc, F16)), res2_16=guarded(pad_cols(inp["res2"], ldc, F16)),
             stats=guarded(torch.stack((inp["mean"], inp["rstd"]), dim=1).contiguous()), Wf=guarded(h16(Wf.float())), c1=guarded(c1.float()), c2=guarded(c2.float()))
    return inp, ref, g


def test_fold_ln_weight_exact(ops):
    """Wf, c1 and c2 of the LayerNorm-folded epilogue's operands, from vda_fold_ln_weight on integer W, ln_w, ln_b: equal to the definition."""
    for case in E.DENSE16_CASES:
        M, N, K, lda, ldc = case
        inp = E.dense16_inputs(case)
        Wf, c1, c2 = sentinel_out_f16(N, K, K), sentinel_out(1, N, N), sentinel_out(1, N, N)
        ops.fold_ln_weight(guarded(inp["W"]), guarded(inp["bias"]), guarded(inp["ln_w"]), guarded(inp["ln_b"]), Wf, c1, c2, N, K)
        for buf, rows, cols in ((Wf, N, K), (c1, 1, N), (c2, 1, N)):
            check_sentinel(buf, rows, cols, f"fold_ln_weight {E.dense_id(case)}")
        rWf, rc1, rc2 = E.fold_ln({k: v.double() for k, v in inp.items()})
        exact(Wf[:N], rWf, "Wf"), exact(c1[0], rc1, "c1"), exact(c2[0], rc2, "c2")


def run_dense_exact(ops, L, case, epi, g, ref, sched=None):
    """One exact epilogue of one dense case under the current variant: sentinel, kernel name, equality. Returns the plan's records."""
    M, N, K, lda, ldc = case
    kw = dict(M=M, N=N, K=K, lda=lda, ldc=ldc)
    what = f"gemm_f16 {E.dense_id(case)} {epi}"
    e = getattr(L, "EPI_" + E.EPI_OF[epi])
    out = (sentinel_out if epi in E.DENSE16_F32_OUT else sentinel_out_f16)(M, N, ldc)
    if epi in ("bias_f16", "bias_f32", "bias_relu"):
        recs = launch(ops, L, g["A"], g["W"], out, e, bias=g["bias"], sched=sched, **kw)
    elif epi == "bias_f16_no_bias":
        recs = launch(ops, L, g["A"], g["W"], out, e, sched=sched, **kw)
    elif epi == "scale_res_in_place_gamma":
        out[:M, :N] = g["res32"][:, :N]
        recs = launch(ops, L, g["A"], g["W"], out, e, bias=g["bias"], gamma=g["gamma"], res=out, sched=sched, **kw)
    elif epi == "scale_res_h_separate_out":
        recs = launch(ops, L, g["A"], g["W"], out, e, bias=g["bias"], res=g["res32"], sched=sched, **kw)
    elif epi == "res":
        recs = launch(ops, L, g["A"], g["W"], out, e, bias=g["bias"], res=g["res16"], sched=sched, **kw)
    elif epi == "res_res2":
        recs = launch(ops, L, g["A"], g["W"], out, e, bias=g["bias"], res=g["res16"], res2=g["res2_16"], sched=sched, **kw)
    elif epi == "ln_bias":
        recs = launch(ops, L, g["A"], g["Wf"], out, e, bias=g["c2"], gamma=g["c1"], stats=g["stats"], sched=sched, **kw)
    else:
        # in place over the two planes; partial statistics [N / 64, M, 2] in a sentinel buffer of their own
        lo, part = sentinel_out_f16(M, N, ldc), sentinel_out(N // 64 * M, 2, 2)
        out[:M, :N], lo[:M, :N] = g["res16"][:, :N], g["res2_16"][:, :N]
        pos = dict(pos=g["stats"]) if epi == "split_pos" else {}
        recs = launch(ops, L, g["A"], g["W"], out, e, bias=g["bias"], gamma=g["gamma"], res=out, res2=lo, out2=lo, stats=part, **pos, sched=sched, **kw)
        check_sentinel(lo, M, N, what + " lo plane"), check_sentinel(part, N // 64 * M, 2, what + " partial statistics")
        assert bool((lo[:M, :N] == 0).all()), f"{what}: the stream is an fp16 value everywhere, so the lo plane is exactly 0"
        p = part[:N // 64 * M].view(N // 64, M, 2)
        exact(p[:, :, 0].t(), ref[epi].reshape(M, N // 64, 64).sum(-1), what + " partial sums")
        stat = torch.empty(M, 2, device="cuda")
        ops.ln_stats_finalize(p.contiguous(), stat, 1e-6, M, N // 64)
        close_finite(stat[:, 0], ref[epi].mean(1), what + " mean", rtol=1e-5, atol=1e-5)
        close_finite(stat[:, 1], (ref[epi].var(1, unbiased=False) + 1e-6).rsqrt(), what + " rstd", rtol=1e-4, atol=0)
    check_sentinel(out, M, N, what)
    exact(out[:M, :N], ref[epi], what)
    return recs


@pytest.mark.parametrize("case", E.DENSE16_CASES, ids=E.dense_id)
def test_gemm_f16_dense_exact(ops, L, gemm_variant, case):
    """Every exact epilogue of the case under the variant (the epilogues share the operands; a failure names its epilogue)."""
    assert gemm_variant in E.VARIANTS16, "a new variant: add it to tests/_exact.py so that the planner coverage test sees its launches"
    M, N, K, lda, ldc = case
    inp, ref, g = dense_data(case)
    if refused(L, gemm_variant, N, ldc):
        out = sentinel_out_f16(M, N, ldc)
        with pytest.raises(L.VdaError, match=re.escape("the 256-row kernel needs N and ldc to be multiples of 8")):
            ops.gemm(g["A"], g["W"], out, L.EPI_BIAS_F16, M=M, N=N, K=K, lda=lda, ldc=ldc, bias=g["bias"])
        torch.cuda.synchronize()
        assert bool((out.view(torch.int16) == E.SENTINEL16_BITS).all()), "a refused call wrote to its output"
        return
    for epi in E.dense16_epis(case):
        if epi in E.DENSE16_EXACT:
            run_dense_exact(ops, L, case, epi, g, ref)


# ---------------------------------------------------------------- dense A, real-valued epilogues
@functools.lru_cache(maxsize=None)
def real_data(case):
    M, N, K, lda, ldc = case
    A, W, b = rnd(M, K, seed=700).to(F16), rnd(N, K, seed=701, scale=K ** -0.5).to(F16), rnd(N, seed=702)
    stats = torch.stack((rnd(M, seed=703) * 0.1, 1.0 + rnd(M, seed=704).abs()), dim=1).contiguous()
    c1 = rnd(N, seed=705)
    Ad, Wd = A.double(), W.double()
    lin = Ad @ Wd.t()
    ref = dict(gelu=F.gelu(lin + b.double()), ln_gelu=F.gelu(stats[:, 1:].double() * (lin - stats[:, :1].double() * c1.double()) + b.double()))
    g = dict(A=guarded(pad_cols(A, lda, F16)), W=guarded(W), bias=guarded(b), stats=guarded(stats), c1=guarded(c1))
    if N % 32 == 0:
        from video_depth_anything_amd import ops as o
        wi, bi = o.pack_geglu(W.float(), b)          # W's rows read as [value (N / 2) | gate (N / 2)]
        val, gate = (lin + b.double()).chunk(2, dim=-1)
        ref["geglu"] = val * F.gelu(gate)
        g.update(Wi=guarded(wi), bi=guarded(bi))
    return ref, g


def run_dense_real(ops, L, case, epi, ref, g, sched=None):
    """One real-valued epilogue of one dense case under the current variant, at tests/test_kernels_gpu.py's tolerances. Returns the plan's records."""
    M, N, K, lda, ldc = case
    kw = dict(M=M, N=N, K=K, lda=lda, sched=sched)
    what = f"gemm_f16 {E.dense_id(case)} {epi}"
    if epi == "gelu":
        out = sentinel_out_f16(M, N, ldc)
        recs = launch(ops, L, g["A"], g["W"], out, L.EPI_BIAS_GELU_F16, bias=g["bias"], ldc=ldc, **kw)
        check_sentinel(out, M, N, what)
        close_finite(out[:M, :N], ref[epi], what)
    elif epi == "ln_gelu":
        out = sentinel_out_f16(M, N, ldc)
        recs = launch(ops, L, g["A"], g["W"], out, L.EPI_LN_GELU_F16, bias=g["bias"], gamma=g["c1"], stats=g["stats"], ldc=ldc, **kw)
        check_sentinel(out, M, N, what)
        close_finite(out[:M, :N], ref[epi], what, rtol=3e-3, atol=6e-3)
    else:
        assert epi == "geglu"
        out = sentinel_out_f16(M, N // 2, N // 2)
        recs = launch(ops, L, g["A"], g["Wi"], out, L.EPI_GEGLU_F16, bias=g["bi"], ldc=N // 2, **kw)
        check_sentinel(out, M, N // 2, what)
        close_finite(out[:M], ref[epi], what)
    return recs


@pytest.mark.parametrize("case", E.DENSE16_CASES, ids=E.dense_id)
def test_gemm_f16_dense_real_valued(ops, L, gemm_variant, case):
    M, N, K, lda, ldc = case
    if refused(L, gemm_variant, N, ldc):
        return                                       # (the refusal itself: test_gemm_f16_dense_exact)
    ref, g = real_data(case)
    for epi in E.dense16_epis(case):
        if epi in E.DENSE16_REAL:
            run_dense_real(ops, L, case, epi, ref, g)


def test_gemm_f16_rows_are_position_independent(ops, L, gemm_variant):
    """One A row at rows 0, 127, 128, 191, 192, 255 and 256 of a 257-row problem - first and last row of every tile height, the lone row
    of a last tile - gives bit-identical output rows: a row's K order and epilogue do not depend on its place in a tile."""
    M, N, K = E.ROWPOS16["M"], E.ROWPOS16["N"], E.ROWPOS16["K"]
    A = rnd(M, K, seed=710).to(F16)
    A[E.ROWPOS16_ROWS] = A[0].clone()
    A, W, b = guarded(A), guarded(rnd(N, K, seed=711, scale=K ** -0.5).to(F16)), guarded(rnd(N, seed=712))
    for epi in (L.EPI_BIAS_F16, L.EPI_BIAS_GELU_F16):
        out = sentinel_out_f16(M, N, N)
        launch(ops, L, A, W, out, epi, bias=b, **E.ROWPOS16)
        check_sentinel(out, M, N, f"epilogue {epi}")
        bits = out.view(torch.int16)
        for r in E.ROWPOS16_ROWS[1:]:
            assert torch.equal(bits[r], bits[0]), f"epilogue {epi}: row {r} differs from row 0 in {int((bits[r] != bits[0]).sum())} columns"


# ---------------------------------------------------------------- broadcast row, tile walks, row split
@pytest.mark.parametrize("case", E.BROADCAST16_CASES, ids=lambda c: "M%d-N%d-K%d" % c)
def test_gemm_f16_broadcast_row_exact(ops, L, gemm_variant, case):
    """lda == 0: A is ONE row (eight NaN rows behind it), every output row is its result."""
    M, N, K = case
    inp = E.walk16_inputs(case)
    row = inp["A"][:1]
    lin = (row.double() @ inp["W"].double().t() + inp["bias"].double()).expand(M, N)
    res = E.ints((M, N), -4, 4, 5990)
    E.assert_exact_safe_f16([row.double().abs() @ inp["W"].double().abs().t() + inp["bias"].double().abs() + 4], [lin])
    A, W, b = guarded(h16(row)), guarded(h16(inp["W"])), guarded(inp["bias"])
    out = sentinel_out_f16(M, N, N)
    launch(ops, L, A, W, out, L.EPI_BIAS_F16, M=M, N=N, K=K, lda=0, bias=b)
    check_sentinel(out, M, N, "broadcast row")
    exact(out[:M], lin, "broadcast row, BIAS_F16")
    x = sentinel_out(M, N, N)
    x[:M] = res.cuda()
    launch(ops, L, A, W, x, L.EPI_SCALE_RES_F32, M=M, N=N, K=K, lda=0, bias=b, res=x)
    check_sentinel(x, M, N, "broadcast row")
    exact(x[:M], lin + res.double(), "broadcast row, SCALE_RES_F32")


@functools.lru_cache(maxsize=None)
def walk_data(case):
    inp = E.walk16_inputs(case)
    d = {k: v.double() for k, v in inp.items()}
    lin = d["A"] @ d["W"].t() + d["bias"]
    E.assert_exact_safe_f16([d["A"].abs() @ d["W"].abs().t() + d["bias"].abs()], [lin])
    return lin, guarded(h16(inp["A"])), guarded(h16(inp["W"])), guarded(inp["bias"])


# (the dynamic draw once per width under each kernel that has it, as tests/_exact.py's f16_launches lists them)
WALKS = [(N, v, dyn) for N in E.WALK16_N for v in E.WALK16_VARIANTS for dyn in (False, True) if not dyn or v in (-1, 5 + 16 * 64)]


@pytest.mark.parametrize("N,variant,dyn", WALKS, ids=lambda x: {True: "dynamic_draw", False: "static"}[x] if isinstance(x, bool) else str(x))
def test_gemm_f16_tile_walk_exact(ops, L, N, variant, dyn):
    """More tiles than persistent workgroups by a few (M from the CU count): one full round and a short last one, in each of the walk's
    three modes, and with the tiles drawn dynamically (args.sched: eight zeroed counters). Every tile lands where it belongs."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    case = E.walk16_case(ncu & ~7, N)
    M, N, K = case
    lin, A, W, b = walk_data(case)
    L.lib.vda_gemm_set_variant(variant)
    try:
        out = sentinel_out_f16(M, N, N)
        sched = torch.zeros(8, dtype=torch.int32, device="cuda") if dyn else None
        recs = launch(ops, L, A, W, out, L.EPI_BIAS_F16, sched=sched, M=M, N=N, K=K, bias=b)
    finally:
        L.lib.vda_gemm_set_variant(-1)
    r = recs[0]
    assert len(recs) == 1 and r.family != L.FAM_128 and -(-M // r.bm) * -(-N // r.bn) > r.per_cu * (ncu & ~7), "more tiles than workgroups"
    assert r.dyn == int(dyn)
    if dyn:
        assert int(sched.sum()) > 0, "no tile was drawn from the counters"
    check_sentinel(out, M, N, f"walk N={N} variant {variant}")
    exact(out[:M], lin, f"walk M={M} N={N} variant {variant} dyn={dyn} ({L.launch_name(r)})")


def test_gemm_f16_row_split_exact(ops, L):
    """A shape the automatic path row-splits (asserted: two records): whole rounds of 256-row tiles + the rest on 192-row tiles. Exact on
    sampled rows - every 61st, those either side of the split and the last - since the fp64 product of all of it is minutes of CPU."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    case = E.split16_case(ncu & ~7)
    M, N, K = case
    L.lib.vda_gemm_set_variant(-1)
    rc, recs = E.plan16(L, E.gemm16_fields(M, N, K, L.EPI_BIAS_F16))
    assert rc == 0 and len(recs) == 2 and (recs[0].bm, recs[1].bm) == (256, 192), "the planner no longer splits this shape: the case covers nothing"
    m1 = recs[1].r0
    inp = E.walk16_inputs(case)
    rows = torch.cat((torch.arange(0, M, 61), torch.arange(m1 - 3, m1 + 3), torch.arange(M - 3, M))).unique()
    d = dict(A=inp["A"][rows].double(), W=inp["W"].double(), bias=inp["bias"].double())
    lin = d["A"] @ d["W"].t() + d["bias"]
    E.assert_exact_safe_f16([d["A"].abs() @ d["W"].abs().t() + d["bias"].abs()], [lin])
    out = sentinel_out_f16(M, N, N)
    got = launch(ops, L, guarded(h16(inp["A"])), guarded(h16(inp["W"])), out, L.EPI_BIAS_F16, M=M, N=N, K=K, bias=guarded(inp["bias"]))
    assert len(got) == 2
    check_sentinel(out, M, N, "row split")
    exact(out[rows.cuda()], lin, f"row split at {m1} of {M}")


# ---------------------------------------------------------------- patch embed / ConvTranspose epilogues, exact
@pytest.mark.parametrize("case", E.PATCH16_CASES, ids=lambda c: "fr%d-P%d-N%d-K%d-ldc%d" % c)
def test_gemm_f16_patch_epilogue_exact(ops, L, gemm_variant, case):
    run_patch_exact(ops, L, case)


def run_patch_exact(ops, L, case):
    fr, P, N, K, ldc = case
    inp = E.patch16_inputs(case)
    d, a = {k: v.double() for k, v in inp.items()}, {k: v.double().abs() for k, v in inp.items()}
    E.assert_exact_safe(E.patch16_ref(a, P))
    tok = sentinel_out(fr * (P + 1), N, ldc)
    recs = launch(ops, L, guarded(h16(inp["A"])), guarded(h16(inp["W"])), tok, L.EPI_PATCH_F32, bias=guarded(inp["bias"]), pos=guarded(inp["pos"]), **E.patch16_kw(case))
    bits = tok.view(torch.int32)[:fr * (P + 1)].reshape(fr, P + 1, ldc)
    assert bool((bits[:, 0] == E.SENTINEL_BITS).all()), "the epilogue must leave every frame's cls row alone"
    tok.view(torch.int32)[:fr * (P + 1)].reshape(fr, P + 1, ldc)[:, 0, :N] = 0
    check_sentinel(tok, fr * (P + 1), N, f"patch epilogue {case}")
    exact(tok[:fr * (P + 1)].reshape(fr, P + 1, ldc)[:, 1:, :N], E.patch16_ref(d, P), f"patch epilogue {case} ({L.launch_name(recs[0])})")
    return recs


@pytest.mark.parametrize("k", E.CONVT_K)
@pytest.mark.parametrize("case", E.CONVT16_CASES, ids=lambda c: "B%d-%dx%d-C%d-Cp%d" % c)
def test_gemm_f16_convtranspose_exact(ops, L, gemm_variant, case, k):
    run_convt_exact(ops, L, case, k)


def run_convt_exact(ops, L, case, k):
    B, h, w_, C, Cp = case
    inp = E.convt16_inputs(case, k)
    d, a = {n: v.double() for n, v in inp.items()}, {n: v.double().abs() for n, v in inp.items()}
    ref = E.convt_ref(d["x"], d["w"], d["bias"], k)
    E.assert_exact_safe_f16([E.convt_ref(a["x"], a["w"], a["bias"], k)], [ref])
    xin = torch.zeros(B, h, w_, Cp, dtype=F16)
    xin[..., :C] = h16(inp["x"].permute(0, 2, 3, 1))
    wp, bp = ops.pack_convt(inp["w"], inp["bias"], Cp)
    rows = B * h * k * w_ * k
    out = sentinel_out_f16(rows, Cp, Cp)
    recs = launch(ops, L, guarded(xin.reshape(B * h * w_, Cp)), guarded(wp), out, L.EPI_CONVT_F16, bias=guarded(bp), **E.convt16_kw(case, k))
    what = f"convT k={k} {case} ({L.launch_name(recs[0])})"
    check_sentinel(out, rows, Cp, what)
    y = out[:rows].reshape(B, h * k, w_ * k, Cp)
    exact(y[..., :C], ref, what)
    assert bool((y[..., C:] == 0).all()), "pad channels must be exactly 0"
    return recs


# ---------------------------------------------------------------- conv3x3, exact
@functools.lru_cache(maxsize=None)
def conv_data(case):
    B, H, W, Cin, Cout, stride, relu_in, ldc = case
    inp = E.conv16_inputs(case)
    ref = E.conv16_check(case, inp)
    from video_depth_anything_amd import ops as o
    M = ref["no_bias"].numel() // Cout
    g = dict(x=guarded(h16(inp["x"].permute(0, 2, 3, 1).contiguous()), pad_elems=(W + 2) * Cin), w=guarded(o.pack_conv3x3(inp["w"])), bias=guarded(inp["bias"]),
             res=guarded(pad_cols(inp["res"].reshape(M, Cout), ldc, F16)), res2=guarded(pad_cols(inp["res2"].reshape(M, Cout), ldc, F16)))
    return {k: v.reshape(M, Cout) for k, v in ref.items()}, g


def run_conv_exact(ops, L, case, tag="", epis=E.CONV16_EPIS, seam_cap=None):
    B, H, W, Cin, Cout, stride, relu_in, ldc = case
    ref, g = conv_data(case)
    kw = E.conv16_kw(case)
    M = kw["M"]
    names = set()
    for epi in epis:
        out = sentinel_out_f16(M, Cout, ldc)
        t = dict(bias_f16=dict(bias=g["bias"]), no_bias={}, bias_relu=dict(bias=g["bias"]), res=dict(bias=g["bias"], res=g["res"]),
                 res_res2=dict(bias=g["bias"], res=g["res"], res2=g["res2"]))[epi]
        recs = launch(ops, L, g["x"], g["w"], out, getattr(L, "EPI_" + E.EPI_OF[epi]), **t, **kw)
        names.add(L.launch_name(recs[0]))
        if seam_cap is not None:
            assert_seam(L, recs, M, Cout, seam_cap)
        what = f"conv3x3_f16 {E.conv16_id(case)} {epi}{tag} ({L.launch_name(recs[0])})"
        check_sentinel(out, M, Cout, what)
        exact(out[:M, :Cout], ref[epi], what)
    return names


@pytest.mark.parametrize("case", E.CONV16_CASES, ids=E.conv16_id)
def test_conv3x3_f16_exact(ops, L, gemm_variant, case):
    names = run_conv_exact(ops, L, case)
    if gemm_variant in (-1, 7) and case[5] == 1 and case[4] <= 64:
        assert names == {"conv3x3_lds_kernel<%d>" % (1 if case[4] <= 32 else 2)}, "the LDS convolution covers this shape"


def test_conv3x3_f16_c64_exact_under_both_lds_kernels(ops, L):
    """The C = 64 -> 64 shape under the persistent LDS kernel (the default) and under the per-pass one it replaces."""
    case = E.CONV16_CASES[3]
    assert case[3] == 64 and 32 < case[4] <= 64 and case[5] == 1
    L.lib.vda_gemm_set_variant(-1)
    try:
        for v in (0, 1):
            L.lib.vda_conv_lds_set_variant(v)
            assert run_conv_exact(ops, L, case, tag=f" conv_lds variant {v}") == {"conv3x3_lds_kernel<2>"}
    finally:
        L.lib.vda_conv_lds_set_variant(0)


# ---------------------------------------------------------------- depth tail without a resize, exact
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("Cc", E.TAIL16_C)
@pytest.mark.parametrize("case", E.TAIL16_CASES, ids=lambda c: "B%d-%dx%d" % c)
def test_depth_tail_identity_resize_exact(ops, L, case, Cc, variant):
    """h == H, w == W: conv3x3(C -> 32) + ReLU + conv1x1 + ReLU with nothing rounded to fp16 between the two (tail.hip), fp32 out: the
    2**24 condition alone. One pixel (eight taps are padding), a tile remainder in both axes, (33, 65) = one past 4 x 2 tiles of 8 x 32."""
    B, H, W = case
    inp = E.tail16_inputs(case, Cc)
    b3 = inp.pop("b3")
    d, a = {k: v.double() for k, v in inp.items()}, {k: v.double().abs() for k, v in inp.items()}
    E.assert_exact_safe(E.tail16_ref(a, abs(b3)), F.conv2d(a["x"], a["w2"], a["b2"], padding=1))
    x = guarded(h16(inp["x"].permute(0, 2, 3, 1).contiguous()), pad_elems=(W + 2) * Cc)
    out = sentinel_out(B * H, W, W)
    L.lib.vda_depth_tail_set_variant(variant)
    try:
        ops.depth_tail(x, guarded(ops.pack_conv3x3(inp["w2"])), guarded(inp["b2"]), guarded(inp["w3"]), b3, out, B, H, W, H, W, Cc)
    finally:
        L.lib.vda_depth_tail_set_variant(0)
    check_sentinel(out, B * H, W, f"depth tail {case} C={Cc}")
    exact(out[:B * H].reshape(B, H, W), E.tail16_ref(d, b3), f"depth tail {case} C={Cc} variant {variant}")


# ---------------------------------------------------------------- tile seams: a persistent workgroup's second and third tile
# vda_set_max_wgs(8 or 16) makes a few thousand rows three rounds of every persistent grid (tests/_exact.py, "tile seams"; what each
# case's launches walk is asserted on the CPU in tests/test_exact_inputs.py). Same operands, references and checks as above.
@pytest.mark.parametrize("dyn", [False, True], ids=["static", "dynamic_draw"])
@pytest.mark.parametrize("spec", E.SEAM16_SPECS, ids=E.seam16_id)
def test_gemm_f16_tile_seams_dense(ops, L, spec, dyn):
    """Every epilogue the spec's tile is built for, under every variant that plans that tile for it: two full rounds and a partial third
    in one of the walk's three modes, five or nine K steps. dyn: the launches whose record draws its tiles, with eight zeroed counters."""
    bm, bn, per_cu, cap, case = spec
    M, N, K, lda, ldc = case
    todo = [t for t in E.seam16_launches(L, spec) if t[3] or not dyn]
    if dyn and not todo:
        assert not L.lib.vda_gemm_built(L.FAM_8P, bm, bn, per_cu, 0, L.EPI_BIAS_F16), "only the 8-phase kernel draws tiles"
        return
    assert todo, "no variant plans this tile for this case: the case covers nothing"
    (inp, ref, g), (rref, rg) = dense_data(case), real_data(case)
    try:
        with capped(L, cap):
            for variant, epi, fam, _ in todo:
                L.lib.vda_gemm_set_variant(variant)
                sched = torch.zeros(8, dtype=torch.int32, device="cuda") if dyn else None
                try:
                    recs = run_dense_exact(ops, L, case, epi, g, ref, sched) if epi in E.DENSE16_EXACT else run_dense_real(ops, L, case, epi, rref, rg, sched)
                except AssertionError as e:
                    raise AssertionError(f"variant {variant}, cap {cap}, dyn={dyn}: {e}") from None
                r = assert_seam(L, recs, M, N, cap)
                assert (r.family, r.bm, r.bn, r.per_cu, r.dyn) == (fam, bm, bn, per_cu, int(dyn)), L.launch_name(r)
                if dyn:
                    assert int(sched.sum()) > 0, f"variant {variant} {epi}: no tile was drawn from the counters"
    finally:
        L.lib.vda_gemm_set_variant(-1)


@pytest.mark.parametrize("stagger", ["1", "2"])
def test_gemm_f16_tile_seams_with_the_last_round_stagger(ops, L, monkeypatch, stagger):
    """VDA_GEMM_STAGGER: the workgroups that sit out the last round start late (stagger_last_round needs a full round and a partial one;
    off by default on the automatic path and the one-barrier kernels, always on under a forced 8-phase variant). A delay only: same bits."""
    monkeypatch.setenv("VDA_GEMM_STAGGER", stagger)
    L.lib.vda_gemm_reload_tuning()
    try:
        for spec in E.SEAM16_SPECS:
            bm, bn, per_cu, cap, case = spec
            if case[2] != 320 or case[1] % 64:
                continue
            inp, ref, g = dense_data(case)
            with capped(L, cap):
                for variant, epi, fam, _ in E.seam16_launches(L, spec):
                    if epi in ("bias_f16", "split"):
                        L.lib.vda_gemm_set_variant(variant)
                        assert_seam(L, run_dense_exact(ops, L, case, epi, g, ref), case[0], case[1], cap)
    finally:
        L.lib.vda_gemm_set_variant(-1)
        monkeypatch.delenv("VDA_GEMM_STAGGER")
        L.lib.vda_gemm_reload_tuning()


def seam_variants(L, fields, variants, fold=False):
    """[(variant, cap)] of a conv / patch / ConvTranspose / folded seam case: the variants that plan a large tile with more than two rounds
    of tiles under vda_set_max_wgs(8) or (16) (E.pick_cap). What they reach is asserted on the CPU."""
    out = []
    for v in variants:
        L.lib.vda_gemm_set_variant(v)
        got = E.pick_cap(L, fields, fold)
        if got is not None:
            out.append((v, got[0]))
    L.lib.vda_gemm_set_variant(-1)
    assert out, "no variant reaches three rounds on this case: it covers nothing"
    return out


@pytest.mark.parametrize("case", E.SEAM_CONV16_CASES[:-1], ids=E.conv16_id)
def test_conv3x3_f16_tile_seams(ops, L, case):
    """Conv A on the large tiles past a workgroup's first tile: set_sources and TapCursor::seek at the seams, windows that cross frame
    borders inside later tiles, with and without the input ReLU (the plain instantiations), every conv epilogue, every conv family."""
    kw = E.conv16_kw(case)
    try:
        for variant, cap in seam_variants(L, E.gemm16_fields(epi=L.EPI_BIAS_F16, **kw), E.SEAM_CONV16_VARIANTS):
            L.lib.vda_gemm_set_variant(variant)
            with capped(L, cap):
                run_conv_exact(ops, L, case, tag=f" variant {variant} cap {cap}", seam_cap=cap)
    finally:
        L.lib.vda_gemm_set_variant(-1)


def test_conv3x3_f16_c64_tile_seams(ops, L):
    """conv3x3_c64_kernel on 8 workgroups: 27 tiles, three or four per workgroup - both patch buffers and the residual prefetch reused -
    and the per-pass kernel on the same case. (Both report as conv3x3_lds_kernel<2>; which one vda_conv_lds_set_variant selects is
    conv_lds.hip's dispatch: variant 0 with Cin = 64 and 32 < Cout <= 64 is the persistent one.)"""
    case = E.SEAM_C64_CASE
    L.lib.vda_gemm_set_variant(-1)
    try:
        with capped(L, 8):
            for v in (0, 1):
                L.lib.vda_conv_lds_set_variant(v)
                assert run_conv_exact(ops, L, case, tag=f" conv_lds variant {v} cap 8", epis=E.SEAM_C64_EPIS) == {"conv3x3_lds_kernel<2>"}
    finally:
        L.lib.vda_conv_lds_set_variant(0)


@pytest.mark.parametrize("case", E.SEAM_PATCH16_CASES, ids=lambda c: "fr%d-P%d-N%d-K%d-ldc%d" % c)
def test_gemm_f16_patch_epilogue_tile_seams(ops, L, case):
    """The patch-embed row map (row -> frame, patch; pos row) on rows of later tiles: frame boundaries inside tiles of rounds 1 and 2."""
    kw = E.patch16_kw(case)
    try:
        for variant, cap in seam_variants(L, E.gemm16_fields(epi=L.EPI_PATCH_F32, **kw), E.SEAM_CONV16_VARIANTS):
            L.lib.vda_gemm_set_variant(variant)
            with capped(L, cap):
                assert_seam(L, run_patch_exact(ops, L, case), kw["M"], kw["N"], cap)
    finally:
        L.lib.vda_gemm_set_variant(-1)


@pytest.mark.parametrize("case,k", E.SEAM_CONVT16, ids=lambda c: "B%d-%dx%d-C%d-Cp%d" % c if isinstance(c, tuple) else "k%d" % c)
def test_gemm_f16_convtranspose_tile_seams(ops, L, case, k):
    """The ConvTranspose scatter on rows of later tiles, three frames."""
    kw = E.convt16_kw(case, k)
    try:
        for variant, cap in seam_variants(L, E.gemm16_fields(epi=L.EPI_CONVT_F16, **kw), E.SEAM_CONV16_VARIANTS):
            L.lib.vda_gemm_set_variant(variant)
            with capped(L, cap):
                assert_seam(L, run_convt_exact(ops, L, case, k), kw["M"], kw["N"], cap)
    finally:
        L.lib.vda_gemm_set_variant(-1)


@pytest.mark.parametrize("case", E.SEAM_FOLD_CASES, ids=lambda c: "k%d-Cin%d-Fe%d-B%d-%dx%d" % c)
def test_gemm_f16_folded_convtranspose_tile_seams(ops, L, case):
    """The folded ConvTranspose + conv on the 8-phase kernel (the one persistent family that takes the mode) under cap 8: three rounds
    and more, each with its own rotation of the column tiles, per-tile K step counts from the tap mask."""
    k, Cin, Fe, B, H, W = case
    t, Wc, Bc, ref = E.seam_fold_data(case)
    f = E.fold_fields(case)
    Mo = B * k * H * k * W
    x = guarded(h16(t.permute(0, 2, 3, 1).reshape(B * H * W, Cin).float()), pad_elems=(W + 2) * Cin)
    wf, bc = guarded(h16(R.pack(Wc).float())), guarded(R.class_bias(Bc).float())
    try:
        for variant, cap in seam_variants(L, f, (-1, 5), fold=True):
            L.lib.vda_gemm_set_variant(variant)
            with capped(L, cap):
                out = sentinel_out_f16(Mo, Fe, Fe)
                recs = launch(ops, L, x, wf, out, L.EPI_CONVT_FOLD_F16, bias=bc, M=f["M"], N=f["N"], K=f["K"], ldc=Fe, conv=(B, H, W, Cin, H, W, 1), convt=(k, H, W, Fe))
            r = assert_seam(L, recs, f["M"], f["N"], cap)
            what = f"folded convT {case} variant {variant} cap {cap} ({L.launch_name(r)})"
            assert r.family == L.FAM_8P
            check_sentinel(out, Mo, Fe, what)
            exact(out[:Mo].reshape(B, k * H, k * W, Fe), ref.permute(0, 2, 3, 1), what)
    finally:
        L.lib.vda_gemm_set_variant(-1)


@pytest.mark.parametrize("variant", [-1, 5])
def test_gemm_f16_blocked_walk_exact_at_five_k_steps(ops, L, variant):
    """The L2-blocked order (N = 2048: eight column tiles in two groups, 32 workgroups per XCD, uncapped) with a K loop that has a steady
    state - test_gemm_f16_tile_walk_exact's K = 64 never enters the pipeline - and a row-dependent epilogue."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count & ~7
    M, N, _ = E.walk16_case(ncu, 2048)
    case = (M, N, E.WALK16_BLOCKED_K)
    lin, res, A, W, b, r16 = blocked_data(case)
    L.lib.vda_gemm_set_variant(variant)
    try:
        for epi, kw, want in ((L.EPI_BIAS_F16, {}, lin), (L.EPI_RES_F16, dict(res=r16), lin + res)):
            out = sentinel_out_f16(M, N, N)
            recs = launch(ops, L, A, W, out, epi, M=M, N=N, K=case[2], bias=b, **kw)
            r = recs[0]
            assert len(recs) == 1 and (r.family, r.bm, r.bn) == (L.FAM_8P, 256, 256) and -(-M // 256) * 8 > ncu, L.launch_name(r)
            assert ncu == 256, "the blocked order needs 32 workgroups per XCD"
            check_sentinel(out, M, N, f"blocked walk variant {variant} epilogue {epi}")
            exact(out[:M], want, f"blocked walk M={M} N={N} K={case[2]} variant {variant} epilogue {epi} ({L.launch_name(r)})")
    finally:
        L.lib.vda_gemm_set_variant(-1)


@functools.lru_cache(maxsize=None)
def blocked_data(case):
    M, N, K = case
    inp = E.walk16_inputs(case)
    d = {k: v.double() for k, v in inp.items()}
    res = E.ints((M, N), -4, 4, 5995)
    lin = d["A"] @ d["W"].t() + d["bias"]
    E.assert_exact_safe_f16([d["A"].abs() @ d["W"].abs().t() + d["bias"].abs() + 4], [lin, lin + res.double(), res.double()])
    return lin, res.double(), guarded(h16(inp["A"])), guarded(h16(inp["W"])), guarded(inp["bias"]), guarded(h16(res))
