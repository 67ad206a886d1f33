"""The split residual stream at the edge of fp16's range, kernel by kernel: VDA_EPI_SCALE_RES_SPLIT in every tile family, a row range
of it, vda_mlp_fused_f16, vda_ln_stats_finalize one step later, and the tap LayerNorm (vda_layernorm_split_check_f16) that reports a
saturated row nothing else reads again. Inputs of tests/_split_range.py: the fp32 result of every element is known exactly (shown on the
CPU in tests/test_split_range_inputs.py, where every comparison used here is also shown able to fail), so

  planes       hi and lo equal the definition bit for bit, +-65 504 and the largest fp32 below 65 520 stay finite, 65 520 / 65 536 / 1e5
               become (+-inf, -+inf); nothing behind the result is written, nothing inside is left;
  isolation    every row that is in range is bit-identical - planes and statistics - to the same launch with the saturated rows' operands
               replaced by zeros;
  statistics   the partial (sum, centred squares) of the rows in range equal the builder's;
  next step    a second residual GEMM over the planes has non-finite partials in exactly the saturated rows, vda_ln_stats_finalize
               raises the flag, every other row's (mean, rstd) is the clean chain's;
  tap          the checked LayerNorm raises the flag for a saturated row it normalises and for no other input, and never changes a bit
               of the output.

Every output is a sentinel buffer with 8 rows behind the result. No tolerance anywhere but the LayerNorm's fp16 output against fp64,
which takes tests/test_kernels_gpu.py's."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _split_range as SR
from _exact import check_sentinel, sentinel_out, sentinel_out_f16
from test_kernels_gpu import gemm_variant, ops  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

FAMILY_KERNEL = {0: "gemm_kernel<", 2: "gemm256s_kernel<", 3: "gemm8p_kernel<"}


@pytest.fixture(scope="module")
def L():
    from video_depth_anything_amd import _lib
    return _lib


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def gemm_case(shape, k, sat_from=0):
    M, N, K = shape
    case = SR.build(M, N, K, SR.scene(M, N, k, sat_from), seed=k)
    return case, SR.zeroed(case)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def split_args(L, ops, M, N, K, A, W, bias, gamma, pos, hi, lo, part):
    a = L.GemmArgs()
    a.A, a.W, a.bias, a.gamma, a.pos = ptr(A), ptr(W), ptr(bias), ptr(gamma), ptr(pos)
    a.out, a.res, a.out2, a.res2, a.stats = ptr(hi), ptr(hi), ptr(lo), ptr(lo), ptr(part)
    a.zero_page = ptr(ops.zero_page(A.device))
    a.M, a.N, a.K, a.lda, a.ldc, a.a_mode, a.epilogue = M, N, K, K, N, L.A_DENSE, L.EPI_SCALE_RES_SPLIT
    return a


def run_args(L, ops, a):
    ops.check(L.lib.vda_gemm_f16(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "vda_gemm_f16")
    return L.lib.vda_gemm_last_kernel().decode()


def residual_step(L, ops, case, planes=None, step2=False, split_at=None):
    """One VDA_EPI_SCALE_RES_SPLIT launch in place over sentinel-backed planes -> (hi, lo, part [nb, M, 2]) as host arrays and the kernel
    names. planes: the (hi, lo) to start from (default: the case's residual planes). step2: the update of the NEXT step - A = 0, bias = 0,
    gamma = 1 and a centre of +-300 in the rows that sit at +-65 504 / +-NA (re-read, NA's planes are 65 520: without a centre the step
    would saturate them itself), so X2 = (hi + lo) - pos2 exactly. split_at: as two row ranges of vda_gemm_row_range."""
    M, N, K = case["M"], case["N"], case["K"]
    nb = N // 64
    hi, lo, part = sentinel_out_f16(M, N, N), sentinel_out_f16(M, N, N), sentinel_out(nb * M, 2, 2)
    h0, l0 = planes if planes is not None else (case["res_hi"], case["res_lo"])
    hi[:M], lo[:M] = dev(h0), dev(l0)
    if step2:
        pos2 = np.zeros((M, 2), dtype=np.float32)
        pos2[:, 1] = 1.0
        for r, v, _, _ in case["placements"]:
            if abs(v) <= SR.NA:
                pos2[r, 0] = np.sign(v) * 300.0
        A, W = torch.zeros(M, K, dtype=torch.float16, device="cuda"), dev(case["W"])
        bias, gamma, pos = torch.zeros(N, device="cuda"), torch.ones(N, device="cuda"), dev(pos2)
    else:
        A, W, bias, gamma, pos = dev(case["A"]), dev(case["W"]), dev(case["bias"]), dev(case["gamma"]), dev(case["pos"])
    a = split_args(L, ops, M, N, K, A, W, bias, gamma, pos, hi, lo, part)
    names = []
    if split_at is None:
        names.append(run_args(L, ops, a))
    else:
        for r0, rows in ((0, split_at), (split_at, M - split_at)):
            b = L.GemmArgs()
            ops.check(L.lib.vda_gemm_row_range(C.byref(a), r0, rows, C.byref(b)), "vda_gemm_row_range")
            assert b.stats_ld == M and b.M == rows
            names.append(run_args(L, ops, b))
    torch.cuda.synchronize()
    what = f"M={M} N={N} {'step 2' if step2 else 'step 1'} {names}"
    check_sentinel(hi, M, N, what + " hi"), check_sentinel(lo, M, N, what + " lo"), check_sentinel(part, nb * M, 2, what + " partials")
    return host(hi[:M]), host(lo[:M]), host(part[:nb * M]).reshape(nb, M, 2), names


def rows_in_range(case):
    return np.flatnonzero(case["kind"] != SR.SATURATED)


def by_row(part):
    return np.ascontiguousarray(part.transpose(1, 0, 2)).reshape(part.shape[1], -1)


def finalize(ops, part):
    nb, M, _ = part.shape
    stat, flag = sentinel_out(M, 2, 2), torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.ln_stats_finalize(dev(part), stat, 1e-6, M, nb, flag)
    torch.cuda.synchronize()
    check_sentinel(stat, M, 2, "ln_stats_finalize")
    return host(stat[:M]), int(flag.item())


def check_step(L, ops, case, z, variant, split_at=None):
    what = f"variant {variant}, M={case['M']} N={case['N']}, placements {case['placements']}" + (f", rows split at {split_at}" if split_at else "")
    hi, lo, part, names = residual_step(L, ops, case, split_at=split_at)
    fam = FAMILY_KERNEL[SR.VARIANT_FAMILY[variant]]
    assert all(n.startswith(fam) for n in names), f"{what}: ran {names}, the table of tests/_split_range.py says {fam}"
    for bad in (SR.planes_mismatch(case, hi, lo), SR.partials_mismatch(case, part)):
        assert bad is None, f"{what}: {bad}"
    # the same launch without the saturated rows: no other row may notice
    zhi, zlo, zpart, _ = residual_step(L, ops, z, split_at=split_at)
    assert SR.planes_mismatch(z, zhi, zlo) is None, what
    ok = rows_in_range(case)
    for got, ref, name in ((hi, zhi, "hi"), (lo, zlo, "lo"), (by_row(part), by_row(zpart), "partial statistics")):
        bad = SR.rows_mismatch(got, ref, ok, f"{what}: {name} against the launch with the saturated rows zeroed")
        assert bad is None, bad
    return (hi, lo), (zhi, zlo)


@pytest.mark.parametrize("shape", SR.GEMM_SHAPES, ids=lambda s: "M%d-N%d-K%d" % s)
def test_residual_gemm_at_the_edge_of_the_range(ops, L, gemm_variant, shape):
    """Planes, isolation and statistics of the step that saturates, then the next step and its finalize - in every tile family (the
    variants that VDA_EPI_SCALE_RES_SPLIT has no large tile for run the 128-row kernel: asserted), over the eight scenes of the shape."""
    assert gemm_variant in SR.VARIANT_FAMILY, "a new variant: add it to tests/_split_range.py, where the CPU test holds it to the planner"
    for k in SR.SCENES:
        case, z = gemm_case(shape, k)
        planes, zplanes = check_step(L, ops, case, z, gemm_variant)
        # one step later: NaN read back into the partials of exactly the saturated rows; finalize raises the flag
        hi2, lo2, part2, _ = residual_step(L, ops, case, planes=planes, step2=True)
        zhi2, zlo2, zpart2, _ = residual_step(L, ops, z, planes=zplanes, step2=True)
        stat, flag = finalize(ops, part2)
        zstat, zflag = finalize(ops, zpart2)
        what = f"variant {gemm_variant}, {shape}, scene {k}"
        assert zflag == 0 and np.isfinite(zstat).all() and np.isfinite(zpart2).all(), f"{what}: the clean chain is not clean"
        bad = SR.next_step_mismatch(case, part2, flag, stat, zstat)
        assert bad is None, f"{what}: {bad}"
        ok = rows_in_range(case)
        with np.errstate(invalid="ignore"):
            x2 = planes[0].astype(np.float32) + planes[1].astype(np.float32)
        for r, v, _, _ in case["placements"]:
            if abs(v) <= SR.NA:
                x2[r] -= np.float32(np.sign(v) * 300.0)
        want = dict(hi=SR.planes_of(x2)[0], lo=SR.planes_of(x2)[1], X=x2)
        bad = SR.planes_mismatch(want, hi2, lo2, rows=ok)
        assert bad is None, f"{what}, step 2: {bad}"
        assert np.isnan(hi2[case["sat_rows"]].astype(np.float32)).any(1).all(), f"{what}: a saturated element reads back as NaN"
        for got, ref, name in ((hi2, zhi2, "hi"), (lo2, zlo2, "lo")):
            bad = SR.rows_mismatch(got, ref, ok, f"{what}, step 2: {name} against the clean chain")
            assert bad is None, bad


def test_residual_gemm_row_range_with_the_saturated_row_in_the_second_part(ops, L, gemm_variant):
    """vda_gemm_row_range: rows [0, 280) and [280, 300) as two launches that share the planes and the [nb, 300, 2] partials (stats_ld).
    Rows 0 .. 270 hold in-range edge values, row 299 or 287 - in the second part - saturates: the same planes, statistics and isolation."""
    shape = SR.GEMM_SHAPES[0]
    for k in (0, 3):
        case, z = gemm_case(shape, k, 280)
        assert case["sat_rows"].tolist() == [[299], [287]][k // 3]
        whole, _ = check_step(L, ops, case, z, gemm_variant)
        parts, _ = check_step(L, ops, case, z, gemm_variant, split_at=280)
        assert np.array_equal(SR.bits16(whole[0]), SR.bits16(parts[0])) and np.array_equal(SR.bits16(whole[1]), SR.bits16(parts[1]))


# ---------------------------------------------------------------- the fused MLP kernel
@pytest.mark.parametrize("shape", SR.MLP_SHAPES, ids=lambda s: "M%d-D%d" % s)
def test_fused_mlp_at_the_edge_of_the_range(ops, L, shape):
    """vda_mlp_fused_f16 with fc1 = 0 (GELU(0) = 0: the branch adds gamma * b2 and nothing else), the edge values placed through the
    planes, b2 and the statistics rows' mean: planes equal the definition, in-range rows exact and untouched by the saturated ones."""
    M, D = shape
    H = 4 * D
    assert L.lib.vda_mlp_fused_supported(D, H) == 1
    g = torch.Generator().manual_seed(5)
    w1, c0 = torch.zeros(H, D, dtype=torch.float16, device="cuda"), torch.zeros(H, device="cuda")
    w2 = torch.randint(-2, 3, (D, H), generator=g).to(torch.float16).cuda()
    w2p = torch.empty_like(w2)
    ops.mlp_permute_w2(w2, w2p, D, H)

    def run(case):
        hi, lo, part = sentinel_out_f16(M, D, D), sentinel_out_f16(M, D, D), sentinel_out(D // 64 * M, 2, 2)
        hi[:M], lo[:M] = dev(case["res_hi"]), dev(case["res_lo"])
        ops.mlp_fused(hi, dev(case["pos"]), w1, c0, c0, w2p, dev(case["bias"]), dev(case["gamma"]), hi, lo, part, M, D, H)
        torch.cuda.synchronize()
        for buf, rows, cols, name in ((hi, M, D, "hi"), (lo, M, D, "lo"), (part, D // 64 * M, 2, "partials")):
            check_sentinel(buf, rows, cols, f"mlp_fused M={M} {name}")
        return host(hi[:M]), host(lo[:M]), host(part[:D // 64 * M]).reshape(D // 64, M, 2)

    for k in SR.SCENES:
        case = SR.build(M, D, 64, SR.scene(M, D, k), seed=20 + k, gemm=False)
        z = SR.zeroed(case)
        what = f"mlp_fused M={M}, placements {case['placements']}"
        hi, lo, part = run(case)
        for bad in (SR.planes_mismatch(case, hi, lo), SR.partials_mismatch(case, part, mode="mlp")):
            assert bad is None, f"{what}: {bad}"
        zhi, zlo, zpart = run(z)
        assert SR.planes_mismatch(z, zhi, zlo) is None, what
        for got, ref, name in ((hi, zhi, "hi"), (lo, zlo, "lo"), (by_row(part), by_row(zpart), "partial statistics")):
            bad = SR.rows_mismatch(got, ref, rows_in_range(case), f"{what}: {name} against the launch with the saturated rows zeroed")
            assert bad is None, bad


# ---------------------------------------------------------------- the tap LayerNorm: the entry that reports the step nothing re-reads
def ln_affine(D):
    g = torch.Generator().manual_seed(900 + D)
    return (torch.randn(D, generator=g) * 0.5 + 1.0), torch.randn(D, generator=g) * 0.3


def run_ln(ops, hi, lo, w, b, D, group, skip, flag="new"):
    """(out rows as host fp16, flag value or None). flag: "new" = a fresh zeroed flag, None = NULL, "plain" = vda_layernorm_split_f16."""
    rows = hi.shape[0]
    rows_out = rows if group == 0 else rows // group * (group - skip)
    out = sentinel_out_f16(rows_out, D, D)
    f = torch.zeros(1, dtype=torch.int32, device="cuda") if flag == "new" else None
    if flag == "plain":
        ops.layernorm_split(dev(hi), dev(lo), out, dev(w.numpy()), dev(b.numpy()), 1e-6, rows, D, group=group, skip=skip)
    else:
        ops.layernorm_split_check(dev(hi), dev(lo), out, dev(w.numpy()), dev(b.numpy()), 1e-6, rows, D, group=group, skip=skip, overflow=f)
    torch.cuda.synchronize()
    check_sentinel(out, rows_out, D, f"layernorm_split D={D} group={group} skip={skip} flag={flag}")
    return host(out[:rows_out]), (None if f is None else int(f.item()))


def ln_reference_mismatch(case, out, rows_in, rows_out, w, b):
    """LayerNorm of the EXACT rows in fp64 against the fp16 output, at tests/test_kernels_gpu.py's tolerance (2e-3 + 2e-3 |ref|)."""
    ex = case["kind"][rows_in] == SR.EXACT
    x = case["X"][rows_in[ex]].astype(np.float64)
    ref = (x - x.mean(1, keepdims=True)) / np.sqrt(x.var(1, keepdims=True) + 1e-6) * w.double().numpy() + b.double().numpy()
    err = np.abs(out[rows_out[ex]].astype(np.float64) - ref)
    bad = err > 2e-3 + 2e-3 * np.abs(ref)
    return f"{int(bad.sum())} elements out of tolerance, worst {err.max():.3g}" if bad.any() else None


@pytest.mark.parametrize("D", SR.LN_D)
@pytest.mark.parametrize("i", range(len(SR.LN_SAT_ROWS)), ids=lambda i: f"row{SR.LN_SAT_ROWS[i]}")
def test_tap_layernorm_reports_a_saturated_row_it_normalises(ops, D, i):
    """One saturated row - first, last, 255, 256, 270; each of the four saturating values, in either block - among rows at +-65 504 and
    +-NA. Plain: flag 1, that row's output is NaN. group = 5, skip = 1 with the row kept: the same. With the row dropped: flag 0, and
    the output is the run without that row, every bit of it. Always: every other row equals the run with that row zeroed, the flag
    changes no bit of the output (NULL flag, and the unchecked entry), the EXACT rows are the LayerNorm of their values."""
    w, b = ln_affine(D)
    for shift in range(4):
        case, row, dropped = SR.ln_case(D, i, shift)
        z = SR.zeroed(case)
        what = f"D={D}, saturated row {row} ({case['placements'][-1]})"
        for group, skip in ((0, 0), (SR.LN_GROUP, SR.LN_SKIP)):
            rows_in, rows_out = SR.ln_kept(SR.LN_ROWS, group, skip)
            out, flag = run_ln(ops, case["hi"], case["lo"], w, b, D, group, skip)
            zout, zflag = run_ln(ops, z["hi"], z["lo"], w, b, D, group, skip)
            normalised = group == 0 or not dropped
            assert flag == int(normalised), f"{what}, group {group}: flag {flag}"
            assert zflag == 0 and np.isfinite(zout.astype(np.float32)).all(), f"{what}: the clean planes raise the flag or give NaN"
            others = rows_out[rows_in != row]
            bad = SR.rows_mismatch(out, zout, others, f"{what}, group {group}: output against the run with that row zeroed")
            assert bad is None, bad
            if normalised:
                assert np.isnan(out[rows_out[rows_in == row]].astype(np.float32)).all(), f"{what}: a saturated row normalises to NaN"
            for other in (None, "plain"):
                same, _ = run_ln(ops, case["hi"], case["lo"], w, b, D, group, skip, flag=other)
                assert np.array_equal(SR.bits16(same), SR.bits16(out)), f"{what}, group {group}: the flag changes the output ({other})"
            bad = ln_reference_mismatch(case, out, rows_in, rows_out, w, b)
            assert bad is None, f"{what}, group {group}: {bad}"


@pytest.mark.parametrize("D", SR.LN_D)
def test_tap_layernorm_does_not_report_a_stream_that_is_in_range(ops, D):
    """+-65 504 and +-NA (planes 65 504 + 16) in every special row and block, nothing beyond: the flag stays 0, the output is finite and
    bit-equal to a call with a NULL flag and to the unchecked entry. A flag that is already 1 stays 1 (the entry never clears it)."""
    w, b = ln_affine(D)
    for k in SR.SCENES:
        case = SR.ln_in_range_case(D, k)
        assert np.isfinite(case["hi"].astype(np.float32)).all() and (np.abs(case["X"]) >= 65504.0).any()
        for group, skip in ((0, 0), (SR.LN_GROUP, SR.LN_SKIP)):
            out, flag = run_ln(ops, case["hi"], case["lo"], w, b, D, group, skip)
            assert flag == 0, f"D={D} scene {k} group {group}: an in-range stream is reported"
            assert np.isfinite(out.astype(np.float32)).all()
            for other in (None, "plain"):
                same, _ = run_ln(ops, case["hi"], case["lo"], w, b, D, group, skip, flag=other)
                assert np.array_equal(SR.bits16(same), SR.bits16(out)), (D, k, group, other)
            rows_in, rows_out = SR.ln_kept(SR.LN_ROWS, group, skip)
            bad = ln_reference_mismatch(case, out, rows_in, rows_out, w, b)
            assert bad is None, f"D={D} scene {k} group {group}: {bad}"
    one = torch.ones(1, dtype=torch.int32, device="cuda")
    out = sentinel_out_f16(SR.LN_ROWS, D, D)
    ops.layernorm_split_check(dev(case["hi"]), dev(case["lo"]), out, dev(w.numpy()), dev(b.numpy()), 1e-6, SR.LN_ROWS, D, overflow=one)
    assert int(one.item()) == 1


def test_tap_layernorm_refuses_a_misaligned_flag(ops, L):
    D, rows = 128, 4
    z = torch.zeros(rows, D, dtype=torch.float16, device="cuda")
    out = sentinel_out_f16(rows, D, D)
    w = torch.ones(D, device="cuda")
    buf = torch.zeros(8, dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.lib.vda_layernorm_split_check_f16(ptr(z), ptr(z), ptr(out), ptr(w), ptr(w), 1e-6, rows, D, 0, 0, C.c_void_p(buf.data_ptr() + 2), stream)
    assert rc != 0 and b"4-byte aligned" in L.lib.vda_last_error()
    torch.cuda.synchronize()
    assert bool((out.view(torch.int16) == 0x7E5A).all()) and not bool(buf.any()), "a refused call wrote"
