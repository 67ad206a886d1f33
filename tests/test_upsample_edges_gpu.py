"""The two fused upsample convolutions of the fp16 forward - vda_conv3x3_up2_f16 (conv_up.hip) and vda_depth_tail_f16 with a resize
(tail.hip: depth_tail_kernel<1> and the persistent depth_tail_up_kernel) - and the unfused vda_bilinear_nhwc, at their tile edges.

A bilinear resize has fractional weights, so small integers alone are not exact. Three input families of tests/_exact.py leave a correct
kernel no room all the same (each shown sound, and each assertion shown able to fail, on the CPU in tests/test_exact_inputs.py):

  constant   every pixel of a (frame, channel) holds one small integer: the interpolated patch is that integer bit for bit, zeros
             outside the image, and the output is the integer convolution of a constant image - torch.equal against fp64. Sees a wrong
             halo pixel at any image or tile border, an unwritten or doubly written output, a stale ring buffer in any k-step, a frame
             mix-up, bias on the wrong cout.
  selector   every cout has a single weight 1 at one (tap, channel): the output IS one interpolated patch value. Against the fp64
             definition within |y - r| <= ulp16(r) / 2 + 2**-22 max(h, w) amax + 2**-22 amax (derived in _exact.up2_selector_bound,
             about 0.03), where a wrong source pixel, tap, channel, k-step, swizzle or cout block is an error of tens.
  dyadic     (the tail and vda_bilinear_nhwc, whose scale is free) scales in {0, 1/4, 1/2, 1, 3/2, 2}: every interpolated value is a
             multiple of 1/16, exact in fp16 at every step of every evaluation order - torch.equal against fp64, under both resizing
             kernels of the tail, with the kernel that ran asserted by name (vda_depth_tail_last_kernel).

Inputs are guarded views (NaN on both sides), outputs sentinel buffers (nothing outside may change, nothing inside may be left, and
everything inside is finite). The fp64 references are built once per case and shared between variants."""
import functools

import pytest
import torch
import torch.nn.functional as F

import _exact as E
from _exact import check_sentinel, guarded, sentinel_out, sentinel_out_f16
from test_kernels_f16_edges_gpu import L, capped, close_finite, exact, h16  # noqa: F401  (L: fixture)
from test_kernels_gpu import ops, rnd  # noqa: F401  (ops: fixture)

pytestmark = pytest.mark.gpu

F16, F32, F64 = torch.float16, torch.float32, torch.float64


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def pack(w):
    from video_depth_anything_amd import ops as O
    return O.pack_conv3x3(w)


# ---------------------------------------------------------------- vda_conv3x3_up2_f16
def run_up2(ops, case, x, wp, bias, offset=0, what=""):
    """One launch into a sentinel buffer (offset: `out` starts that many fp16 elements into its allocation); returns [B, 2h, 2w, N] on
    the host after the sentinel and finiteness checks."""
    B, h, w, C, N, ldc = case
    M = B * 4 * h * w
    if offset:
        flat = sentinel_out_f16(M + 9, ldc, ldc, extra_rows=0).view(-1)
        out = flat[offset:offset + (M + 8) * ldc].view(M + 8, ldc)
        assert out.data_ptr() % 16 == 2 * offset == 8, "8-byte alignment only: the narrow store path"
    else:
        flat = out = sentinel_out_f16(M, N, ldc)
    ops.conv3x3_up2(x, wp, bias, out, B, h, w, C, N, ldc)
    torch.cuda.synchronize()
    check_sentinel(out, M, N, what)
    if offset:
        bits = flat.view(torch.int16).cpu()
        assert bool((bits[:offset] == E.SENTINEL16_BITS).all()) and bool((bits[offset + (M + 8) * ldc:] == E.SENTINEL16_BITS).all()), f"{what}: wrote outside the view"
    y = out[:M, :N].cpu()
    assert bool(torch.isfinite(y).all()), f"{what}: {int((~torch.isfinite(y)).sum())} non-finite outputs (a guard or a pad leaked)"
    return y.reshape(B, 2 * h, 2 * w, N)


@functools.lru_cache(maxsize=None)
def up2_const_data(case):
    inp = E.up2_const_inputs(case)
    ref = E.up2_const_ref(case, inp)                      # (asserts the family's preconditions)
    C, w = case[3], case[2]
    return ref, guarded(h16(nhwc(inp["x"])), pad_elems=(w + 2) * C), guarded(pack(inp["w"])), guarded(inp["bias"])


@functools.lru_cache(maxsize=None)
def up2_selector_data(case):
    B, h, w, C, N, ldc = case
    x = E.up2_selector_x(case)
    amax = float(x.abs().max())
    sets = []
    for wsel, _ in E.up2_selector_sets(case):
        ref = E.fused_emulate(x, wsel.double(), 2 * h, 2 * w, "f64")
        sets.append((guarded(pack(wsel)), ref, E.up2_selector_bound(ref, h, w, amax)))
    assert E.up2_selector_coverage(case) == {(t, k, c) for t in range(9) for k in range(C // 16) for c in range(2)}
    return guarded(h16(nhwc(x)), pad_elems=(w + 2) * C), sets


UP2_RUNS = [(c, 0) for c in E.UP2_CASES] + [(c, 4) for c in E.UP2_OFFSET_CASES]
up2_run_id = lambda r: E.up2_id(r[0]) + ("-out+8B" if r[1] else "")      # noqa: E731


def assert_up2_geometry(case, offset):
    g = E.up2_geometry(case)
    assert g["rows"] <= E.UP2_SH and g["cols"] <= E.UP2_SW, "the source window fits the kernel's"
    if case == E.UP2_CASES[3]:
        assert g["per_xcd"] == 2 and g["idle"] == 4 and not g["wide"]
    if case in E.UP2_CASES[4:6]:
        assert (g["rows"], g["cols"], g["CB"]) == (10, 18, 4)
    if offset:
        assert case[5] % 4 == 0


@pytest.mark.parametrize("run", UP2_RUNS, ids=up2_run_id)
def test_conv3x3_up2_constant_image_exact(ops, run):
    """The constant family: equality with the integer convolution of the constant image."""
    case, offset = run
    assert_up2_geometry(case, offset)
    ref, x, wp, bias = up2_const_data(case)
    y = run_up2(ops, case, x, wp, bias, offset, f"conv3x3_up2 constant {up2_run_id(run)}")
    exact(y, ref, f"conv3x3_up2 constant {up2_run_id(run)}")


@pytest.mark.parametrize("run", UP2_RUNS, ids=up2_run_id)
def test_conv3x3_up2_selector_weights_within_the_derived_bound(ops, run):
    """The selector family: every output is one interpolated patch value, |y - r| <= ulp16(r) / 2 + 2**-22 max(h, w) amax + 2**-22 amax
    (one rounding to fp16; an fma-contracted src - i0 in either axis; the four-term fp32 sum - derived in _exact.up2_selector_bound,
    checked against two evaluation orders and both coordinate forms in test_exact_inputs.py: worst error 0.98 of the bound there and,
    measured, 0.983 on the device - nearly all of it the rounding to fp16)."""
    case, offset = run
    assert_up2_geometry(case, offset)
    x, sets = up2_selector_data(case)
    for i, (wp, ref, bound) in enumerate(sets):
        what = f"conv3x3_up2 selector {up2_run_id(run)} set {i}"
        y = run_up2(ops, case, x, wp, None, offset, what).double()
        err = (y - ref).abs()
        bad = err > bound
        ratio = float((err / bound).max())
        print(f"{what}: worst error / bound {ratio:.3f}")
        if bool(bad.any()):
            first = bad.nonzero()[0].tolist()
            couts = bad.reshape(-1, bad.shape[-1]).any(0).nonzero().flatten().tolist()
            raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} outputs outside the bound, worst error {float(err.max()):.4g} ({ratio:.1f} bounds), first at {first}: "
                                 f"{float(y[tuple(first)])} for {float(ref[tuple(first)]):.6g}; couts {couts[:6]}..{couts[-1]}")


@pytest.mark.parametrize("case", [c for c in E.UP2_CASES if 9 * c[3] % 64 == 0], ids=E.up2_id)
def test_conv3x3_up2_against_the_unfused_pair(ops, L, case):
    """Real-valued operands, as test_kernels_gpu.py::test_conv3x3_over_fused_2x_upsample: the fused kernel against vda_bilinear_nhwc_f16
    followed by the conv GEMM (default dispatch) - one fp16 ulp of the largest value, fewer than 12 % of the elements differing - and
    against torch at that test's tolerance. The unfused resize itself is pinned exactly by the dyadic tests below."""
    B, h, w, C, N, ldc = case
    H, W = 2 * h, 2 * w
    x = rnd(B, C, h, w, seed=311).to(F16)
    wt, b = rnd(N, C, 3, 3, seed=312, scale=(9 * C) ** -0.5), rnd(N, seed=313)
    xin, wp, bd = guarded(nhwc(x), pad_elems=(w + 2) * C), guarded(pack(wt)), guarded(b)
    y = run_up2(ops, case, xin, wp, bd, 0, f"conv3x3_up2 {E.up2_id(case)}")
    up = F.interpolate(x.float(), size=(H, W), mode="bilinear", align_corners=True).to(F16).float()
    close_finite(y, F.conv2d(up, wt.to(F16).float(), b, padding=1).permute(0, 2, 3, 1), what="conv3x3 over the fused upsample")
    upd = sentinel_out_f16(B * H * W, C, C)
    ops.bilinear_nhwc(xin, upd, B, h, w, H, W, C)
    check_sentinel(upd, B * H * W, C, "bilinear_nhwc")
    two = sentinel_out_f16(B * H * W, N, N)
    L.lib.vda_gemm_set_variant(-1)
    ops.gemm(upd, wp, two, L.EPI_BIAS_F16, M=B * H * W, N=N, K=9 * C, bias=bd, conv=(B, H, W, C, H, W, 1))
    check_sentinel(two, B * H * W, N, "conv GEMM")
    two = two[:B * H * W].cpu().float().reshape(B, H, W, N)
    d = (y.float() - two).abs()
    assert float(d.max()) <= 2.0 ** -9 * max(1.0, float(two.abs().max())), float(d.max())      # one fp16 ulp of the largest value
    assert float((d > 0).float().mean()) < 0.12, "the fused and the unfused path agree bit for bit almost everywhere"


# ---------------------------------------------------------------- vda_depth_tail_f16 with a resize
@functools.lru_cache(maxsize=None)
def tailup_data(case, Cc):
    B, h, w, H, W = case
    inp = E.tailup_inputs(case, Cc)
    b3 = inp.pop("b3")
    ref = E.tailup_ref(case, inp, b3)                     # (asserts the dyadic preconditions)
    return (ref, b3, guarded(h16(nhwc(inp["x"])), pad_elems=(w + 2) * Cc), guarded(pack(inp["w2"])), guarded(inp["b2"]), guarded(inp["w3"]))


def run_tailup(ops, L, case, Cc, variant):
    B, h, w, H, W = case
    ref, b3, x, w2, b2, w3 = tailup_data(case, Cc)
    out = sentinel_out(B * H, W, W)
    what = f"depth tail {E.tailup_id(case)} C={Cc} variant {variant}"
    L.lib.vda_depth_tail_set_variant(variant)
    try:
        ops.depth_tail(x, w2, b2, w3, b3, out, B, h, w, H, W, Cc)
        torch.cuda.synchronize()
        ran = L.lib.vda_depth_tail_last_kernel().decode()
    finally:
        L.lib.vda_depth_tail_set_variant(0)
    assert ran == E.tailup_kernel(case, variant), f"{what}: ran {ran}, the case is written for {E.tailup_kernel(case, variant)}"
    check_sentinel(out, B * H, W, what)
    exact(out[:B * H].reshape(B, H, W), ref, what)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("Cc", E.TAILUP_C)
@pytest.mark.parametrize("case", E.TAILUP_CASES, ids=E.tailup_id)
def test_depth_tail_dyadic_resize_exact(ops, L, case, Cc, variant):
    """Scales in {0, 1/4, 1/2, 1, 3/2, 2}, x in [-3, 3]: every step of bilinear8's packed-fp16 chain, of the MFMA chain and of the
    fp32 epilogue is exact, so the fp32 output equals the fp64 reference bit for bit under the persistent kernel (variant 0, where the
    source region fits 256 pixels) and under depth_tail_kernel<1> (variant 1, and the dispatcher's own fallback)."""
    run_tailup(ops, L, case, Cc, variant)


@pytest.mark.parametrize("variant", [0, 1])
def test_depth_tail_dyadic_resize_more_tiles_than_compute_units(ops, L, variant):
    """The persistent loop's second tile: more 16 x 32 tiles than the device has compute units."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    case = E.tailup_many_tiles_case(ncu)
    B, h, w, H, W = case
    assert B * -(-H // 16) * -(-W // 32) > ncu
    run_tailup(ops, L, case, 32, variant)


def test_depth_tail_dyadic_resize_tile_seams(ops, L):
    """The persistent loop's third and fourth tile: 27 tiles of 16 x 32 on the 8 workgroups of vda_set_max_wgs(8). (The test above keeps
    covering the full grid, where a workgroup has two tiles at the most.)"""
    B, h, w, H, W = case = E.SEAM_TAILUP_CASE
    assert B * -(-H // 16) * -(-W // 32) >= 3 * 8 and E.tailup_kernel(case) == E.TAIL_KERNELS[2]
    with capped(L, 8):
        run_tailup(ops, L, case, 32, 0)


# ---------------------------------------------------------------- vda_bilinear_nhwc_f16 / _f32 at dyadic scales
@functools.lru_cache(maxsize=None)
def bilinear_data(case, Cc):
    inp = E.bilinear_dyadic_inputs(case, Cc)
    return E.bilinear_dyadic_refs(case, inp) + (nhwc(inp["x"]), nhwc(inp["add"]))


@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
@pytest.mark.parametrize("with_add", [False, True], ids=["noadd", "add"])
@pytest.mark.parametrize("Cc", E.BILINEAR_DYADIC_C)
@pytest.mark.parametrize("case", E.TAILUP_CASES, ids=E.tailup_id)
def test_bilinear_nhwc_dyadic_exact(ops, case, Cc, with_add, dtype):
    """The unfused resize on the tail's dyadic geometries: the nested fp32 lerp, the addend and the store are exact (multiples of 1/16
    up to 7), so both dtypes equal the fp64 reference."""
    B, h, w, H, W = case
    up, both, x, add = bilinear_data(case, Cc)
    xd = guarded(x.to(dtype), pad_elems=(w + 2) * Cc)
    ad = guarded(add.to(dtype)) if with_add else None
    out = (sentinel_out_f16 if dtype == F16 else sentinel_out)(B * H * W, Cc, Cc)
    ops.bilinear_nhwc(xd, out, B, h, w, H, W, Cc, add=ad)
    torch.cuda.synchronize()
    what = f"bilinear_nhwc {E.tailup_id(case)} C={Cc}"
    check_sentinel(out, B * H * W, Cc, what)
    exact(out[:B * H * W].reshape(B, H, W, Cc), both if with_add else up, what)
