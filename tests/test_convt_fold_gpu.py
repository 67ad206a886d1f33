"""GPU: the folded ConvTranspose2d(k == stride) + 3x3 conv (vda_set_option "convt_fold"; include/vda.h, VDA_EPI_CONVT_FOLD_F16).

  device pack   vda_fold_convt_weight against the reference composer (tests/_convt_fold_ref.py) on small-integer weights: every
                composed weight and bias is an exact integer in fp32 and fp16, so the comparison is bit equality.
  folded GEMM   against the unfused pair (ConvTranspose GEMM, then the 3x3 conv) on operands whose every intermediate and result is
                an integer of magnitude <= 2048 (t, Wt in {-1, 0, 1}, Wr with at most three +-1 per tap and output channel): the
                fp16 l1 of the unfused arm is exact too, so the two arms are equal bit for bit - on both kernel families.
  model         a custom tiny config wide enough for the fold to be active: both settings against the CPU oracle, the stage hook,
                toggling, and the handle against the Python engine.
"""
import numpy as np
import pytest
import torch

import _convt_fold_ref as R
import _exact as E

pytestmark = pytest.mark.gpu

F16, F32, F64 = torch.float16, torch.float32, torch.float64
GRIDS = [(1, 1), (2, 3), (5, 7), (19, 23)]        # (19, 23): 874 rows - row tiles cut image rows, the last tile is partial
CPU_REF_MAX = 5 * 7                               # the fp64 CPU reference of the pair is evaluated up to this grid; beyond it the unfused GPU arm alone
FAMILIES = [pytest.param(0, "gemm_fold_kernel<128, 128>", id="rows128"), pytest.param(5, "gemm8p_kernel<256, 1, 13, 1, 256, false>", id="8phase256")]
BT = 2


@pytest.fixture(scope="module")
def L():
    from video_depth_anything_amd import _lib
    yield _lib
    _lib.lib.vda_gemm_set_variant(-1)


_memo = {}


def case(k, Cin, Fe, grid):
    """Operands, the reference composition and the unfused pair's GPU result of one shape, built once for both kernel families."""
    key = (k, Cin, Fe, grid)
    if key in _memo:
        return _memo[key]
    from video_depth_anything_amd import _lib, ops
    H, W = grid
    t, wt, bt, wr = R.exact_inputs(k, Cin, Fe, BT, H, W, seed=1000 * k + Cin + Fe + 7 * H + W)
    Wc, Bc = R.compose(wt, bt, wr)
    l1 = torch.nn.functional.conv_transpose2d(t, wt, bt, stride=k)
    ref = R.unfused(t, wt, bt, wr, k) if H * W <= CPU_REF_MAX else None
    # exactness: |operand| bounds of every contraction below 2**24, everything stored as fp16 an integer <= 2048
    # (each output sums at most 27 entries of l1 - 9 taps x 3 non-zero weights - so 27 |l1|max bounds every partial sum of the conv)
    bound = torch.nn.functional.conv_transpose2d(t.abs(), wt.abs(), bt.abs(), stride=k) * 27
    E.assert_exact_safe_f16([bound], [l1, R.pack(Wc), R.class_bias(Bc)] + ([ref] if ref is not None else []))
    x = E.guarded(t.permute(0, 2, 3, 1).reshape(BT * H * W, Cin).to(F16), pad_elems=(W + 2) * Cin)
    # the unfused arm, planner's choice of kernels
    wtp, btp = ops.pack_convt(wt.to(F32).cuda(), bt.to(F32).cuda(), Cin)
    l1d = torch.empty(BT * k * H * k * W, Cin, dtype=F16, device="cuda")
    ops.gemm(x, wtp, l1d, _lib.EPI_CONVT_F16, M=BT * H * W, N=k * k * Cin, K=Cin, ldc=Cin, bias=btp, convt=(k, H, W, Cin))
    assert torch.equal(l1d.cpu().double().view(BT, k * H, k * W, Cin).permute(0, 3, 1, 2), l1), "the unfused arm's l1 is not the exact ConvTranspose"
    un = torch.empty(BT * k * H * k * W, Fe, dtype=F16, device="cuda")
    ops.gemm(l1d, ops.pack_conv3x3(wr.to(F32).cuda()), un, _lib.EPI_BIAS_F16, M=BT * k * H * k * W, N=Fe, K=9 * Cin, conv=(BT, k * H, k * W, Cin, k * H, k * W, 1))
    torch.cuda.synchronize()
    d = dict(x=x, wt=wt, bt=bt, wr=wr, Wc=Wc, Bc=Bc, ref=ref, unfused=un.cpu())
    _memo[key] = d
    return d


@pytest.mark.parametrize("Ci,Cip", [(64, 64), (128, 128), (56, 64)], ids=["c64", "c128", "c56pad64"])
@pytest.mark.parametrize("Fe", [64, 256])
@pytest.mark.parametrize("k", [2, 4])
def test_device_pack_equals_the_reference_composer(L, k, Fe, Ci, Cip):
    from video_depth_anything_amd import ops
    _, wt, bt, wr = R.exact_inputs(k, Ci, Fe, 1, 1, 1, seed=31 * k + Ci + Fe)
    Wc, Bc = R.compose(wt, bt, wr)
    want_w, want_b = R.pack(Wc, Cip), R.class_bias(Bc)
    E.assert_exact_safe_f16([R.pack(R.compose(wt.abs(), bt.abs(), wr.abs())[0])], [want_w, want_b])
    assert R.tap_blocks(Wc) == (36 if k == 4 else 16)
    wf, bc = ops.fold_convt_weight(wt.to(F32).cuda(), bt.to(F32).cuda(), wr.to(F32).cuda(), Cip)
    torch.cuda.synchronize()
    assert wf.shape == (k * k * Fe, 9 * Cip) and bc.shape == (k * k, 9, Fe)
    assert torch.equal(wf.cpu(), want_w.to(F16)), f"{int((wf.cpu() != want_w.to(F16)).sum())} folded weights differ"
    assert torch.equal(bc.cpu(), want_b.to(F32)), f"{int((bc.cpu() != want_b.to(F32)).sum())} class biases differ"


@pytest.mark.parametrize("variant,kernel", FAMILIES)
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("Fe", [64, 256])
@pytest.mark.parametrize("Cin", [64, 128])
@pytest.mark.parametrize("k", [2, 4])
def test_folded_gemm_equals_the_unfused_pair(L, k, Cin, Fe, grid, variant, kernel):
    from video_depth_anything_amd import ops
    d = case(k, Cin, Fe, grid)
    H, W = grid
    Mo = BT * k * H * k * W
    wf = R.pack(d["Wc"]).to(F16).cuda()
    bc = R.class_bias(d["Bc"]).to(F32).cuda()
    out = E.sentinel_out_f16(Mo, Fe, Fe)
    L.lib.vda_gemm_set_variant(variant)
    try:
        ops.gemm(d["x"], wf, out, L.EPI_CONVT_FOLD_F16, M=BT * H * W, N=k * k * Fe, K=9 * Cin, ldc=Fe, bias=bc, conv=(BT, H, W, Cin, H, W, 1), convt=(k, H, W, Fe))
        torch.cuda.synchronize()
        assert L.lib.vda_gemm_last_kernel().decode() == kernel
    finally:
        L.lib.vda_gemm_set_variant(-1)
    E.check_sentinel(out, Mo, Fe, "folded GEMM")
    got = out[:Mo].cpu()
    bad = got != d["unfused"]
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} elements differ from the unfused pair (first rows {bad.any(dim=1).nonzero()[:4].flatten().tolist()})"
    if d["ref"] is not None:
        ref = d["ref"].permute(0, 2, 3, 1).reshape(Mo, Fe)
        assert torch.equal(got.double(), ref), "both arms agree but are not the exact result"


def test_only_the_two_families_take_the_folded_mode(L):
    """Every forced variant plans the folded mode on the 8-phase 256 x 256 tile or the 128-row kernel; a dense A operand, a stride or a
    grid that does not match the ConvTranspose's is refused at validation."""
    import ctypes as C
    f = dict(M=2 * 37 * 37, N=16 * 256, K=9 * 256, lda=9 * 256, ldc=256, a_mode=1, epilogue=L.EPI_CONVT_FOLD_F16, cB=2, cH=37, cW=37, cCin=256, cHo=37, cWo=37, cStride=1,
             tK=4, tH=37, tW=37, tCout=256)
    def plan(**kw):
        a, p = L.GemmArgs(**dict(f, **kw)), L.GemmPlan()
        return L.lib.vda_gemm_plan(C.byref(a), 0, 256, 0, C.byref(p)), p
    try:
        for v in E.VARIANTS16:
            L.lib.vda_gemm_set_variant(v)
            rc, p = plan()
            r = p.rec[0]
            assert rc == 0 and p.n == 1 and ((r.family, r.bm, r.bn) in ((L.FAM_128, 128, 128), (L.FAM_8P, 256, 256))) and r.dyn == 0, (v, r.family, r.bm, r.bn)
            assert L.lib.vda_gemm_built(r.family, r.bm, r.bn, r.per_cu, 1, L.EPI_CONVT_FOLD_F16) == 1
    finally:
        L.lib.vda_gemm_set_variant(-1)
    rc, p = plan(M=32 * 37 * 37, cB=32)
    assert rc == 0 and L.launch_name(p.rec[0]) == "gemm8p_kernel<256, 1, 13, 1, 256, false>"
    for fam in range(5):
        for bm, bn in ((0, 32), (0, 64), (128, 64), (192, 128), (192, 256), (192, 384), (256, 128)):
            assert L.lib.vda_gemm_built(fam, bm, bn, 1, 1, L.EPI_CONVT_FOLD_F16) == 0
        assert L.lib.vda_gemm_built(fam, 256, 256, 1, 0, L.EPI_CONVT_FOLD_F16) == 0
    for bad in (dict(a_mode=0), dict(tH=36), dict(tK=1, N=256), dict(N=8 * 256), dict(tCout=252)):
        assert plan(**bad)[0] != 0, bad


# ------------------------------------------------------------------------------------------------ the model
def wide_tiny():
    from video_depth_anything_amd.config import get_config
    from video_depth_anything_amd.video_depth import VideoDepthAnything
    from video_depth_anything_amd.weights import synthetic_state_dict
    cfg = get_config("tiny", features=256, out_channels=(64, 128, 64, 128))
    m = VideoDepthAnything(encoder="tiny", features=cfg.features, out_channels=list(cfg.out_channels))
    sd = synthetic_state_dict(cfg, seed=5)
    m.load_state_dict(sd, strict=True)
    return m.to("cuda").eval(), cfg, sd


def rel_l1(y, ref):
    y, ref = np.asarray(y, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(y - ref).mean() / max(np.abs(ref).mean(), 1e-12))


def test_model_with_the_fold_on_and_off():
    """T = 2, 70 x 98: the 5 x 7 grid's rn1 / rn2 convs (256 wide) run on the 128-row kernel, so both levels fold.
    Measured on the MI355X (profiles/r11/convt_fold/README.txt): e_off = 4.985e-03, e_on = 4.741e-03."""
    from oracle import vda_oracle as O
    m, cfg, sd = wide_tiny()
    x = torch.randn(1, 2, 3, 70, 98, generator=torch.Generator().manual_seed(12))
    ref = O.forward(sd, cfg, x).numpy()
    xd = x.cuda()
    eng = m.engine
    out, stages = {}, {}
    for on in (0, 1, 0, 1):                                         # (toggling between forwards, twice)
        eng.set_option("convt_fold", on)
        d = m.forward(xd, fp32=False).clone()
        st = {n: eng.stage(n)[0].clone() for n in ("layer_1", "layer_2")}
        torch.cuda.synchronize()
        if on in out:
            assert torch.equal(out[on], d), f"convt_fold={on}: the second forward with that setting differs from the first"
        out[on], stages[on] = d, st
    eng.set_option("convt_fold", -1)
    assert not torch.equal(out[0], out[1]), "the fold is not active at this width: the case tests nothing"
    for n in ("layer_1", "layer_2"):
        assert torch.equal(stages[0][n], stages[1][n]), f"stage {n} with the fold on differs from the unfused forward's"
    e_off, e_on = rel_l1(out[0].cpu().numpy(), ref), rel_l1(out[1].cpu().numpy(), ref)
    print(f"convt_fold model case: e_off = {e_off:.4e}, e_on = {e_on:.4e}, rel-L1 between the arms = {rel_l1(out[1].cpu().numpy(), out[0].cpu().numpy()):.4e}")
    assert e_on <= 1.5 * e_off, f"folded {e_on:.3e} against unfused {e_off:.3e} (rel-L1 to the fp32 oracle)"


def test_handle_equals_the_python_engine_with_the_fold_on():
    m, cfg, sd = wide_tiny()
    py = m.python_engine()
    x = torch.randn(1, 2, 3, 70, 98, generator=torch.Generator().manual_seed(13)).cuda()
    m.engine.set_option("ln_fold", 0)
    m.engine.set_option("convt_fold", 1)
    py.convt_fold = True
    try:
        a = m.forward(x, fp32=False).clone()
        st = {}
        b = py.forward(x, stages=st, fp32=False).clone()
        assert py._fold_level(0, 2, 5, 7, 64, 256) and py._fold_level(1, 2, 5, 7, 128, 256), "the engine did not fold: the case tests nothing"
        assert torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} elements differ"
        for n in ("layer_1", "layer_2"):
            assert torch.equal(m.engine.stage(n)[0], st[n][0].reshape(m.engine.stage(n)[0].shape)), n
    finally:
        m.engine.set_option("ln_fold", 1)
        m.engine.set_option("convt_fold", -1)
