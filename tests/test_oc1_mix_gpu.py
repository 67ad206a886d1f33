"""GPU: option "oc1_mix" (include/vda.h) - refinenet1's out_conv + output_conv1 over the 2x upsample as one GEMM at half resolution and
the gather-and-add pass vda_oc1_mix_combine_f16.

  kernel path   pack -> GEMM -> combine through the C entries, B = 3 in chunks of 1 and of 2 frames, against the fp64 reference
                (tests/_oc1_mix_ref.py) under a bound derived from the reference's own intermediates, every element inside it:
                    E = 1.25 * 2^-11 * ( sum_{tap, j} a_j (|Wz| |r| + |z_tap|)[s_j] + |ref| ) + 2^-24
                (2^-11 = fp16's unit roundoff, once each for the composed weight, the z sample and the output; 1.25 covers the fp32
                accumulation over at most 256 + 36 terms and the second-order products). The unfused pair (out_conv GEMM, then
                vda_conv3x3_up2_f16) is held against the same reference under the bound of ITS roundings (Wo, p1c, the interpolated
                pixel, W1, the output):
                    E_u = 1.25 * 2^-11 * ( |W1| * interp(|Wo| |r| + |c|) + 2 |W1| * |interp(c)| + |ref| ) + 2^-24     (* = the 3x3 conv)
                Both print their largest err / bound.
  combine       alone on exact inputs: h = w = 1 with small-integer z (all weights 0 or 1) is the integer sum of the inside taps bit
                for bit; NaN in the neighbouring frames' z rows and around the buffer never reaches a frame's output.
  model         the tiny config at features 256: both settings against the fp32 oracle, stage("path_1") equal under either, toggling,
                the handle against the Python engine with the option on, vda_workspace_bytes independent of it.
"""
import numpy as np
import pytest
import torch

import _exact as E
import _oc1_mix_ref as R

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
B = 3
U = 2.0 ** -11

_memo = {}


def case(grid, Fe, Fhp):
    """Operands (fp32 weights, fp16 activations), the fp64 reference and both bounds of one shape, built once for both chunk sizes."""
    key = (grid, Fe, Fhp)
    if key in _memo:
        return _memo[key]
    import torch.nn.functional as Fn
    h, w = grid
    r, W1, Wo, bo, b1 = R.inputs(B, h, w, Fe, Fhp, seed=7 * h + 11 * w + Fe + Fhp)
    W1, Wo, bo, b1 = (a.astype(np.float32) for a in (W1, Wo, bo, b1))                  # what the pack entry is given
    r16 = torch.from_numpy(r).to(F16)
    rd = r16.double().numpy()
    ref, z = R.mix(rd, W1, Wo, bo, b1)
    Wz, _ = R.compose(W1, Wo, bo)
    mag = np.einsum("byxi,toi->byxto", np.abs(rd), np.abs(Wz)) + np.abs(z)
    bound = 1.25 * U * (R.gather(mag) + np.abs(ref)) + 2.0 ** -24
    # the unfused pair's bound, NCHW fp64
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    x = t(rd).permute(0, 3, 1, 2)
    up = lambda a: Fn.interpolate(a, scale_factor=2, mode="bilinear", align_corners=True)
    c = Fn.conv2d(x, t(Wo).reshape(Fe, Fe, 1, 1), t(bo))
    cm = Fn.conv2d(x.abs(), t(Wo).abs().reshape(Fe, Fe, 1, 1)) + c.abs()
    a1 = t(W1).abs()
    bound_u = 1.25 * U * ((Fn.conv2d(up(cm), a1, padding=1) + 2 * Fn.conv2d(up(c).abs(), a1, padding=1)).permute(0, 2, 3, 1).numpy() + np.abs(ref)) + 2.0 ** -24
    d = dict(r16=E.guarded(r16.reshape(B * h * w, Fe), pad_elems=Fe), W1=torch.from_numpy(W1).cuda(), Wo=torch.from_numpy(Wo).cuda(), bo=torch.from_numpy(bo).cuda(),
             b1=torch.from_numpy(b1).cuda(), ref=ref, bound=bound, bound_u=bound_u)
    _memo[key] = d
    return d


def worst(got, ref, bound, what):
    err = np.abs(got - ref)
    ratio = float((err / bound).max())
    i = np.unravel_index(np.argmax(err / bound), err.shape)
    print(f"{what}: max err / bound = {ratio:.3f} at {tuple(int(v) for v in i)} (err {err[i]:.3e}, bound {bound[i]:.3e}, |ref| {abs(ref[i]):.3e})")
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    assert ratio <= 1.0, f"{what}: {int((err > bound).sum())} of {err.size} elements outside the bound, worst err / bound = {ratio:.3f}"
    return ratio


@pytest.mark.parametrize("chunk", [1, 2])
@pytest.mark.parametrize("Fhp", [32, 128])
@pytest.mark.parametrize("Fe", [64, 256])
@pytest.mark.parametrize("grid", R.GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_pack_gemm_combine_against_the_fp64_reference(grid, Fe, Fhp, chunk):
    from video_depth_anything_amd import _lib, ops
    d = case(grid, Fe, Fhp)
    h, w = grid
    ldz = _lib.lib.vda_oc1_mix_ldz(Fhp)                  # z's row as the forward lays it out: 288 at Fhp = 32, 1280 (padded) at Fhp = 128
    assert ldz == {32: 288, 128: 1280}[Fhp]
    wz, bz = ops.fold_oc1_weight(d["W1"], d["Wo"].reshape(Fe, Fe), d["bo"], Fhp)
    assert wz.shape == (ldz, Fe) and bz.shape == (ldz,)
    assert not bool(wz[9 * Fhp:].any()) and not bool(bz[9 * Fhp:].any()), "the padding rows of the composed weight are not zero"
    Mo = B * 4 * h * w
    out = E.sentinel_out_f16(Mo, Fhp, Fhp)
    # one z buffer of `chunk` frames with NaN behind it: a chunk edge falls inside the batch, the last chunk is partial
    z = E.guarded(torch.zeros(chunk * h * w, ldz, dtype=F16), pad_elems=ldz)
    for f0 in range(0, B, chunk):
        nf = min(chunk, B - f0)
        ops.gemm(d["r16"][f0 * h * w:(f0 + nf) * h * w], wz, z, _lib.EPI_BIAS_F16, M=nf * h * w, N=ldz, K=Fe, bias=bz)
        ops.oc1_mix_combine(z, d["b1"], out[f0 * 4 * h * w:(f0 + nf) * 4 * h * w], nf, h, w, Fhp, ldz)
    torch.cuda.synchronize()
    E.check_sentinel(out, Mo, Fhp, "combine")
    got = out[:Mo].cpu().double().numpy().reshape(B, 2 * h, 2 * w, Fhp)
    worst(got, d["ref"], d["bound"], f"oc1_mix {h}x{w} Fe={Fe} Fhp={Fhp} chunk={chunk}")


@pytest.mark.parametrize("Fhp", [32, 128])
@pytest.mark.parametrize("Fe", [64, 256])
@pytest.mark.parametrize("grid", R.GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_unfused_pair_against_the_same_reference(grid, Fe, Fhp):
    from video_depth_anything_amd import _lib, ops
    d = case(grid, Fe, Fhp)
    h, w = grid
    c = torch.empty(B * h * w, Fe, dtype=F16, device="cuda")
    ops.gemm(d["r16"], ops.pack_linear(d["Wo"].reshape(Fe, Fe)), c, _lib.EPI_BIAS_F16, M=B * h * w, N=Fe, K=Fe, bias=d["bo"])
    out = torch.empty(B * 4 * h * w, Fhp, dtype=F16, device="cuda")
    ops.conv3x3_up2(c, ops.pack_conv3x3(d["W1"], Fhp, Fe), d["b1"], out, B, h, w, Fe, Fhp, Fhp)
    torch.cuda.synchronize()
    got = out.cpu().double().numpy().reshape(B, 2 * h, 2 * w, Fhp)
    worst(got, d["ref"], d["bound_u"], f"oc1_fused {h}x{w} Fe={Fe} Fhp={Fhp}")


# ------------------------------------------------------------------------------------------------ the combine kernel alone
@pytest.mark.parametrize("pad", [0, 128], ids=["dense", "padded"])
@pytest.mark.parametrize("Fhp", [32, 96, 128])
def test_combine_of_a_single_pixel_is_the_integer_sum_of_the_inside_taps(Fhp, pad):
    """(padded: z rows of 9 Fhp + 128 channels, NaN in the padding - never read)"""
    from video_depth_anything_amd import ops
    z = E.ints((B, 1, 1, 9, Fhp), -8, 8, seed=Fhp)
    b1 = E.ints((Fhp,), -4, 4, seed=Fhp + 1)
    want = torch.from_numpy(R.gather(z.double().numpy(), b1.double().numpy()))             # |.| <= 76: exact in fp16
    out = E.sentinel_out_f16(B * 4, Fhp, Fhp)
    zp = E.pad_cols(z.reshape(B, 9 * Fhp), 9 * Fhp + pad, F16)
    ops.oc1_mix_combine(E.guarded(zp, pad_elems=9 * Fhp), b1.cuda(), out, B, 1, 1, Fhp, 9 * Fhp + pad)
    torch.cuda.synchronize()
    E.check_sentinel(out, B * 4, Fhp, "combine 1x1")
    assert torch.equal(out[:B * 4].cpu().double().reshape(B, 2, 2, Fhp), want)


@pytest.mark.parametrize("Fhp", [32, 128])
@pytest.mark.parametrize("grid", R.GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_nan_in_the_neighbouring_frames_never_reaches_a_frame(grid, Fhp):
    """Frame 1 of three, frames 0 and 2 all NaN (and NaN around the buffer): frame 1's output is finite and, bit for bit, what the frame
    gives alone."""
    from video_depth_anything_amd import ops
    h, w = grid
    g = torch.Generator().manual_seed(h * 100 + w + Fhp)
    z = torch.full((3, h * w, 9 * Fhp), E.NAN)
    z[1] = torch.randn(h * w, 9 * Fhp, generator=g)
    b1 = torch.randn(Fhp, generator=g).cuda()
    zd = E.guarded(z.to(F16).reshape(3 * h * w, 9 * Fhp), pad_elems=9 * Fhp)
    out3 = E.sentinel_out_f16(3 * 4 * h * w, Fhp, Fhp)
    ops.oc1_mix_combine(zd, b1, out3, 3, h, w, Fhp)
    alone = E.sentinel_out_f16(4 * h * w, Fhp, Fhp)
    ops.oc1_mix_combine(E.guarded(z[1].to(F16), pad_elems=9 * Fhp), b1, alone, 1, h, w, Fhp)
    torch.cuda.synchronize()
    E.check_sentinel(out3, 3 * 4 * h * w, Fhp, "combine, three frames")
    E.check_sentinel(alone, 4 * h * w, Fhp, "combine, one frame")
    mid = out3[4 * h * w:8 * h * w].cpu()
    assert bool(torch.isfinite(mid).all()), f"{int((~torch.isfinite(mid)).sum())} non-finite outputs in the middle frame"
    assert torch.equal(mid, alone[:4 * h * w].cpu())
    want = R.gather(z[1].to(F16).double().numpy().reshape(1, h, w, 9, Fhp), b1.cpu().double().numpy())
    bound = 1.25 * U * (R.gather(np.abs(z[1].to(F16).double().numpy()).reshape(1, h, w, 9, Fhp)) + np.abs(want)) + 2.0 ** -24
    worst(mid.double().numpy().reshape(1, 2 * h, 2 * w, Fhp), want, bound, f"combine alone {h}x{w} Fhp={Fhp}")


def test_entries_refuse_bad_arguments():
    from video_depth_anything_amd import _lib
    lib = _lib.lib
    assert lib.vda_oc1_mix_combine_f16(None, None, None, 1, 1, 1, 32, 288, None) != 0 and b"null" in lib.vda_last_error()
    assert lib.vda_fold_oc1_weight(None, None, None, None, None, 32, 64, 32, 288, None) != 0 and b"null" in lib.vda_last_error()
    z = torch.zeros(288, dtype=F16, device="cuda")
    for bad in (dict(Fhp=36), dict(ldz=280), dict(ldz=292)):                   # Fhp, ldz multiples of 8; ldz >= 9 Fhp
        a = dict(dict(Fhp=32, ldz=288), **bad)
        assert lib.vda_oc1_mix_combine_f16(z.data_ptr(), None, z.data_ptr(), 1, 1, 1, a["Fhp"], a["ldz"], None) != 0 and b"geometry" in lib.vda_last_error(), bad
    assert lib.vda_oc1_mix_frames() >= 1 and lib.vda_oc1_mix_default(256) in (0, 1)
    assert [lib.vda_oc1_mix_ldz(f) for f in (32, 64, 96, 128)] == [288, 576, 864, 1280]


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


def test_model_with_the_option_on_and_off():
    """T = 6 > the chunk of frames, 70 x 98 (refinenet1 on a 20 x 28 grid): both settings against the fp32 oracle under the bound the
    folded-ConvTranspose model case uses (the new arm at most 1.5 x the old arm's rel-L1), stage("path_1") equal, toggling twice, the
    workspace size independent of the option.
    Measured on the MI355X (profiles/r12/oc1_mix/README.txt): e_off = 3.500e-03, e_on = 3.441e-03."""
    from oracle import vda_oracle as O
    m, cfg, sd = wide_tiny()
    x = torch.randn(1, 6, 3, 70, 98, generator=torch.Generator().manual_seed(12))
    ref = O.forward(sd, cfg, x).numpy()
    xd = x.cuda()
    eng = m.engine
    out, stages, ws = {}, {}, {}
    for on in (0, 1, 0, 1):
        eng.set_option("oc1_mix", on)
        ws.setdefault(on, eng.workspace_bytes(1, 6, 70, 98, False))
        d = m.forward(xd, fp32=False).clone()
        st = eng.stage("path_1")[0].clone()
        torch.cuda.synchronize()
        if on in out:
            assert torch.equal(out[on], d), f"oc1_mix={on}: the second forward with that setting differs from the first"
        out[on], stages[on] = d, st
    eng.set_option("oc1_mix", -1)
    assert ws[0] == ws[1], "vda_workspace_bytes depends on the option"
    assert not torch.equal(out[0], out[1]), "the option changes nothing: the case tests nothing"
    assert torch.equal(stages[0], stages[1]), "stage path_1 with the option on differs from the unfused forward's"
    e_off, e_on = rel_l1(out[0].cpu().numpy(), ref), rel_l1(out[1].cpu().numpy(), ref)
    print(f"oc1_mix model case: e_off = {e_off:.4e}, e_on = {e_on:.4e}, rel-L1 between the arms = {rel_l1(out[1].cpu().numpy(), out[0].cpu().numpy()):.4e}")
    assert np.isfinite(out[1].cpu().numpy()).all()
    assert e_on <= 1.5 * e_off, f"mixed {e_on:.3e} against fused {e_off:.3e} (rel-L1 to the fp32 oracle)"


def test_handle_equals_the_python_engine_with_the_option_on():
    m, cfg, sd = wide_tiny()
    py = m.python_engine()
    x = torch.randn(1, 6, 3, 70, 98, generator=torch.Generator().manual_seed(13)).cuda()
    m.engine.set_option("ln_fold", 0)
    m.engine.set_option("oc1_mix", 1)
    py.oc1_mix = True
    try:
        a = m.forward(x, fp32=False).clone()
        st = {}
        b = py.forward(x, stages=st, fp32=False).clone()
        assert torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} elements differ"
        half = torch.empty_like(st["path_1_half"][0])
        m.engine._check_stage_exists("p1c")
        import ctypes as C
        from video_depth_anything_amd import _lib
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert _lib.lib.vda_debug_copy(m.engine._h, b"p1c", C.c_void_p(half.data_ptr()), half.numel() * 2, stream) == 0
        torch.cuda.synchronize()
        assert torch.equal(half, st["path_1_half"][0]), "the rebuilt p1c differs from the engine's"
    finally:
        m.engine.set_option("ln_fold", 1)
        m.engine.set_option("oc1_mix", -1)
