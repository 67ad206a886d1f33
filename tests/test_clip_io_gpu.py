"""The kernels that bring a clip in and take the depth out, compared bit for bit with plain references, past the first pass of their
grid-stride loops: csrc/resample.hip (normalize_u8, gather_normalize_u8, gather_resize_normalize_u8, bilinear_plane,
pos_embed_resample, readout_concat, head_out) and csrc/stitch.hip (stitch_window and affine_clamp called directly, lsq_scale_shift
against the exact rational fit).

The inputs, case lists, references and the assertion (`mismatch`) come from tests/_clip_io_inputs.py; tests/test_clip_io_inputs.py
shows on the CPU that each equality is sound (the preconditions hold, fp32 is exact in any order, fused or not) and that the assertion
can fail (every twin - the reference with one mistake built in - fails it). Every output buffer is pre-filled with NaN and carries one
guard element behind the last output: the guard keeps its NaN, no output stays NaN unless the input put one there. Every equality is a
comparison of bits; the two tolerances are the project's own for pos_embed_resample (against the same F.interpolate call) and the derived
1 ulp of lsq_scale_shift. Parity with cv2's own INTER_CUBIC arithmetic stays unpinned: cv2 is not available offline."""
import numpy as np
import pytest
import torch

import _clip_io_inputs as CI
from _clip_io_inputs import F32, PASS
from _exact import guarded
from test_kernels_gpu import ops  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def nan_out(n, dtype=torch.float32):
    """(buffer of n + 1 NaN, its first n elements): the output and one guard element behind it."""
    buf = torch.full((n + 1,), float("nan"), dtype=dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf[:n]


def host(buf):
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_idx(idx):
    return torch.tensor(idx, dtype=torch.int32, device="cuda")


def check(buf, want, what):
    bad = CI.mismatch(host(buf), want)
    assert bad is None, f"{what}: {bad}"


# ---------------------------------------------------------------- A. resample.hip
@pytest.fixture(scope="module")
def clip():
    """The 9-frame uint8 video (host, device) and the normalised gather of CLIP_IDX, computed once."""
    CI.assert_wraps()
    v = CI.clip_video()
    return v, dev(v), CI.normalize_ref(v, CI.CLIP_IDX)


@pytest.mark.parametrize("n", CI.NORMALIZE_N)
def test_normalize_u8_past_one_and_two_passes(ops, clip, n):
    """601 x 587 frames: n = 3 is 1 058 361 pixels (past one pass of 4096 x 256), n = 7 is 2 469 509 (past two). Bit-equal to the
    256 x 3 table float32((float64(float32(v) / float32(255)) - mean) / std) gathered by pixel value."""
    v, v_dev, _ = clip
    H, W = CI.H_CLIP, CI.W_CLIP
    assert n * H * W > (1 if n == 3 else 2) * PASS
    buf, out = nan_out(n * 3 * H * W)
    ops.normalize_u8(v_dev[:n], out, n, H, W)
    check(buf, CI.normalize_ref(v[:n]), f"normalize_u8 n={n}")


def test_gather_normalize_u8_past_two_passes(ops, clip):
    """idx = [8, 0, 3, 3, 7, 1, 8] into the 9-frame video: bit-equal to the table reference of video[idx]."""
    v, v_dev, want = clip
    H, W, n = CI.H_CLIP, CI.W_CLIP, len(CI.CLIP_IDX)
    buf, out = nan_out(n * 3 * H * W)
    ops.gather_normalize_u8(v_dev, dev_idx(CI.CLIP_IDX), out, n, H, W)
    check(buf, want, "gather_normalize_u8")


def test_gather_resize_normalize_u8_at_identity_size_is_the_normalised_gather(ops, clip):
    """(H, W) = (H0, W0): the cubic weights are exactly (0, 1, 0, 0), so for arbitrary bytes the result is bit-equal to
    gather_normalize_u8's (and to the table reference); 2 469 509 outputs, past two passes."""
    v, v_dev, want = clip
    H, W, n = CI.H_CLIP, CI.W_CLIP, len(CI.CLIP_IDX)
    idx = dev_idx(CI.CLIP_IDX)
    buf, out = nan_out(n * 3 * H * W)
    ops.gather_resize_normalize_u8(v_dev, idx, out, n, H, W, H, W)
    buf2, out2 = nan_out(n * 3 * H * W)
    ops.gather_normalize_u8(v_dev, idx, out2, n, H, W)
    torch.cuda.synchronize()
    assert torch.equal(buf[:-1].view(torch.int32), buf2[:-1].view(torch.int32)), "identity resize differs from gather_normalize_u8"
    check(buf, want, "gather_resize_normalize_u8 at identity size")


@pytest.mark.parametrize("case", CI.RESIZE_EXACT, ids=CI.resize_id)
def test_gather_resize_normalize_u8_exact_ratios(ops, case):
    """Ratios 1, 1/2, 1/4, 2, 3/2 on images with values in {0, 255}: random frames, and single-pixel impulses at the four corners, one
    mid-edge pixel per side and one interior pixel. Bit-equal to the fp64 restatement of the definition (a = -0.75, half-pixel centres,
    taps clamped to the border, horizontal pass first, (acc - mean) / std in fp64, cast to fp32): the fp32 evaluation is exact in any
    order here (tests/test_clip_io_inputs.py)."""
    (H0, W0), (H, W) = case
    n = len(CI.RESIZE_IDX)
    idx = dev_idx(CI.RESIZE_IDX)
    for name, v in CI.binary_videos(H0, W0):
        buf, out = nan_out(n * 3 * H * W)
        ops.gather_resize_normalize_u8(dev(v), idx, out, n, H0, W0, H, W)
        check(buf, CI.resize_ref(v, CI.RESIZE_IDX, H, W), f"gather_resize_normalize_u8 {CI.resize_id(case)} {name}")


def test_gather_resize_normalize_u8_past_one_pass(ops):
    """364 x 364 -> 728 x 728, n = 2: 1 059 968 outputs, the second pass starts inside the last frame."""
    H0, W0, H, W, n = CI.RESIZE_WRAP
    assert n * H * W > PASS
    v = CI.resize_wrap_video()
    buf, out = nan_out(n * 3 * H * W)
    ops.gather_resize_normalize_u8(dev(v), dev_idx(CI.RESIZE_WRAP_IDX), out, n, H0, W0, H, W)
    check(buf, CI.resize_ref(v, CI.RESIZE_WRAP_IDX, H, W), "gather_resize_normalize_u8 364 -> 728")


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("case", CI.BILINEAR_CASES, ids=CI.bilinear_id)
def test_bilinear_plane_dyadic_scales(ops, case, relu):
    """Integers in [-512, 512], (h - 1) / (H - 1) in {0, 1/4, 1/2, 2}: bit-equal to the fp64 align-corners definition, whether the
    compiler fuses the multiply-adds or not. (129, 129) -> (513, 513) x 5 is 1 315 845 outputs, past one pass. The planes sit in a
    buffer with NaN on either side: a source index past the last column of the last row reads one."""
    h, w, H, W, B = case[0]
    x = CI.bilinear_input(case)
    buf, out = nan_out(B * H * W)
    ops.bilinear_plane(guarded(torch.from_numpy(x), rows_after=1, pad_elems=4), out, B, h, w, H, W, relu=relu)
    check(buf, CI.bilinear_ref(x, H, W, relu), f"bilinear_plane {CI.bilinear_id(case)} relu={relu}")


@pytest.mark.parametrize("ph,pw,D", CI.POS_EMBED_CASES)
def test_pos_embed_resample_past_one_pass(ops, ph, pw, D):
    """(37, 74, 384): 1 051 776 elements; (91, 37, 1024): 3 448 832, the widest grid max_res 1280 allows at ViT-L width. Reference,
    tolerance and call of test_pos_embed_resample_matches_the_reference_call (F.interpolate with the explicit scale factors,
    rtol = 1e-5, atol = 2e-6); row 0 is a bit-exact copy."""
    import torch.nn.functional as F
    g = CI.POS_EMBED_G
    assert (1 + ph * pw) * D > PASS
    pe = (torch.randn(1 + g * g, D, generator=torch.Generator().manual_seed(80)) * 0.2).float()
    buf, out = nan_out((1 + ph * pw) * D)
    ops.pos_embed_resample(pe.cuda(), out, g, ph, pw, D)
    grid = pe[1:].reshape(1, g, g, D).permute(0, 3, 1, 2)
    sy, sx = float(ph + 0.1) / g, float(pw + 0.1) / g
    ref = F.interpolate(grid, scale_factor=(sy, sx), mode="bicubic", antialias=False)
    assert ref.shape[-2:] == (ph, pw)
    ref = torch.cat((pe[:1], ref.permute(0, 2, 3, 1).reshape(-1, D)), dim=0)
    got = torch.from_numpy(host(buf))
    assert bool(torch.isnan(got[-1])) and not bool(torch.isnan(got[:-1]).any()), "the guard was written, or an output left NaN"
    y = got[:-1].view(1 + ph * pw, D)
    assert torch.equal(y[0].view(torch.int32), pe[0].view(torch.int32)), "row 0 is not a bit-exact copy"
    err = (y.double() - ref.double()).abs()
    tol = 2e-6 + 1e-5 * ref.double().abs()
    assert bool((err <= tol).all()), f"pos-embed bicubic: max err {float(err.max()):.3g}, worst {float((err / tol).max()):.3g} of the tolerance"


@pytest.mark.parametrize("dtype", [np.float16, F32], ids=["f16", "f32"])
def test_readout_concat_past_one_pass(ops, dtype):
    """frames = 4, P = 1369, D = 1024: 1 401 856 eight-element vectors. Bit-equal to cat(patch tokens, the frame's cls token)."""
    frames, P, D = CI.READOUT_CASE
    assert frames * P * 2 * (D // 8) > PASS
    tok = CI.readout_input(frames, P, D, dtype)
    t = torch.from_numpy(tok)
    want = torch.cat((t[:, 1:], t[:, :1].expand(frames, P, D)), dim=2).contiguous().numpy()
    assert CI.mismatch(CI.with_guard(CI.readout_ref(tok)), want) is None, "the restatement is torch.cat"
    buf, out = nan_out(frames * P * 2 * D, torch.float16 if dtype == np.float16 else torch.float32)
    ops.readout_concat(guarded(t.reshape(frames * (P + 1), D), rows_after=1), out, frames, P, D)
    check(buf, want, f"readout_concat {np.dtype(dtype).name}")


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("Cpad", CI.HEAD_CPAD)
@pytest.mark.parametrize("rows", CI.HEAD_ROWS)
def test_head_out_exact_integers(ops, rows, Cpad, dtype):
    """|x| <= 8, |w| <= 4: the 32-term sum is exact in any order. rows = 64 fills one 256-thread workgroup, 65 starts a second; the
    pad channels [32, Cpad) hold NaN. Bit-equal to max(sum + bias, 0) in integers."""
    x, w = CI.head_inputs(rows, Cpad)
    buf, out = nan_out(rows)
    ops.head_out(guarded(torch.from_numpy(x).to(dtype), rows_after=1), dev(w), CI.HEAD_BIAS, out, rows, Cpad)
    check(buf, CI.head_ref(x, w, CI.HEAD_BIAS), f"head_out rows={rows} Cpad={Cpad} {dtype}")


# ---------------------------------------------------------------- B. stitch.hip
def run_stitch(ops, win, ss, tail, wts):
    """One vda_stitch_window_f32 launch on guarded buffers: (chunk, tail, ref1) as host arrays with their guard elements. `tail`
    is updated in place."""
    px = win.shape[1]
    cbuf, chunk = nan_out(22 * px)
    tbuf, t = nan_out(8 * px)
    rbuf, ref1 = nan_out(px)
    t.copy_(dev(tail).reshape(-1))
    ops.stitch_window(dev(win), dev(np.array(ss, dtype=F32)), chunk, t, ref1, px, dev(wts))
    return host(cbuf), host(tbuf), host(rbuf)


@pytest.mark.parametrize("ss", CI.SCALE_SHIFT, ids=lambda s: "sc%g_sh%g" % s)
@pytest.mark.parametrize("px", CI.STITCH_PX)
def test_stitch_window_called_directly(ops, px, ss):
    """px on both sides of one and of four 256-thread workgroups; window frames 0 and 1 are NaN and must not be read; the previous
    tail is random and is replaced in place after the cross-fade has read it. chunk, the new tail and ref1 are bit-equal to numpy
    float32 with the operations of scheduler._clamped_affine and scheduler.crossfade. (1.7, -0.4) rounds the product: a fused
    multiply-add (stitch.hip built without -ffp-contract=off) fails here."""
    from video_depth_anything_amd import stitch
    wts = stitch.crossfade_weights()
    assert np.array_equal(CI.bits(wts), CI.bits(CI.crossfade_weights()))
    win, tail = CI.stitch_inputs(px)
    want = CI.stitch_window_ref(win, ss, tail, wts)
    bad = CI.stitch_mismatch(run_stitch(ops, win, ss, tail, wts), want)
    assert bad is None, f"stitch_window px={px} scale_shift={ss}: {bad}"


def test_stitch_window_keeps_a_nan_in_its_slots_and_nowhere_else(ops):
    """NaN in window frames 5, 12 and 30 at one pixel: it stays NaN in chunk slot 3, in ref1 and chunk slot 10, in tail slot 6, and
    appears nowhere else; every other element keeps its bits."""
    px, ss, pixel = CI.STITCH_NAN_CASE
    wts = CI.crossfade_weights()
    win, tail = CI.stitch_inputs(px, nan_pixel=pixel)
    want = CI.stitch_window_ref(win, ss, tail, wts)
    assert [int(np.isnan(w).sum()) for w in want] == [2, 1, 1]
    bad = CI.stitch_mismatch(run_stitch(ops, win, ss, tail, wts), want)
    assert bad is None, f"stitch_window with NaN inputs: {bad}"


@pytest.mark.parametrize("ss", CI.SCALE_SHIFT, ids=lambda s: "sc%g_sh%g" % s)
@pytest.mark.parametrize("n", CI.AFFINE_N)
def test_affine_clamp_is_the_stitch_s_own_alignment(ops, n, ss):
    """Bit-equal to the numpy restatement, and - applied to window frames 24..31 - to the tail stitch_window leaves for the same
    window: the contract stated beside affine_clamp_kernel."""
    wts = CI.crossfade_weights()
    win, tail = CI.stitch_inputs(n)
    ssd = dev(np.array(ss, dtype=F32))
    for x in (win[24], win[24:]):
        buf, out = nan_out(x.size)
        ops.affine_clamp(dev(x), ssd, out)
        check(buf, CI.clamped_affine(x.reshape(-1), *ss), f"affine_clamp n={x.size} scale_shift={ss}")
    _, tail_after, _ = run_stitch(ops, win, ss, tail, wts)
    assert np.array_equal(CI.bits(host(buf)[:-1]), CI.bits(tail_after[:-1])), "affine_clamp(win[24:32]) differs from the tail stitch_window leaves"


def run_lsq(ops, pred, target):
    buf, ss = nan_out(2)
    ws = torch.full((4 * ops.LSQ_BLOCKS + 1,), float("nan"), dtype=torch.float64, device="cuda")
    ops.lsq_scale_shift(dev(pred), dev(target), ws[:4 * ops.LSQ_BLOCKS], ss)
    got = host(buf)
    assert bool(torch.isnan(ws[-1])), "wrote past the workspace"
    return got


@pytest.mark.parametrize("n", CI.LSQ_N)
def test_lsq_scale_shift_against_the_exact_rational_fit(ops, n):
    """Integer pred in [0, 15] and target in [0, 31], outliers at n - 1 and at 65536: every device sum, product and difference is an
    integer below 2**53, so the only roundings are one fp64 division and the cast - within 1 fp32 ulp of float32 of the exact
    Fraction result. n on both sides of one pass of LSQ_BLOCKS x 256 elements, and past two."""
    assert ops.LSQ_BLOCKS * 256 == CI.LSQ_PASS
    pred, target = CI.lsq_inputs(n)
    bad = CI.lsq_mismatch(run_lsq(ops, pred, target), pred, target)
    assert bad is None, f"lsq_scale_shift n={n}: {bad}"


def test_lsq_scale_shift_singular_systems_give_exactly_1_0(ops):
    """n = 1, and all pred equal: det = 0 exactly, the result is (1, 0)."""
    for pred, target in ((np.array([7], dtype=F32), np.array([3], dtype=F32)), (np.full(300, 5, dtype=F32), CI.lsq_inputs(300)[1])):
        bad = CI.mismatch(run_lsq(ops, pred, target), np.array([1, 0], dtype=F32))
        assert bad is None, f"lsq_scale_shift singular n={len(pred)}: {bad}"
