"""Inputs, case lists and plain numpy restatements for the kernels that bring a clip in and take the depth out, shared by
tests/test_clip_io_inputs.py (CPU: the preconditions hold, the restatements meet the assertion, the twins fail it) and
tests/test_clip_io_gpu.py (GPU: the kernels meet it).

csrc/resample.hip: normalize_u8, gather_normalize_u8, gather_resize_normalize_u8, bilinear_plane, pos_embed_resample, readout_concat,
head_out. csrc/stitch.hip: lsq_scale_shift, stitch_window, affine_clamp.

Every capped_grid kernel of resample.hip launches at most 4096 workgroups of 256 threads: one pass of its grid-stride loop covers PASS
work items and the loop brings the rest. WRAP_CASES lists the calls that go past one pass (or two), with the work items of each.

Each operation is restated once (the reference) and again with a single mistake built in (a "twin"): a twin must fail, in at least one
listed case, the very assertion the GPU test applies - `mismatch`, a comparison of bits - or the test could not see that mistake in a
kernel. The equalities rest on inputs chosen so that fp32 arithmetic is exact in any order, fused or not:

  bicubic gather   values in {0, 255} (0 or 1 after / 255) and size ratios 1, 2, 4, 1/2, 3/2: the phases are multiples of 1/4, every
                   coefficient a multiple of 2**-8, every partial sum a multiple of 2**-16 below 4.
  bilinear_plane   integers in [-512, 512] and (h - 1) / (H - 1) in {0, 1/4, 1/2, 1, 2}: weights are multiples of 1/4, every
                   intermediate a multiple of 1/16 below 1024.
  head_out         |x| <= 8, |w| <= 4 integers: a 32-term sum below 2**24.
  lsq_scale_shift  integer pred and target: every fp64 sum, product and difference is an integer below 2**53, so the fit is one fp64
                   division of exact integers and one cast - within 1 fp32 ulp of the exactly rounded rational result.
  stitch_window, affine_clamp   nothing is exact; the reference is numpy float32 with the operations of scheduler._clamped_affine and
                   scheduler.crossfade, which round the affine step twice. stitch.hip is built with -ffp-contract=off so that the
                   device does too: the fused twin shows that the test sees it if that ever stops.
The CPU file asserts each of these."""
import fractions

import numpy as np

F32, F64 = np.float32, np.float64
NAN = float("nan")

PASS = 4096 * 256       # capped_grid (csrc/resample.hip): at most 256 * 16 workgroups of 256 threads - the work items of one grid pass

MEAN = np.array([0.485, 0.456, 0.406], dtype=F64)
STD = np.array([0.229, 0.224, 0.225], dtype=F64)


# ------------------------------------------------------------------------------------------------ the assertion
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.int16, 4: np.int32}[a.dtype.itemsize])


def with_guard(a):
    """A result as the GPU test reads it back: flat, one guard element (NaN, as the buffer was pre-filled) behind the last output."""
    a = np.ascontiguousarray(a)
    return np.concatenate([a.reshape(-1), np.full(1, NAN, dtype=a.dtype)])


def mismatch(got_with_guard, want):
    """The assertion of every equality here: None, or what is wrong. got_with_guard: the flat output buffer, one element longer than
    `want`, pre-filled with NaN before the launch. The guard keeps its NaN; an output is NaN exactly where `want` is (where the
    input put one: payloads may differ between host and device); every other element has the bits of `want`."""
    want = np.ascontiguousarray(want).reshape(-1)
    got_with_guard = np.ascontiguousarray(got_with_guard).reshape(-1)
    if got_with_guard.dtype != want.dtype or got_with_guard.size != want.size + 1:
        return f"got {got_with_guard.dtype}[{got_with_guard.size}] for {want.dtype}[{want.size}] + 1 guard"
    if not np.isnan(got_with_guard[-1]):
        return "the guard element behind the last output was written"
    got = got_with_guard[:-1]
    gn, wn = np.isnan(got), np.isnan(want)
    if not np.array_equal(gn, wn):
        left, extra = np.flatnonzero(gn & ~wn), np.flatnonzero(~gn & wn)
        return f"{left.size} outputs are NaN (unwritten, or reached by a NaN they must not read), first at {left[:4].tolist()}; {extra.size} lost a NaN of the input"
    bad = np.flatnonzero((bits(got) != bits(want)) & ~wn)
    if bad.size:
        i = int(bad[0])
        return f"{bad.size} of {want.size} outputs differ in bits, first at {i}: got {got[i]!r}, want {want[i]!r}"
    return None


# ------------------------------------------------------------------------------------------------ work items against PASS
H_CLIP, W_CLIP = 601, 587                   # odd sizes: no frame boundary falls on a pass seam
CLIP_FRAMES = 9
CLIP_IDX = [8, 0, 3, 3, 7, 1, 8]            # a repeat, the last frame, not monotone
NORMALIZE_N = [3, 7]
RESIZE_WRAP = (364, 364, 728, 728, 2)       # (H0, W0, H, W, n)
BILINEAR_WRAP = (129, 129, 513, 513, 5)     # (h, w, H, W, B)
POS_EMBED_CASES = [(37, 74, 384), (91, 37, 1024)]       # (ph, pw, D); g = 37. The second: the widest grid max_res 1280 allows at ViT-L width
POS_EMBED_G = 37
READOUT_CASE = (4, 1369, 1024)              # (frames, P, D)

# (what, work items of the launch, whole passes it must go beyond)
WRAP_CASES = [
    ("normalize_u8 n=3", 3 * H_CLIP * W_CLIP, 1),
    ("normalize_u8 n=7", 7 * H_CLIP * W_CLIP, 2),
    ("gather_normalize_u8", len(CLIP_IDX) * H_CLIP * W_CLIP, 2),
    ("gather_resize_normalize_u8 identity", len(CLIP_IDX) * H_CLIP * W_CLIP, 2),
    ("gather_resize_normalize_u8 2x", RESIZE_WRAP[4] * RESIZE_WRAP[2] * RESIZE_WRAP[3], 1),
    ("bilinear_plane", BILINEAR_WRAP[4] * BILINEAR_WRAP[2] * BILINEAR_WRAP[3], 1),
    ("pos_embed_resample 37x74x384", (1 + 37 * 74) * 384, 1),
    ("pos_embed_resample 91x37x1024", (1 + 91 * 37) * 1024, 3),
    ("readout_concat", READOUT_CASE[0] * READOUT_CASE[1] * 2 * (READOUT_CASE[2] // 8), 1),
]


def assert_wraps(cases=WRAP_CASES):
    for what, items, passes in cases:
        assert passes >= 1 and items > passes * PASS, f"{what}: {items} work items are not above {passes} x PASS = {passes * PASS}"


def drop_after_first_pass(out_items_first):
    """Twin of every grid-stride loop: the kernel body without the loop - work items from PASS on are never written (NaN).
    out_items_first: the output arranged with the work item as its first axis."""
    o = np.array(out_items_first, copy=True)
    o[PASS:] = NAN
    return o


# ------------------------------------------------------------------------------------------------ normalize_u8, gather_normalize_u8
def clip_video(frames=CLIP_FRAMES, H=H_CLIP, W=W_CLIP, seed=11):
    return np.random.default_rng(seed).integers(0, 256, (frames, H, W, 3), dtype=np.uint8)


def normalize_table():
    """[256, 3]: float32((float64(float32(v) / float32(255)) - mean) / std)."""
    v = np.arange(256).astype(F32) / F32(255)
    return ((v.astype(F64)[:, None] - MEAN) / STD).astype(F32)


NORMALIZE_TWINS = ["first_pass_only", "neighbour_pixel", "idx_ignored"]


def normalize_ref(video, idx=None, twin=None):
    """uint8 [N, H, W, 3] -> fp32 [n, 3, H, W] of the frames idx (all, in order, without idx), by table.
    Twins: first_pass_only; neighbour_pixel - every value lands one pixel late in its plane; idx_ignored - output frame i reads
    frame i."""
    assert video.dtype == np.uint8 and video.shape[-1] == 3
    if idx is not None and twin != "idx_ignored":
        video = video[np.asarray(idx)]
    elif idx is not None:
        video = video[:len(idx)]
    t = normalize_table()
    n, H, W, _ = video.shape
    out = np.empty((n, 3, H, W), dtype=F32)
    for c in range(3):
        out[:, c] = t[:, c][video[..., c]]
    if twin == "neighbour_pixel":
        out = np.roll(out.reshape(n, 3, H * W), 1, axis=2).reshape(n, 3, H, W)
    if twin == "first_pass_only":
        items = drop_after_first_pass(out.reshape(n, 3, H * W).transpose(0, 2, 1).reshape(n * H * W, 3))
        out = items.reshape(n, H * W, 3).transpose(0, 2, 1).reshape(n, 3, H, W)
    return np.ascontiguousarray(out)


# ------------------------------------------------------------------------------------------------ gather_resize_normalize_u8
# (H0, W0) -> (H, W): ratios 1, 1/2, 1/4, 2, 3/2 of source to destination size
RESIZE_EXACT = [((12, 12), (12, 12)), ((12, 16), (6, 8)), ((16, 16), (4, 4)), ((6, 8), (12, 16)), ((12, 18), (8, 12))]
RESIZE_IDX = [2, 0, 2, 1]
RESIZE_TWINS = ["tap_base", "border_wrap", "idx_ignored", "half_pixel"]


def resize_id(c):
    return "%dx%d-%dx%d" % (c[0] + c[1])


def impulse_places(H0, W0):
    """The four corners, one mid-edge pixel per side, one interior pixel."""
    return [(0, 0), (0, W0 - 1), (H0 - 1, 0), (H0 - 1, W0 - 1), (0, W0 // 2), (H0 - 1, W0 // 2), (H0 // 2, 0), (H0 // 2, W0 - 1), (H0 // 2, W0 // 3)]


def binary_videos(H0, W0, seed=23):
    """[(name, uint8 [3, H0, W0, 3] with values in {0, 255})]: three random frames, and per impulse place a video whose frame k holds
    the impulse in channel k alone (frames differ: a wrong frame is seen)."""
    rng = np.random.default_rng(seed + 131 * H0 + W0)
    out = [("random", (rng.integers(0, 2, (3, H0, W0, 3)) * 255).astype(np.uint8))]
    for y, x in impulse_places(H0, W0):
        v = np.zeros((3, H0, W0, 3), dtype=np.uint8)
        for k in range(3):
            v[k, y, x, k] = 255
        out.append((f"impulse({y},{x})", v))
    return out


def cubic_coeffs(t, dtype):
    """resample.hip's cubic_coeffs (a = -0.75) on an array of phases, every operation in `dtype`."""
    t = t.astype(dtype)
    A, one, two = dtype(-0.75), dtype(1), dtype(2)
    x0, x1, x2, x3 = t + one, t, one - t, two - t
    c0 = ((A * x0 - dtype(5) * A) * x0 + dtype(8) * A) * x0 - dtype(4) * A
    c1 = ((A + two) * x1 - (A + dtype(3))) * x1 * x1 + one
    c2 = ((A + two) * x2 - (A + dtype(3))) * x2 * x2 + one
    c3 = ((A * x3 - dtype(5) * A) * x3 + dtype(8) * A) * x3 - dtype(4) * A
    out = np.stack([c0, c1, c2, c3])
    assert out.dtype == dtype
    return out


def cubic_axis(n_in, n_out, dtype, twin=None):
    """(coefficients [4, n_out], source indices [4, n_out], phases) of one axis: half-pixel centres, taps i - 1 .. i + 2 clamped to the
    border. The scale is the kernel's fp32 quotient."""
    s = dtype(F32(n_in) / F32(n_out))
    d = np.arange(n_out).astype(dtype)
    f = d * s if twin == "half_pixel" else (d + dtype(0.5)) * s - dtype(0.5)
    f0 = np.floor(f)
    t = f - f0
    base = f0.astype(np.int64) - (0 if twin == "tap_base" else 1)
    taps = base[None, :] + np.arange(4)[:, None]
    taps = taps % n_in if twin == "border_wrap" else np.clip(taps, 0, n_in - 1)
    return cubic_coeffs(t, dtype), taps, t


def resize_ref(video, idx, H, W, dtype=F64, reverse=False, twin=None):
    """gather + bicubic resize + normalise: uint8 [N, H0, W0, 3] -> fp32 [n, 3, H, W]. The horizontal pass first, the four taps added
    in order from 0 (in reverse order on request), then (acc - mean) / std in fp64, cast to fp32."""
    assert video.dtype == np.uint8
    idx = np.asarray(idx)
    frames = video[np.arange(len(idx)) % video.shape[0]] if twin == "idx_ignored" else video[idx]
    v = (frames.astype(F32) / F32(255)).astype(dtype)
    n, H0, W0, _ = v.shape
    cx, tx, _ = cubic_axis(W0, W, dtype, twin)
    cy, ty, _ = cubic_axis(H0, H, dtype, twin)
    order = range(3, -1, -1) if reverse else range(4)
    row = np.zeros((n, H0, W, 3), dtype=dtype)
    for b in order:
        row = row + cx[b][None, None, :, None] * v[:, :, tx[b], :]
    acc = np.zeros((n, H, W, 3), dtype=dtype)
    for a in order:
        acc = acc + cy[a][None, :, None, None] * row[:, ty[a]]
    assert acc.dtype == dtype
    return np.ascontiguousarray(((acc.astype(F64) - MEAN) / STD).astype(F32).transpose(0, 3, 1, 2))


def resize_wrap_video(seed=29):
    H0, W0 = RESIZE_WRAP[:2]
    return (np.random.default_rng(seed).integers(0, 2, (3, H0, W0, 3)) * 255).astype(np.uint8)


RESIZE_WRAP_IDX = [2, 0]


# ------------------------------------------------------------------------------------------------ bilinear_plane
# (h, w, H, W, B) and the value of fl32(h - 1) / fl32(H - 1), fl32(w - 1) / fl32(W - 1) each must have (0 where the output has one row / column)
BILINEAR_CASES = [
    ((129, 129, 513, 513, 5), (0.25, 0.25)),
    ((5, 9, 9, 17, 2), (0.5, 0.5)),
    ((9, 17, 5, 9, 2), (2.0, 2.0)),
    ((1, 1, 4, 4, 2), (0.0, 0.0)),
    ((3, 5, 1, 1, 2), (0.0, 0.0)),
    ((2, 7, 1, 13, 2), (0.0, 0.5)),
]
assert BILINEAR_CASES[0][0] == BILINEAR_WRAP
BILINEAR_TWINS = ["scale_h_over_H", "x1_unclamped", "relu_first"]


def bilinear_id(c):
    return "%dx%d-%dx%d-B%d" % c[0]


def bilinear_input(case, seed=31):
    h, w, H, W, B = case[0]
    x = np.random.default_rng(seed + 7 * h + w).integers(-512, 513, (B, h, w)).astype(F32)
    x[0, 0, 0], x[1, 0, 0] = -max(abs(x[0, 0, 0]), 1), max(abs(x[1, 0, 0]), 1)          # the ReLU has something to do in a 1 x 1 plane too
    return x


def lerp_scale(n_in, n_out):
    """resample.hip's lerp_coord: the fp32 quotient, 0 for a single output."""
    return F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0)


def lerp_axis(n_in, n_out, dtype, twin=None, clamp1=True):
    scale = dtype(F32(n_in) / F32(n_out)) if twin == "scale_h_over_H" else dtype(lerp_scale(n_in, n_out))
    src = scale * np.arange(n_out).astype(dtype)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1) if clamp1 else i0 + 1
    return i0, i1, (src - i0.astype(dtype)).astype(dtype)


def bilinear_ref(x, H, W, relu, dtype=F64, fused=False, twin=None):
    """align_corners=True bilinear resize of fp32 planes [B, h, w] -> [B, H, W] as bilinear_plane_kernel writes it:
    top = in[y0, x0] * (1 - wx) + in[y0, x1] * wx, bot likewise, top * (1 - wy) + bot * wy, then the optional ReLU. fused: every
    a * b + c as one fused multiply-add (what the compiler may make of it). The planes are read through a flat view with one NaN
    behind the last plane, as the GPU test lays them out: an index past a row's end reads the neighbour, past the end a NaN."""
    B, h, w = x.shape
    flat = np.concatenate([x.reshape(-1), np.full(1, NAN, dtype=F32)]).astype(dtype)
    if twin == "relu_first" and relu:
        flat = np.where(flat < 0, dtype(0), flat)
    y0, y1, wy = lerp_axis(h, H, dtype, twin)
    x0, x1, wx = lerp_axis(w, W, dtype, twin, clamp1=twin != "x1_unclamped")
    base = (np.arange(B) * h * w)[:, None, None]
    at = lambda yy, xx: flat[base + yy[None, :, None] * w + xx[None, None, :]]      # noqa: E731
    one = dtype(1)
    wx_, wy_ = wx[None, None, :], wy[None, :, None]

    def fma(a, b, c):
        if not fused:
            return a * b + c
        return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(dtype)      # the product of two fp32 values is exact in fp64

    top = fma(at(y0, x1), wx_, at(y0, x0) * (one - wx_))
    bot = fma(at(y1, x1), wx_, at(y1, x0) * (one - wx_))
    o = fma(bot, wy_, top * (one - wy_))
    assert o.dtype == dtype
    if relu and twin != "relu_first":
        o = np.where(o < 0, dtype(0), o)           # fmaxf(o, 0): NaN -> 0 on the device, NaN here - no listed input holds one
    return np.ascontiguousarray(o.astype(F32))


# ------------------------------------------------------------------------------------------------ readout_concat
READOUT_TWINS = ["cls_of_frame_0", "patch_row_without_plus_1", "first_pass_only"]


def readout_input(frames, P, D, dtype, seed=37):
    return np.random.default_rng(seed).standard_normal((frames, P + 1, D), dtype=F32).astype(dtype)


def readout_ref(tok, twin=None):
    """[frames, P + 1, D] (cls token first) -> [frames, P, 2 D] = cat(patch token, the frame's cls token)."""
    frames, P1, D = tok.shape
    P = P1 - 1
    patch = tok[:, :P] if twin == "patch_row_without_plus_1" else tok[:, 1:]
    cls = tok[:1, :1] if twin == "cls_of_frame_0" else tok[:, :1]
    out = np.concatenate([patch, np.broadcast_to(cls, (frames, P, D))], axis=2)
    if twin == "first_pass_only":
        out = drop_after_first_pass(out.reshape(-1, 8)).reshape(frames, P, 2 * D)      # the work item: one 8-element vector
    return np.ascontiguousarray(out)


# ------------------------------------------------------------------------------------------------ head_out
HEAD_ROWS = [64, 65]                        # 4 lanes per row: 256 and 260 threads, both sides of one workgroup
HEAD_CPAD = [32, 64]
HEAD_BIAS = 3.0
HEAD_TWINS = ["pad_channels_read", "no_relu", "neighbour_row"]


def head_inputs(rows, Cpad, seed=41):
    """x [rows, Cpad] integers with |x| <= 8 in the 32 live channels and NaN in the pad channels; w [32] integers, |w| <= 4."""
    rng = np.random.default_rng(seed + rows + Cpad)
    x = np.full((rows, Cpad), NAN, dtype=F32)
    x[:, :32] = rng.integers(-8, 9, (rows, 32))
    return x, rng.integers(-4, 5, 32).astype(F32)


def head_ref(x, w, bias, twin=None):
    """out[r] = max(sum_c x[r, c] w[c] + bias, 0) over the 32 live channels, in Python-exact integers."""
    rows, Cpad = x.shape
    live = x[:, Cpad - 32:] if twin == "pad_channels_read" else x[:, :32]
    if twin == "neighbour_row":
        live = np.roll(live, -1, axis=0)
    s = (live.astype(F64) * w.astype(F64)).sum(1) + bias
    return (s if twin == "no_relu" else np.where(s < 0, 0.0, s)).astype(F32)


# ------------------------------------------------------------------------------------------------ stitch_window, affine_clamp
STITCH_PX = [1, 255, 256, 257, 1029]
SCALE_SHIFT = [(1.0, 0.0), (0.5, 0.25), (1.7, -0.4), (-1.0, 2.0)]
STITCH_NAN_FRAMES = (5, 12, 30)             # -> chunk slot 3, chunk slot 10 and ref1, tail slot 6
STITCH_NAN_CASE = (257, (1.7, -0.4), 200)   # (px, scale_shift, pixel)
AFFINE_N = [1, 255, 256, 257]
STITCH_TWINS = ["fused_affine", "fused_crossfade", "weights_swapped", "frame_off_by_one", "ref1_from_13", "tail_written_first"]


def crossfade_weights():
    """stitch.crossfade_weights(), restated: [1 - w_0 .. 1 - w_7, w_0 .. w_7] with w = 0, 1/7, ..., 6/7, 1 in Python floats, rounded to fp32."""
    step = 1.0 / 7
    w = [0.0] + [i * step for i in range(1, 7)] + [1.0]
    return np.array([1.0 - x for x in w] + w, dtype=F32)


def stitch_inputs(px, nan_pixel=None, seed=43):
    """win [32, px] in [0, 5) with frames 0 and 1 NaN (the kernel must not read them), the previous tail [8, px]."""
    rng = np.random.default_rng(seed + px)
    win = (rng.random((32, px)) * 5).astype(F32)
    win[:2] = NAN
    tail = (rng.random((8, px)) * 5).astype(F32)
    if nan_pixel is not None:
        for f in STITCH_NAN_FRAMES:
            win[f, nan_pixel] = NAN
    return win, tail


def clamped_affine(d, sc, sh, fused=False):
    """scheduler._clamped_affine on float32: out = d * scale + shift (two roundings); out[out < 0] = 0. fused: one rounding."""
    sc, sh = F32(sc), F32(sh)
    out = (d.astype(F64) * F64(sc) + F64(sh)).astype(F32) if fused else d * sc + sh
    assert out.dtype == F32
    out = np.array(out, copy=True)
    out[out < 0] = 0
    return out


def stitch_window_ref(win, scale_shift, tail, wts, twin=None):
    """(chunk [22, px], new tail [8, px], ref1 [px]) of vda_stitch_window_f32, numpy float32:
    chunk[j] = tail[j] * (1 - w_j) + aff(win[2 + j]) * w_j (j < 8); chunk[8 + j] = aff(win[10 + j]) (j < 14); tail[j] = aff(win[24 + j]);
    ref1 = aff(win[12]). The cross-fade reads the OLD tail and rounds both products before it adds them."""
    sc, sh = scale_shift
    shift = 1 if twin == "frame_off_by_one" else 0
    aff = lambda f: clamped_affine(win[(f + shift) % 32], sc, sh, fused=twin == "fused_affine")       # noqa: E731
    px = win.shape[1]
    new_tail = np.stack([aff(24 + j) for j in range(8)])
    old = new_tail if twin == "tail_written_first" else tail
    wa, wb = (wts[8:], wts[:8]) if twin == "weights_swapped" else (wts[:8], wts[8:])
    chunk = np.empty((22, px), dtype=F32)
    for j in range(8):
        if twin == "fused_crossfade":           # a + v * w as one fused multiply-add: what a contracting build makes of the cross-fade
            chunk[j] = ((old[j] * wa[j]).astype(F64) + aff(2 + j).astype(F64) * F64(wb[j])).astype(F32)
        else:
            chunk[j] = old[j] * wa[j] + aff(2 + j) * wb[j]
    for j in range(14):
        chunk[8 + j] = aff(10 + j)
    ref1 = aff(13 if twin == "ref1_from_13" else 12)
    assert chunk.dtype == F32 and new_tail.dtype == F32
    return chunk, new_tail, ref1


def stitch_mismatch(got, want):
    """got / want: (chunk, tail, ref1); got with a guard element each."""
    for name, g, w in zip(("chunk", "tail", "ref1"), got, want):
        bad = mismatch(g, w)
        if bad:
            return f"{name}: {bad}"
    return None


# ------------------------------------------------------------------------------------------------ lsq_scale_shift
LSQ_N = [2, 255, 256, 257, 65535, 65536, 65537, 131075]
LSQ_PASS = 256 * 256                        # ops.LSQ_BLOCKS blocks of 256 threads: the elements of one pass of plane_partial
LSQ_TWINS = ["last_dropped", "element_65536_dropped", "second_pass_twice"]


def lsq_inputs(n, seed=47):
    """Integer-valued pred in [0, 15] and target in [0, 31]; outliers (pred 15, target 0) at n - 1 and, where it exists, at 65536."""
    rng = np.random.default_rng(seed + n)
    pred, target = rng.integers(0, 16, n).astype(F32), rng.integers(0, 32, n).astype(F32)
    for i in (n - 1, LSQ_PASS):
        if 0 <= i < n:
            pred[i], target[i] = 15, 0
    return pred, target


def lsq_sums(pred, target, twin=None):
    """(sum p p, sum p, n, sum p t, sum t) as Python integers. The twins change which elements are counted; n stays the caller's."""
    p, t = pred.astype(np.int64), target.astype(np.int64)
    assert np.array_equal(p, pred) and np.array_equal(t, target), "integers"
    n = len(p)
    w = np.ones(n, dtype=np.int64)
    if twin == "last_dropped":
        w[-1] = 0
    elif twin == "element_65536_dropped":
        w[LSQ_PASS] = 0
    elif twin == "second_pass_twice":
        w[LSQ_PASS:2 * LSQ_PASS] = 2
    return int((w * p * p).sum()), int((w * p).sum()), n, int((w * p * t).sum()), int((w * t).sum())


def lsq_twin_applies(twin, n):
    return n > LSQ_PASS if twin != "last_dropped" else True


def lsq_exact(pred, target):
    """(scale, shift) of the least-squares fit target ~ scale * pred + shift as Fractions; (1, 0) for a singular system."""
    a00, a01, a11, b0, b1 = lsq_sums(pred, target)
    det = a00 * a11 - a01 * a01
    if det == 0:
        return fractions.Fraction(1), fractions.Fraction(0)
    return fractions.Fraction(a11 * b0 - a01 * b1, det), fractions.Fraction(a00 * b1 - a01 * b0, det)


def lsq_model(pred, target, twin=None):
    """The device's arithmetic (reduce64.h solve_2x2 on fp64 sums, cast to fp32) with every intermediate asserted to be an integer
    below 2**53 - so the order of the additions cannot matter and the only roundings are the division and the cast."""
    a00, a01, a11, b0, b1 = lsq_sums(pred, target, twin)
    terms = [a00, a01, a11, b0, b1, a00 * a11, a01 * a01, a11 * b0, a01 * b1, a00 * b1, a01 * b0,
             a00 * a11 - a01 * a01, a11 * b0 - a01 * b1, a00 * b1 - a01 * b0]
    assert all(abs(v) < 2 ** 53 for v in terms), "an fp64 intermediate is not exact"
    det = F64(a00) * F64(a11) - F64(a01) * F64(a01)
    if det == 0.0:
        return np.array([1.0, 0.0], dtype=F32)
    sc = (F64(a11) * F64(b0) - F64(a01) * F64(b1)) / det
    sh = (F64(a00) * F64(b1) - F64(a01) * F64(b0)) / det
    return np.array([sc, sh], dtype=F64).astype(F32)


def f32_of_fraction(q):
    """The fp32 value nearest to the rational q (ties to even)."""
    x = F32(float(q))
    cands = sorted({float(np.nextafter(x, F32(-np.inf))), float(x), float(np.nextafter(x, F32(np.inf)))})
    best = min(cands, key=lambda c: (abs(fractions.Fraction(c) - q), int(bits(np.array([c], dtype=F32))[0]) & 1))
    return F32(best)


def ordered(v):
    """fp32 -> integers in the order of the values: neighbours differ by 1 (-0 and +0 coincide)."""
    b = int(bits(np.array([v], dtype=F32))[0])
    return b if b >= 0 else -(b & 0x7FFFFFFF)


def lsq_mismatch(got_with_guard, pred, target):
    """Within 1 fp32 ulp of float32(exact scale), float32(exact shift); the guard behind the two outputs keeps its NaN."""
    got = np.asarray(got_with_guard).reshape(-1)
    if got.dtype != F32 or got.size != 3 or not np.isnan(got[2]):
        return "scale_shift: wrong buffer, or the guard element was written"
    if np.isnan(got[:2]).any():
        return f"scale_shift = {got[:2].tolist()}"
    for name, g, q in zip(("scale", "shift"), got[:2], lsq_exact(pred, target)):
        want = f32_of_fraction(q)
        d = abs(ordered(g) - ordered(want))
        if d > 1:
            return f"{name} = {g!r} is {d} ulp from float32({float(q)!r}) = {want!r}"
    return None
