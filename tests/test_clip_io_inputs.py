"""CPU side of tests/test_clip_io_gpu.py: the inputs of tests/_clip_io_inputs.py meet the preconditions their equalities rest on
(asserted for every case), the plain numpy restatement of each operation meets the very assertion the GPU test applies to the
kernels (`mismatch`, a comparison of bits, or the derived 1 ulp of `lsq_mismatch`), and the same restatement with one mistake built
in - a twin - fails it in at least one listed case. No threshold here was fitted to what a kernel returns."""
import fractions

import numpy as np
import pytest

import _clip_io_inputs as CI
from _clip_io_inputs import F32, F64, PASS


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(CI.bits(a), CI.bits(b))


# ---------------------------------------------------------------- the assertion itself, and the pass arithmetic
def test_pass_is_the_capped_grid_and_every_wrap_case_goes_beyond_the_passes_it_claims():
    import pathlib
    import re
    src = (pathlib.Path(__file__).resolve().parent.parent / "video_depth_anything_amd" / "csrc" / "resample.hip").read_text()
    cap = re.search(r"inline unsigned capped_grid\(size_t work_items\) \{.*?const size_t cap = (\d+) \* (\d+);", src, re.S)
    assert cap and int(cap.group(1)) * int(cap.group(2)) * 256 == PASS == 1 << 20
    CI.assert_wraps()
    assert dict((w, n) for w, n, _ in CI.WRAP_CASES) == {
        "normalize_u8 n=3": 1058361, "normalize_u8 n=7": 2469509, "gather_normalize_u8": 2469509, "gather_resize_normalize_u8 identity": 2469509,
        "gather_resize_normalize_u8 2x": 1059968, "bilinear_plane": 1315845, "pos_embed_resample 37x74x384": 1051776,
        "pos_embed_resample 91x37x1024": 3448832, "readout_concat": 1401856}
    with pytest.raises(AssertionError, match="not above"):
        CI.assert_wraps([("exactly one pass", PASS, 1)])
    with pytest.raises(AssertionError, match="not above"):
        CI.assert_wraps([("claims two", 2 * PASS - 1, 2)])
    for n in CI.NORMALIZE_N + [len(CI.CLIP_IDX)]:
        seams = {k * PASS for k in range(1, 3)}
        assert not seams & {f * CI.H_CLIP * CI.W_CLIP for f in range(1, n + 1)}, "a frame boundary on a pass seam"


def test_the_assertion_sees_one_bit_one_nan_and_the_guard():
    want = np.arange(1, 9, dtype=F32)
    good = CI.with_guard(want)
    assert CI.mismatch(good, want) is None
    for change in (lambda g: g.__setitem__(3, np.nextafter(g[3], F32(100))), lambda g: g.__setitem__(7, np.nan), lambda g: g.__setitem__(8, 0.0),
                   lambda g: g.__setitem__(0, -g[0])):
        g = good.copy()
        change(g)
        assert CI.mismatch(g, want) is not None
    assert CI.mismatch(good[:-1], want) is not None and CI.mismatch(good.astype(np.float16), want) is not None
    want_nan = want.copy()
    want_nan[2] = np.nan
    g = CI.with_guard(want_nan)
    g[2] = np.array([0x7FC5A5A5], dtype=np.int32).view(F32)[0]                   # another payload
    assert CI.mismatch(g, want_nan) is None, "NaN-ness is compared where the input put a NaN, not the payload"
    assert CI.mismatch(CI.with_guard(want), want_nan) is not None, "a NaN of the input that does not come out is seen"
    assert CI.mismatch(CI.with_guard(np.array([0.0], dtype=F32)), np.array([-0.0], dtype=F32)) is not None, "bits, not values"


# ---------------------------------------------------------------- normalize_u8, gather_normalize_u8
@pytest.fixture(scope="module")
def video():
    return CI.clip_video()


def test_the_normalise_table_is_the_kernels_expression_and_tells_values_apart():
    t = CI.normalize_table()
    assert t.shape == (256, 3) and t.dtype == F32
    for c in range(3):
        assert bool((np.diff(t[:, c]) > 0).all()), "255 distinct steps per channel: a wrong byte is a wrong output"
    v = F32(200) / F32(255)
    assert t[200, 1] == F32((F64(v) - 0.456) / 0.224) and len({float(t[200, c]) for c in range(3)}) == 3


def test_normalize_restated_and_its_twins(video):
    assert sorted(CI.CLIP_IDX) != CI.CLIP_IDX and len(set(CI.CLIP_IDX)) < len(CI.CLIP_IDX) and max(CI.CLIP_IDX) == CI.CLIP_FRAMES - 1
    for n in CI.NORMALIZE_N:
        want = CI.normalize_ref(video[:n])
        assert want.shape == (n, 3, CI.H_CLIP, CI.W_CLIP) and not np.isnan(want).any()
        assert CI.mismatch(CI.with_guard(want), want) is None
        for twin in ("first_pass_only", "neighbour_pixel"):
            assert CI.mismatch(CI.with_guard(CI.normalize_ref(video[:n], twin=twin)), want) is not None, f"{twin} goes unnoticed at n={n}"
    want = CI.normalize_ref(video, CI.CLIP_IDX)
    assert same_bits(want[1], CI.normalize_ref(video[:1])[0]) and same_bits(want[0], want[6]) and same_bits(want[2], want[3])
    for twin in CI.NORMALIZE_TWINS:
        assert CI.mismatch(CI.with_guard(CI.normalize_ref(video, CI.CLIP_IDX, twin=twin)), want) is not None, f"{twin} goes unnoticed in the gather"
    lost = np.isnan(CI.normalize_ref(video[:3], twin="first_pass_only"))
    assert int(lost.sum()) == 3 * (3 * CI.H_CLIP * CI.W_CLIP - PASS) and lost[2].any() and not lost[:2].any(), "only the last frame reaches the second pass at n = 3"
    lost7 = np.isnan(CI.normalize_ref(video[:7], twin="first_pass_only"))
    assert lost7[5].all() and lost7[6].all(), "at n = 7 the third pass (from item 2 PASS, in frame 5) writes the end of frame 5 and frame 6"
    assert 5 * CI.H_CLIP * CI.W_CLIP < 2 * PASS < 6 * CI.H_CLIP * CI.W_CLIP


# ---------------------------------------------------------------- gather_resize_normalize_u8
def test_cubic_coefficients_at_identity_are_exactly_0_1_0_0_and_dyadic_at_the_listed_ratios():
    """The weights of the identity resize are exactly (0, 1, 0, 0) in fp32 - so the resized clip IS the normalised gather for any
    bytes -, and at ratios 2, 4, 1/2, 3/2 every phase is a multiple of 1/4 and the fp32 coefficients equal the fp64 ones."""
    for n in (12, 587, 601):
        c, taps, t = CI.cubic_axis(n, n, F32)
        assert not t.any() and np.array_equal(c, np.tile(np.array([[0], [1], [0], [0]], dtype=F32), (1, n)))
        assert not np.signbit(c).any(), "no -0 among the weights: 0 * v adds +0"
        assert np.array_equal(taps[1], np.arange(n))
    for (H0, W0), (H, W) in CI.RESIZE_EXACT + [(CI.RESIZE_WRAP[:2], CI.RESIZE_WRAP[2:4])]:
        for n_in, n_out in ((H0, H), (W0, W)):
            c32, taps32, t32 = CI.cubic_axis(n_in, n_out, F32)
            c64, taps64, t64 = CI.cubic_axis(n_in, n_out, F64)
            assert float(F32(n_in) / F32(n_out)) in (1.0, 2.0, 4.0, 0.5, 1.5)
            assert np.array_equal(t32 * 4, np.round(t32 * 4)) and np.array_equal(t32.astype(F64), t64) and np.array_equal(taps32, taps64)
            assert np.array_equal(c32.astype(F64), c64) and np.array_equal(c64 * 256, np.round(c64 * 256))
            assert bool((c64.sum(0) == 1.0).all())
    c32, _, t32 = CI.cubic_axis(16, 12, F32)                               # a scale of 4/3 (phases in thirds) is NOT exact: no equality uses it, nor 3/4
    assert not np.array_equal(c32.astype(F64), CI.cubic_axis(16, 12, F64)[0]) and not np.array_equal(t32 * 4, np.round(t32 * 4))
    assert all(float(F32(a[0]) / F32(b[0])) not in (0.75, 4 / 3) for a, b in CI.RESIZE_EXACT)


@pytest.mark.parametrize("case", CI.RESIZE_EXACT, ids=CI.resize_id)
def test_binary_images_resize_exactly_in_any_order_and_the_twins_fail(case):
    """Values in {0, 255}: the fp32 evaluation in the kernel's tap order, in the reverse order and the fp64 evaluation agree bit for
    bit, for every listed input. Each twin fails for at least one input of the case, wherever the case can show it: at identity the
    outer weights are 0 (no border, no half-pixel offset to see), and 16 -> 4 takes taps 4 X .. 4 X + 3, never past the border."""
    (H0, W0), (H, W) = case
    caught = {t: 0 for t in CI.RESIZE_TWINS}
    videos = CI.binary_videos(H0, W0)
    assert len(videos) == 10 and len({p for p in CI.impulse_places(H0, W0)}) == 9
    for name, v in videos:
        assert set(np.unique(v)) <= {0, 255} and v.shape == (3, H0, W0, 3)
        want = CI.resize_ref(v, CI.RESIZE_IDX, H, W, F64)
        fwd, rev = CI.resize_ref(v, CI.RESIZE_IDX, H, W, F32), CI.resize_ref(v, CI.RESIZE_IDX, H, W, F32, reverse=True)
        assert same_bits(fwd, want) and same_bits(rev, want), f"{name}: fp32 is not exact here"
        assert CI.mismatch(CI.with_guard(fwd), want) is None
        for t in CI.RESIZE_TWINS:
            caught[t] += CI.mismatch(CI.with_guard(CI.resize_ref(v, CI.RESIZE_IDX, H, W, F64, twin=t)), want) is not None
    if (H0, W0) == (H, W):
        assert same_bits(CI.resize_ref(videos[0][1], CI.RESIZE_IDX, H, W, F32), CI.normalize_ref(videos[0][1], CI.RESIZE_IDX))
    blind = {((12, 12), (12, 12)): {"border_wrap", "half_pixel"}, ((16, 16), (4, 4)): {"border_wrap"}}.get(case, set())
    assert {t for t, k in caught.items() if not k} == blind, f"a twin goes unnoticed at {CI.resize_id(case)}: {caught}"


def test_every_resize_twin_is_seen_by_an_impulse_where_it_should_be():
    """Border twins are seen by border impulses, the tap base by any, in the 2x upsampling case."""
    (H0, W0), (H, W) = CI.RESIZE_EXACT[3]
    for name, v in CI.binary_videos(H0, W0)[1:]:
        want = CI.resize_ref(v, CI.RESIZE_IDX, H, W)
        assert CI.mismatch(CI.with_guard(CI.resize_ref(v, CI.RESIZE_IDX, H, W, twin="tap_base")), want) is not None, name
        assert CI.mismatch(CI.with_guard(CI.resize_ref(v, CI.RESIZE_IDX, H, W, twin="idx_ignored")), want) is not None, name
        if "(0,0)" in name:
            assert CI.mismatch(CI.with_guard(CI.resize_ref(v, CI.RESIZE_IDX, H, W, twin="border_wrap")), want) is not None, name


def test_identity_resize_equals_the_normalised_gather_for_arbitrary_bytes():
    v = CI.clip_video(4, 37, 41, seed=5)
    for dtype in (F32, F64):
        assert same_bits(CI.resize_ref(v, [3, 0, 3, 1], 37, 41, dtype), CI.normalize_ref(v, [3, 0, 3, 1]))


def test_the_resize_wrap_case_is_exact_too():
    H0, W0, H, W, n = CI.RESIZE_WRAP
    v = CI.resize_wrap_video()
    assert len(CI.RESIZE_WRAP_IDX) == n and set(np.unique(v)) <= {0, 255}
    want = CI.resize_ref(v, CI.RESIZE_WRAP_IDX, H, W, F64)
    assert same_bits(CI.resize_ref(v, CI.RESIZE_WRAP_IDX, H, W, F32), want) and same_bits(CI.resize_ref(v, CI.RESIZE_WRAP_IDX, H, W, F32, reverse=True), want)
    assert n * H * W > PASS and (n - 1) * H * W < PASS, "the second pass starts inside the last frame"
    for t in CI.RESIZE_TWINS:
        assert CI.mismatch(CI.with_guard(CI.resize_ref(v, CI.RESIZE_WRAP_IDX, H, W, twin=t)), want) is not None, t


# ---------------------------------------------------------------- bilinear_plane
def test_bilinear_scales_are_the_dyadic_values_claimed():
    for (h, w, H, W, B), (sy, sx) in CI.BILINEAR_CASES:
        gy, gx = CI.lerp_scale(h, H), CI.lerp_scale(w, W)
        assert gy.dtype == F32 and float(gy) == sy and float(gx) == sx and sy in (0.0, 0.25, 0.5, 1.0, 2.0) and sx in (0.0, 0.25, 0.5, 1.0, 2.0)
        if H > 1:
            assert fractions.Fraction(h - 1, H - 1) == fractions.Fraction(sy)
        if W > 1:
            assert fractions.Fraction(w - 1, W - 1) == fractions.Fraction(sx)
    assert {s for _, ss in CI.BILINEAR_CASES for s in ss} == {0.0, 0.25, 0.5, 2.0} and float(CI.lerp_scale(5, 5)) == 1.0
    assert CI.BILINEAR_CASES[0][0] == CI.BILINEAR_WRAP


@pytest.mark.parametrize("case", CI.BILINEAR_CASES, ids=CI.bilinear_id)
def test_bilinear_integers_interpolate_exactly_fused_or_not(case):
    """fp32 with separate multiplies and adds, fp32 with every multiply-add fused, and fp64 give the same bits: every intermediate is
    a multiple of 1/16 below 1024. No result is -0 (fmaxf(-0, +0) may return either)."""
    h, w, H, W, B = case[0]
    x = CI.bilinear_input(case)
    assert x.shape == (B, h, w) and np.array_equal(x, np.round(x)) and float(np.abs(x).max()) <= 512 and bool((x < 0).any())
    for relu in (False, True):
        want = CI.bilinear_ref(x, H, W, relu, F64)
        assert want.shape == (B, H, W) and not np.isnan(want).any()
        assert np.array_equal(want * 16, np.round(want * 16)) and not (np.signbit(want) & (want == 0)).any()
        for fused in (False, True):
            assert same_bits(CI.bilinear_ref(x, H, W, relu, F32, fused=fused), want), f"relu={relu} fused={fused}"
        assert CI.mismatch(CI.with_guard(want), want) is None
        if relu:
            assert bool((want == 0).any()) and bool((want > 0).any())


def test_every_bilinear_twin_fails_in_at_least_one_case():
    seen = {t: [] for t in CI.BILINEAR_TWINS}
    for case in CI.BILINEAR_CASES:
        h, w, H, W, B = case[0]
        x = CI.bilinear_input(case)
        for relu in (False, True):
            want = CI.bilinear_ref(x, H, W, relu)
            for t in CI.BILINEAR_TWINS:
                if CI.mismatch(CI.with_guard(CI.bilinear_ref(x, H, W, relu, twin=t)), want) is not None:
                    seen[t].append((CI.bilinear_id(case), relu))
    assert all(seen.values()), seen
    assert len(seen["x1_unclamped"]) >= 8, "wx = 0 at the last column: the unclamped read is seen through the NaN behind the last plane"
    assert all(relu for _, relu in seen["relu_first"]) and len(seen["relu_first"]) >= 3
    assert (CI.bilinear_id(CI.BILINEAR_CASES[0]), False) in seen["scale_h_over_H"]


# ---------------------------------------------------------------- readout_concat
@pytest.mark.parametrize("dtype", [np.float16, F32], ids=["f16", "f32"])
def test_readout_restated_and_its_twins(dtype):
    frames, P, D = CI.READOUT_CASE
    tok = CI.readout_input(frames, P, D, dtype)
    assert tok.dtype == dtype and not np.isnan(tok).any()
    want = CI.readout_ref(tok)
    assert want.shape == (frames, P, 2 * D) and want.dtype == dtype
    f, p = 2, 1368
    assert np.array_equal(want[f, p, :D], tok[f, p + 1]) and np.array_equal(want[f, p, D:], tok[f, 0])
    assert CI.mismatch(CI.with_guard(want), want) is None
    for t in CI.READOUT_TWINS:
        assert CI.mismatch(CI.with_guard(CI.readout_ref(tok, twin=t)), want) is not None, t


# ---------------------------------------------------------------- head_out
def test_head_out_sums_are_exact_and_the_twins_fail():
    seen = {t: 0 for t in CI.HEAD_TWINS}
    for rows in CI.HEAD_ROWS:
        for Cpad in CI.HEAD_CPAD:
            x, w = CI.head_inputs(rows, Cpad)
            assert np.isnan(x[:, 32:]).all() and not np.isnan(x[:, :32]).any() and float(np.abs(x[:, :32]).max()) <= 8 and float(np.abs(w).max()) <= 4
            assert np.array_equal(x[:, :32].astype(np.float16).astype(F32), x[:, :32]), "fp16 holds the activations"
            assert 32 * 8 * 4 + CI.HEAD_BIAS < 2 ** 24 and float(CI.HEAD_BIAS).is_integer()
            want = CI.head_ref(x, w, CI.HEAD_BIAS)
            assert bool((want == 0).any()) and bool((want > 0).any()) and np.array_equal(want, np.round(want))
            for order in (np.arange(32), np.arange(31, -1, -1), np.random.default_rng(rows).permutation(32)):
                acc = F32(0)
                for c in order:
                    acc = acc + x[:, c] * w[c]
                assert acc.dtype == F32 and same_bits(np.where(acc + F32(CI.HEAD_BIAS) < 0, F32(0), acc + F32(CI.HEAD_BIAS)), want)
            assert CI.mismatch(CI.with_guard(want), want) is None
            for t in CI.HEAD_TWINS:
                seen[t] += CI.mismatch(CI.with_guard(CI.head_ref(x, w, CI.HEAD_BIAS, twin=t)), want) is not None
    assert seen["no_relu"] == 4 and seen["neighbour_row"] == 4 and seen["pad_channels_read"] == 2, seen
    assert [(4 * r + 255) // 256 for r in CI.HEAD_ROWS] == [1, 2], "both sides of one 256-thread workgroup"


# ---------------------------------------------------------------- stitch_window, affine_clamp
def test_the_restated_stitch_is_the_schedulers_arithmetic():
    """stitch_window_ref applies scheduler._clamped_affine and scheduler.crossfade per the slot table of stitch.hip; the weights are
    stitch.crossfade_weights() (restated here: importing stitch loads the library)."""
    from video_depth_anything_amd import scheduler
    wts = CI.crossfade_weights()
    assert wts.dtype == F32 and wts.shape == (16,) and wts[0] == 1 and wts[7] == 0 and wts[8] == 0 and wts[15] == 1
    step = 1.0 / 7
    assert [float(x) for x in wts[8:]] == [float(F32(x)) for x in [0.0] + [i * step for i in range(1, 7)] + [1.0]]
    for ss in CI.SCALE_SHIFT:
        win, tail = CI.stitch_inputs(257)
        sc, sh = F32(ss[0]), F32(ss[1])
        chunk, new_tail, ref1 = CI.stitch_window_ref(win, ss, tail, wts)
        aff = [None, None] + [scheduler._clamped_affine(win[f], sc, sh) for f in range(2, 32)]
        assert all(a.dtype == F32 for a in aff[2:])
        faded = scheduler.crossfade([tail[j] for j in range(8)], aff[2:10])
        assert all(same_bits(chunk[j], faded[j]) for j in range(8))
        assert all(same_bits(chunk[8 + j], aff[10 + j]) for j in range(14))
        assert all(same_bits(new_tail[j], aff[24 + j]) for j in range(8)) and same_bits(ref1, aff[12])
        assert not np.isnan(chunk).any() and not np.isnan(new_tail).any() and not np.isnan(ref1).any(), "frames 0 and 1 are never read"
    try:
        from video_depth_anything_amd import stitch
    except Exception:           # the library is not built here: the restated weights stand on the lines above
        return
    assert same_bits(stitch.crossfade_weights(), wts)


def test_the_clamp_is_exercised_and_the_fused_affine_differs():
    """(1.7, -0.4) and (-1, 2) make many results negative. The one-rounding affine differs from numpy's two roundings in more than a
    thousand of 4096 elements for (1.7, -0.4) - which is what makes the build's -ffp-contract=off observable. For (1, 0), (0.5, 0.25)
    and (-1, 2) it CANNOT differ: d * 1, d * 0.5 and d * -1 are exact, so both forms round d * scale + shift once (asserted: 0
    differences); those pairs test the clamp and the slots, (1.7, -0.4) the contraction."""
    d = (np.random.default_rng(3).random(4096) * 5).astype(F32)
    for ss, clamps in zip(CI.SCALE_SHIFT, (False, False, True, True)):
        two, one = CI.clamped_affine(d, *ss), CI.clamped_affine(d, *ss, fused=True)
        assert bool(((d * F32(ss[0]) + F32(ss[1])) < 0).any()) == clamps
        differ = int((CI.bits(two) != CI.bits(one)).sum())
        if ss == (1.7, -0.4):
            assert differ > 1000, f"{ss}: {differ} of 4096 differ"
        else:
            assert differ == 0 and np.array_equal((d * F32(ss[0])).astype(F64), d.astype(F64) * ss[0]), "an exact product: one rounding or two, the same"


STITCH_CASES = [(px, ss) for px in CI.STITCH_PX for ss in CI.SCALE_SHIFT]


def test_stitch_restated_meets_the_assertion_and_every_twin_fails():
    wts = CI.crossfade_weights()
    seen = {t: [] for t in CI.STITCH_TWINS}
    for px, ss in STITCH_CASES:
        win, tail = CI.stitch_inputs(px)
        assert np.isnan(win[:2]).all() and not np.isnan(win[2:]).any() and float(win[2:].min()) >= 0 and float(win[2:].max()) < 5
        want = CI.stitch_window_ref(win, ss, tail, wts)
        assert CI.stitch_mismatch([CI.with_guard(w) for w in want], want) is None
        for t in CI.STITCH_TWINS:
            got = CI.stitch_window_ref(win, ss, tail, wts, twin=t)
            if CI.stitch_mismatch([CI.with_guard(g) for g in got], want) is not None:
                seen[t].append((px, ss))
    big = [c for c in STITCH_CASES if c[0] >= 255]                   # (one pixel can clamp to 0 in both frames 12 and 13)
    for t in CI.STITCH_TWINS:
        if t != "fused_affine":                                       # (fused_crossfade: seen at every scale and shift, (1, 0) included)
            assert set(big) <= set(seen[t]) and (t == "fused_crossfade" or len(seen[t]) >= len(STITCH_CASES) - 1), f"{t} goes unnoticed in {sorted(set(STITCH_CASES) - set(seen[t]))}"
    assert {c for c in big if c[1] == (1.7, -0.4)} == set(seen["fused_affine"]) - {(1, (1.7, -0.4))}, "the fused affine: seen for (1.7, -0.4) at every size, and only there"


def test_the_stitch_nan_case_keeps_each_nan_in_its_slot():
    px, ss, pixel = CI.STITCH_NAN_CASE
    win, tail = CI.stitch_inputs(px, nan_pixel=pixel)
    chunk, new_tail, ref1 = CI.stitch_window_ref(win, ss, tail, CI.crossfade_weights())
    assert np.argwhere(np.isnan(chunk)).tolist() == [[3, pixel], [10, pixel]]
    assert np.argwhere(np.isnan(new_tail)).tolist() == [[6, pixel]] and np.flatnonzero(np.isnan(ref1)).tolist() == [pixel]
    clean = CI.stitch_window_ref(*[CI.stitch_inputs(px)[0], ss, tail, CI.crossfade_weights()])
    assert CI.stitch_mismatch([CI.with_guard(g) for g in clean], (chunk, new_tail, ref1)) is not None, "a NaN that does not come out is seen"


def test_affine_clamp_restated_equals_the_tail_of_the_stitch():
    for n in CI.AFFINE_N:
        win, tail = CI.stitch_inputs(n)
        for ss in CI.SCALE_SHIFT:
            want = CI.clamped_affine(win[24:].reshape(-1), *ss)
            assert same_bits(want.reshape(8, n), CI.stitch_window_ref(win, ss, tail, CI.crossfade_weights())[1])
            if n >= 255 and ss == (1.7, -0.4):
                assert CI.mismatch(CI.with_guard(CI.clamped_affine(win[24:].reshape(-1), *ss, fused=True)), want) is not None
            assert bool((want >= 0).all())


# ---------------------------------------------------------------- lsq_scale_shift
def test_lsq_blocks_are_what_the_pass_arithmetic_assumes():
    import pathlib
    import re
    src = (pathlib.Path(__file__).resolve().parent.parent / "video_depth_anything_amd" / "ops.py").read_text()
    assert int(re.search(r"^LSQ_BLOCKS = (\d+)$", src, re.M).group(1)) * 256 == CI.LSQ_PASS == 65536
    assert {n - CI.LSQ_PASS for n in CI.LSQ_N} >= {-1, 0, 1} and max(CI.LSQ_N) > 2 * CI.LSQ_PASS, "both sides of one pass, and a third pass"


@pytest.mark.parametrize("n", CI.LSQ_N)
def test_lsq_model_is_exact_up_to_the_division_and_the_twins_miss_one_ulp(n):
    """Every device sum, product and difference is an integer below 2**53 (asserted inside lsq_model); the model is then within 1 ulp
    of the exactly rounded rational result - in fact equal: the fp64 quotient of exact integers is correctly rounded, the cast rounds
    once more, and 1 ulp covers that double rounding. Every twin misses the bound wherever it applies."""
    pred, target = CI.lsq_inputs(n)
    assert pred.dtype == F32 and float(pred.max()) <= 15 and float(target.max()) <= 31 and float(pred.min()) >= 0 and float(target.min()) >= 0
    assert (pred[n - 1], target[n - 1]) == (15, 0) and (n <= CI.LSQ_PASS or (pred[CI.LSQ_PASS], target[CI.LSQ_PASS]) == (15, 0))
    got = CI.lsq_model(pred, target)
    assert CI.lsq_mismatch(CI.with_guard(got), pred, target) is None
    sc, sh = CI.lsq_exact(pred, target)
    assert sc.denominator != 1 or n == 2, "the fit is not trivially representable"
    for t in CI.LSQ_TWINS:
        if CI.lsq_twin_applies(t, n):
            assert CI.lsq_mismatch(CI.with_guard(CI.lsq_model(pred, target, twin=t)), pred, target) is not None, f"{t} goes unnoticed at n={n}"
    bumped = got.copy()
    bumped[0] = np.nextafter(np.nextafter(bumped[0], F32(9)), F32(9))
    assert CI.lsq_mismatch(CI.with_guard(bumped), pred, target) is not None, "2 ulp pass"
    assert CI.lsq_mismatch(CI.with_guard(got)[:2], pred, target) is not None


def test_lsq_singular_systems_give_exactly_1_0():
    for pred, target in ((np.array([7], dtype=F32), np.array([3], dtype=F32)), (np.full(300, 5, dtype=F32), CI.lsq_inputs(300)[1])):
        assert CI.lsq_exact(pred, target) == (1, 0)
        assert same_bits(CI.lsq_model(pred, target), np.array([1, 0], dtype=F32))


def test_the_exact_fp32_rounding_and_the_ulp_distance():
    q = fractions.Fraction(1, 3)
    assert CI.f32_of_fraction(q) == F32(1 / 3) and CI.f32_of_fraction(-q) == F32(-1 / 3) and CI.f32_of_fraction(fractions.Fraction(0)) == 0
    tie = fractions.Fraction(1) + fractions.Fraction(1, 2 ** 24)             # half way between 1 and 1 + 2**-23: to even
    assert CI.f32_of_fraction(tie) == F32(1) and CI.f32_of_fraction(tie + fractions.Fraction(1, 2 ** 60)) == np.nextafter(F32(1), F32(2))
    assert CI.f32_of_fraction(fractions.Fraction(3) * fractions.Fraction(1, 2 ** 24) + 1) == F32(1 + 2 ** -22)
    one = F32(1)
    assert CI.ordered(np.nextafter(one, F32(2))) - CI.ordered(one) == 1 and CI.ordered(F32(-0.0)) == CI.ordered(F32(0.0)) == 0
    tiny = np.nextafter(F32(0), F32(1))
    assert CI.ordered(tiny) == 1 and CI.ordered(-tiny) == -1
