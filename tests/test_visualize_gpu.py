"""visualize.colorize / vda_depth_vis_u8 (csrc/visualize.hip) on the MI355X: the device's bytes are the host twin colorize_numpy's
bytes and the reference's recorded frames (tests/golden/vis_frames.npz), exactly; no pixel is excluded anywhere.

The kernel peels a head of up to 3 pixels until its output address is a multiple of 4, maps groups of four pixels to whole dwords
with a grid-stride loop over at most 2048 workgroups x 256 threads (one pass = 2^21 pixels), and finishes with up to 3 single
pixels. So the flat sizes are 1, 2, 3 (no whole group), 5, 7 (one group with a head and / or a tail), 5 883 = 3 * 37 * 53 (more
than one workgroup), 2^20 + 3 and 2^21 + 7 (the second is past one pass of the capped grid whatever the head is), each with the
depth starting at pixel offsets 0..3 of a larger buffer and the output at byte offsets 0..3. Every call writes into a buffer
pre-filled with 0xA5 with 64 guard bytes on both sides: nothing outside the output may change."""
import sys
import types

import numpy as np
import pytest
import torch

from _visualize_inputs import (CASES, LARGE_SIZES, ONE_PASS, SMALL_SIZES, SPECIALS_RANGE, case, flat, golden, random_table, specials,
                               specials_levels)

pytestmark = pytest.mark.gpu
FILL, GUARD = 0xA5, 64
FLAT_RANGE = (0.3, 7.3)                  # flat(n) holds both ends for n >= 2; for n = 1 the range is handed in all the same
_twins = {}


def twin_levels(n):
    """The host twin's levels of flat(n) in FLAT_RANGE, computed once per size and shared (colour is table[levels])."""
    from video_depth_anything_amd.visualize import colorize_numpy
    if n not in _twins:
        k = colorize_numpy(flat(n).reshape(1, 1, n), *FLAT_RANGE, grayscale=True).reshape(-1)
        k.setflags(write=False)
        _twins[n] = k
    return _twins[n]


def device_table(table):
    return None if table is None else torch.from_numpy(np.array(table)).cuda()


def run_kernel(depth, minmax, table, depth_off=0, out_off=0):
    """One call of ops.depth_vis: `depth` (numpy, flat) sits at pixel offset depth_off of a larger device buffer, the output at
    byte offset out_off behind GUARD bytes of 0xA5. minmax: a (min, max) pair or a device tensor. Returns the output bytes;
    checked here: the guards on both sides are untouched."""
    from video_depth_anything_amd import ops
    n, ch = depth.size, 1 if table is None else 3
    src = torch.full((n + 8,), float("nan"), dtype=torch.float32, device="cuda")
    src[depth_off:depth_off + n] = torch.from_numpy(np.array(depth)).cuda()
    buf = torch.full((GUARD + out_off + n * ch + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0 and src.data_ptr() % 16 == 0
    if not isinstance(minmax, torch.Tensor):
        minmax = torch.tensor([np.float32(minmax[0]), np.float32(minmax[1])], dtype=torch.float32, device="cuda")
    first = GUARD + out_off
    ops.depth_vis(src[depth_off:depth_off + n], minmax, device_table(table), buf[first:first + n * ch])
    torch.cuda.synchronize()
    whole = buf.cpu().numpy()
    assert (whole[:first] == FILL).all(), "bytes in front of the output were written"
    assert (whole[first + n * ch:] == FILL).all(), "bytes behind the output were written"
    return whole[first:first + n * ch]


def report_difference(got, want, what):
    """Where the bytes differ: printed before the assertion so that a failure says which byte."""
    bad = np.nonzero(got != want)[0]
    if bad.size:
        print(f"{what}: {bad.size} of {want.size} bytes differ, first at {bad[0]} (got {got[bad[0]]}, want {want[bad[0]]}), last at {bad[-1]}")
    return bad.size == 0


@pytest.mark.parametrize("colour", [True, False], ids=["colour", "gray"])
@pytest.mark.parametrize("n", SMALL_SIZES)
def test_flat_sizes_at_every_offset(n, colour):
    table = random_table() if colour else None
    want = table[twin_levels(n)].reshape(-1) if colour else twin_levels(n)
    for depth_off in range(4):
        for out_off in range(4):
            got = run_kernel(flat(n), FLAT_RANGE, table, depth_off, out_off)
            assert report_difference(got, want, f"n={n} depth+{depth_off} out+{out_off}")


@pytest.mark.parametrize("colour", [True, False], ids=["colour", "gray"])
@pytest.mark.parametrize("n", LARGE_SIZES)
def test_large_sizes(n, colour):
    table = random_table() if colour else None
    want = table[twin_levels(n)].reshape(-1) if colour else twin_levels(n)
    for depth_off, out_off in ((0, 0), (1, 3), (3, 1), (2, 2)):
        got = run_kernel(flat(n), FLAT_RANGE, table, depth_off, out_off)
        assert report_difference(got, want, f"n={n} depth+{depth_off} out+{out_off}")
    assert LARGE_SIZES[-1] - 3 > ONE_PASS                                 # past one pass of the grid even with a head of 3


@pytest.mark.parametrize("name", CASES)
def test_fixture_cases(name):
    """Tensor in / tensor out and numpy in / numpy out against the reference's frames, with the range found on each path's own side."""
    from video_depth_anything_amd.visualize import colorize
    g = golden()
    depth = g[f"{name}_depth"]
    x = torch.from_numpy(np.array(depth)).cuda()
    for grayscale, want in ((False, g[f"{name}_colour"]), (True, g[f"{name}_gray"])):
        got = colorize(x, grayscale=grayscale)
        assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == want.shape
        assert report_difference(got.cpu().numpy().reshape(-1), want.reshape(-1), f"case {name} tensor gray={grayscale}")
        got = colorize(depth, grayscale=grayscale)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == want.shape
        assert report_difference(got.reshape(-1), want.reshape(-1), f"case {name} numpy gray={grayscale}")
    one = colorize(x[1], d_min=depth.min(), d_max=depth.max())          # [H,W]: a view that starts 1 961 (or 512, 99) pixels in
    assert tuple(one.shape) == depth.shape[1:] + (3,) and np.array_equal(one.cpu().numpy(), g[f"{name}_colour"][1])


def test_frames_inside_a_video_buffer():
    """Frame by frame from [N,37,53] into [N,37,53,3] and [N,37,53]: frame i starts 1 961 i pixels and 5 883 i / 1 961 i bytes in,
    so frames 1 and 2 are aligned to nothing; each call leaves the other frames' bytes alone."""
    from video_depth_anything_amd import ops
    g = golden()
    depth = g["A_depth"]
    x = torch.from_numpy(np.array(depth)).cuda()
    minmax = torch.tensor([depth.min(), depth.max()], dtype=torch.float32, device="cuda")
    lut = device_table(g["table"])
    colour = torch.full(depth.shape + (3,), FILL, dtype=torch.uint8, device="cuda")
    gray = torch.full(depth.shape, FILL, dtype=torch.uint8, device="cuda")
    for i in (2, 0, 1):
        ops.depth_vis(x[i], minmax, lut, colour[i])
        ops.depth_vis(x[i], minmax, None, gray[i])
        if i == 2:
            assert (colour[:2] == FILL).all() and (gray[:2] == FILL).all()
    assert np.array_equal(colour.cpu().numpy(), g["A_colour"]) and np.array_equal(gray.cpu().numpy(), g["A_gray"])


def test_clamp_constant_and_subnormal():
    from video_depth_anything_amd.visualize import colorize, colorize_numpy
    d = specials()
    gray = run_kernel(d, SPECIALS_RANGE, None, 1, 1)
    for i, k in specials_levels().items():
        assert gray[i] == k, (i, d[i], gray[i], k)
    assert np.array_equal(gray, colorize_numpy(d.reshape(1, 1, -1), *SPECIALS_RANGE, grayscale=True).reshape(-1))
    t = random_table()
    assert np.array_equal(run_kernel(d, SPECIALS_RANGE, t, 2, 3), t[gray].reshape(-1))
    # a constant video, an inverted range and a NaN range: span = 1e-12 and no division by zero
    const = np.full(1961, 3.25, np.float32)
    assert not run_kernel(const, (3.25, 3.25), None).any()
    assert not colorize(torch.from_numpy(const).cuda().reshape(1, 37, 53), grayscale=True).any()
    assert (colorize(const.reshape(1, 37, 53)) == golden()["table"][0]).all()
    three = np.array([1.0, 2.0, 3.0], np.float32)
    assert run_kernel(three, (2.0, 1.0), None).tolist() == [0, 0, 255]
    assert not run_kernel(flat(5883), (np.nan, 1.0), None).any()
    # a subnormal range: the subtraction, the division and the range itself keep their subnormals on both sides
    tiny = np.linspace(0, 1e-39, 257).astype(np.float32).reshape(1, 1, -1)
    want = colorize_numpy(tiny, grayscale=True)
    assert want.max() == 255 and np.unique(want).size > 200
    assert np.array_equal(colorize(torch.from_numpy(tiny).cuda(), grayscale=True).cpu().numpy(), want)


def test_range_from_minmax_accum_on_the_same_stream():
    """The range left on the device by vda_minmax_accum_f32 feeds the mapping with no host round trip: the same bytes as the
    host-supplied range, on a side stream and mixed with a given end."""
    from video_depth_anything_amd import ops
    from video_depth_anything_amd.visualize import colorize, colorize_numpy
    depth = case("A")
    flatd = depth.reshape(-1)
    want = colorize_numpy(depth, grayscale=True).reshape(-1)
    side = torch.cuda.Stream()
    x = torch.from_numpy(np.array(flatd)).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        minmax = torch.tensor([float("inf"), float("-inf")], dtype=torch.float32, device="cuda")
        ops.minmax_accum(x, minmax)
        out = torch.full((flatd.size,), FILL, dtype=torch.uint8, device="cuda")
        ops.depth_vis(x, minmax, None, out)
    side.synchronize()
    assert minmax.cpu().numpy().tolist() == [depth.min(), depth.max()]
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(run_kernel(flatd, (depth.min(), depth.max()), None), want)
    xt = x.reshape(depth.shape)
    for kw in ({}, dict(d_min=depth.min()), dict(d_max=depth.max()), dict(d_min=depth.min(), d_max=depth.max())):
        assert np.array_equal(colorize(xt, grayscale=True, **kw).cpu().numpy().reshape(-1), want), kw
    lo, hi = 1.1, 6.9                                                    # a given range inside the data: both clamps, rounded to float32
    assert np.array_equal(colorize(xt, lo, hi).cpu().numpy(), colorize_numpy(depth, lo, hi))


def test_numpy_in_numpy_out_block_by_block(monkeypatch, tmp_path):
    from video_depth_anything_amd import visualize
    depth = case("A")
    t = random_table()
    want = visualize.colorize_numpy(depth, palette=t)
    np.save(tmp_path / "d.npy", depth)
    mm = np.load(tmp_path / "d.npy", mmap_mode="r")
    for pixels in (1 << 25, 37 * 53, 2 * 37 * 53 + 5):                   # the whole video at once, one frame, two frames at a time
        monkeypatch.setattr(visualize, "_BLOCK_PIXELS", pixels)
        for src in (depth, mm):
            got = visualize.colorize(src, palette=t, device="cuda")
            assert isinstance(got, np.ndarray) and np.array_equal(got, want)
        assert np.array_equal(visualize.colorize(mm, grayscale=True), visualize.colorize_numpy(depth, grayscale=True))


class _Recorder:
    def __init__(self, path, **kwargs):
        self.frames = []
        _Recorder.last = self

    def append_data(self, f):
        self.frames.append(np.array(f))

    def close(self):
        pass


@pytest.mark.parametrize("grayscale", [False, True])
def test_save_video_on_the_device_writes_the_host_bytes(monkeypatch, tmp_path, grayscale):
    from utils import dc_utils
    mod = types.ModuleType("imageio")
    mod.get_writer = _Recorder
    monkeypatch.setitem(sys.modules, "imageio", mod)
    monkeypatch.setattr(dc_utils, "SAVE_BLOCK", 7)
    rng = np.random.default_rng(4)
    depth = (rng.random((17, 20, 28)) * 37.5 + 1.25).astype(np.float32)  # two full blocks and a ragged one
    for palette in (random_table(), None):
        dc_utils.save_video(depth, str(tmp_path / "v.mp4"), is_depths=True, grayscale=grayscale, palette=palette, device="cuda")
        on_device = np.stack(_Recorder.last.frames)
        host_palette = golden()["table"] if palette is None else palette
        dc_utils.save_video(depth, str(tmp_path / "v.mp4"), is_depths=True, grayscale=grayscale, palette=host_palette)
        assert np.array_equal(on_device, np.stack(_Recorder.last.frames))
        assert on_device.shape == depth.shape + (() if grayscale else (3,))


def test_two_runs_are_bit_identical():
    from video_depth_anything_amd import ops
    n = LARGE_SIZES[-1]
    x = torch.from_numpy(np.array(flat(n))).cuda()
    minmax = torch.tensor(FLAT_RANGE, dtype=torch.float32, device="cuda")
    lut = device_table(random_table())
    runs = []
    for _ in range(2):
        out = torch.full((3 * n,), FILL, dtype=torch.uint8, device="cuda")
        ops.depth_vis(x, minmax, lut, out)
        runs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(runs[0], runs[1])
    assert np.array_equal(runs[0].cpu().numpy(), random_table()[twin_levels(n)].reshape(-1))
