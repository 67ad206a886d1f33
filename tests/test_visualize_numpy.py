"""visualize.colorize_numpy, the host twin of csrc/visualize.hip, against the frames the reference's save_video handed to its writer
(tests/golden/vis_frames.npz, made by tools/gen_vis_golden.py), and save_video's palette keyword: no GPU needed, byte equality
everywhere."""
import sys
import types

import numpy as np
import pytest

from _visualize_inputs import CASES, SPECIALS_RANGE, case, flat, golden, random_table, specials, specials_levels
from utils import dc_utils
from utils.dc_utils import save_video
from video_depth_anything_amd import visualize
from video_depth_anything_amd.visualize import colorize_numpy, inferno_table


@pytest.mark.parametrize("name", CASES)
def test_fixture_inputs_are_the_shared_builders(name):
    assert np.array_equal(golden()[f"{name}_depth"].view(np.uint32), case(name).view(np.uint32))


@pytest.mark.parametrize("name", CASES)
def test_twin_reproduces_the_reference_frames(name):
    g = golden()
    depth = g[f"{name}_depth"]
    colour, gray = colorize_numpy(depth, palette=g["table"]), colorize_numpy(depth, grayscale=True)
    assert colour.dtype == np.uint8 and colour.shape == depth.shape + (3,) and np.array_equal(colour, g[f"{name}_colour"])
    assert gray.dtype == np.uint8 and gray.shape == depth.shape and np.array_equal(gray, g[f"{name}_gray"])
    assert np.array_equal(colorize_numpy(depth), g[f"{name}_colour"])                 # the default palette is the reference's
    # the range handed in instead of found; one frame at a time with the video's range
    assert np.array_equal(colorize_numpy(depth, d_min=depth.min(), d_max=depth.max()), g[f"{name}_colour"])
    one = colorize_numpy(depth[1], d_min=depth.min(), d_max=depth.max())
    assert one.shape == depth.shape[1:] + (3,) and np.array_equal(one, g[f"{name}_colour"][1])


def test_shipped_table_is_the_reference_table():
    t = inferno_table()
    assert t.dtype == np.uint8 and t.shape == (256, 3) and not t.flags.writeable
    assert np.array_equal(t, golden()["table"])


def test_shipped_table_is_matplotlibs():
    matplotlib = pytest.importorskip("matplotlib")
    colors = np.array(matplotlib.colormaps["inferno"].colors)
    assert np.array_equal(inferno_table(), (colors * 255).astype(np.uint8))


def test_boundary_ramp_uses_every_row():
    gray = colorize_numpy(case("B"), grayscale=True)
    assert np.array_equal(np.unique(gray), np.arange(256))
    assert (case("B")[gray == 255] == 255).all()


def test_clamp_rules():
    d = specials()
    gray = colorize_numpy(d.reshape(1, 1, -1), *SPECIALS_RANGE, grayscale=True).reshape(-1)
    for i, k in specials_levels().items():
        assert gray[i] == k, (i, d[i], gray[i], k)
    inside = np.isfinite(d) & (d >= 1) & (d <= 3)
    want = ((d[inside] - np.float32(1)) / np.float32(2) * np.float32(255)).astype(np.uint8)    # numpy is defined here
    assert np.array_equal(gray[inside], want)
    t = random_table()
    assert np.array_equal(colorize_numpy(d.reshape(1, 1, -1), *SPECIALS_RANGE, palette=t).reshape(-1, 3), t[gray])
    # a range given as Python floats is rounded to float32: 0.1 and 0.7 are not float32 values
    x = flat(5883).reshape(3, 37, 53)
    assert np.array_equal(colorize_numpy(x, 0.1, 0.7, grayscale=True), colorize_numpy(x, np.float32(0.1), np.float32(0.7), grayscale=True))
    # NaN as the range: every pixel 0
    assert not colorize_numpy(x, np.nan, 1.0, grayscale=True).any()


def test_constant_video_maps_to_zero():
    d = np.full((2, 5, 7), 3.25, np.float32)
    assert not colorize_numpy(d, grayscale=True).any()
    assert (colorize_numpy(d) == inferno_table()[0]).all()
    # an inverted range is no range either: span = 1e-12, everything below d_min is 0 and everything above is 255
    g = colorize_numpy(np.array([[1.0, 2.0, 3.0]], np.float32), 2.0, 1.0, grayscale=True)
    assert g.tolist() == [[0, 0, 255]]


def test_refusals():
    with pytest.raises(ValueError, match="float32"):
        colorize_numpy(np.zeros((1, 2, 3), np.float64))
    with pytest.raises(ValueError, match="float32"):
        colorize_numpy(np.zeros((1, 2, 3), np.float16))
    with pytest.raises(ValueError, match=r"\[N,H,W\]"):
        colorize_numpy(np.zeros((2, 2, 2, 2), np.float32))
    with pytest.raises(ValueError, match="not empty"):
        colorize_numpy(np.zeros((0, 2, 3), np.float32))
    with pytest.raises(ValueError, match="palette"):
        colorize_numpy(np.zeros((1, 2, 3), np.float32), palette=np.zeros((256, 4), np.uint8))
    with pytest.raises(ValueError, match="palette"):
        colorize_numpy(np.zeros((1, 2, 3), np.float32), palette=np.zeros((256, 3), np.float32))


def test_result_does_not_depend_on_the_block_size(monkeypatch, tmp_path):
    depth = case("A")
    want = colorize_numpy(depth)
    for pixels in (1, 37 * 53, 2 * 37 * 53 + 5):                                       # one frame, one frame, two frames at a time
        monkeypatch.setattr(visualize, "_BLOCK_PIXELS", pixels)
        assert np.array_equal(colorize_numpy(depth), want)
    np.save(tmp_path / "d.npy", depth)
    assert np.array_equal(colorize_numpy(np.load(tmp_path / "d.npy", mmap_mode="r")), want)   # a memory map as the source


class _Recorder:
    def __init__(self, path, **kwargs):
        self.frames = []
        _Recorder.last = self

    def append_data(self, f):
        self.frames.append(np.array(f))

    def close(self):
        pass


@pytest.fixture
def recorded(monkeypatch):
    """A stand-in imageio whose writer keeps the frames save_video hands it: no encoder stands between the mapping and the test."""
    mod = types.ModuleType("imageio")
    mod.get_writer = _Recorder
    monkeypatch.setitem(sys.modules, "imageio", mod)
    return lambda: np.stack(_Recorder.last.frames)


@pytest.mark.parametrize("grayscale", [False, True])
def test_save_video_with_a_palette_writes_table_of_norm(recorded, monkeypatch, tmp_path, grayscale):
    g = golden()
    for name in CASES:
        depth = g[f"{name}_depth"]
        assert save_video(depth, str(tmp_path / "v.mp4"), fps=5, is_depths=True, grayscale=grayscale, palette=inferno_table()).endswith(".mp4")
        assert np.array_equal(recorded(), g[f"{name}_gray" if grayscale else f"{name}_colour"])
    # 75 frames: two full blocks and a ragged one; another block size; a memory map; the range handed in; another table
    rng = np.random.default_rng(4)
    depth = (rng.random((75, 20, 28)) * 37.5 + 1.25).astype(np.float32)
    t = random_table()
    want = colorize_numpy(depth, grayscale=grayscale, palette=t)
    save_video(depth, str(tmp_path / "v.mp4"), is_depths=True, grayscale=grayscale, palette=t)
    assert np.array_equal(recorded(), want)
    np.save(tmp_path / "d.npy", depth)
    monkeypatch.setattr(dc_utils, "SAVE_BLOCK", 7)
    save_video(np.load(tmp_path / "d.npy", mmap_mode="r"), str(tmp_path / "v.mp4"), is_depths=True, grayscale=grayscale, palette=t,
               d_min=depth.min(), d_max=depth.max())
    assert np.array_equal(recorded(), want)


def test_save_video_gif_with_a_palette_reads_back(tmp_path):
    """Without an encoder save_video writes a GIF; a gray GIF of one frame is lossless (256 gray levels are its whole palette)."""
    Image = pytest.importorskip("PIL.Image")
    try:
        import imageio  # noqa: F401
        pytest.skip("an H.264 encoder is installed: the GIF path is not taken")
    except ImportError:
        pass
    depth = case("B")[:1]
    path = save_video(depth, str(tmp_path / "g.mp4"), is_depths=True, grayscale=True, palette=inferno_table(), d_min=0.0, d_max=255.0)
    assert path.endswith(".gif")
    back = np.asarray(Image.open(path).convert("L"))
    assert np.array_equal(back, golden()["B_gray"][0])


@pytest.mark.parametrize("grayscale", [False, True])
def test_default_save_video_is_the_polynomial_path(recorded, tmp_path, grayscale):
    depth = case("A")
    norm = ((depth - depth.min()) / max(float(depth.max() - depth.min()), 1e-12) * 255).astype(np.uint8)
    save_video(depth, str(tmp_path / "v.mp4"), is_depths=True, grayscale=grayscale)
    assert np.array_equal(recorded(), norm if grayscale else dc_utils._inferno(norm))
    if not grayscale:
        assert not np.array_equal(recorded(), golden()["A_colour"])                   # which is not the reference's colour map
    # frames that are no depth pass through whatever the new keywords say
    rgb = np.random.default_rng(1).integers(0, 256, (3, 4, 5, 3), dtype=np.uint8)
    save_video(rgb, str(tmp_path / "v.mp4"), palette=inferno_table())
    assert np.array_equal(recorded(), rgb)
