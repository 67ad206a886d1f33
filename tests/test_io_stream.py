"""save_video block by block (utils/dc_utils.py) and the growing depth file of run.py --stream: the bytes written are those of the
whole-array mapping."""
import os

import numpy as np
import pytest

from utils import dc_utils
from utils.dc_utils import save_video


def whole_array_vis(depth, grayscale):
    """What save_video computed before it worked block-wise (the reference's dc_utils.py:75-83 on the whole array)."""
    d_min, d_max = depth.min(), depth.max()
    norm = ((depth - d_min) / max(float(d_max - d_min), 1e-12) * 255).astype(np.uint8)
    return norm if grayscale else dc_utils._inferno(norm)


@pytest.mark.parametrize("grayscale", [False, True])
def test_blockwise_depth_video_writes_the_same_bytes(tmp_path, monkeypatch, grayscale):
    pytest.importorskip("PIL")
    try:
        import imageio  # noqa: F401
        pytest.skip("an H.264 encoder is installed: the GIF path is not taken")
    except ImportError:
        pass
    from PIL import Image
    rng = np.random.default_rng(4)
    depth = (rng.random((75, 20, 28)) * 37.5 + 1.25).astype(np.float32)          # 75 frames: two full blocks and a ragged one
    vis = whole_array_vis(depth, grayscale)
    ims = [Image.fromarray(f) for f in vis]
    want = str(tmp_path / "want.gif")
    ims[0].save(want, save_all=True, append_images=ims[1:], duration=200, loop=0)
    got = save_video(depth, str(tmp_path / "got.mp4"), fps=5, is_depths=True, grayscale=grayscale)
    assert got.endswith(".gif") and open(got, "rb").read() == open(want, "rb").read()
    # the range handed in, a memory map as the source, another block size
    np.save(tmp_path / "d.npy", depth)
    mm = np.load(tmp_path / "d.npy", mmap_mode="r")
    monkeypatch.setattr(dc_utils, "SAVE_BLOCK", 7)
    got2 = save_video(mm, str(tmp_path / "got2.mp4"), fps=5, is_depths=True, grayscale=grayscale, d_min=depth.min(), d_max=depth.max())
    assert open(got2, "rb").read() == open(want, "rb").read()


def test_growing_depth_file_is_a_valid_npy(tmp_path):
    from run import GrowingNpy
    rng = np.random.default_rng(5)
    pieces = [rng.random((c, 6, 9)).astype(np.float32) for c in (24, 22, 22, 3)]
    path = str(tmp_path / "x_depths.npy")
    g = GrowingNpy(path)
    for p in pieces:
        g.append(p)
    mm = g.close()
    assert isinstance(mm, np.memmap) and mm.shape == (71, 6, 9) and mm.dtype == np.float32
    assert np.array_equal(np.load(path), np.concatenate(pieces))
    assert os.path.getsize(path) == 128 + 71 * 6 * 9 * 4
