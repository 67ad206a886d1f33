"""scale.resize_frames / vda_resize_linear_u8 (csrc/resize_u8.hip) on the MI355X: the device's bytes are the host twin
resize_frames_numpy's on every shape, for gray and RGB frames, three frames that differ (plane indexing).

A thread owns four consecutive bytes of an output row and a workgroup RU8_TILE of them (read from the kernel's source), stored as
dwords when the base is 4-aligned and a row is a multiple of 4 bytes and byte by byte otherwise; the source is staged through LDS a
group of 8 output rows at a time when it is 4-aligned with rows of a multiple of 4 bytes and the group's part fits, in groups of 4,
2 or 1 rows when only that fits, and read from global memory otherwise. So the shapes take: output rows of 93 / 31 bytes (no
multiple of 4: byte stores with a ragged last thread), 60 / 20 (dwords), source rows of 159 / 53 bytes (not staged) and 120 / 40
(staged), a single row and a single column, a 3 x reduction (groups of 4 rows) and a 100 x reduction (nothing fits), more groups
than the grid has rows of workgroups, widths one pixel under, at and over a workgroup's tile and an exact multiple of it, bases
offset by 1, 2 and 3 bytes - both, and the output alone - up- and downscaling, and one frame of the size the kernel is for. Then the
readers of utils.dc_utils on an .avi and an .npy that are scaled and thinned, and run.py on that .avi, plain and with --stream."""
import os
import re

import numpy as np
import pytest
import torch

from _resize_u8_inputs import clip, frames

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = int(re.search(r"constexpr int RU8_TILE = (\d+);", open(os.path.join(REPO, "video_depth_anything_amd", "csrc", "resize_u8.hip")).read()).group(1))
SHAPES = [((37, 53), (23, 31)), ((64, 40), (32, 20)), ((5, 7), (10, 14)), ((1, 1), (3, 3)), ((9, 40), (1, 27)), ((40, 9), (27, 1)), ((37, 53), (37, 53)),
          ((96, 1200), (32, 400)), ((300, 2400), (3, 24)), ((90000, 4), (180000, 1))]
_twins = {}


def twin(n, src, dst, c):
    """The host twin's result, computed once per case and shared."""
    from video_depth_anything_amd.scale import resize_frames_numpy
    key = (n, src, dst, c)
    if key not in _twins:
        _twins[key] = resize_frames_numpy(frames(n, *src, c), *dst)
    return _twins[key]


def report_difference(got, want, what):
    bad = np.argwhere(got != want)
    if bad.size:
        print(f"{what}: {bad.shape[0]} of {want.size} bytes differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}, "
              f"worst {np.abs(got.astype(int) - want.astype(int)).max()}")


def check(n, src, dst, c):
    from video_depth_anything_amd.scale import resize_frames
    x, want = frames(n, *src, c), twin(n, src, dst, c)
    out = resize_frames(torch.from_numpy(x).cuda(), *dst)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == want.shape
    got = out.cpu().numpy()
    report_difference(got, want, f"{src} -> {dst} x {c}")
    assert np.array_equal(got, want)
    return x, want


@pytest.mark.parametrize("c", [1, 3], ids=["gray", "rgb"])
@pytest.mark.parametrize("src,dst", SHAPES, ids=[f"{s[0]}x{s[1]}to{d[0]}x{d[1]}" for s, d in SHAPES])
def test_device_resize_is_the_twin_byte_for_byte(src, dst, c):
    from video_depth_anything_amd.scale import resize_frames
    x, want = check(3, src, dst, c)
    staged = resize_frames(x, *dst)                                              # numpy in, numpy out, staged through the device
    assert isinstance(staged, np.ndarray) and np.array_equal(staged, want)
    assert np.array_equal(resize_frames(torch.from_numpy(x).cuda(), *dst).cpu().numpy(), want)      # a second launch: the same bytes


def test_numpy_in_staged_two_frames_at_a_time(monkeypatch):
    """Five frames through a staging block of two (2, 2, 1): the twin's bytes, and the bytes of the call that takes them at once."""
    from video_depth_anything_amd import scale
    x, want = frames(5, 9, 17, 3), twin(5, (9, 17), (14, 11), 3)
    at_once = scale.resize_frames(x, 14, 11)
    monkeypatch.setattr(scale, "_BLOCK_BYTES", 2 * x[0].nbytes)
    staged = scale.resize_frames(x, 14, 11)
    report_difference(staged, want, "staged")
    assert isinstance(staged, np.ndarray) and np.array_equal(staged, want) and np.array_equal(staged, at_once)


@pytest.mark.parametrize("c", [1, 3], ids=["gray", "rgb"])
def test_widths_around_a_workgroups_tile(c):
    """Output rows one pixel under, at and one pixel over the bytes a workgroup covers, and an exact multiple of them."""
    px = TILE // c
    for W in sorted({px - 1, px, px + 1, TILE}):
        check(3, (9, W + W // 2 + 1), (6, W), c)


@pytest.mark.parametrize("c", [1, 3], ids=["gray", "rgb"])
@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("both", [True, False], ids=["both", "output"])
def test_unaligned_bases_take_the_byte_paths(offset, c, both):
    """Input and output (or the output alone: the source is staged then) as slices of larger buffers that start 1, 2 and 3 bytes off:
    rows of 20 / 60 bytes would be stored as dwords and rows of 40 / 120 bytes staged otherwise."""
    from video_depth_anything_amd import ops
    src, dst = (64, 40), (32, 20)
    x, want = frames(3, *src, c), twin(3, src, dst, c)
    buf_in = torch.zeros(x.size + 8, dtype=torch.uint8, device="cuda")
    buf_out = torch.full((want.size + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    at = offset if both else 0
    dev_in, dev_out = buf_in[at:at + x.size].view(x.shape), buf_out[offset:offset + want.size].view(want.shape)
    assert dev_in.data_ptr() % 4 == at and dev_out.data_ptr() % 4 == offset
    dev_in.copy_(torch.from_numpy(x))
    ops.resize_linear_u8(dev_in, dev_out)
    got = buf_out.cpu().numpy()
    report_difference(got[offset:offset + want.size].reshape(want.shape), want, f"offset {offset} x {c}")
    assert np.array_equal(got[offset:offset + want.size].reshape(want.shape), want)
    assert (got[:offset] == 0xA5).all() and (got[offset + want.size:] == 0xA5).all()     # nothing written around the output


def test_one_frame_of_the_real_size():
    check(1, (1080, 1920), (720, 1280), 3)


def test_reading_an_avi_scaled_and_strided_on_the_device(tmp_path):
    """8 frames of 48 x 80 at 12 fps, read at 6 fps under max_res 40: frames 0, 2, 4, 6 at 24 x 40. read_video_blocks and
    read_video_frames give the same bytes, and they are the twin's resize of the twin's decoding of the kept frames."""
    from utils.dc_utils import read_video_blocks, read_video_frames
    from video_depth_anything_amd import mjpeg
    from video_depth_anything_amd.scale import resize_frames_numpy
    jpegs = mjpeg.encode_jpeg_numpy(clip(8, 48, 80), 90)
    path = str(tmp_path / "clip.avi")
    mjpeg.write_avi(path, jpegs, 12.0, 80, 48)
    want = resize_frames_numpy(mjpeg.decode_jpeg_numpy(jpegs[::2]), 24, 40)
    whole, fps = read_video_frames(path, -1, 6, 40, device="cuda")
    assert fps == 6 and whole.shape == (4, 24, 40, 3)
    report_difference(whole, want, "read_video_frames")
    assert np.array_equal(whole, want)
    blocks, bfps = read_video_blocks(path, -1, 6, 40, device="cuda", block=3)
    blocks = list(blocks)
    assert bfps == 6 and [b.shape[0] for b in blocks] == [3, 1] and np.array_equal(np.concatenate(blocks), want)
    cut = np.concatenate(list(read_video_blocks(path, 5, 6, 40, device="cuda")[0]))         # 5 source frames: 0, 2, 4
    assert np.array_equal(cut, want[:3])


@pytest.mark.parametrize("stream", [False, True], ids=["plain", "stream"])
def test_run_py_scales_and_thins_an_avi_on_the_device(tmp_path, stream):
    """The CLI end to end on the same clip, --max_res 40 --target_fps 6: depths of frames 0, 2, 4, 6 at 24 x 40, and <name>_src.avi holds
    exactly the frames the model saw - the twin's resize of the twin's decoding, coded by the encoder's twin - plain and with --stream
    (where read_video_blocks feeds the stream and a second pass writes <name>_src.avi block by block)."""
    import subprocess
    import sys
    from video_depth_anything_amd import mjpeg
    from video_depth_anything_amd.scale import resize_frames_numpy
    jpegs = mjpeg.encode_jpeg_numpy(clip(8, 48, 80), 90)
    mjpeg.write_avi(str(tmp_path / "clip.avi"), jpegs, 12.0, 80, 48)
    want = resize_frames_numpy(mjpeg.decode_jpeg_numpy(jpegs[::2]), 24, 40)
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(REPO, "run.py"), "--input_video", str(tmp_path / "clip.avi"), "--output_dir", str(out), "--encoder", "vits",
                        "--input_size", "70", "--checkpoint", "synthetic", "--save_npz", "--mjpeg", "--max_res", "40", "--target_fps", "6"]
                       + (["--stream"] if stream else []), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    depths = np.load(out / "clip_depths.npz")["depths"]
    assert depths.shape == (4, 24, 40) and np.isfinite(depths).all()
    src, fps, width, height = mjpeg.read_avi(str(out / "clip_src.avi"))
    assert (fps, width, height) == (6.0, 40, 24) and src == mjpeg.encode_jpeg_numpy(want, 90)


def test_run_py_stream_scales_an_npy_for_the_gif_or_mp4_writer(tmp_path):
    """--stream without --mjpeg on an .npy that is scaled: fed in blocks, and <name>_src comes from read_video_frames once more."""
    import subprocess
    import sys
    np.save(tmp_path / "clip.npy", clip(5, 48, 80))
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(REPO, "run.py"), "--input_video", str(tmp_path / "clip.npy"), "--output_dir", str(out), "--encoder", "vits",
                        "--input_size", "70", "--checkpoint", "synthetic", "--max_res", "40", "--stream"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    depths = np.load(out / "clip_depths.npy")
    assert depths.shape == (5, 24, 40) and np.isfinite(depths).all()
    assert [p.name for p in out.iterdir() if p.name.startswith("clip_src.")], "no <name>_src written"


def test_reading_an_npy_scaled_on_the_device(tmp_path):
    """A memory-mapped .npy under max_res with a device: block by block the twin's bytes, and read_video_frames' too."""
    from utils.dc_utils import read_video_blocks, read_video_frames
    from video_depth_anything_amd.scale import resize_frames_numpy
    x = frames(7, 48, 80)
    path = str(tmp_path / "clip.npy")
    np.save(path, x)
    want = resize_frames_numpy(x[::2], 24, 40)
    blocks = list(read_video_blocks(path, -1, 12, 40, device="cuda", block=3)[0])
    assert [b.shape[0] for b in blocks] == [3, 1] and np.array_equal(np.concatenate(blocks), want)
    assert np.array_equal(read_video_frames(path, -1, 12, 40, device="cuda")[0], want)
