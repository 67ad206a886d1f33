"""mjpeg.encode_jpeg / vda_mjpeg_encode_u8 (csrc/mjpeg.hip) on the MI355X: the device's streams are the host twin encode_jpeg_numpy's
streams, byte for byte, for every case of _mjpeg_inputs.py - whose coverage of the entropy coder's hard cases (ZRL, stuffed FF,
blocks without EOB, the largest DC and AC categories, a wrapping restart counter) tests/test_mjpeg_numpy.py asserts from the twin's
record. The shapes put one block, ragged edges, a tile row that ends inside a workgroup's third chunk of 8 tiles (17 tiles) and
gray input in front of the transform kernel, and 1 to 51 blocks per restart interval in front of the entropy kernel; every call is
a few milliseconds. The output buffer is pre-filled and guarded: nothing behind the last frame's EOI may change."""
import numpy as np
import pytest
import torch

import _mjpeg_inputs as inp

pytestmark = pytest.mark.gpu
FILL, GUARD = 0xA5, 64


@pytest.mark.parametrize("case", inp.CASES, ids=inp.case_id)
def test_device_stream_is_the_twins_stream(case):
    from video_depth_anything_amd import mjpeg
    shape, content, q = case
    want, _ = inp.reference(*case)
    got = mjpeg.encode_jpeg(inp.frames(shape, content), q, device="cuda")
    assert [len(j) for j in got] == [len(j) for j in want]
    assert got == want


# The entropy kernel walks an interval 256 blocks at a time and stuffs it 256 words (1 KiB) at a time, carrying the bit and byte
# offsets over: 88 tiles x 3 components = 264 blocks cross the first, any busy row the second. Two rows, the second ragged.
WIDE = (1, 9, 700, 3)


@pytest.mark.parametrize("content,q", [("noise", 100), ("ramp", 90), ("impulses", 50), ("flat", 100)])
def test_an_interval_longer_than_one_pass_of_the_workgroup(content, q):
    from video_depth_anything_amd import mjpeg
    want, cover = inp.reference(WIDE, content, q)
    head = len(mjpeg.jpeg_header(9, 700, 3, q))
    assert (700 + 7) // 8 * 3 > 256 and cover["intervals"] == 2
    if content == "noise":
        assert len(want[0]) - head > 2 * 1024 * 4                            # both rows well past one pass of the stuffing loop
    assert mjpeg.encode_jpeg(inp.frames(WIDE, content), q, device="cuda") == want


@pytest.mark.parametrize("shape", inp.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tensor_in_gives_payload_and_lengths_and_writes_nothing_else(shape):
    from video_depth_anything_amd import mjpeg, ops
    n, h, w = shape[:3]
    ch = 3 if len(shape) == 4 else 1
    want, _ = inp.reference(shape, "noise", 100)
    head = mjpeg.jpeg_header(h, w, ch, 100)
    x = torch.from_numpy(np.array(inp.frames(shape, "noise"))).cuda()
    payload, lengths = mjpeg.encode_jpeg(x, 100)
    assert payload.is_cuda and payload.dtype == torch.uint8 and lengths.is_cuda and lengths.dtype == torch.int64 and lengths.shape == (n,)
    assert payload.numel() == ops.mjpeg_out_bytes(n, h, w, ch)
    assert lengths.tolist() == [len(j) - len(head) for j in want]
    assert mjpeg.split_payload(head, payload, lengths) == want
    # the raw entry point into a guarded, pre-filled buffer: the scans, then nothing
    cap = ops.mjpeg_out_bytes(n, h, w, ch)
    buf = torch.full((GUARD + cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    work = torch.empty(ops.mjpeg_workspace_bytes(n, h, w, ch), dtype=torch.uint8, device="cuda")
    ln = torch.zeros(n, dtype=torch.int64, device="cuda")
    ops.mjpeg_encode(x, np.ascontiguousarray(mjpeg.quant_tables(100)[:2 if ch == 3 else 1], dtype=np.uint16), work, buf[GUARD:GUARD + cap], ln)
    got = buf.cpu().numpy()
    total = int(ln.sum())
    assert got[GUARD:GUARD + total].tobytes() == b"".join(j[len(head):] for j in want)
    assert (got[:GUARD] == FILL).all() and (got[GUARD + total:] == FILL).all()


@pytest.mark.parametrize("shape", [(5, 16, 24, 3), (5, 9, 17)], ids=["rgb", "gray"])
def test_numpy_in_staged_two_frames_at_a_time(shape, monkeypatch):
    """Five frames through a staging block of two (2, 2, 1): the twin's list, and the list of the call that takes them at once."""
    from video_depth_anything_amd import mjpeg
    x = np.random.default_rng(shape).integers(0, 256, size=shape, dtype=np.uint8)
    want = mjpeg.encode_jpeg_numpy(x, 90)
    at_once = mjpeg.encode_jpeg(x, 90, device="cuda")
    monkeypatch.setattr(mjpeg, "_BLOCK_BYTES", 2 * x[0].nbytes)
    staged = mjpeg.encode_jpeg(x, 90, device="cuda")
    assert isinstance(staged, list) and [len(j) for j in staged] == [len(j) for j in want]
    assert staged == want and staged == at_once


def test_two_calls_give_identical_bytes():
    """The bits of neighbouring blocks meet in shared words through OR-atomics, whose result does not depend on their order."""
    from video_depth_anything_amd import mjpeg
    x = torch.from_numpy(np.array(inp.frames((3, 40, 136, 3), "noise"))).cuda()
    first = [t.clone() for t in mjpeg.encode_jpeg(x, 90)]
    for _ in range(3):
        again = mjpeg.encode_jpeg(x, 90)
        total = int(first[1].sum())
        assert torch.equal(first[1], again[1]) and torch.equal(first[0][:total], again[0][:total])


def test_save_video_writes_the_same_file_from_the_device(tmp_path, monkeypatch):
    from utils import dc_utils
    from video_depth_anything_amd.visualize import inferno_table
    monkeypatch.setattr(dc_utils, "SAVE_BLOCK", 2)
    rng = np.random.default_rng(3)
    depths = (np.add.outer(np.arange(37), np.arange(53))[None] * (1 + np.arange(5))[:, None, None] + rng.random((5, 37, 53))).astype(np.float32)
    for gray in (False, True):
        kw = dict(fps=24, is_depths=True, grayscale=gray, palette=inferno_table(), codec="mjpeg")
        host = dc_utils.save_video(depths, str(tmp_path / f"host{gray}.mp4"), device=None, **kw)
        dev = dc_utils.save_video(depths, str(tmp_path / f"dev{gray}.mp4"), device="cuda", **kw)
        assert host.endswith(".avi") and dev.endswith(".avi") and open(host, "rb").read() == open(dev, "rb").read()
    frames = inp.frames((3, 40, 136, 3), "ramp")
    host = dc_utils.save_video(frames, str(tmp_path / "src_host.mp4"), fps=24, codec="mjpeg", quality=75)
    dev = dc_utils.save_video(frames, str(tmp_path / "src_dev.mp4"), fps=24, codec="mjpeg", quality=75, device="cuda")
    assert open(host, "rb").read() == open(dev, "rb").read()


def test_run_py_mjpeg_leaves_two_avi_files_that_read_back(tmp_path):
    """The CLI end to end: `run.py --mjpeg` writes <name>_vis.avi and <name>_src.avi (no GIF, no mp4) that decode to the input's frame
    count and size, and its own output reads back as an input video."""
    import os
    import subprocess
    import sys
    from utils.dc_utils import read_video_frames
    from video_depth_anything_amd import mjpeg
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    frames = inp.frames((3, 40, 136, 3), "ramp")
    src, out = tmp_path / "clip.npz", tmp_path / "out"
    np.savez(src, frames=frames, fps=12.0)
    r = subprocess.run([sys.executable, os.path.join(repo, "run.py"), "--input_video", str(src), "--output_dir", str(out), "--encoder", "vits",
                        "--input_size", "70", "--checkpoint", "synthetic", "--mjpeg", "--mjpeg_quality", "85"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["clip_src.avi", "clip_vis.avi"]
    for name in ("clip_src.avi", "clip_vis.avi"):
        jpegs, fps, w, h = mjpeg.read_avi(str(out / name))
        assert (len(jpegs), fps, w, h) == (3, 12.0, 136, 40)
        assert all(j.startswith(mjpeg.jpeg_header(40, 136, 3, 85)) for j in jpegs)
    assert mjpeg.read_avi(str(out / "clip_src.avi"))[0] == mjpeg.encode_jpeg_numpy(frames, 85)
    back, fps = read_video_frames(str(out / "clip_vis.avi"), -1)
    assert back.shape == frames.shape and back.dtype == np.uint8 and fps == 12.0
