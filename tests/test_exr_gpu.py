"""csrc/exr.hip against its twin on the MI355X: the device's files are exr.encode_exr_numpy's byte for byte for every case of
_exr_inputs.py (test_exr_numpy.py holds the twin itself to the format and proves on the CPU that the cases reach the compressed and
the raw path), through the tensor form, a strided view, and the numpy form whatever the staging size; the files written from them
read back bit-identical; run.py --save_exr writes them."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _exr_inputs as xinp

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def files_of(payload, offsets, w, h):
    from video_depth_anything_amd import exr
    assert payload.is_cuda and offsets.is_cuda and payload.dtype == torch.uint8 and offsets.dtype == torch.int64
    off = offsets.cpu().numpy()
    assert off[0] == 0 and (np.diff(off) > 0).all()
    data = payload.cpu().numpy()
    head = exr.exr_header(w, h)
    return tuple(head + data[off[i]:off[i + 1]].tobytes() for i in range(off.size - 1))


def device_files(x, view=None):
    """The tensor form on a copy of `x`. view=(gap, lead): the copy's frames lie `gap` floats apart, the first `lead` floats into an
    allocation that is filled with another pattern around them."""
    from video_depth_anything_amd import exr
    n, h, w = x.shape
    t = torch.from_numpy(np.array(x).view(np.int32))                           # as integers: no copy may touch a NaN's payload
    if view is None:
        d = t.cuda()
    else:
        gap, lead = view
        buf = torch.full((lead + n * (h * w + gap),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        d = buf[lead:].view(n, h * w + gap)[:, :h * w].view(n, h, w)
        d.copy_(t)
        assert d.storage_offset() == lead and (n == 1 or d.stride(0) == h * w + gap)      # (a single frame has no stride to speak of)
    payload, offsets = exr.encode_exr(d.view(torch.float32))
    return files_of(payload, offsets, w, h)


def first_difference(got, want):
    for f, (a, b) in enumerate(zip(got, want)):
        if a != b:
            n = min(len(a), len(b))
            at = next((i for i in range(n) if a[i] != b[i]), n)
            return f"frame {f}: {len(a)} bytes against the twin's {len(b)}, first difference at byte {at}"
    return f"{len(got)} files against the twin's {len(want)}"


@pytest.mark.parametrize("name", xinp.names())
def test_the_device_files_are_the_twins(name):
    want = xinp.twin(name)[0]
    got = device_files(xinp.case(name))
    assert got == want, first_difference(got, want)


@pytest.mark.parametrize("name", ["two_chunks_one_row_tail", "three_chunks_five_row_tail", "mixed", "special_bits"])
def test_a_strided_view_at_an_offset_gives_the_same_bytes(name):
    want = xinp.twin(name)[0]
    for view in ((5, 3), (1, 1), (0, 7)):
        got = device_files(xinp.case(name), view)
        assert got == want, (view, first_difference(got, want))


@pytest.mark.parametrize("name", ["three_chunks_five_row_tail", "two_chunks_one_row_tail", "noise"])
def test_the_numpy_form_does_not_depend_on_the_staging_size(name):
    from video_depth_anything_amd import exr
    x, want = xinp.case(name), list(xinp.twin(name)[0])
    assert exr.encode_exr(x) == want
    assert exr.encode_exr(x, frames_per_block=1) == want
    assert exr.encode_exr(x, frames_per_block=2) == want                      # three frames: a block of two and a block of one


def test_two_runs_are_identical():
    x = xinp.case("three_chunks_five_row_tail")
    assert device_files(x, (2, 1)) == device_files(x, (2, 1))


def test_write_exr_sequence_reads_back(tmp_path):
    from video_depth_anything_amd import exr
    d = xinp.fixture_depths("tiny_video")
    paths = exr.write_exr_sequence(d, str(tmp_path / "clip_depths_exr"), device="cuda", frames_per_block=5)
    assert [os.path.basename(p) for p in paths] == [f"frame_{i:05d}.exr" for i in range(d.shape[0])]
    for p, frame in zip(paths, d):
        got = exr.read_exr(p)
        assert list(got) == ["Z"] and got["Z"].dtype == np.float32 and got["Z"].tobytes() == np.ascontiguousarray(frame).tobytes()
    # the files are the twin's (two frames of them: the twin is a Python loop)
    for i in (0, d.shape[0] - 1):
        assert open(paths[i], "rb").read() == exr.encode_exr_numpy(d[i])
    # a cuda tensor and a memory map give the same files
    again = exr.write_exr_sequence(torch.from_numpy(d).cuda(), str(tmp_path / "from_tensor"), pattern="z{:03d}.exr")
    np.save(tmp_path / "d.npy", d)
    mapped = exr.write_exr_sequence(np.load(tmp_path / "d.npy", mmap_mode="r"), str(tmp_path / "from_map"), frames_per_block=7)
    assert os.path.basename(again[1]) == "z001.exr"
    for a, b, c in zip(paths, again, mapped):
        assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()


@pytest.mark.parametrize("stream", [False, True], ids=["plain", "stream"])
def test_run_py_save_exr_writes_a_readable_file_per_frame(tmp_path, stream):
    """The CLI end to end as a child process: <name>_depths_exr/frame_00000.exr ... hold the depths that --save_npz saved, bit for bit."""
    from video_depth_anything_amd import exr
    y, x = np.mgrid[0:40, 0:136]
    frames = np.stack([np.stack([(x + 9 * f) % 256, (2 * y + x) % 256, (y * x + f) % 256], -1) for f in range(3)]).astype(np.uint8)
    src, out = tmp_path / "clip.npy", tmp_path / "out"
    np.save(src, frames)
    r = subprocess.run([sys.executable, os.path.join(REPO, "run.py"), "--input_video", str(src), "--output_dir", str(out), "--encoder", "vits",
                        "--input_size", "70", "--checkpoint", "synthetic", "--mjpeg", "--save_npz", "--save_exr"] + (["--stream"] if stream else []),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    depths = np.load(out / "clip_depths.npz")["depths"]
    assert depths.shape == (3, 40, 136) and depths.dtype == np.float32
    assert sorted(os.listdir(out / "clip_depths_exr")) == ["frame_00000.exr", "frame_00001.exr", "frame_00002.exr"]
    for i in range(3):
        got = exr.read_exr(str(out / "clip_depths_exr" / f"frame_{i:05d}.exr"))
        assert list(got) == ["Z"] and got["Z"].tobytes() == depths[i].tobytes()
