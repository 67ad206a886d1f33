"""csrc/deflate.hip against its twin: the device stream is deflate.deflate_numpy byte for byte and the device CRC is zlib's, for every
input of _deflate_inputs.py at input offsets 0..3, through the tensor form and the numpy form, whatever the staging size; and the
.npz written from those streams loads back bit-identical through np.load."""
import os
import sys
import zipfile
import zlib

import numpy as np
import pytest
import torch

import _deflate_inputs as dinp

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = dinp.CHUNK


def device_stream(x, offset=0, final=True):
    """The tensor form on a copy of `x` that starts `offset` bytes into its allocation."""
    from video_depth_anything_amd import deflate
    buf = torch.zeros(offset + x.size + 8, dtype=torch.uint8, device="cuda")
    buf[:offset] = 0xA5
    buf[offset:offset + x.size] = torch.from_numpy(np.array(x)).cuda()
    payload, length, crc = deflate.deflate(buf[offset:offset + x.size], final=final)
    assert payload.is_cuda and payload.numel() == length
    return payload.cpu().numpy().tobytes(), crc


@pytest.mark.parametrize("name", dinp.names())
def test_the_device_stream_is_the_twins(name):
    x = dinp.case(name)
    want, crc = dinp.twin_stream(name), zlib.crc32(x)
    for offset in range(4):
        got, got_crc = device_stream(x, offset)
        assert got == want, (name, offset, len(got), len(want))
        assert got_crc == crc, (name, offset)


@pytest.mark.parametrize("name", ["len_0", "len_3", "len_32771", "run_sweep", "noise_3_chunks"])
def test_an_open_piece_is_the_twins(name):
    x = dinp.case(name)
    got, crc = device_stream(x, 1, final=False)
    assert got == dinp.twin_stream(name, final=False) and crc == zlib.crc32(x)


@pytest.mark.parametrize("name", ["len_32771", "run_straddles_chunks", "tiny_video", "noise_3_chunks", "len_0"])
def test_the_numpy_form_does_not_depend_on_the_staging_size(name):
    from video_depth_anything_amd import deflate
    x = dinp.case(name)
    want = (dinp.twin_stream(name), zlib.crc32(x))
    assert deflate.deflate(x) == want
    assert deflate.deflate(x.tobytes(), block_bytes=CHUNK) == want            # staged a chunk at a time
    assert deflate.deflate(x, block_bytes=3 * CHUNK) == want


def test_two_runs_are_identical():
    x = dinp.case("tiny_metric_video")
    assert device_stream(x, 2) == device_stream(x, 2)


def test_the_per_chunk_crcs():
    from video_depth_anything_amd import ops
    x = dinp.case("len_32771")
    d = torch.from_numpy(np.array(x)).cuda()
    work = torch.empty(ops.deflate_workspace_bytes(x.size), dtype=torch.uint8, device="cuda")
    out = torch.empty(ops.deflate_out_bytes(x.size), dtype=torch.uint8, device="cuda")
    length = torch.empty(1, dtype=torch.int64, device="cuda")
    crcs = torch.empty(3, dtype=torch.int32, device="cuda")
    ops.deflate(d, True, work, out, length, crcs)
    got = (crcs.cpu().numpy().astype(np.int64) & 0xFFFFFFFF).tolist()
    assert got == [zlib.crc32(x[i:i + CHUNK]) for i in range(0, x.size, CHUNK)]
    assert int(length.item()) == len(dinp.twin_stream("len_32771"))


def fixture_depths(name):
    return np.load(os.path.join(dinp.GOLDEN, name + ".npz"))["depths"]


def loads_back(path, arrays):
    with np.load(path) as z:
        assert sorted(z.files) == sorted(arrays)
        for k, v in arrays.items():
            assert z[k].dtype == v.dtype and z[k].shape == v.shape and z[k].tobytes() == np.ascontiguousarray(v).tobytes(), k
    with zipfile.ZipFile(path) as z:
        assert z.testzip() is None


def test_savez_compressed_on_the_device(tmp_path):
    from video_depth_anything_amd import deflate
    d = fixture_depths("tiny_video")
    mm = np.lib.format.open_memmap(str(tmp_path / "mm.npy"), mode="w+", dtype=np.float32, shape=d.shape)
    mm[:] = fixture_depths("tiny_metric_video")
    mm.flush()
    arrays = dict(depths=d, mapped=np.load(str(tmp_path / "mm.npy"), mmap_mode="r"), empty=np.zeros((0, 2), np.float32), view=d[:, ::3, 2::5],
                  scalar=np.array(7, np.int64))
    for kw in (dict(), dict(_block_bytes=2 * CHUNK, _zip64_limit=5000)):
        path = deflate.savez_compressed(str(tmp_path / "dev.npz"), device="cuda", **kw, **arrays)
        loads_back(path, arrays)
    # the container is the one the twin fills: the same file, byte for byte
    twin = deflate.savez_compressed(str(tmp_path / "twin.npz"), device=None, _twin=True, _block_bytes=2 * CHUNK, _zip64_limit=5000, **arrays)
    assert open(path, "rb").read() == open(twin, "rb").read()


def test_run_py_saves_through_the_device(tmp_path):
    sys.path.insert(0, REPO)
    try:
        import run
    finally:
        sys.path.remove(REPO)
    d = fixture_depths("tiny_video")[:3, :30, :41].copy()
    path = run.save_depths_npz(str(tmp_path / "clip_depths.npz"), d, "cuda")
    assert path == str(tmp_path / "clip_depths.npz")
    loads_back(path, dict(depths=d))
    with zipfile.ZipFile(path) as z:
        body_at = z.infolist()[0].header_offset + 30 + len("depths.npy")
        size = z.infolist()[0].compress_size
    from video_depth_anything_amd import deflate
    raw = open(path, "rb").read()[body_at:body_at + size]
    assert raw[5 + 128:] == deflate.deflate_numpy(d)                           # the device's stream, not zlib's
    # without a device nothing changes: numpy's own writer
    plain = run.save_depths_npz(str(tmp_path / "plain_depths.npz"), d, None)
    loads_back(plain, dict(depths=d))
