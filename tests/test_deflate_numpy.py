"""deflate.deflate_numpy - the integer host twin of csrc/deflate.hip and the contract of the device stream - judged by zlib's inflate,
which rejects over-subscribed and incomplete codes; the CRC-32 combination; and the hand-written .npz container read back by np.load
and zipfile. No GPU needed. profiles/deflate/ records the sizes beside zlib level 6."""
import os
import zipfile
import zlib

import numpy as np
import pytest

import _deflate_inputs as dinp
from video_depth_anything_amd import deflate

CHUNK = deflate.CHUNK


def zlib_raw(data, strategy):
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(data) + c.flush()


def test_the_inputs_are_the_ones_the_kernel_can_go_wrong_at():
    sizes = {x.size for _, x in dinp.cases()}
    assert {0, 1, 2, 3, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3} <= sizes
    assert dinp.case("fibonacci").size == 17710
    # the length limit: `fibonacci` as it stands codes in 11 bits (end-of-block's count of 1 lets two chains grow side by side), so
    # `fibonacci_with_eob` counts end-of-block as F(1): its unlimited code is 18 bits deep
    info = []
    deflate.deflate_numpy(dinp.case("fibonacci_with_eob"), info=info)
    count = dict(dinp.histograms())["fibonacci_with_eob"]
    assert max(deflate.code_lengths(count, max_bits=64)) == 18 and max(info[0]["lengths"]) == 15 and not info[0]["stored"]
    info = []
    deflate.deflate_numpy(dinp.case("noise_3_chunks"), info=info)
    assert [d["stored"] for d in info] == [True] * 3
    info = []
    deflate.deflate_numpy(dinp.case("run_sweep"), info=info)
    assert not any(d["stored"] for d in info) and sum(d["matches"] for d in info) >= 260
    info = []
    deflate.deflate_numpy(dinp.case("all_256_no_neighbours"), info=info)
    assert info[0]["matches"] == 0 and info[0]["tokens"] == CHUNK
    info = []
    deflate.deflate_numpy(dinp.case("two_symbols"), info=info)
    assert sum(1 for b in info[0]["lengths"][:256] if b) == 2


@pytest.mark.parametrize("name", dinp.names())
def test_zlib_inflates_the_stream_to_the_input(name):
    x = dinp.case(name)
    s = dinp.twin_stream(name)
    assert zlib.decompress(s, -15) == x.tobytes()
    assert len(s) <= x.size + 5 * max(1, -(-x.size // CHUNK)) == deflate.out_bytes(x.size)


@pytest.mark.parametrize("name", dinp.names())
def test_pieces_concatenate(name):
    x = dinp.case(name)
    cut1, cut2 = (x.size // 3) // 7 * 7, x.size // 2
    pieces = [deflate.deflate_numpy(x[:cut1], final=False), deflate.deflate_numpy(x[cut1:cut1], final=False),
              deflate.deflate_numpy(x[cut1:cut2], final=False), deflate.deflate_numpy(x[cut2:], final=True)]
    assert pieces[1] == b""
    assert zlib.decompress(b"".join(pieces), -15) == x.tobytes()
    # cut at a chunk boundary, the pieces ARE the stream: nothing depends on how the input was staged
    if x.size > CHUNK:
        assert deflate.deflate_numpy(x[:CHUNK], final=False) + deflate.deflate_numpy(x[CHUNK:], final=True) == dinp.twin_stream(name)


@pytest.mark.parametrize("total", dinp.RUN_TOTALS)
def test_a_run_is_a_literal_full_matches_and_a_tail(total):
    x = np.asarray(dinp.case(f"run_{total}"))
    pos, sym, nextra, extra, is_m = deflate.chunk_tokens(x)
    rest = total - 1
    full, tail = divmod(rest, 258)
    want = [("lit", 9), ("lit", 200)] + [("match", 258)] * full + ([("match", tail)] if tail >= 3 else [("lit", 200)] * tail) + [("lit", 9), ("lit", 8)]
    got = []
    for s, ne, ev, m in zip(sym, nextra, extra, is_m):
        if m:
            ln = [l for l in range(3, 259) if deflate.length_symbol(l) == (s, ne, ev)]
            assert len(ln) == 1
            got.append(("match", ln[0]))
        else:
            got.append(("lit", int(s)))
    assert got == want


def test_no_match_reaches_across_a_chunk_boundary():
    x = dinp.case("run_straddles_chunks")
    info = []
    s = deflate.deflate_numpy(x, info=info)
    assert s == deflate.encode_chunk(x[:CHUNK], False) + deflate.encode_chunk(x[CHUNK:], True)
    pos = deflate.chunk_tokens(np.asarray(x[CHUNK:]))[0]
    assert pos[0] == 0                                                         # the second chunk starts with a literal of its own


@pytest.mark.parametrize("name", dinp.names())
def test_crc32_combine_over_chunk_crcs(name):
    x = dinp.case(name)
    crcs = [zlib.crc32(x[i:i + CHUNK]) for i in range(0, x.size, CHUNK)]
    crc = 0
    for i, c in enumerate(crcs):
        crc = deflate.crc32_combine(crc, c, min(CHUNK, x.size - i * CHUNK))
    assert crc == zlib.crc32(x) == deflate.combine_chunk_crcs(crcs, x.size)
    assert deflate.combine_chunk_crcs(crcs, x.size, zlib.crc32(b"in front")) == zlib.crc32(b"in front" + x.tobytes())


@pytest.mark.parametrize("name", ["tiny_video", "tiny_metric_video"])
def test_the_fixtures_beat_huffman_only(name, capsys):
    data = dinp.case(name).tobytes()
    ours, huff = len(dinp.twin_stream(name)), len(zlib_raw(data, zlib.Z_HUFFMAN_ONLY))
    with capsys.disabled():
        print(f"\n{name}: {len(data)} bytes -> {ours}; zlib raw: level 6 {len(zlib_raw(data, zlib.Z_DEFAULT_STRATEGY))}, Z_RLE "
              f"{len(zlib_raw(data, zlib.Z_RLE))}, Z_HUFFMAN_ONLY {huff}")
    assert ours <= huff


# --------------------------------------------------------------------------------------------------------------- the container
def the_arrays(tmp_path):
    rng = np.random.default_rng(6)
    depths = (rng.random((5, 42, 56)) * 10).astype(np.float32)
    depths[:, :10] = 0
    mm = np.lib.format.open_memmap(str(tmp_path / "mm.npy"), mode="w+", dtype=np.float32, shape=(3, 42, 56))
    mm[:] = depths[:3] * 2
    mm.flush()
    return dict(depths=depths, second=np.linspace(0, 1, 77).reshape(7, 11), empty=np.zeros((0, 4), np.float32), scalar=np.array(2.5, np.float32),
                view=depths[:, ::2, 1::3], mapped=np.load(str(tmp_path / "mm.npy"), mmap_mode="r"))


def check_npz(path, arrays):
    with np.load(path) as z:
        assert sorted(z.files) == sorted(arrays)
        for k, v in arrays.items():
            assert z[k].dtype == v.dtype and z[k].shape == v.shape and z[k].tobytes() == np.ascontiguousarray(v).tobytes(), k
    with zipfile.ZipFile(path) as z:
        assert z.testzip() is None
        assert all(i.compress_type == zipfile.ZIP_DEFLATED for i in z.infolist())


def test_device_none_is_numpys_writer(tmp_path):
    arrays = the_arrays(tmp_path)
    path = deflate.savez_compressed(str(tmp_path / "plain"), device=None, **arrays)
    assert path.endswith("plain.npz")
    check_npz(path, arrays)


@pytest.mark.parametrize("limit", [deflate.ZIP64_LIMIT, 2000, 40])
def test_the_hand_written_container(tmp_path, limit):
    """Fed by the twin. limit 2000: the large members get ZIP64 size fields and the file ZIP64 end records; 40: every member and offset does."""
    arrays = the_arrays(tmp_path)
    path = deflate.savez_compressed(str(tmp_path / "byhand.npz"), device=None, _twin=True, _zip64_limit=limit, _block_bytes=CHUNK, **arrays)
    check_npz(path, arrays)
    raw = open(path, "rb").read()
    assert (b"PK\x06\x06" in raw) == (limit < deflate.ZIP64_LIMIT) == (b"PK\x06\x07" in raw)
    with zipfile.ZipFile(path) as z:
        member = z.infolist()[0]
        assert member.filename == "depths.npy" and member.file_size == 128 + arrays["depths"].nbytes
        # the member's stream: the .npy header stored, then the twin's stream of the array bytes
        with open(path, "rb") as f:
            f.seek(member.header_offset + 30 + len("depths.npy") + (20 if limit < deflate.ZIP64_LIMIT else 0))
            body = f.read(member.compress_size)
    assert body[:5] == b"\x00\x80\x00\x7f\xff" and body[5 + 128:] == deflate.deflate_numpy(arrays["depths"])


def test_what_is_refused(tmp_path):
    with pytest.raises(TypeError, match="object"):
        deflate.savez_compressed(str(tmp_path / "o.npz"), device=None, _twin=True, a=np.array([{}], dtype=object))
    with pytest.raises(ValueError, match="multiple of 16384"):
        deflate.savez_compressed(str(tmp_path / "o.npz"), device=None, _twin=True, _block_bytes=1000, a=np.zeros(3))
