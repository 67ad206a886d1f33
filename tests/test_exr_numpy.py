"""exr.encode_exr_numpy - the integer host twin of csrc/exr.hip and the contract of the device's bytes - and exr.read_exr, on the CPU.
The files are judged by a walker written here from the format's layout (not by read_exr) and by zlib's inflate, which also judges
the Adler-32; read_exr is judged by files built by hand here."""
import struct
import zlib

import numpy as np
import pytest

import _exr_inputs as xinp
from video_depth_anything_amd import exr

MAGIC = bytes([0x76, 0x2F, 0x31, 0x01])


def cstr(buf, at):
    end = buf.index(b"\0", at)
    return buf[at:end], end + 1


def walk_header(buf):
    """([(name, type, value)], position behind the header) of a file's bytes."""
    assert buf[:4] == MAGIC and buf[4:8] == bytes([2, 0, 0, 0])
    at, attrs = 8, []
    while buf[at]:
        name, at = cstr(buf, at)
        kind, at = cstr(buf, at)
        size, = struct.unpack_from("<i", buf, at)
        attrs.append((name, kind, buf[at + 4:at + 4 + size]))
        at += 4 + size
    return attrs, at + 1


def unfilter_loop(f):
    """The filter undone by a plain loop: the predictor, then the two halves interleaved."""
    t = bytearray(f)
    for i in range(1, len(t)):
        t[i] = (t[i - 1] + t[i] - 128) & 255
    half = (len(t) + 1) // 2
    raw = bytearray(len(t))
    for i in range(len(t)):
        raw[i] = t[i // 2] if i % 2 == 0 else t[half + i // 2]
    return bytes(raw)


def filter_loop(raw):
    L = len(raw)
    half = (L + 1) // 2
    t = [raw[2 * i] if i < half else raw[2 * (i - half) + 1] for i in range(L)]
    return bytes([t[0]] + [(t[i] - t[i - 1] + 128) & 255 for i in range(1, L)])


def walk_file(buf, frame, flevel=bytes([0x01])):
    """Checks one file against the frame it was made of; returns per block whether it is compressed. flevel: the second byte of a
    zlib stream (01 from the twin and the device, 9C from zlib.compress at its default level)."""
    h, w = frame.shape
    attrs, at = walk_header(buf)
    assert at == 277
    nb = -(-h // 16)
    table = struct.unpack_from(f"<{nb}Q", buf, at)
    want_at = at + 8 * nb
    flags = []
    for b, pos in enumerate(table):
        assert pos == want_at, (b, pos, want_at)                              # the blocks follow the table back to back, in order
        y, size = struct.unpack_from("<ii", buf, pos)
        assert y == 16 * b
        rows = min(16, h - 16 * b)
        L = 4 * w * rows
        data = buf[pos + 8:pos + 8 + size]
        assert len(data) == size
        raw = np.ascontiguousarray(frame[16 * b:16 * b + rows]).tobytes()
        if size == L:
            assert data == raw
        else:
            assert size < L                                                   # compressed only when strictly shorter
            assert data[:1] == bytes([0x78]) and data[1:2] == flevel
            f = zlib.decompress(data)                                         # judges the deflate stream and the Adler-32
            assert len(f) == L
            assert unfilter_loop(f) == raw                                    # the exact input bits
        flags.append(size < L)
        want_at = pos + 8 + size
    assert want_at == len(buf)
    assert len(buf) <= 277 + 16 * nb + 4 * w * h                              # the structural guarantee
    return flags


def test_the_header_is_277_bytes_with_the_documented_fields():
    head = exr.exr_header(518, 37)
    assert len(head) == 277
    attrs, end = walk_header(head)
    assert end == 277
    window = struct.pack("<4i", 0, 0, 517, 36)
    chlist = b"Z\0" + struct.pack("<i", 2) + bytes([0, 0, 0, 0]) + struct.pack("<ii", 1, 1) + b"\0"
    assert len(chlist) == 19
    assert attrs == [(b"channels", b"chlist", chlist), (b"compression", b"compression", bytes([3])), (b"dataWindow", b"box2i", window),
                     (b"displayWindow", b"box2i", window), (b"lineOrder", b"lineOrder", bytes([0])),
                     (b"pixelAspectRatio", b"float", struct.pack("<f", 1.0)), (b"screenWindowCenter", b"v2f", struct.pack("<ff", 0.0, 0.0)),
                     (b"screenWindowWidth", b"float", struct.pack("<f", 1.0))]
    assert exr.exr_header(518, 37, compression="zips")[:277] != head and len(exr.exr_header(3, 3, channel="depth")) == 281
    with pytest.raises(ValueError):
        exr.exr_header(0, 4)
    with pytest.raises(ValueError):
        exr.exr_header(4, 4, compression="piz")


@pytest.mark.parametrize("name", xinp.names())
def test_the_twins_files_hold_the_input_bits(name):
    x = xinp.case(name)
    files, flags = xinp.twin(name)
    assert len(files) == x.shape[0]
    walked = []
    for frame, buf in zip(x, files):
        walked += walk_file(buf, frame)
    assert tuple(walked) == flags
    assert walked.count(False) == xinp.raw_blocks(name) and len(walked) == xinp.n_blocks(name)


def test_the_cases_reach_the_compressed_and_the_raw_path():
    """What keeps the GPU tests from passing on one path only."""
    for name in ("mixed", "one_chunk", "exactly_16384", "two_chunks_one_row_tail", "three_chunks_five_row_tail", "constant"):
        assert any(xinp.twin(name)[1]), name
    assert not any(xinp.twin("noise")[1])
    mixed = xinp.twin("mixed")[1]
    assert any(mixed) and not all(mixed)


@pytest.mark.parametrize("name", xinp.names())
def test_read_exr_gives_the_twins_input_back(name):
    x = xinp.case(name)
    for frame, buf in zip(x, xinp.twin(name)[0]):
        got = exr.read_exr(buf)
        assert list(got) == ["Z"] and got["Z"].dtype == np.float32 and got["Z"].shape == frame.shape
        assert got["Z"].tobytes() == np.ascontiguousarray(frame).tobytes()


def test_read_exr_reads_a_path(tmp_path):
    p = tmp_path / "a.exr"
    p.write_bytes(xinp.twin("one_chunk")[0][0])
    assert exr.read_exr(str(p))["Z"].tobytes() == xinp.case("one_chunk")[0].tobytes()


def hand_file(w, h, channels, compression, lines, rows_of, compress):
    """A file built here: channels [(name, pixel type)], rows_of(y0, y1) -> the raw bytes of scanlines y0..y1-1."""
    def attr(name, kind, value):
        return name + b"\0" + kind + b"\0" + struct.pack("<i", len(value)) + value
    chlist = b"".join(n + b"\0" + struct.pack("<iB3xii", t, 0, 1, 1) for n, t in channels) + b"\0"
    window = struct.pack("<4i", 0, 0, w - 1, h - 1)
    head = (MAGIC + struct.pack("<I", 2) + attr(b"channels", b"chlist", chlist) + attr(b"compression", b"compression", bytes([compression]))
            + attr(b"dataWindow", b"box2i", window) + attr(b"displayWindow", b"box2i", window) + attr(b"lineOrder", b"lineOrder", b"\0")
            + attr(b"pixelAspectRatio", b"float", struct.pack("<f", 1.0)) + attr(b"screenWindowCenter", b"v2f", bytes(8))
            + attr(b"screenWindowWidth", b"float", struct.pack("<f", 1.0)) + b"\0")
    blocks = []
    for y in range(0, h, lines):
        raw = rows_of(y, min(h, y + lines))
        data = raw
        if compress:
            z = zlib.compress(filter_loop(raw))
            data = z if len(z) < len(raw) else raw
        blocks.append(struct.pack("<ii", y, len(data)) + data)
    at, table = len(head) + 8 * len(blocks), []
    for blk in blocks:
        table.append(at)
        at += len(blk)
    return head + struct.pack(f"<{len(table)}Q", *table) + b"".join(blocks)


def test_read_exr_reads_an_uncompressed_file():
    z = (np.arange(5 * 7, dtype=np.float32).reshape(5, 7) / 3).astype(np.float32)
    buf = hand_file(7, 5, [(b"Z", 2)], 0, 1, lambda a, b: z[a:b].tobytes(), False)
    got = exr.read_exr(buf)
    assert list(got) == ["Z"] and got["Z"].tobytes() == z.tobytes()


def test_read_exr_reads_a_zips_file():
    z = np.repeat(np.arange(9, dtype=np.float32), 33).reshape(9, 33) + 0.25
    buf = hand_file(33, 9, [(b"Z", 2)], 2, 1, lambda a, b: z[a:b].tobytes(), True)
    assert len(buf) < 277 + 8 * 9 + 8 * 9 + z.nbytes                           # some line really is compressed
    assert exr.read_exr(buf)["Z"].tobytes() == z.tobytes()


def test_read_exr_reads_half_and_float_channels_of_one_file():
    """Two channels, A (HALF) before Z (FLOAT) within every scanline, ZIP blocks of 16 lines with a 4-line tail; and a UINT one."""
    h, w = 20, 11
    a = (np.arange(h * w).reshape(h, w) % 7).astype(np.float16)
    z = np.floor(np.arange(h * w, dtype=np.float32).reshape(h, w) / 5)
    rows = lambda y0, y1: b"".join(a[y].tobytes() + z[y].tobytes() for y in range(y0, y1))
    got = exr.read_exr(hand_file(w, h, [(b"A", 1), (b"Z", 2)], 3, 16, rows, True))
    assert list(got) == ["A", "Z"]
    assert got["A"].dtype == np.float16 and got["A"].tobytes() == a.tobytes()
    assert got["Z"].dtype == np.float32 and got["Z"].tobytes() == z.tobytes()
    ids = np.arange(h * w, dtype=np.uint32).reshape(h, w) * 77777
    got = exr.read_exr(hand_file(w, h, [(b"id", 0)], 3, 16, lambda y0, y1: ids[y0:y1].tobytes(), True))
    assert got["id"].dtype == np.uint32 and np.array_equal(got["id"], ids)


def test_read_exr_refuses_what_it_does_not_read():
    good = xinp.twin("one_chunk")[0][0]
    for flag, word in ((0x200, "tiled"), (0x800, "deep"), (0x1000, "multi-part")):
        with pytest.raises(ValueError, match=word):
            exr.read_exr(good[:4] + struct.pack("<I", 2 | flag) + good[8:])
    with pytest.raises(ValueError, match="magic"):
        exr.read_exr(b"\0" + good[1:])
    at = good.index(b"compression\0compression\0") + 24 + 4
    with pytest.raises(ValueError, match="compression 4"):
        exr.read_exr(good[:at] + bytes([4]) + good[at + 1:])                  # PIZ


@pytest.mark.parametrize("L", [1, 2, 3, 4, 7, 8, 255, 256, 1001, 4096])
def test_the_filter_is_the_plain_loop(L):
    raw = np.random.default_rng(L).integers(0, 256, L, dtype=np.uint8)
    f = exr.filter_bytes(raw)
    assert f.tobytes() == filter_loop(raw.tobytes())
    assert exr.unfilter_bytes(f).tobytes() == raw.tobytes() == unfilter_loop(f.tobytes())
    assert exr.adler32(f) == zlib.adler32(f.tobytes())


def test_the_chunks_are_balanced():
    assert exr.block_chunks(4) == (1, 64) and exr.block_chunks(16384) == (1, 16384) and exr.block_chunks(16448) == (2, 8256)
    assert exr.block_chunks(4 * 518 * 16) == (3, 11072)
    for L in range(4, 64 * 65535 + 1, 4 * 997):                               # every chunk holds bytes and at most 16384 of them
        k, q = exr.block_chunks(L)
        assert q % 64 == 0 and q <= 16384 and (k - 1) * q < L <= k * q


def test_the_zlib_writer_round_trips():
    for name in ("three_chunks_five_row_tail", "mixed", "noise", "special_bits", "one_pixel"):
        for frame in xinp.case(name):
            buf = exr.encode_exr_numpy(frame, compress=zlib.compress)
            walk_file(buf, frame, bytes([0x9C]))
            assert exr.read_exr(buf)["Z"].tobytes() == np.ascontiguousarray(frame).tobytes()


def test_write_exr_sequence_on_the_host(tmp_path):
    d = xinp.fixture_depths("tiny_video")[:3, :20, :50]
    paths = exr.write_exr_sequence(d, str(tmp_path / "clip_depths_exr"), device=None)
    assert [p.split("/")[-1] for p in paths] == ["frame_00000.exr", "frame_00001.exr", "frame_00002.exr"]
    for p, frame in zip(paths, d):
        assert exr.read_exr(p)["Z"].tobytes() == np.ascontiguousarray(frame).tobytes()


def test_run_py_saves_exr_without_a_device(tmp_path):
    """run.save_depths_exr on a machine without a GPU: the OpenEXR library when it imports, the host writer otherwise; either way one
    file per frame under the reference's names that read_exr reads back."""
    import os
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, repo)
    try:
        import run
    finally:
        sys.path.remove(repo)
    d = xinp.fixture_depths("tiny_metric_video")[:2, :17, :33].copy()
    paths = run.save_depths_exr(str(tmp_path / "clip_depths_exr"), d, None)
    assert [os.path.basename(p) for p in paths] == ["frame_00000.exr", "frame_00001.exr"]
    for p, frame in zip(paths, d):
        assert exr.read_exr(p)["Z"].tobytes() == frame.tobytes()
