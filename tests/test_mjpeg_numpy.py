"""The Motion-JPEG path on the host (video_depth_anything_amd/mjpeg.py): the integer twin's streams decode with PIL's libjpeg, reach
the hard cases of the entropy coder (asserted from the twin's coverage record, so that the GPU comparison of the same inputs cannot
pass by never meeting them), keep up with PIL's own encoder at the same tables, and travel through the AVI container. No GPU."""
import io
import os
import struct

import numpy as np
import pytest
from PIL import Image

import _mjpeg_inputs as inp
from utils import dc_utils
from video_depth_anything_amd import mjpeg, visualize

PSNR_MARGIN_DB = 0.5           # the twin may be at most this far below PIL's encoder at the same tables


def pil_decode(jpg):
    im = Image.open(io.BytesIO(jpg))
    im.load()
    return im


def pil_tables(im):
    """{id: list} in natural (row-major) order: what PIL hands out and takes since 8.3."""
    return {k: list(v) for k, v in im.quantization.items()}


# ------------------------------------------------------------------------------------------------------------- streams decode
@pytest.mark.parametrize("case", inp.CASES, ids=inp.case_id)
def test_every_frame_decodes_to_the_right_size_mode_and_tables(case):
    shape, content, q = case
    jpegs, _ = inp.reference(*case)
    n, h, w = shape[:3]
    ch = 3 if len(shape) == 4 else 1
    assert len(jpegs) == n
    head = mjpeg.jpeg_header(h, w, ch, q)
    qt = mjpeg.quant_tables(q)
    for j in jpegs:
        assert j[:len(head)] == head and j[-2:] == b"\xff\xd9"
        im = pil_decode(j)
        assert im.size == (w, h) and im.mode == ("RGB" if ch == 3 else "L")
        assert pil_tables(im) == {t: qt[t].tolist() for t in range(2 if ch == 3 else 1)}


def test_decoded_pixels_are_the_source_at_quality_100():
    for shape in inp.SHAPES:
        src = inp.frames(shape, "ramp")
        for f, j in zip(src, inp.reference(shape, "ramp", 100)[0]):
            assert inp.psnr(np.asarray(pil_decode(j)), f) > 38.0             # 4:4:4, divisors of 1: rounding and the YCbCr round trip only


def test_huffman_and_quant_tables_are_the_ones_libjpeg_writes():
    """PIL's libjpeg writes the Annex K tables by default: its DHT and (quality 50 = unscaled) DQT segments equal the header's."""
    buf = io.BytesIO()
    Image.fromarray(inp.frames((2, 17, 23, 3), "noise")[0]).save(buf, "JPEG", quality=50, subsampling=0)

    def segments(data, marker):
        out, i = [], 2
        while data[i + 1] != 0xDA:
            ln = struct.unpack(">H", data[i + 2:i + 4])[0]
            if data[i + 1] == marker:
                out.append(data[i + 4:i + 2 + ln])
            i += 2 + ln
        return b"".join(out)
    head = mjpeg.jpeg_header(17, 23, 3, 50)
    assert segments(head, 0xC4) == segments(buf.getvalue(), 0xC4)
    assert segments(head, 0xDB) == segments(buf.getvalue(), 0xDB)


# ---------------------------------------------------------------------------------------------------------- coverage conditions
def test_noise_at_quality_100_stuffs_a_byte_and_fills_a_block():
    for shape in inp.SHAPES:
        cover = inp.reference(shape, "noise", 100)[1]
        assert cover["stuffed_ff"] >= 1 and cover["no_eob_blocks"] >= 1, (shape, cover)


def test_impulses_at_quality_50_need_a_zrl():
    assert any(inp.reference(shape, "impulses", 50)[1]["zrl"] >= 1 for shape in inp.SHAPES)
    assert inp.reference((3, 40, 136, 3), "impulses", 50)[1]["zrl"] >= 1


def test_checkerboard_at_quality_100_reaches_the_largest_ac_category():
    for shape in inp.SHAPES:
        assert inp.reference(shape, "checker", 100)[1]["max_ac_category"] == 10, shape


def test_some_case_reaches_dc_category_10():
    assert max(inp.reference(*c)[1]["max_dc_category"] for c in inp.CASES) >= 10
    assert inp.reference((2, 24, 40), "flat", 100)[1]["max_dc_category"] >= 10


def test_the_tall_case_has_ten_intervals_and_wraps_the_restart_counter():
    jpegs, cover = inp.reference((1, 80, 8, 3), "noise", 90)
    assert cover["intervals"] == 10
    scan = jpegs[0][len(mjpeg.jpeg_header(80, 8, 3, 90)):]
    marks = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
    assert marks == [0xD0 + (i & 7) for i in range(9)]


def test_coverage_record_counts_what_the_stream_holds():
    jpegs, cover = inp.reference((3, 40, 136, 3), "noise", 100)
    head = len(mjpeg.jpeg_header(40, 136, 3, 100))
    assert sum(j[head:-2].count(b"\xff\x00") for j in jpegs) == cover["stuffed_ff"]


# --------------------------------------------------------------------------------------------------- quality against PIL's encoder
def quality_images():
    d = (np.add.outer(np.arange(136), np.arange(200)) / 336).astype(np.float32)[None]
    return {"ramp": visualize.colorize_numpy(d)[0], "noise": np.random.default_rng(5).integers(0, 256, (136, 200, 3), dtype=np.uint8),
            "gray ramp": visualize.colorize_numpy(d, grayscale=True)[0]}


def psnr_pair(img, q):
    """(twin, PIL's encoder) PSNR to the source in dB: the same tables, 4:4:4, both streams decoded by PIL."""
    qt = mjpeg.quant_tables(q)
    ours = np.asarray(pil_decode(mjpeg.encode_jpeg_numpy(img[None], q)[0]))
    tabs = [qt[t].tolist() for t in range(2 if img.ndim == 3 else 1)]
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", qtables=tabs, subsampling=0)
    theirs_im = pil_decode(buf.getvalue())
    assert pil_tables(theirs_im) == {t: qt[t].tolist() for t in range(len(tabs))}       # PIL did use these tables
    return inp.psnr(ours, img), inp.psnr(np.asarray(theirs_im), img)


@pytest.mark.parametrize("q", [50, 75, 90])
def test_quality_is_within_the_margin_of_pils_encoder(q):
    for name, img in quality_images().items():
        ours, theirs = psnr_pair(img, q)
        print(f"{name} q{q}: twin {ours:.3f} dB, PIL {theirs:.3f} dB, {ours - theirs:+.3f}")
        assert ours >= theirs - PSNR_MARGIN_DB, (name, q, ours, theirs)


# ------------------------------------------------------------------------------------------------------------------ container
def avi_case():
    jpegs = [j for c in ("noise", "ramp") for j in inp.reference((2, 17, 23, 3), c, 90)[0]]
    assert len({len(j) & 1 for j in jpegs}) == 2                             # odd and even lengths: the padding is exercised
    return jpegs


def test_avi_round_trip_and_structure(tmp_path):
    jpegs = avi_case()
    path = str(tmp_path / "a.avi")
    assert mjpeg.write_avi(path, jpegs, 23.976, 23, 17) == len(jpegs)
    back, fps, w, h = mjpeg.read_avi(path)
    assert back == jpegs and (w, h) == (23, 17) and fps == pytest.approx(23.976, abs=1e-9)
    data = open(path, "rb").read()
    assert mjpeg.is_mjpeg_avi(path)
    assert data[:4] == b"RIFF" and struct.unpack_from("<I", data, 4)[0] == len(data) - 8 and data[8:12] == b"AVI "
    # every chunk at an even offset, the lists' sizes consistent with what they hold, the top level ending with the file
    seen = []

    def walk(lo, hi):
        while lo < hi:
            assert lo % 2 == 0
            tag, size = data[lo:lo + 4], struct.unpack_from("<I", data, lo + 4)[0]
            assert lo + 8 + size <= hi
            seen.append(tag if tag != b"LIST" else tag + data[lo + 8:lo + 12])
            if tag == b"LIST":
                walk(lo + 12, lo + 8 + size)
            lo += 8 + size + (size & 1)
        assert lo == hi
    walk(12, len(data))
    assert seen == [b"LISThdrl", b"avih", b"LISTstrl", b"strh", b"strf", b"LISTmovi"] + [b"00dc"] * len(jpegs) + [b"idx1"]
    movi = data.index(b"movi")
    idx = data.rindex(b"idx1")
    for i, j in enumerate(jpegs):
        tag, flags, off, ln = struct.unpack_from("<4sIII", data, idx + 8 + 16 * i)
        assert tag == b"00dc" and ln == len(j) and data[movi + off:movi + off + 4] == b"00dc" and data[movi + off + 8:movi + off + 8 + ln] == j
    avih = data.index(b"avih") + 8
    assert struct.unpack_from("<I", data, avih + 16)[0] == len(jpegs)           # dwTotalFrames
    strh = data.index(b"strh") + 8
    assert data[strh:strh + 8] == b"vidsMJPG" and struct.unpack_from("<II", data, strh + 20) == (1000, 23976)
    assert struct.unpack_from("<I", data, strh + 32)[0] == len(jpegs)           # dwLength
    strf = data.index(b"strf") + 8
    assert struct.unpack_from("<Iii", data, strf) == (40, 23, 17) and data[strf + 16:strf + 20] == b"MJPG"


def test_avi_takes_a_generator_of_unknown_length(tmp_path):
    jpegs = avi_case()
    a, b = str(tmp_path / "a.avi"), str(tmp_path / "b.avi")
    mjpeg.write_avi(a, jpegs, 10, 23, 17)
    mjpeg.write_avi(b, (j for j in jpegs), 10, 23, 17)
    assert open(a, "rb").read() == open(b, "rb").read()


def test_avi_refuses_to_pass_4_gib(tmp_path, monkeypatch):
    jpegs = avi_case()
    real = mjpeg._file_size
    monkeypatch.setattr(mjpeg, "_file_size", lambda f: real(f) + (1 << 32) - 4000)      # as if 4 GiB - 4000 bytes were written already
    with pytest.raises(ValueError, match=r"4 GiB.*frame 2"):
        mjpeg.write_avi(str(tmp_path / "big.avi"), jpegs, 10, 23, 17)


def test_read_avi_refuses_what_it_did_not_write(tmp_path):
    path = str(tmp_path / "a.avi")
    mjpeg.write_avi(path, avi_case(), 10, 23, 17)
    data = open(path, "rb").read()
    bad = str(tmp_path / "bad.avi")
    open(bad, "wb").write(data[:-3])
    with pytest.raises(ValueError, match="RIFF"):
        mjpeg.read_avi(bad)
    open(bad, "wb").write(data.replace(b"vidsMJPG", b"vidsH264"))
    with pytest.raises(ValueError, match="MJPG"):
        mjpeg.read_avi(bad)
    assert not mjpeg.is_mjpeg_avi(bad)


# --------------------------------------------------------------------------------------------------------------- the callers
def test_save_video_mjpeg_on_source_frames_and_back_through_read_video_frames(tmp_path):
    frames = np.concatenate([inp.frames((3, 40, 136, 3), "ramp"), inp.frames((3, 40, 136, 3), "impulses")])
    path = dc_utils.save_video(frames, str(tmp_path / "clip_src.mp4"), fps=12, codec="mjpeg", quality=90)
    assert path == str(tmp_path / "clip_src.avi") and os.path.exists(path) and not os.path.exists(str(tmp_path / "clip_src.mp4"))
    jpegs, fps, w, h = mjpeg.read_avi(path)
    assert jpegs == mjpeg.encode_jpeg_numpy(frames, 90) and fps == 12 and (w, h) == (136, 40)
    back, fps = dc_utils.read_video_frames(path, -1)
    assert back.shape == frames.shape and back.dtype == np.uint8 and fps == 12
    direct = np.stack([np.asarray(pil_decode(j)) for j in jpegs])
    assert np.array_equal(back, direct) and inp.psnr(back[:3], frames[:3]) > 35.0
    assert dc_utils.read_video_frames(path, 2)[0].shape == (2, 40, 136, 3)


def test_save_video_mjpeg_on_depth(tmp_path, monkeypatch):
    monkeypatch.setattr(dc_utils, "SAVE_BLOCK", 2)                           # three blocks: the file does not depend on the block size
    rng = np.random.default_rng(11)
    depths = (np.add.outer(np.arange(37), np.arange(53))[None] * (1 + np.arange(5))[:, None, None] + rng.random((5, 37, 53))).astype(np.float32)
    table = visualize.inferno_table()
    for gray in (False, True):
        path = dc_utils.save_video(depths, str(tmp_path / f"d{gray}_vis.mp4"), fps=24, is_depths=True, grayscale=gray, palette=table, codec="mjpeg")
        assert path.endswith("_vis.avi")
        vis = visualize.colorize_numpy(depths, grayscale=gray, palette=table)
        jpegs, fps, w, h = mjpeg.read_avi(path)
        assert jpegs == mjpeg.encode_jpeg_numpy(vis, 90) and fps == 24 and (w, h) == (53, 37)
        back = np.stack([np.asarray(pil_decode(j)) for j in jpegs])
        assert back.shape == vis.shape
        for i, f in enumerate(vis):                                          # the bound of the quality test, on these very frames
            _, theirs = psnr_pair(f, 90)
            assert inp.psnr(back[i], f) >= theirs - PSNR_MARGIN_DB, (gray, i)
    with pytest.raises(ValueError, match="codec"):
        dc_utils.save_video(depths, str(tmp_path / "x.mp4"), is_depths=True, codec="h264")
    with pytest.raises(ValueError, match="quality"):
        dc_utils.save_video(depths, str(tmp_path / "x.mp4"), is_depths=True, codec="mjpeg", quality=0)


def test_the_kernel_sources_constants_are_the_twins():
    """csrc/mjpeg.hip holds the DCT matrix, the zig-zag positions and the Huffman codes as literals: the same numbers as the twin's,
    which derives them (the GPU tests compare the bytes; this pins the tables without a GPU)."""
    import re
    text = open(os.path.join(os.path.dirname(mjpeg.__file__), "csrc", "mjpeg.hip")).read()

    def literal(name):
        body = text[text.index(name):]
        body = body[body.index("=") + 1:body.index(";")]
        return [int(v, 0) for v in re.findall(r"-?(?:0x[0-9a-fA-F]+|\d+)", body)]
    assert literal("MJ_DCT[8][8]") == mjpeg.DCT_MATRIX.reshape(-1).tolist()
    assert literal("MJ_ZIGZAG_OF[64]") == np.argsort(mjpeg.ZIGZAG).tolist()
    assert literal("MJ_HUFF[2][MJ_HUFF_N]") == mjpeg.huffman_words().reshape(-1).tolist()
