"""The decoder's host twin mjpeg.decode_jpeg_numpy (the contract of csrc/mjpeg_decode.hip), on the CPU: PIL's pixels
byte for byte on the golden streams, the encoder's own streams, streams without DHT, the corrupt corpus' statuses, what is refused
as unsupported, and the container's incremental reader. profiles/mjpeg/decode_quality.txt records the comparison with PIL."""
import importlib.util
import io
import os

import numpy as np
import pytest

import _mjpeg_decode_inputs as dinp
import _mjpeg_inputs as inp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN, MADE_BY = dinp.golden()


def pil():
    try:
        from PIL import Image
        return Image
    except ImportError:
        return None


@pytest.mark.parametrize("item", GOLDEN, ids=dinp.golden_id)
def test_twin_gives_pils_pixels_on_the_golden_streams(item):
    """No tolerance: the arithmetic is libjpeg's, and the fixture has no frame narrower than 5 pixels (where libjpeg-turbo's
    upsampler takes another edge path)."""
    from video_depth_anything_amd import mjpeg
    meta, jpeg, want = item
    assert meta["w"] >= 5
    got = mjpeg.decode_jpeg_numpy([jpeg])
    assert got.dtype == np.uint8 and got.shape == (1,) + want.shape
    assert np.array_equal(got[0], want)


def test_the_golden_streams_cover_what_they_claim():
    from video_depth_anything_amd import mjpeg
    seen = {key: set() for key in ("sampling", "quality", "restart", "content", "shape")}
    intervals = {}
    for meta, jpeg, _ in GOLDEN:
        info = mjpeg.parse_jpeg(jpeg)
        assert (info.height, info.width) == (meta["h"], meta["w"])
        assert (info.components, info.hs, info.vs) == {"444": (3, 1, 1), "422": (3, 2, 1), "420": (3, 2, 2), "gray": (1, 1, 1)}[meta["sampling"]]
        iv, status = mjpeg.scan_intervals(jpeg, info)
        assert status == 0
        mw, mh = info.mcus
        assert iv.shape[0] == {"none": 1, "mcu": mw * mh, "row": mh}[meta["restart"]]
        for key in seen:
            seen[key].add((meta["sampling"], (meta["h"], meta["w"]) if key == "shape" else meta[key]))
        if (meta["h"], meta["w"], meta["restart"]) == (40, 136, "mcu"):
            intervals[meta["sampling"]] = iv.shape[0]
    assert [len(seen[k]) for k in ("sampling", "quality", "restart", "content", "shape")] == [4, 12, 12, 12, 20]
    assert intervals["444"] == 85 and intervals["420"] == 27          # more than 8: the RSTm number wraps; more than a workgroup's 64 lanes


def test_the_fixture_regenerates_to_identical_bytes():
    Image = pil()
    if Image is None:
        pytest.skip("PIL is not importable: the fixture cannot be regenerated here")
    import PIL
    from PIL import features
    turbo = features.version("libjpeg_turbo") if features.check_feature("libjpeg_turbo") else None
    if (PIL.__version__, turbo) != (MADE_BY["pil"], MADE_BY["turbo"]):
        pytest.skip(f"the fixture was made by PIL {MADE_BY['pil']} / libjpeg-turbo {MADE_BY['turbo']}, here are {PIL.__version__} / {turbo}")
    spec = importlib.util.spec_from_file_location("gen_mjpeg_decode_golden", os.path.join(REPO, "tools", "gen_mjpeg_decode_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    made = gen.build()
    stored = np.load(dinp.GOLDEN)
    assert sorted(made) == sorted(stored.files)
    for name in stored.files:
        assert np.array_equal(made[name], stored[name]), name


MARGIN_DB = 3.0


def documented_noise_db():
    """{quality: dB} from profiles/mjpeg/quality.txt: the twin encoder's PSNR on noise, the smaller of the two sizes recorded."""
    out = {}
    for line in open(os.path.join(REPO, "profiles", "mjpeg", "quality.txt")):
        cells = [c.strip() for c in line.split("|")]
        if cells[0].startswith("noise,"):
            out[int(cells[1])] = min(out.get(int(cells[1]), np.inf), float(cells[2]))
    return out


def psnr_floor(content, q):
    """The least PSNR to the source that a right decode of an OWN case can have, whether PIL is there or not.

    noise, ramp: the encoder's documented figure for NOISE at that quality (profiles/mjpeg/quality.txt: 50.42 dB at 100, 29.94 at 90)
    less MARGIN_DB. Noise is the content on which every coefficient of every block carries a full quantisation error, so no other
    content is coded worse at the same tables; the ramp's own documented figure (49 dB at 90) is for a 136 x 200 frame whose colours
    change a third as fast per pixel as those of the 8 x 8 and 17 x 23 ramps here, and does not carry over to them. The margin, a
    factor of 2 in mean squared error, covers the spread of a mean over as few as 64 pixels against one over 27 200.
    checker: quality.txt has no such content, so the floor is proved instead. R = G = B, so Cb = Cr = 128 exactly and the chroma
    blocks are all zero: the error is the luminance's. Each of its 64 coefficients is off by at most Q / 2 and the DCT is
    orthonormal, so the root mean squared error is at most sqrt(mean(Q^2) / 4), plus 1 level for the fixed-point transforms' and the
    colour conversion's roundings; clamping to 0..255 only brings a sample closer to a source that is in range."""
    if content == "checker":
        from video_depth_anything_amd import mjpeg
        rms = np.sqrt(np.mean(mjpeg.quant_tables(q)[0].astype(np.float64) ** 2) / 4) + 1.0
        return 10 * np.log10(255.0 ** 2 / rms ** 2)
    return documented_noise_db()[q] - MARGIN_DB


def test_the_psnr_floors_are_the_documented_figures():
    assert documented_noise_db() == {50: 16.771, 75: 22.279, 90: 29.942, 95: 35.771, 100: 50.419}
    assert psnr_floor("noise", 100) == pytest.approx(47.419) and psnr_floor("ramp", 90) == pytest.approx(26.942)
    assert 16.5 < psnr_floor("checker", 50) < 18.5        # Annex K luminance at quality 50: sqrt(mean(Q^2)) / 2 + 1 is about 34 levels


@pytest.mark.parametrize("case", dinp.OWN, ids=dinp.own_id)
def test_twin_on_the_encoders_streams(case):
    """Every decoded frame is the source within the encoder's documented loss (psnr_floor, with or without PIL), and is PIL's
    decode of the same bytes when PIL is there."""
    shape, content, q = case
    jpegs = dinp.own(case)
    got = dinp.twin_pixels(tuple(jpegs))
    src = inp.frames(shape, content)
    assert got.shape == src.shape and got.dtype == np.uint8
    floor = psnr_floor(content, q)
    for i, (g, f) in enumerate(zip(got, src)):
        db = inp.psnr(g, f)
        print(f"{dinp.own_id(case)} frame {i}: {db:.3f} dB, floor {floor:.3f}")
        assert db >= floor, (i, db, floor)
    Image = pil()
    if Image is not None:
        for g, j in zip(got, jpegs):
            assert np.array_equal(g, np.asarray(Image.open(io.BytesIO(j))))


@pytest.mark.parametrize("case", dinp.OWN, ids=dinp.own_id)
def test_a_stream_without_dht_decodes_with_the_annex_k_tables(case):
    from video_depth_anything_amd import mjpeg
    jpegs = dinp.own(case)
    bare = [dinp.strip_dht(j) for j in jpegs]
    assert all(b"\xff\xc4" not in b[:mjpeg.parse_jpeg(b).scan_offset] and len(b) < len(j) for b, j in zip(bare, jpegs))
    assert np.array_equal(mjpeg.decode_jpeg_numpy(bare), dinp.twin_pixels(tuple(jpegs)))


@pytest.mark.parametrize("name,jpeg,want", dinp.corrupt(), ids=[c[0] for c in dinp.corrupt()])
def test_a_corrupt_stream_raises_with_its_status(name, jpeg, want):
    from video_depth_anything_amd import mjpeg
    coef, status = mjpeg.decode_coefficients(jpeg)
    assert mjpeg.DECODE_STATUS[status] == want
    good = dinp.good_17x23()
    with pytest.raises(ValueError) as e:
        mjpeg.decode_jpeg_numpy([good, jpeg] if mjpeg.parse_jpeg(jpeg).width == 23 else [jpeg])
    assert not isinstance(e.value, mjpeg.UnsupportedJpeg)
    assert want in str(e.value) and f"frame {1 if mjpeg.parse_jpeg(jpeg).width == 23 else 0}" in str(e.value)


def test_every_status_has_a_name_and_a_case():
    from video_depth_anything_amd import mjpeg
    assert sorted(mjpeg.DECODE_STATUS) == list(range(8)) and mjpeg.DECODE_STATUS[0] == "ok"
    assert {c[2] for c in dinp.corrupt()} == {mjpeg.DECODE_STATUS[s] for s in range(1, 8)}


@pytest.mark.parametrize("name,jpeg,word", dinp.unsupported(), ids=[c[0] for c in dinp.unsupported()])
def test_what_is_not_read_raises_unsupported(name, jpeg, word):
    from video_depth_anything_amd import mjpeg
    assert issubclass(mjpeg.UnsupportedJpeg, ValueError)
    for fn in (mjpeg.parse_jpeg, lambda j: mjpeg.decode_jpeg_numpy([j])):
        with pytest.raises(mjpeg.UnsupportedJpeg, match=word):
            fn(jpeg)


def test_garbage_is_refused_not_crashed_on():
    from video_depth_anything_amd import mjpeg
    good = dinp.good_17x23()
    for bad in (b"", b"\xff\xd8", b"not a jpeg at all", good[:40], good[:mjpeg.parse_jpeg(good).scan_offset - 3]):
        with pytest.raises(mjpeg.UnsupportedJpeg):
            mjpeg.parse_jpeg(bad)
    # 16-bit DQT: the precision nibble of the first table
    dqt = good.index(b"\xff\xdb")
    with pytest.raises(mjpeg.UnsupportedJpeg, match="16-bit DQT"):
        mjpeg.parse_jpeg(good[:dqt + 4] + b"\x10" + good[dqt + 5:])
    with pytest.raises(ValueError, match="frame 1 is 8 x 8"):
        mjpeg.decode_jpeg_numpy([good, dinp.own(((1, 8, 8, 3), "noise", 100))[0]])
    with pytest.raises(ValueError, match="no frames"):
        mjpeg.decode_jpeg_numpy([])


def test_device_call_inputs_lay_the_scans_back_to_back():
    """The host side of a device call: frames of one header grouped, the intervals' offsets inside the concatenated scans."""
    from video_depth_anything_amd import mjpeg
    a, b = dinp.own(((2, 17, 23, 3), "noise", 90)), dinp.own(((2, 17, 23, 3), "noise", 100))
    groups = mjpeg._device_groups(a + b)
    assert [(g[1], g[2]) for g in groups] == [(0, 2), (2, 2)]
    info = groups[0][0]
    scan, iv, status = mjpeg.device_call_inputs(a, info)
    assert iv.dtype == np.int32 and iv.shape == (6, 5) and status.tolist() == [0, 0]
    assert iv[:, 0].tolist() == [0, 0, 0, 1, 1, 1] and iv[:, 3].tolist() == [0, 3, 6] * 2 and iv[:, 4].tolist() == [3] * 6
    so = info.scan_offset
    assert scan.tobytes() == a[0][so:] + a[1][so:]
    for f, lo, ln, _, _ in iv.tolist():
        assert 0 <= lo and lo + ln <= scan.size
        at = lo - (0 if f == 0 else len(a[0]) - so)
        assert scan[lo:lo + ln].tobytes() == a[f][so + at:so + at + ln]


def test_iter_avi_yields_read_avis_frames(tmp_path):
    from video_depth_anything_amd import mjpeg
    jpegs = dinp.own(((3, 40, 136, 3), "ramp", 90)) + dinp.own(((3, 40, 136, 3), "noise", 100))
    path = str(tmp_path / "clip.avi")
    mjpeg.write_avi(path, jpegs, 12.5, 136, 40)
    want, fps, w, h = mjpeg.read_avi(path)
    it = mjpeg.iter_avi(path)
    assert next(it) == (fps, w, h) == (12.5, 136, 40)
    assert list(it) == want == jpegs
    blocks = list(mjpeg.avi_frame_blocks(path, block=4))
    assert [b.shape for b in blocks] == [(4, 40, 136, 3), (2, 40, 136, 3)]
    assert np.array_equal(np.concatenate(blocks), dinp.twin_pixels(tuple(jpegs)))
    from video_depth_anything_amd.scheduler import STEP
    assert [b.shape[0] for b in mjpeg.avi_frame_blocks(path)] == [min(STEP, 6)]
    bad = tmp_path / "bad.avi"
    bad.write_bytes(b"RIFF\0\0\0\0WAVEfmt ")
    with pytest.raises(ValueError, match="not a RIFF AVI"):
        next(mjpeg.iter_avi(str(bad)))
    # a file that ends inside a frame, or between two frames inside the next chunk's header: a ValueError either way
    data = open(path, "rb").read()
    first = data.index(b"movi") + 4
    assert data[first:first + 4] == b"00dc"
    second = first + 8 + len(jpegs[0]) + (len(jpegs[0]) & 1)
    assert data[second:second + 4] == b"00dc"
    for cut, word in ((first + 8 + 100, "ends inside a frame"), (second + 3, "ends inside its movi list")):
        bad.write_bytes(data[:cut])
        with pytest.raises(ValueError, match=word):
            list(mjpeg.iter_avi(str(bad)))


def test_read_video_frames_without_a_device_is_unchanged(tmp_path, monkeypatch):
    """device=None is the default and takes the path it always took (decord, cv2, or read_avi + PIL): decode_jpeg is not called.
    Where PIL is missing too, that path ends in its ImportError as it always did - still without touching the device decoder."""
    from utils import dc_utils
    from video_depth_anything_amd import mjpeg
    jpegs = dinp.own(((3, 40, 136, 3), "ramp", 90))
    path = str(tmp_path / "clip.avi")
    mjpeg.write_avi(path, jpegs, 12.0, 136, 40)

    def never(*a, **k):
        raise AssertionError("the device decoder was called without a device")
    monkeypatch.setattr(mjpeg, "decode_jpeg", never)
    for kw in ({}, {"device": None}):
        if pil() is None:
            with pytest.raises(ImportError):
                dc_utils.read_video_frames(path, -1, **kw)
            continue
        frames, fps = dc_utils.read_video_frames(path, -1, **kw)
        assert fps == 12.0 and np.array_equal(frames, mjpeg.decode_jpegs(jpegs))
        assert np.array_equal(frames, dinp.twin_pixels(tuple(jpegs)))
