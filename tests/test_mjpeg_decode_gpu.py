"""mjpeg.decode_jpeg / vda_mjpeg_decode_u8 (csrc/mjpeg_decode.hip) on the MI355X: the device's pixels are the host twin
decode_jpeg_numpy's pixels, byte for byte, for every good stream of _mjpeg_decode_inputs.py (PIL's 4:4:4, 4:2:2, 4:2:0 and gray
streams of 8x8 to 40x136 with and without restart markers, the project's own streams, streams without DHT), and its statuses for
the corrupt corpus - which tests/test_mjpeg_decode_core_host.py has run through the same decoder text under sanitizers on the
host. The shapes put one block, ragged edges, odd chroma planes, one interval per frame (a single lane), and 85 intervals (more
than a workgroup's 64 lanes, a wrapping RSTm number) in front of the kernels; every call is a few milliseconds."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _mjpeg_decode_inputs as dinp
import _mjpeg_inputs as inp

pytestmark = pytest.mark.gpu
FILL, GUARD = 0xA5, 64
GOLDEN = dinp.golden()[0]


@pytest.mark.parametrize("item", GOLDEN, ids=dinp.golden_id)
def test_device_pixels_are_the_twins_on_the_golden_streams(item):
    from video_depth_anything_amd import mjpeg
    _, jpeg, pil_pixels = item
    got = mjpeg.decode_jpeg([jpeg], device="cuda")
    assert got.dtype == np.uint8 and np.array_equal(got, dinp.twin_pixels((jpeg,)))
    assert np.array_equal(got[0], pil_pixels)


@pytest.mark.parametrize("case", dinp.OWN, ids=dinp.own_id)
def test_device_pixels_are_the_twins_on_the_encoders_streams(case):
    from video_depth_anything_amd import mjpeg
    jpegs = dinp.own(case)
    want = dinp.twin_pixels(tuple(jpegs))
    assert np.array_equal(mjpeg.decode_jpeg(jpegs, device="cuda"), want)
    assert np.array_equal(mjpeg.decode_jpeg([dinp.strip_dht(j) for j in jpegs], device="cuda"), want)        # the Annex K tables implied


def test_a_stream_without_restart_markers_takes_one_lane_per_frame():
    from video_depth_anything_amd import mjpeg
    items = [it for it in GOLDEN if it[0]["restart"] == "none" and (it[0]["h"], it[0]["w"]) == (40, 136)]
    assert items
    for _, jpeg, px in items:
        info = mjpeg.parse_jpeg(jpeg)
        scan, iv, _ = mjpeg.device_call_inputs([jpeg] * 3, info)
        assert iv.shape[0] == 3 and iv[:, 4].tolist() == [info.mcus[0] * info.mcus[1]] * 3
        got = mjpeg.decode_jpeg([jpeg] * 3, device="cuda")
        assert all(np.array_equal(g, px) for g in got)


def test_more_intervals_than_one_workgroup_holds():
    from video_depth_anything_amd import mjpeg
    items = [it for it in GOLDEN if it[0]["restart"] == "mcu" and (it[0]["h"], it[0]["w"]) == (40, 136)]
    assert {it[0]["sampling"] for it in items} >= {"444", "420"}
    for meta, jpeg, px in items:
        info = mjpeg.parse_jpeg(jpeg)
        n_iv = mjpeg.scan_intervals(jpeg, info)[0].shape[0]
        assert n_iv == info.mcus[0] * info.mcus[1] and (meta["sampling"] != "444" or n_iv == 85)
        got = mjpeg.decode_jpeg([jpeg, jpeg], device="cuda")                 # 170 intervals in 4:4:4: three workgroups, the last ragged
        assert np.array_equal(got[0], px) and np.array_equal(got[1], px)


def test_frames_with_different_headers_are_grouped_into_two_calls(monkeypatch):
    from video_depth_anything_amd import mjpeg, ops
    a, b = dinp.own(((3, 40, 136, 3), "ramp", 90)), dinp.own(((3, 40, 136, 3), "noise", 100))
    calls = []
    real = ops.mjpeg_decode
    monkeypatch.setattr(ops, "mjpeg_decode", lambda *args: (calls.append(args[7].shape[0]), real(*args))[1])
    got = mjpeg.decode_jpeg(a + b[:2], device="cuda")
    assert calls == [3, 2]
    assert np.array_equal(got, np.concatenate([dinp.twin_pixels(tuple(a)), dinp.twin_pixels(tuple(b))[:2]]))


@pytest.mark.parametrize("sampling", ["444", "420", "gray"])
def test_tensor_out_and_nothing_written_outside_it(sampling):
    from video_depth_anything_amd import mjpeg, ops
    meta, jpeg, px = next(it for it in GOLDEN if it[0]["sampling"] == sampling and (it[0]["h"], it[0]["w"]) == (33, 50))
    t = mjpeg.decode_jpeg([jpeg, jpeg], device="cuda", to_host=False)
    assert t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == (2,) + px.shape
    assert np.array_equal(t.cpu().numpy()[1], px)
    # the raw entry point into a guarded, pre-filled buffer: the pixels, then nothing
    info = mjpeg.parse_jpeg(jpeg)
    scan, iv, _ = mjpeg.device_call_inputs([jpeg, jpeg], info)
    cap = 2 * px.size
    buf = torch.full((GUARD + cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    work = torch.empty(ops.mjpeg_decode_workspace_bytes(2, 33, 50, info.components, info.hs, info.vs, iv.shape[0]), dtype=torch.uint8, device="cuda")
    st = torch.full((2 + 2,), 99, dtype=torch.int32, device="cuda")
    ops.mjpeg_decode(torch.from_numpy(scan.copy()).cuda(), iv, mjpeg.decode_tables(info), info.qtables, info.hs, info.vs, work,
                     buf[GUARD:GUARD + cap].view((2,) + px.shape), st[1:3])
    got = buf.cpu().numpy()
    assert np.array_equal(got[GUARD:GUARD + cap].reshape((2,) + px.shape), np.stack([px, px]))
    assert (got[:GUARD] == FILL).all() and (got[GUARD + cap:] == FILL).all()
    assert st.tolist() == [99, 0, 0, 99]


def test_two_calls_give_identical_bytes():
    from video_depth_anything_amd import mjpeg
    jpegs = dinp.own(((3, 40, 136, 3), "noise", 100))
    first = mjpeg.decode_jpeg(jpegs, device="cuda", to_host=False).clone()
    for _ in range(3):
        assert torch.equal(first, mjpeg.decode_jpeg(jpegs, device="cuda", to_host=False))


def test_the_corrupt_corpus_gives_the_twins_statuses_and_the_device_carries_on():
    from video_depth_anything_amd import mjpeg
    good = dinp.good_17x23()
    for name, jpeg, want in dinp.corrupt():
        with pytest.raises(ValueError) as e:
            mjpeg.decode_jpeg([jpeg], device="cuda")
        assert want in str(e.value) and "frame 0" in str(e.value), name
        assert not isinstance(e.value, mjpeg.UnsupportedJpeg)
    # one call with good frames around the bad ones: each frame its own status, the first bad one reported
    bad = [c[1] for c in dinp.corrupt() if mjpeg.parse_jpeg(c[1]).header == mjpeg.parse_jpeg(good).header]
    assert len(bad) >= 6
    with pytest.raises(ValueError, match="frame 1 "):
        mjpeg.decode_jpeg([good] + bad + [good], device="cuda")
    torch.cuda.synchronize()
    assert np.array_equal(mjpeg.decode_jpeg([good], device="cuda"), dinp.twin_pixels((good,)))


def test_corrupt_frames_leave_the_twins_coefficients_pixels():
    """Bit-identical for corrupt streams too: a frame that ends in a status still has defined pixels - the coefficients decoded
    before the error, zeros behind it - and they are the twin's."""
    from video_depth_anything_amd import mjpeg, ops
    for name, jpeg, _ in dinp.corrupt():
        info = mjpeg.parse_jpeg(jpeg)
        coef, status = mjpeg.decode_coefficients(jpeg, info)
        want = mjpeg.pixels_from_coefficients(coef[None], info)
        scan, iv, host_status = mjpeg.device_call_inputs([jpeg], info)
        out = torch.empty(want.shape, dtype=torch.uint8, device="cuda")
        work = torch.empty(ops.mjpeg_decode_workspace_bytes(1, info.height, info.width, info.components, info.hs, info.vs, iv.shape[0]),
                           dtype=torch.uint8, device="cuda")
        st = torch.empty(1, dtype=torch.int32, device="cuda")
        ops.mjpeg_decode(torch.from_numpy(scan.copy()).cuda(), iv, mjpeg.decode_tables(info), info.qtables, info.hs, info.vs, work, out, st)
        assert max(int(st[0]), int(host_status[0])) == status, name
        assert np.array_equal(out.cpu().numpy(), want), name


def test_round_trip_through_both_device_codecs():
    from video_depth_anything_amd import mjpeg
    shape = (3, 40, 136, 3)
    x = inp.frames(shape, "ramp")
    jpegs = mjpeg.encode_jpeg(x, 90, device="cuda")
    assert jpegs == inp.reference(shape, "ramp", 90)[0]
    assert np.array_equal(mjpeg.decode_jpeg(jpegs, device="cuda"), dinp.twin_pixels(tuple(jpegs)))


def test_read_video_frames_and_frame_blocks_on_the_device(tmp_path):
    from utils.dc_utils import read_video_frames
    from video_depth_anything_amd import mjpeg
    jpegs = dinp.own(((3, 40, 136, 3), "ramp", 90)) + dinp.own(((3, 40, 136, 3), "noise", 100))
    path = str(tmp_path / "clip.avi")
    mjpeg.write_avi(path, jpegs, 12.0, 136, 40)
    want = dinp.twin_pixels(tuple(jpegs))
    frames, fps = read_video_frames(path, -1, device="cuda")
    assert fps == 12.0 and np.array_equal(frames, want)
    blocks = list(mjpeg.avi_frame_blocks(path, device="cuda", block=4))
    assert [b.shape[0] for b in blocks] == [4, 2] and np.array_equal(np.concatenate(blocks), want)


@pytest.mark.parametrize("stream", [False, True], ids=["plain", "stream"])
def test_run_py_reads_an_mjpeg_avi_as_it_reads_the_same_frames_from_npz(tmp_path, stream):
    """The CLI end to end: clip.avi (written by write_avi) decoded on the device gives the _depths.npz that the same frames give
    as clip.npz, plain and with --stream (where avi_frame_blocks feeds the stream)."""
    from video_depth_anything_amd import mjpeg
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    jpegs = dinp.own(((3, 40, 136, 3), "ramp", 90))
    mjpeg.write_avi(str(tmp_path / "clip.avi"), jpegs, 12.0, 136, 40)
    np.savez(tmp_path / "clip.npz", frames=dinp.twin_pixels(tuple(jpegs)), fps=12.0)
    depths = {}
    for ext in ("avi", "npz"):
        out = tmp_path / f"out_{ext}"
        r = subprocess.run([sys.executable, os.path.join(repo, "run.py"), "--input_video", str(tmp_path / f"clip.{ext}"), "--output_dir", str(out),
                            "--encoder", "vits", "--input_size", "70", "--checkpoint", "synthetic", "--save_npz", "--mjpeg"]
                           + (["--stream"] if stream else []), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        depths[ext] = np.load(out / "clip_depths.npz")["depths"]
    assert depths["avi"].shape == (3, 40, 136) and np.array_equal(depths["avi"], depths["npz"])
