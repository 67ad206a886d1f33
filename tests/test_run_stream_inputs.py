"""What run.py --stream holds in memory, on the CPU: an .npy is fed to the stream block by block and <name>_src is written from the
memory map itself when nothing is scaled or dropped (run.stream_input, run.frames_for_writer); a source its decoder returns whole is
decoded once and that array reused."""
import types

import numpy as np

from _resize_u8_inputs import clip, frames


def source(path, max_len=-1, target_fps=-1, max_res=-1):
    return (str(path), max_len, target_fps, max_res)


def test_an_unscaled_npy_is_never_one_array(tmp_path):
    from run import frames_for_writer, stream_input
    from video_depth_anything_amd.scheduler import STEP
    x = frames(50, 12, 20, seed=7)
    np.save(tmp_path / "clip.npy", x)
    for src in (source(tmp_path / "clip.npy"), source(tmp_path / "clip.npy", max_res=1280), source(tmp_path / "clip.npy", max_len=47)):
        fed, fps, whole = stream_input(src, None)
        assert whole is None and fps == 24.0 and isinstance(fed, types.GeneratorType)
        blocks = list(fed)
        n = 47 if src[1] > 0 else 50
        assert [b.shape[0] for b in blocks] == [STEP, STEP, n - 2 * STEP] and np.array_equal(np.concatenate(blocks), x[:n])
        for_writer = frames_for_writer(src, None, whole)
        assert isinstance(for_writer, np.memmap) and for_writer.shape == (n, 12, 20, 3)          # still on disk: save_video reads it by blocks


def test_a_scaled_or_thinned_npy_is_fed_in_blocks_and_written_from_the_same_frames(tmp_path):
    from run import frames_for_writer, stream_input
    np.save(tmp_path / "clip.npy", frames(50, 12, 20, seed=7))
    for src in (source(tmp_path / "clip.npy", max_res=16), source(tmp_path / "clip.npy", target_fps=12)):
        fed, fps, whole = stream_input(src, None)
        assert whole is None and isinstance(fed, types.GeneratorType)
        assert np.array_equal(np.concatenate(list(fed)), frames_for_writer(src, None, whole))


def test_a_source_that_is_decoded_whole_is_decoded_once(tmp_path, monkeypatch):
    from run import frames_for_writer, stream_input
    from utils import dc_utils
    from video_depth_anything_amd import mjpeg
    x = clip(6, 16, 24)
    np.savez(tmp_path / "clip.npz", frames=x, fps=12.0)
    mjpeg.write_avi(str(tmp_path / "clip.avi"), mjpeg.encode_jpeg_numpy(x, 90), 12.0, 24, 16)
    calls = []
    decode = dc_utils._decode
    monkeypatch.setattr(dc_utils, "_decode", lambda path: calls.append(path) or decode(path))
    for name in ("clip.npz", "clip.avi"):                     # without a device the .avi is read whole by the host decoders
        del calls[:]
        src = source(tmp_path / name, max_res=16)
        fed, fps, whole = stream_input(src, None)
        assert fps == 12.0 and isinstance(whole, np.ndarray) and fed is whole and whole.shape == (6, 11, 16, 3)
        assert frames_for_writer(src, None, whole) is whole and len(calls) == 1


def test_reads_in_blocks_names_the_two_bounded_sources(tmp_path):
    from utils.dc_utils import reads_in_blocks
    from video_depth_anything_amd import mjpeg
    np.save(tmp_path / "clip.npy", frames(2, 4, 4))
    mjpeg.write_avi(str(tmp_path / "clip.avi"), mjpeg.encode_jpeg_numpy(clip(2, 8, 8), 90), 12.0, 8, 8)
    (tmp_path / "frames.npy").mkdir()
    assert reads_in_blocks(str(tmp_path / "clip.npy")) and reads_in_blocks(str(tmp_path / "clip.npy"), "cuda")
    assert reads_in_blocks(str(tmp_path / "clip.avi"), "cuda") and not reads_in_blocks(str(tmp_path / "clip.avi"))
    assert not reads_in_blocks(str(tmp_path / "clip.npz"), "cuda") and not reads_in_blocks(str(tmp_path / "frames.npy"), "cuda")
