"""staging.Staged on the MI355X: every block's device view holds the source slice bit for bit - for an array, a memory map, a
strided source and uint8 frames - the casting rule is numpy's, an empty source yields nothing, and a consumer that never
synchronises still sees every block (the upload of a block is finished before its host block is written again)."""
import numpy as np
import pytest
import torch

from video_depth_anything_amd.staging import Staged

pytestmark = pytest.mark.gpu


def source():
    """float32 [7,3,5] whose bits are all different, NaNs with payloads among them (frame 1 and frame 6)."""
    bits = (np.arange(7 * 3 * 5, dtype=np.int32) * 40503 + 12345).reshape(7, 3, 5)
    bits[1] |= 0x7FC00000
    bits[6, 0] = np.int32(-1) ^ np.arange(5, dtype=np.int32)                # 0xFFFFFFFF ...: negative quiet NaNs
    return bits.view(np.float32)


def walk(staged, src, view_as, **kw):
    """[(lo, m)] of the blocks, every view compared with the source slice as integers of type `view_as`."""
    seen = []
    for lo, m, x in staged.blocks(src, **kw):
        assert x.is_cuda and x.shape[0] == m and x.data_ptr() == staged.dev.data_ptr()
        got = x.cpu().numpy()
        assert np.array_equal(got.view(view_as), np.ascontiguousarray(src[lo:lo + m]).view(view_as))
        seen.append((lo, m))
    return seen


def test_blocks_hold_the_source_bit_for_bit(tmp_path):
    a = source()
    assert np.isnan(a).sum() >= 20
    staged = Staged(3, (3, 5), torch.float32)
    assert staged.host.is_pinned() and tuple(staged.host.shape) == (3, 3, 5) and staged.dev.is_cuda and staged.dev.shape == staged.host.shape
    assert walk(staged, a, np.int32) == [(0, 3), (3, 3), (6, 1)]
    mm = np.memmap(tmp_path / "a.bin", dtype=np.float32, mode="w+", shape=a.shape)
    mm[:] = a
    mm.flush()
    assert walk(staged, np.memmap(tmp_path / "a.bin", dtype=np.float32, mode="r", shape=a.shape), np.int32) == [(0, 3), (3, 3), (6, 1)]
    wide = np.zeros((7, 6, 5), np.float32)
    wide[:, ::2] = a
    strided = wide[:, ::2]
    assert not strided.flags.c_contiguous
    assert walk(staged, strided, np.int32) == [(0, 3), (3, 3), (6, 1)]      # the same Staged again: its blocks start over
    frames = np.random.default_rng(5).integers(0, 256, size=(5, 4, 6, 3), dtype=np.uint8)
    assert walk(Staged(2, (4, 6, 3), torch.uint8), frames, np.uint8) == [(0, 2), (2, 2), (4, 1)]
    assert walk(Staged(9, (4, 6, 3), torch.uint8), frames, np.uint8) == [(0, 5)]


def test_casting_is_numpys():
    d = np.arange(7 * 3 * 5, dtype=np.float64).reshape(7, 3, 5) / 3
    staged = Staged(3, (3, 5), torch.float32)
    got = np.concatenate([x.cpu().numpy() for _, _, x in staged.blocks(d, casting="same_kind")])
    assert got.dtype == np.float32 and np.array_equal(got, d.astype(np.float32))
    with pytest.raises(TypeError, match="Cannot cast"):
        next(staged.blocks(d))


def test_an_empty_source_yields_nothing():
    assert list(Staged(3, (3, 5), torch.float32).blocks(np.zeros((0, 3, 5), np.float32))) == []
    assert list(Staged(16, (), torch.uint8).blocks(np.zeros(0, np.uint8))) == []


def test_a_consumer_that_never_synchronises_sees_every_block():
    """64 blocks of one 1 MiB frame, frame k filled with k, added into an accumulator on the device with nothing between the blocks
    but the stream's order: every element is 0 + 1 + ... + 63 = 2016, exactly. (This runs the wait on the upload's event; it
    cannot show that a race is absent.)"""
    px = 1 << 18                                                            # int32: 1 MiB
    src = np.repeat(np.arange(64, dtype=np.int32)[:, None], px, axis=1)
    acc = torch.zeros(px, dtype=torch.int32, device="cuda")
    blocks = []
    for lo, m, x in Staged(1, (px,), torch.int32).blocks(src):
        acc.add_(x[0])
        blocks.append((lo, m))
    assert blocks == [(k, 1) for k in range(64)]
    got = acc.cpu().numpy()
    assert got.min() == 2016 and got.max() == 2016
