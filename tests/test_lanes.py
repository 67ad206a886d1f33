"""lanes.py, the machinery infer_video_depth and infer_video_depth_stream share: frame validation and the run coalescer on the CPU,
the pinned device-to-host ring on the MI355X."""
import numpy as np
import pytest

from video_depth_anything_amd import lanes as L
from video_depth_anything_amd.scheduler import plan_windows

U8 = np.random.default_rng(3).integers(0, 256, (5, 6, 7, 3), dtype=np.uint8)


def test_as_u8_frames_accepts_8_bit_values_in_any_dtype():
    assert L.as_u8_frames(U8) is U8
    for dtype in (np.int64, np.float32):
        got = L.as_u8_frames(U8.astype(dtype))
        assert got.dtype == np.uint8 and np.array_equal(got, U8)
    assert np.array_equal(L.as_u8_frames(U8.tolist()), U8)
    assert L.as_u8_frames(U8, shape=(6, 7)) is U8
    for empty in (U8[:0], U8[:0].astype(np.float32)):
        got = L.as_u8_frames(empty, shape=(6, 7))
        assert got.dtype == np.uint8 and got.shape == (0, 6, 7, 3)


def test_as_u8_frames_refuses_everything_else():
    nan = U8.astype(np.float32)
    nan[2, 3, 4, 1] = np.nan
    for bad in (U8.astype(np.float32) / 255.0, U8.astype(np.float32) + 0.5, U8.astype(np.int32) * 2, nan):
        with pytest.raises(TypeError, match="8-bit"):
            L.as_u8_frames(bad)
    for bad in (U8[0], U8[..., :2]):                         # ndim 3 at the top level, a last dimension of 2
        with pytest.raises(ValueError, match=r"\[N, H, W, 3\]"):
            L.as_u8_frames(bad)
        with pytest.raises(ValueError, match=r"\[N, H, W, 3\]"):
            L.check_frames(bad)
    with pytest.raises(ValueError, match="first frame's size"):
        L.as_u8_frames(U8, shape=(6, 8))


def test_coalesce_runs():
    assert L.coalesce_runs([(5, 1), (6, 2), (7, 3), (9, 4), (10, 5)]) == [(5, 1, 3), (9, 4, 2)]      # frames 5..7 and 9..10
    assert L.coalesce_runs([(86, 86), (87, 1)]) == [(86, 86, 1), (87, 1, 1)]                           # the ring wraps: slot jump
    assert L.coalesce_runs([(3, 0), (4, 1), (5, 3)]) == [(3, 0, 2), (5, 3, 1)]
    assert L.coalesce_runs([]) == []


@pytest.mark.parametrize("n", [1, 23, 100])
def test_coalesced_runs_cover_each_window(n):
    """As the array path uploads: every distinct frame of a window exactly once, into the slot it was given."""
    plan = plan_windows(n)
    slot_of = {f: i for i, f in enumerate(sorted({f for w in plan for f in w}))}
    for win in plan:
        need = sorted(set(win))
        runs = L.coalesce_runs([(f, slot_of[f]) for f in need])
        assert [f0 + i for f0, _, m in runs for i in range(m)] == need
        assert all(s0 + i == slot_of[f0 + i] for f0, s0, m in runs for i in range(m))
        assert not any((a[0] + a[2], a[1] + a[2]) == b[:2] for a, b in zip(runs, runs[1:])), "neighbouring runs could be one"


def test_upload_runs_pages_in_what_cannot_be_copied_directly():
    """The copies themselves, on CPU tensors: a source that delivers a run in pieces, read-only and strided ones among them."""
    import torch
    src = np.random.default_rng(4).integers(0, 256, (12, 2, 3, 3), dtype=np.uint8)
    locked = src.copy()
    locked.flags.writeable = False

    def fetch(f0, f1):                                       # pieces of at most 2 frames: plain, read-only, strided
        for lo in range(f0, f1, 2):
            hi = min(lo + 2, f1)
            yield lo, (src[lo:hi], locked[lo:hi], src[:, :, ::-1][lo:hi][:, :, ::-1])[lo % 3]

    video = torch.zeros(9, 2, 3, 3, dtype=torch.uint8)
    pairs = [(2, 1), (3, 2), (4, 3), (5, 4), (6, 5), (9, 6), (10, 8)]
    L.upload_runs(video, pairs, fetch)
    for f, s in pairs:
        assert np.array_equal(video[s].numpy(), src[f])
    assert not video[0].any() and not video[7].any()


# ------------------------------------------------------------------ the pinned ring, on the device
COUNTS = [24, 22, 22, 1, 22, 8, 3]


@pytest.mark.gpu
@pytest.mark.parametrize("nbuf", [2, 4])
def test_host_copy_ring(nbuf):
    """Pieces started in order and harvested nbuf - 1 steps late - one late with 2 buffers as stitch_stream and the streamed path
    do, three late with 4 as collect_pieces does. The contract: the view of piece i is read before piece i + nbuf is started (it
    is that piece's buffer), so the harvest copies."""
    import torch
    H0, W0 = 37, 45
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device="cuda").manual_seed(7)
    src = [torch.randn(24, H0, W0, generator=g, device=dev) for _ in COUNTS]
    want = [s[:c].cpu().numpy() for s, c in zip(src, COUNTS)]
    ring = L.HostCopyRing(nbuf, 24, H0, W0, dev)
    inflight, got = [], []
    for s, c in zip(src, COUNTS):
        inflight.append(ring.start(s, c))
        if len(inflight) == nbuf:                            # piece i - (nbuf - 1): the next start takes its buffer
            got.append(ring.wait(inflight.pop(0)).numpy().copy())
    for token in inflight:
        assert token[0] in ring.done                         # the token's event, as collect_pieces hands it to on_copied
        got.append(ring.wait(token).numpy().copy())
    ring.join()
    assert len(got) == len(COUNTS)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape == (COUNTS[i], H0, W0) and np.array_equal(a, b), i
