"""Host logic of infer_video_depth_stream without a GPU: the incremental window planner against plan_windows and the reference's
recorded window sources, the frame ring's slot allocator under the real issue order, and run_windows_stream (planner + chunk-wise
stitch, positions, trimming) against run_windows."""
import os

import numpy as np
import pytest

from video_depth_anything_amd import scheduler as S
from video_depth_anything_amd.config import INFER_LEN, INTERP_LEN

Z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "index_logic.npz"))
ARRIVALS = [1, 7, 22, 32, 64, None]                  # frames per block; None: all at once


def blocks_of(n, per):
    per = n if per is None else per
    return [min(per, n - i) for i in range(0, n, per)]


def feed_all(n, per):
    """Every window the planner returns for an n-frame stream arriving `per` frames at a time, with the arrival count at which
    each was returned (n + 1 stands for "at the end call")."""
    p = S.WindowPlanner()
    got, when = [], []
    for m in blocks_of(n, per):
        new = p.feed(m)
        got += new
        when += [p.arrived] * len(new)
        assert p.emitted == len(got)
    new = p.feed(end=True)
    got += new
    when += [n + 1] * len(new)
    return got, when


@pytest.mark.parametrize("per", ARRIVALS)
def test_incremental_planner_equals_plan_windows(per):
    for n in range(1, 151):
        got, _ = feed_all(n, per)
        assert got == S.plan_windows(n), (n, per)


@pytest.mark.parametrize("n", [1, 5, 22, 23, 32, 33, 54, 55, 100, 1024])
def test_incremental_planner_equals_the_references_loop(n):
    ref = Z[f"win_{n}"]
    for per in (1, 7, 64):
        got, _ = feed_all(n, per)
        assert ref.shape == (len(got), INFER_LEN)
        assert np.array_equal(np.array(got, dtype=np.int32), ref)


@pytest.mark.parametrize("per", ARRIVALS)
def test_windows_are_emitted_exactly_when_decidable(per):
    """Window k is decidable once frames through 22 k + 31 have arrived, or at the end: never returned earlier, always returned by
    the feed() call that makes it so."""
    for n in range(1, 151):
        got, when = feed_all(n, per)
        arrivals = np.cumsum(blocks_of(n, per)).tolist()
        for k, at in enumerate(when):
            need = S.STEP * k + INFER_LEN
            first = next((a for a in arrivals if a >= need), n + 1)         # the first call after which it is decidable
            assert at == first, (n, per, k, at, first)


def test_planner_refuses_an_empty_stream_and_use_after_the_end():
    with pytest.raises(ValueError, match="empty video"):
        S.WindowPlanner().feed(end=True)
    p = S.WindowPlanner()
    p.feed(3, end=True)
    with pytest.raises(RuntimeError):
        p.feed(1)


def test_named_bounds():
    assert S.READ_AHEAD == 52 and S.READ_AHEAD <= 3 * INFER_LEN == 96
    assert S.RING_FRAMES == 87 and S.RING_FRAMES <= 4 * INFER_LEN


@pytest.mark.parametrize("n", [1, 31, 32, 33, 54, 100, 1023, 1024, 10000])
def test_frame_ring_under_the_issue_order(n):
    """The device path's order: reserve window 0; then for every window k: issue it, reserve (prefetch) window k + 1; windows k - 1 and k
    count as in flight. No slot is reassigned while a reserved, unissued window references its frame (the ring asserts it, and it is
    re-checked here from the outside), frame 0 keeps slot 0, the slots in use never exceed the named capacity, and every window reads
    the frames it planned."""
    plan = S.plan_windows(n)
    ring = S.FrameRing()
    assert ring.capacity == S.RING_FRAMES
    content = {}                                     # slot -> frame, as the uploads would leave the device buffer

    def reserve(k):
        todo, evicted_reader = ring.reserve(k, plan[k])
        unissued = set(plan[k])
        for f, s in todo:
            old = content.get(s)
            assert old != 0 or f == 0, "frame 0 evicted"
            assert old is None or old not in unissued, (k, f, old)
            content[s] = f
        # what the upload stream waits for (the consumer's `freed` event of window k - 3) covers every window that read an evicted slot
        assert evicted_reader == -1 or evicted_reader <= k - 3, (k, evicted_reader)     # -1: nothing was evicted
        assert ring.in_use() <= S.RING_FRAMES and len(content) <= S.RING_FRAMES

    reserve(0)
    for k in range(len(plan)):
        slots = ring.slots(plan[k])
        assert [content[s] for s in slots] == plan[k], k              # the gather reads the planned frames
        if k >= 1:                                                    # window k - 1 may still be running: its frames are intact too
            assert all(content[ring.slot_of[f]] == f for f in plan[k - 1])
        ring.issued(k, plan[k])
        if k + 1 < len(plan):
            reserve(k + 1)
            assert all(content[ring.slot_of[f]] == f for f in plan[k]) and all(content[ring.slot_of[f]] == f for f in plan[k - 1] if k >= 1)
        assert content[0] == 0 and ring.slot_of[0] == 0
    assert ring.peak <= S.RING_FRAMES
    if n >= 200:
        assert ring.peak == S.RING_FRAMES, "the named capacity is the one that is needed, not a loose bound"


def test_frame_ring_refuses_a_capacity_below_the_schedules():
    plan = S.plan_windows(300)
    ring = S.FrameRing(S.RING_FRAMES - 2 * S.STEP - 12)              # too small for a window and its key frame
    with pytest.raises(AssertionError):
        ring.reserve(0, plan[0])
        for k in range(len(plan) - 1):
            ring.issued(k, plan[k])
            ring.reserve(k + 1, plan[k + 1])


def fake_window_fn(frames_u8):
    """Deterministic stand-in for the network: depends on the frame, on its slot and on its neighbours in the window."""
    x = frames_u8.astype(np.float32).mean(axis=-1)                   # [32,H0,W0]
    slot = np.arange(x.shape[0], dtype=np.float32)[:, None, None]
    return (x * (1.0 + 0.01 * slot) + 0.05 * np.roll(x, 1, axis=0) + 3.0 + x.mean() * 0.1).astype(np.float32)


@pytest.mark.parametrize("metric", [False, True])
@pytest.mark.parametrize("n", [1, 21, 22, 23, 24, 32, 33, 44, 50, 100])
def test_run_windows_stream_equals_run_windows(n, metric):
    rng = np.random.default_rng(n)
    frames = rng.integers(0, 256, (n, 6, 8, 3), dtype=np.uint8)
    want = S.run_windows(frames, fake_window_fn, metric=metric)
    sizes = rng.integers(1, 9, size=n)

    def ragged():
        i = 0
        for m in sizes:
            if i >= n:
                return
            yield frames[i] if m == 1 else frames[i:i + m]
            i += int(m)

    for source in (iter(frames), ragged(), iter([frames])):
        pieces = list(S.run_windows_stream(source, fake_window_fn, metric=metric))
        pos = 0
        for first, d in pieces:
            assert first == pos and d.dtype == np.float32 and d.shape[1:] == (6, 8) and d.shape[0] > 0
            pos += d.shape[0]
        assert pos == n
        natural = [INFER_LEN - INTERP_LEN] + [S.STEP] * (len(S.plan_windows(n)) - 1) + [INTERP_LEN]
        assert [d.shape[0] for _, d in pieces] == [c for c in np.diff(np.minimum(np.cumsum([0] + natural), n)).tolist() if c > 0]
        assert np.array_equal(np.concatenate([d for _, d in pieces]), want)


def test_run_windows_stream_refuses_an_empty_source():
    with pytest.raises(ValueError, match="empty video"):
        list(S.run_windows_stream(iter([]), fake_window_fn))
