"""Sliding-window schedule, multi-GPU sharding and window stitching of infer_video_depth.

Host logic only (numpy); mirrors /root/reference/video_depth_anything/video_depth.py:187-254
and /root/reference/utils/util.py:40-74.

Key property: the overlap slots of window k are refilled from the previous
window's INPUT (video_depth.py:200-201), never from an output, so every window's 32 input
frames are a pure function of the source video. `plan_windows` resolves that recursion into
source-frame indices up front; windows are then independent units that can be computed in any
order / on any rank, and only the final stitch is sequential.
"""
from typing import Callable, List, Sequence, Tuple

import numpy as np

from .config import IMAGENET_MEAN, IMAGENET_STD, INFER_LEN, INTERP_LEN, KEYFRAMES, OVERLAP, PATCH


# ------------------------------------------------------------------ preprocessing geometry
def network_size(height: int, width: int, input_size: int = 518) -> Tuple[int, int]:
    """Network input (H, W) for a source frame: aspect guard (video_depth.py:167-171) then the
    keep-aspect, lower-bound, multiple-of-14 rule of Resize.get_size (util/transform.py:51-107)."""
    ratio = max(height, width) / min(height, width)
    if ratio > 1.78:
        input_size = int(input_size * 1.777 / ratio)
        input_size = round(input_size / 14) * 14

    def constrain(x, min_val):
        y = int(np.round(x / PATCH) * PATCH)
        if y < min_val:
            y = int(np.ceil(x / PATCH) * PATCH)
        return y

    scale = max(input_size / height, input_size / width)
    return constrain(scale * height, input_size), constrain(scale * width, input_size)


# ------------------------------------------------------------------ window schedule
STEP = INFER_LEN - OVERLAP                       # 22 new frames per window
PIECE_FRAMES = INFER_LEN - INTERP_LEN            # 24: the frames window 0 makes final, the largest piece; later windows fill STEP of it


def piece_position(k: int) -> Tuple[int, int]:
    """(first output frame, frame count) of the piece window k makes final (the device stitcher's chunk, its owner's piece)."""
    return (0, PIECE_FRAMES) if k == 0 else (STEP * k + (OVERLAP - INTERP_LEN), STEP)


def tail_position(n_windows: int) -> int:
    """First output frame of the INTERP_LEN-frame tail that is final once no window follows the n_windows-th."""
    return STEP * (n_windows - 1) + PIECE_FRAMES


def plan_windows(n_frames: int) -> List[List[int]]:
    """Source-frame index of every input slot of every window.

    video_depth.py:188-201: stride 22, the video is padded with copies of its last frame
    ((22 - n % 22) % 22 + 10 of them), and for k > 0 slots 0..9 are the previous window's
    slots KEYFRAMES. Padded positions map back to the last real frame."""
    if n_frames <= 0:
        raise ValueError("empty video")
    windows: List[List[int]] = []
    prev = None
    for start in range(0, n_frames, STEP):
        cur = [min(start + i, n_frames - 1) for i in range(INFER_LEN)]
        if prev is not None:
            cur[:OVERLAP] = [prev[k] for k in KEYFRAMES]
        windows.append(cur)
        prev = cur
    return windows


def shard_windows(n_windows: int, world: int, rank: int) -> range:
    """Round-robin partition: rank r computes windows r, r + world, r + 2*world, ... Round j of the job therefore holds the
    CONSECUTIVE windows j*world .. j*world + world - 1, one per rank: the all-gather of a round delivers windows in stitch
    order and the stitcher can run behind the rounds with a bounded ring of gathered windows."""
    return range(rank, n_windows, world)


def rounds(n_windows: int, world: int) -> int:
    return (n_windows + world - 1) // world


def drive_windows(n_windows: int, world: int, rank: int, send, recv, compute, gather, ready=None, release=None):
    """THE multi-rank schedule of infer_video_depth (device path and CPU rehearsal alike): yields every window's depth map,
    in window order, on every rank.

      send     ring of >= 2 buffers [32,H0,W0]: compute(k, s) fills send[s] with window k
      recv     ring of >= 2 buffers [world,32,H0,W0] (None when world == 1)
      gather   gather(s) -> handle with .wait() (or None when the call is synchronous): recv[s][r] = rank r's send[s]
      ready    ready(s): called before anything of slot s is yielded (device path: the consumer's stream waits for the slot's
               compute stream - slots are computed on their own HIP streams so that two windows are in flight)
      release  release(s): called once the consumer has taken (queued its reads of) everything yielded from slot s, i.e. before
               the slot is overwritten two rounds later (device path: records the event the slot's next compute waits for)

    Round j: this rank computes window j*world + rank (if it exists) into slot j % 2 and starts the round's all-gather; the
    PREVIOUS round's gather is then waited for and its windows are yielded, so the exchange of round j runs under the compute
    of round j + 1 and the consumer (the stitcher) works one round behind."""
    nslot = len(send)
    if world == 1:
        for k in range(n_windows):
            s = k % nslot
            compute(k, s)
            if ready is not None:
                ready(s)
            yield send[s]
            if release is not None:
                release(s)
        return
    pending = None

    def harvest(p):
        j, s, h = p
        if h is not None:
            h.wait()
        if ready is not None:
            ready(s)
        for r in range(world):
            if j * world + r < n_windows:
                yield recv[s][r]
        if release is not None:
            release(s)

    for j in range(rounds(n_windows, world)):
        s = j % nslot
        k = j * world + rank
        if k < n_windows:
            compute(k, s)
        h = gather(s)
        if pending is not None:
            yield from harvest(pending)
        pending = (j, s, h)
    yield from harvest(pending)


# ------------------------------------------------------------------ the exchange that moves only what the stitch chain needs
# SURVEY.md section 8(e), "optional refinement": the only dependence BETWEEN windows in video_depth.py:216-250 is the chain
#   (scale_k, shift_k) = lsq(window k slots [0, 1]  ->  [window 0 slot 0, aligned window k-1 slot 12])
# plus the 8-frame cross-fade of window k's slots 2..9 into window k-1's aligned slots 24..31. So instead of all-gathering whole
# windows (32 frames per rank and round) the ranks all-gather 11 KEY frames per window - slots 0, 1 (the alignment pair), 12 (the
# next reference) and 24..31 (the tail the next window's owner cross-fades into) -, every rank runs the scale/shift chain on them,
# and each rank FINALISES ITS OWN windows: window k > 0 yields the 22 output frames 22k+2 .. 22k+23, window 0 the frames 0..23,
# the last window also its tail. Only those final pieces travel to the ranks that want the video.
# Per round and rank: 11 frames all-gathered + 22..24 sent to each result rank, against 32 all-gathered; a rank that is not a
# result rank receives 7 x 11 instead of 7 x 32 frames on 8 GPUs, and the stitch work is spread over the ranks.
KEY_SLOTS = (0, 1, 12, 24, 25, 26, 27, 28, 29, 30, 31)


def drive_windows_keys(n_windows: int, world: int, rank: int, ops, result_ranks=None):
    """The key-frame schedule (device path and CPU rehearsal alike): yields (first output frame, count, frames[count..]) pieces,
    every piece of the video exactly once, on the ranks in `result_ranks` (None = every rank); nothing elsewhere.

    ops.compute(k, s)          window k into slot s of a two-slot ring, its KEY_SLOTS frames into the slot's key buffer
    ops.gather_keys(s)         start the all-gather of the slot's key buffers; returns a handle with .wait() or None
    ops.chain(k, s, r)         advance the scale/shift chain by window k, whose key frames are rank r's entry of slot s's gather
                               (called on every rank for every window, in window order)
    ops.finalise(k, s)         this rank's window k (still in slot s) -> its final piece, in the slot's piece buffer
    ops.deliver(s, j)          collective: the pieces of round j's windows to the result ranks; returns [(k, frames)] there, [] elsewhere
    ops.last_tail(k, owner)    the last window's aligned tail (8 frames): the chain holds it on every rank (its key frames are slots 24..31)
    Round j's key gather runs under round j + 1's compute; the chain, the finalisation and the delivery of a round happen one
    round behind, exactly as drive_windows harvests (and are issued before the next round's gather)."""
    mine = lambda k: k % world == rank                     # noqa: E731 - round-robin shards (shard_windows)
    wanted = result_ranks is None or rank in result_ranks
    pending = None

    def harvest(p):
        j, s, h = p
        if h is not None:
            h.wait()
        for r in range(world):
            k = j * world + r
            if k < n_windows:
                ops.chain(k, s, r)
        k = j * world + rank
        if k < n_windows:
            ops.finalise(k, s)
        for k2, frames in ops.deliver(s, j):
            pos, cnt = piece_position(k2)
            yield pos, cnt, frames

    nround = rounds(n_windows, world)
    for j in range(nround):
        s = j % 2
        k = j * world + rank
        if k < n_windows:
            ops.compute(k, s)
        # Round j-1's delivery is issued BEFORE round j's key gather: on the process group's one RCCL stream a collective queues
        # behind the ones issued before it, and gather_keys(j) waits for round j's compute - behind it the pieces of round j-1
        # would reach the result ranks a whole round late. Every rank issues the collectives in this same order.
        if pending is not None:
            yield from harvest(pending)
        h = ops.gather_keys(s)
        pending = (j, s, h)
    yield from harvest(pending)
    last = n_windows - 1
    tail = ops.last_tail(last, last % world)
    if wanted and tail is not None:
        yield tail_position(n_windows), INTERP_LEN, tail


class HostKeyOps:
    """drive_windows_keys on the host: numpy arithmetic identical to stitch_windows (so the result is bit-equal to the single-rank
    stitch), torch.distributed (gloo) on CPU tensors for the exchanges. The CPU tests' stand-in for the device ops."""

    def __init__(self, frames, plan, window_fn, metric, world, rank, result_ranks, group=None):
        import torch
        self.torch, self.frames, self.plan, self.window_fn, self.metric = torch, frames, plan, window_fn, metric
        self.world, self.rank, self.result_ranks, self.group = world, rank, result_ranks, group
        H0, W0 = frames.shape[1:3]
        self.win = [None, None]
        self.keys_send = [torch.zeros(len(KEY_SLOTS), H0, W0) for _ in range(2)]
        self.keys_recv = [torch.zeros(world, len(KEY_SLOTS), H0, W0) for _ in range(2)]
        self.piece = [torch.zeros(PIECE_FRAMES, H0, W0) for _ in range(2)]
        self.anchor = self.ref1 = None
        self.scale, self.shift = 1.0, 0.0
        self.tail = None                    # aligned slots 24..31 of the window the chain saw last
        self.my = {}                        # window -> (scale, shift, previous window's aligned tail) for the windows this rank owns
        self.last_tail_frames = None

    def compute(self, k, s):
        w = np.ascontiguousarray(self.window_fn(self.frames[self.plan[k]]), dtype=np.float32)
        self.win[s] = w
        self.keys_send[s].copy_(self.torch.from_numpy(w[list(KEY_SLOTS)]))

    def gather_keys(self, s):
        import torch.distributed as dist
        if self.world == 1:
            self.keys_recv[s][0].copy_(self.keys_send[s])
            return None
        n = len(KEY_SLOTS)
        return dist.all_gather_into_tensor(self.keys_recv[s].view(self.world * n, *self.keys_send[s].shape[1:]), self.keys_send[s],
                                           group=self.group, async_op=True)

    def chain(self, k, s, r):
        keys = self.keys_recv[s][r].numpy()
        prev_tail = self.tail
        if k == 0:
            self.anchor, self.ref1 = keys[0].copy(), keys[2].copy()
            self.scale, self.shift = 1.0, 0.0
            self.tail = [keys[3 + i].copy() for i in range(INTERP_LEN)]
        else:
            if not self.metric:
                self.scale, self.shift = compute_scale_and_shift(np.concatenate([keys[0], keys[1]]), np.concatenate([self.anchor, self.ref1]))
            self.ref1 = _clamped_affine(keys[2], self.scale, self.shift)
            self.tail = [_clamped_affine(keys[3 + i], self.scale, self.shift) for i in range(INTERP_LEN)]
        if k % self.world == self.rank:
            self.my[k] = (self.scale, self.shift, prev_tail)

    def finalise(self, k, s):
        w = self.win[s]
        scale, shift, prev_tail = self.my.pop(k)
        if k == 0:
            out = [w[i] for i in range(PIECE_FRAMES)]
        else:
            post = [_clamped_affine(w[i], scale, shift) for i in range(OVERLAP - INTERP_LEN, OVERLAP)]
            out = crossfade(prev_tail, post) + [_clamped_affine(w[i], scale, shift) for i in range(OVERLAP, INFER_LEN - INTERP_LEN)]
        self.piece[s][:len(out)].copy_(self.torch.from_numpy(np.stack(out)))

    def deliver(self, s, j):
        import torch.distributed as dist
        ks = [j * self.world + r for r in range(self.world)]
        if self.world == 1:
            return [(ks[0], self.piece[s].numpy().copy())]
        got = []
        dsts = range(self.world) if self.result_ranks is None else self.result_ranks
        for dst in dsts:
            bufs = [self.torch.empty_like(self.piece[s]) for _ in range(self.world)] if self.rank == dst else None
            dist.gather(self.piece[s], bufs, dst=dst, group=self.group)
            if self.rank == dst:
                got = [(k, bufs[r].numpy()) for r, k in enumerate(ks) if k < len(self.plan)]
        return got

    def last_tail(self, k, owner):
        return np.stack(self.tail)          # every rank ran the whole chain on key frames that include slots 24..31: already here


# ------------------------------------------------------------------ stitching
def compute_scale_and_shift(prediction: np.ndarray, target: np.ndarray) -> Tuple[float, float]:
    """Closed-form least squares target ~ scale*prediction + shift over all pixels
    (utils/util.py:40-62 with the all-ones mask of video_depth.py:232): fp32 sums, identity if det == 0."""
    prediction = prediction.astype(np.float32)
    target = target.astype(np.float32)
    ones = np.ones_like(target, dtype=np.float32)
    a_00 = np.sum(ones * prediction * prediction)
    a_01 = np.sum(ones * prediction)
    a_11 = np.sum(ones)
    b_0 = np.sum(ones * prediction * target)
    b_1 = np.sum(ones * target)
    det = a_00 * a_11 - a_01 * a_01
    if det != 0:
        return (a_11 * b_0 - a_01 * b_1) / det, (-a_01 * b_0 + a_00 * b_1) / det
    return 1, 0


def crossfade(pre: Sequence[np.ndarray], post: Sequence[np.ndarray]) -> List[np.ndarray]:
    """utils/util.py:65-74: weight of `post` ramps 0, 1/7, ..., 6/7, 1."""
    n = len(pre)
    assert n == len(post)
    step = 1.0 / (n - 1)
    wts = [0.0] + [i * step for i in range(1, n - 1)] + [1.0]
    return [pre[i] * (1 - wts[i]) + post[i] * wts[i] for i in range(n)]


def _clamped_affine(d, scale, shift):
    out = d * scale + shift
    out[out < 0] = 0
    return out


def stitch_windows(window_depths: Sequence[np.ndarray], n_frames: int, metric: bool = False) -> np.ndarray:
    """video_depth.py:216-254 over per-window depth [32,H0,W0] arrays (window order).
    metric=True: scale, shift = 1, 0 (metric_depth/video_depth_anything/video_depth.py:132)."""
    align_len = OVERLAP - INTERP_LEN
    kf_align = KEYFRAMES[:align_len]
    aligned: List[np.ndarray] = []
    ref_align: List[np.ndarray] = []
    for k, wd in enumerate(window_depths):
        frames = [wd[i] for i in range(INFER_LEN)]
        if k == 0:
            aligned += frames
            ref_align = [frames[kf] for kf in kf_align]
            continue
        if metric:
            scale, shift = 1.0, 0.0
        else:
            scale, shift = compute_scale_and_shift(np.concatenate(frames[:align_len]), np.concatenate(ref_align))
        post = [_clamped_affine(frames[i], scale, shift) for i in range(align_len, OVERLAP)]
        aligned[-INTERP_LEN:] = crossfade(aligned[-INTERP_LEN:], post)
        for i in range(OVERLAP, INFER_LEN):
            aligned.append(_clamped_affine(frames[i], scale, shift))
        ref_align = ref_align[:1] + [_clamped_affine(frames[kf], scale, shift) for kf in kf_align[1:]]
    return np.stack(aligned[:n_frames], axis=0)


# ------------------------------------------------------------------ a video of unknown length: incremental plan, frame ring
# The streamed path (infer_video_depth_stream) keeps the single-rank issue order of drive_windows: window k is queued on its lane,
# window k + 1's frames are uploaded under it, and only then is window k - 1's finished piece taken. So when a piece is handed out,
# frames through the end of the window TWO ahead of it have been drawn: window k + 1 ends at frame STEP (k + 1) + INFER_LEN - 1 and
# piece k - 1 ends at frame STEP (k - 1) + PIECE_FRAMES - 1.
READ_AHEAD = 2 * STEP + INFER_LEN - (INFER_LEN - INTERP_LEN)                      # 52 frames drawn beyond the last one handed out
# Frames that must be resident in HBM at that moment: windows k - 1 and k may still be running (their gathers read the ring), window
# k + 1 is being uploaded. The oldest frame any of them reads (frame 0 aside) is window k - 1's key frame STEP (k - 2) + KEYFRAMES[1],
# the newest is STEP (k + 1) + INFER_LEN - 1: a contiguous run of 2 STEP + INFER_LEN + (STEP - KEYFRAMES[1]) frames, plus the slot frame 0
# keeps for the whole video. Independent of the video's length.
RING_SPAN = 2 * STEP + INFER_LEN + (STEP - KEYFRAMES[1])                          # 86
RING_FRAMES = 1 + RING_SPAN                                                       # 87 slots
assert KEYFRAMES[0] == 0 and KEYFRAMES[2:] == list(range(INFER_LEN - INTERP_LEN, INFER_LEN)), "frame 0, one key frame, the previous tail"
assert READ_AHEAD <= 3 * INFER_LEN and RING_FRAMES <= 4 * INFER_LEN


class WindowPlanner:
    """plan_windows for a video whose length is not known yet: told how many frames have arrived (and, finally, that there are no
    more), it returns each window as soon as it is decidable - all of its 32 source frames have arrived (frames through
    STEP k + INFER_LEN - 1: nothing is padded, whatever the final length turns out to be), or the end is known (padded slots map to
    the last real frame). For every n the windows returned, in order, are exactly plan_windows(n)."""

    def __init__(self):
        self.arrived = 0
        self.ended = False
        self.emitted = 0                 # windows returned so far
        self._prev = None

    def decidable(self) -> int:
        """Number of windows decidable from what is known now."""
        if self.ended:
            return (self.arrived + STEP - 1) // STEP
        return 0 if self.arrived < INFER_LEN else (self.arrived - INFER_LEN) // STEP + 1

    def feed(self, count: int = 0, end: bool = False) -> List[List[int]]:
        """`count` more frames have arrived; end=True: the stream is exhausted. Returns the windows that became decidable."""
        if self.ended:
            raise RuntimeError("WindowPlanner.feed after the end of the stream")
        if count < 0:
            raise ValueError("negative frame count")
        self.arrived += count
        if end:
            if self.arrived <= 0:
                raise ValueError("empty video")
            self.ended = True
        out = []
        while self.emitted < self.decidable():
            start = STEP * self.emitted
            last = self.arrived - 1                  # clips only once the end is known: before that start + 31 <= last
            cur = [min(start + i, last) for i in range(INFER_LEN)]
            if self._prev is not None:
                cur[:OVERLAP] = [self._prev[k] for k in KEYFRAMES]
            out.append(cur)
            self._prev = cur
            self.emitted += 1
        return out


class FrameRing:
    """Slot allocator of the fixed-capacity uint8 frame ring in HBM that stands in for the whole-video buffer of infer_video_depth.
    Frame 0 is pinned to slot 0; frame f > 0 lives in slot 1 + (f - 1) % (capacity - 1), so placing frame f evicts frame
    f - (capacity - 1). Host bookkeeping only; it ASSERTS what the schedule promises instead of trusting it:

      reserve(k, window)   before window k's frames are uploaded: places the frames that are not resident, returns
                           ([(frame, slot)] to upload, newest window that READ an evicted frame or -1). A frame may only be evicted
                           when no reserved window still waits to be issued with it, and never frame 0.
      issued(k, window)    window k's slot-consuming kernel (the gather) has been queued on its lane.

    What makes the reuse safe ON THE DEVICE is the caller's business: the upload stream has to be ordered behind the gathers of the
    windows that read an evicted slot. RING_FRAMES is sized so that when window k + 1 is reserved those are windows <= k - 2
    (returned for the caller to assert), whose `freed` event - recorded by the consumer behind the stitch of window k - 2, hence behind
    its forward and its gather - the upload stream waits for. Stream order on a lane is NOT enough: uploads run on their own stream."""

    def __init__(self, capacity: int = RING_FRAMES):
        assert capacity >= 2
        self.capacity = capacity
        self.frame_at = [None] * capacity        # slot -> frame
        self.slot_of = {}                        # resident frame -> slot
        self.waiting = {}                        # frame -> reserved, not yet issued windows that read it
        self.reader = {}                         # resident frame -> newest issued window that read it
        self.peak = 0

    def _slot(self, f):
        return 0 if f == 0 else 1 + (f - 1) % (self.capacity - 1)

    def in_use(self) -> int:
        return len(self.slot_of)

    def reserve(self, k, window):
        need = sorted(set(window))
        todo, evicted_reader = [], -1
        for f in need:
            if f not in self.slot_of:
                s = self._slot(f)
                old = self.frame_at[s]
                if old is not None:
                    assert old != 0, "frame 0 is pinned"
                    assert self.waiting.get(old, 0) == 0, f"frame {old} evicted by {f} while a reserved window still needs it"
                    evicted_reader = max(evicted_reader, self.reader.pop(old, -1))
                    del self.slot_of[old]
                    self.waiting.pop(old, None)
                self.frame_at[s] = f
                self.slot_of[f] = s
                todo.append((f, s))
        for f in need:                           # after every placement: a window's own frames must not have evicted each other
            assert f in self.slot_of and self.frame_at[self.slot_of[f]] == f, f"window {k}: frame {f} lost its slot to another of its frames"
            self.waiting[f] = self.waiting.get(f, 0) + 1
        self.peak = max(self.peak, len(self.slot_of))
        assert len(self.slot_of) <= self.capacity
        return todo, evicted_reader

    def issued(self, k, window):
        for f in set(window):
            self.waiting[f] -= 1
            self.reader[f] = k

    def slots(self, window):
        return [self.slot_of[f] for f in window]


class HostStitcher:
    """stitch_windows one window at a time (the same numpy operations on the same operands, so bit-equal): push(window) returns the
    frames that became final - 24 after window 0, 22 after each later one -, tail() the last 8 once no window follows."""

    def __init__(self, metric: bool = False):
        self.metric = metric
        self.k = 0
        self._tail = None
        self._ref = None

    def push(self, wd: np.ndarray) -> List[np.ndarray]:
        align_len = OVERLAP - INTERP_LEN
        kf_align = KEYFRAMES[:align_len]
        frames = [wd[i] for i in range(INFER_LEN)]
        if self.k == 0:
            out = frames[:INFER_LEN - INTERP_LEN]
            self._tail = frames[INFER_LEN - INTERP_LEN:]
            self._ref = [frames[kf] for kf in kf_align]
        else:
            if self.metric:
                scale, shift = 1.0, 0.0
            else:
                scale, shift = compute_scale_and_shift(np.concatenate(frames[:align_len]), np.concatenate(self._ref))
            post = [_clamped_affine(frames[i], scale, shift) for i in range(align_len, OVERLAP)]
            rest = [_clamped_affine(frames[i], scale, shift) for i in range(OVERLAP, INFER_LEN)]
            out = crossfade(self._tail, post) + rest[:-INTERP_LEN]
            self._tail = rest[-INTERP_LEN:]
            self._ref = self._ref[:1] + [_clamped_affine(frames[kf], scale, shift) for kf in kf_align[1:]]
        self.k += 1
        return out

    def tail(self) -> List[np.ndarray]:
        return self._tail


def _as_block(block) -> np.ndarray:
    """One item of a frame iterable as a [m,H,W,3] array: a single [H,W,3] frame becomes a block of one."""
    block = np.asarray(block) if not isinstance(block, np.ndarray) else block
    if block.ndim == 3:
        block = block[None]
    return block


def run_windows_stream(frames_iter, window_fn: Callable[[np.ndarray], np.ndarray], metric: bool = False):
    """infer_video_depth_stream's host logic without a GPU (the twin of run_windows for one rank): frames arrive as [H,W,3] frames or
    [m,H,W,3] blocks from an iterable of unknown length, the incremental planner decides the windows, the stitcher runs window by
    window. Yields (first output frame, float32 [c,H0,W0]) pieces - in order, contiguous, trimmed to the video's length once that
    is known; their concatenation is bit-equal to run_windows on the concatenated frames. Only the frames a later window can still
    read are kept."""
    planner = WindowPlanner()
    st = HostStitcher(metric)
    held = {}                                    # frame index -> [H0,W0,3]
    done = 0                                     # windows computed
    it = iter(frames_iter)
    ended = False
    while not ended:
        try:
            block = _as_block(next(it))
            base = planner.arrived
            for i in range(block.shape[0]):
                held[base + i] = block[i]
            windows = planner.feed(block.shape[0])
        except StopIteration:
            windows = planner.feed(end=True)
            ended = True
        for win in windows:
            w = np.ascontiguousarray(window_fn(np.stack([held[f] for f in win])), dtype=np.float32)
            out = st.push(w)
            pos, _ = piece_position(done)
            done += 1
            # a window decided before the end is known lies wholly inside the video: only the end can trim
            hi = min(pos + len(out), planner.arrived) if planner.ended else pos + len(out)
            if hi > pos:
                yield pos, np.stack(out[:hi - pos])
            oldest = STEP * (done - 1) + KEYFRAMES[1]           # the next window's key frame: nothing older (frame 0 aside) is read again
            for f in [f for f in held if 0 < f < oldest]:
                del held[f]
    n = planner.arrived
    pos = tail_position(done)
    if n > pos:
        yield pos, np.stack(st.tail()[:n - pos])


# ------------------------------------------------------------------ host driver (CPU rehearsal of the multi-rank schedule)
def run_windows(frames: np.ndarray, window_fn: Callable[[np.ndarray], np.ndarray], metric: bool = False, group=None, exchange: str = "windows",
                result_ranks=None):
    """infer_video_depth's schedule on the host: `window_fn(frames_u8[32,H0,W0,3]) -> float32 [32,H0,W0]` per window, the
    same `drive_windows` rounds / ring / gather order the device path uses (gloo on CPU tensors instead of RCCL), then the
    numpy stitcher. Every rank returns the full sequence. Used by the CPU tests (world size 1, 2, 3).
    exchange="keys": the key-frame schedule (drive_windows_keys); ranks outside result_ranks return None."""
    import torch
    import torch.distributed as dist

    n = frames.shape[0]
    H0, W0 = frames.shape[1:3]
    plan = plan_windows(n)
    world = dist.get_world_size(group) if (dist.is_available() and dist.is_initialized()) else 1
    rank = dist.get_rank(group) if world > 1 else 0
    if exchange == "keys":
        ops = HostKeyOps(frames, plan, window_fn, metric, world, rank, result_ranks, group)
        out = np.zeros((n, H0, W0), dtype=np.float32) if (result_ranks is None or rank in result_ranks) else None
        seen = np.zeros(n, dtype=np.int32)
        for pos, cnt, piece in drive_windows_keys(len(plan), world, rank, ops, result_ranks):
            hi = min(pos + cnt, n)
            if hi > pos:
                out[pos:hi] = piece[:hi - pos]
                seen[pos:hi] += 1
        assert out is None or (seen == 1).all(), "every output frame exactly once"
        return out
    send = [torch.zeros(INFER_LEN, H0, W0, dtype=torch.float32) for _ in range(2)]
    recv = [torch.empty(world, INFER_LEN, H0, W0, dtype=torch.float32) for _ in range(2)] if world > 1 else None

    def compute(k, s):
        send[s].copy_(torch.from_numpy(np.ascontiguousarray(window_fn(frames[plan[k]]), dtype=np.float32)))

    def gather(s):
        return dist.all_gather_into_tensor(recv[s].view(world * INFER_LEN, H0, W0), send[s], group=group, async_op=True)

    wins = [w.numpy().copy() for w in drive_windows(len(plan), world, rank, send, recv, compute, gather)]
    return stitch_windows(wins, n, metric)


def normalize_frames_host(frames_u8: np.ndarray) -> np.ndarray:
    """Reference arithmetic of video_depth.py:198 + util/transform.py:134,147 for frames already at
    network size (host version, used by CPU-side tests of the plumbing)."""
    img = frames_u8.astype(np.float32) / 255.0
    img = (img - list(IMAGENET_MEAN)) / list(IMAGENET_STD)
    return np.ascontiguousarray(np.moveaxis(img, -1, -3)).astype(np.float32)
