"""The device machinery infer_video_depth (video_depth.py) and infer_video_depth_stream (stream.py) share.

The two paths plan windows and keep frames resident in their own ways; everything they queue on the GPU goes through here - frame
validation, the upload of frame runs, a window on its lane (WindowLanes), the device-to-host ring of pinned buffers (HostCopyRing,
also under stitch.stitch_stream and stitch.collect_pieces) and the session around a video (video_session). "The same kernels on the
same lanes in the same order" is therefore a property of this module, not of two texts kept alike.
"""
import contextlib

import numpy as np
import torch

from . import ops
from .config import INFER_LEN


# ------------------------------------------------------------------ frames from the caller
def check_frames(block, shape=None):
    """[N, H, W, 3], and the frame size `shape` = (H, W) when one is given. Reads no pixel."""
    if block.ndim != 4 or block.shape[-1] != 3:
        raise ValueError("infer_video_depth: frames must be [N, H, W, 3], got shape %r" % (tuple(block.shape),))
    if shape is not None and tuple(block.shape[1:3]) != tuple(shape):
        raise ValueError("infer_video_depth: every frame must have the first frame's size %r, got shape %r" % (tuple(shape), tuple(block.shape)))


def as_u8_frames(block, shape=None):
    """`block` as uint8 [N, H, W, 3] (check_frames' rules; an empty block passes).
    The reference computes frame.astype(float32) / 255 on whatever it is handed (video_depth.py:198). The device path keeps the
    video as uint8 in HBM, which is the same arithmetic exactly when the values ARE 0..255 integers: arrays of any dtype holding
    such values (wider integers, float32 frames out of a cv2 pipeline) are converted; values that are not 8-bit (fractions,
    negatives, > 255, NaN) are refused rather than silently truncated."""
    if not isinstance(block, np.ndarray):
        block = np.asarray(block)
    check_frames(block, shape)
    if block.dtype != np.uint8:
        ok = bool(block.size == 0 or (block.min() >= 0 and block.max() <= 255 and
                                      (np.issubdtype(block.dtype, np.integer) or np.array_equal(block, np.rint(block)))))
        if not ok:
            raise TypeError("infer_video_depth: frames must hold 8-bit values (uint8, or any dtype whose values are integers "
                            "within 0..255); got dtype %s with other values" % block.dtype)
        block = block.astype(np.uint8)
    return block


# ------------------------------------------------------------------ host -> HBM
def coalesce_runs(pairs):
    """Sorted [(frame, slot)] -> [(first frame, first slot, count)]: stretches in which frame and slot both advance by 1."""
    runs = []
    for f, s in pairs:
        if runs and (f, s) == (runs[-1][0] + runs[-1][2], runs[-1][1] + runs[-1][2]):
            runs[-1][2] += 1
        else:
            runs.append([f, s, 1])
    return [tuple(r) for r in runs]


def upload_runs(video, pairs, fetch):
    """Queue, on the current stream, the copies that put every frame of the sorted [(frame, slot)] `pairs` into video[slot]: one
    copy per run of coalesce_runs and piece of the source. fetch(f0, f1) yields frames f0 .. f1-1 as (first frame, uint8 array)
    pieces."""
    for f0, s0, m in coalesce_runs(pairs):
        for lo, run in fetch(f0, f0 + m):
            if not (run.flags.c_contiguous and run.flags.writeable):
                run = np.array(run)                          # a memory-mapped or strided source: page this run in
            d0 = s0 + (lo - f0)
            video[d0:d0 + run.shape[0]].copy_(torch.from_numpy(run), non_blocking=True)


# ------------------------------------------------------------------ windows on their lanes
class WindowLanes:
    """Windows are independent, so TWO are kept in flight on this GPU, each on its own HIP stream (lane) with its own input buffer,
    workspace slot and output slot send[s]: the tail rounds and launch gaps of one window's kernels are filled by the other's
    (measured: +6 % ViT-L, +17 % ViT-S frames/s over one window at a time, tools/two_stream.py).
    video: the uint8 frames in HBM [slots, H0, W0, 3] the windows gather from; (H, W): the network size. The consumer (stitcher,
    exchange) works on the stream that is current when this is built."""

    def __init__(self, eng, video, H, W, fp32, nslot=2):
        dev = eng.device
        self.eng, self.video, self.H, self.W, self.fp32 = eng, video, H, W, fp32
        H0, W0 = video.shape[1:3]
        self.consumer = torch.cuda.current_stream(dev)
        self.lanes = [torch.cuda.Stream(device=dev) for _ in range(nslot)]
        self.computed = [torch.cuda.Event() for _ in range(nslot)]     # slot's window is in send[s] (recorded on its lane)
        self.freed = [torch.cuda.Event() for _ in range(nslot)]        # the consumer is done with the slot (recorded on its stream)
        self.used = [False] * nslot
        self.xin = [torch.empty(1, INFER_LEN, 3, H, W, dtype=torch.float32, device=dev) for _ in range(nslot)]
        self.send = [torch.empty(INFER_LEN, H0, W0, dtype=torch.float32, device=dev) for _ in range(nslot)]

    def acquire(self, s):
        """Before anything of slot s is overwritten: its lane waits until the consumer has finished with what the slot held two
        rounds ago."""
        if self.used[s]:
            self.lanes[s].wait_event(self.freed[s])
        self.used[s] = True

    def ready(self, s):
        self.consumer.wait_event(self.computed[s])

    def release(self, s):
        self.freed[s].record(self.consumer)

    def run(self, slots, s, upload, keys=None):
        """The window whose 32 frames are video[slots], on lane s behind the `upload` stream: gather (+ resize to the network size)
        + normalise (video_depth.py:197-201, util/transform.py:109-147), forward, resize to the source size (video_depth.py:207-208)
        into send[s] [32,H0,W0] (keys: the window's KEY_SLOTS frames are copied there too - three contiguous runs)."""
        lane, video, xin, send, H, W = self.lanes[s], self.video, self.xin[s], self.send[s], self.H, self.W
        H0, W0 = video.shape[1:3]
        lane.wait_stream(upload)
        self.acquire(s)
        with torch.cuda.stream(lane):
            idx = torch.tensor(slots, dtype=torch.int32, device=video.device)
            if (H0, W0) == (H, W):
                ops.gather_normalize_u8(video, idx, xin, INFER_LEN, H0, W0)
            else:
                # cv2.resize(INTER_CUBIC) in the reference (util/transform.py:113); cv2 is absent offline, so this leg is
                # PARITY UNPINNED against cv2 itself: the kernel evaluates cv2's published definition (a = -0.75, half-pixel
                # centres, clamped taps) and is tested against that definition on the CPU.
                ops.gather_resize_normalize_u8(video, idx, xin, INFER_LEN, H0, W0, H, W)
            depth = self.eng.forward(xin, fp32=self.fp32, slot=s)                # [1,32,H,W] fp32
            ops.bilinear_plane(depth.view(INFER_LEN, H, W), send, INFER_LEN, H, W, H0, W0)
            if keys is not None:
                keys[0:2].copy_(send[0:2])
                keys[2].copy_(send[12])
                keys[3:].copy_(send[INFER_LEN - 8:])
            self.computed[s].record(lane)

    def behind(self, s, fn):
        """fn() on slot s's lane behind its window - the exchanges of the multi-rank schedules. A rank with no window in this round
        still takes part, so the slot is acquired here too; computed[s] is recorded again behind fn, and the consumer's stream
        waits for that event in ready(s): nothing depends on which stream happens to be current when the round is harvested."""
        self.acquire(s)
        with torch.cuda.stream(self.lanes[s]):
            fn()
            self.computed[s].record(self.lanes[s])


# ------------------------------------------------------------------ HBM -> host
class HostCopyRing:
    """Device-to-host copies of up to `rows` frames [H0,W0] fp32 each, through `nbuf` pinned buffers on a side stream: piece i
    uses buffer i % nbuf, so the view wait() returns for piece i is valid until piece i + nbuf is started."""

    def __init__(self, nbuf, rows, H0, W0, device):
        self.device = device
        self.copy_stream = torch.cuda.Stream(device=device)
        self.pinned = [torch.empty(rows, H0, W0, dtype=torch.float32, pin_memory=True) for _ in range(nbuf)]
        self.done = [torch.cuda.Event() for _ in range(nbuf)]
        self.started = 0

    def start(self, src, cnt):
        """Queue the copy of src[:cnt] behind what the current stream holds now; returns the token (event, pinned view)."""
        b = self.started % len(self.pinned)
        self.started += 1
        self.copy_stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self.copy_stream):
            self.pinned[b][:cnt].copy_(src[:cnt], non_blocking=True)
            self.done[b].record(self.copy_stream)
        return self.done[b], self.pinned[b][:cnt]

    def wait(self, token):
        """Block the host until the token's copy has landed; returns its pinned view [cnt,H0,W0]."""
        token[0].synchronize()
        return token[1]

    def join(self):
        torch.cuda.current_stream(self.device).wait_stream(self.copy_stream)


# ------------------------------------------------------------------ the session around one video
@contextlib.contextmanager
def video_session(eng, dyn_sched, synchronize=False):
    """Handle options for a video, restored on every way out. Yields (consumer stream, streams): the caller appends the streams it
    creates to `streams`, and the consumer stream waits for them on the way out (synchronize: the host then waits for it too).
    enc_split: two windows in flight on two lanes already fill each other's idle time; the encoder's frame-half split measured
    -2 % on a 1024-frame video on top of them (profiles/r05), so it is off for the video.
    head_lanes: the same lane stream and the same reasoning, off for the video as well.
    dyn_sched: multi-rank, the per-round all-gather runs beside the next windows' kernels - GEMMs that find CUs taken by it should
    lose those CUs, not a whole shift of tiles (dynamic tile draw).
    The device is current while this is entered and left, not in between: a generator holds a session across its yields, and its
    consumer's current device is not ours to change - the body enters torch.cuda.device itself wherever it queues work."""
    dev = eng.device
    keep = {k: eng.options.get(k, -1) for k in ("enc_split", "head_lanes")}      # (-1: the library's default)
    for k in keep:
        eng.set_option(k, 0)
    try:
        eng.set_option("dyn_sched", dyn_sched)
        with torch.cuda.device(dev):
            consumer = torch.cuda.current_stream(dev)
        streams = []
        try:
            yield consumer, streams
        finally:
            with torch.cuda.device(dev):
                for s in streams:
                    consumer.wait_stream(s)
                if synchronize:
                    consumer.synchronize()
    finally:
        for k, v in keep.items():
            eng.set_option(k, v)
