"""`VideoDepthAnything.infer_video_depth_stream`: infer_video_depth for a video of unknown length, in bounded memory.

The same kernels on the same lanes in the same order as the single-rank path of infer_video_depth (two windows in flight, the
next window's frames uploaded under the current one, the device stitcher, one device-to-host copy per finished chunk through a
pinned ring), so every output frame is bit-identical. What differs is what is kept:

  host    frames that were drawn from the source and are not uploaded yet (at most scheduler.READ_AHEAD beyond the last frame
          handed out, plus the rest of the block the source delivered them in); finished pieces belong to the caller
  HBM     a ring of scheduler.RING_FRAMES uint8 frames instead of the whole video (scheduler.FrameRing: frame 0 pinned, every
          other frame until the last window that reads it has been issued); everything else is per-lane and was constant already

The windows come from scheduler.WindowPlanner, which decides window k once frames through 22 k + 31 have arrived or the source
is exhausted; scheduler.run_windows_stream is the CPU rehearsal of the host logic here.
"""
import collections

import numpy as np
import torch

from . import ops
from .config import INFER_LEN, INTERP_LEN
from .scheduler import STEP, FrameRing, WindowPlanner, network_size
from .stitch import FIRST, DeviceStitcher


def _as_u8_block(block, shape):
    """One item drawn from the source as uint8 [m,H0,W0,3] (a single [H0,W0,3] frame is a block of one), under the rules
    infer_video_depth applies to its array: [.., H, W, 3], one frame size, 8-bit values in whatever dtype."""
    if not isinstance(block, np.ndarray):
        block = np.asarray(block)
    if block.ndim == 3:
        block = block[None]
    if block.ndim != 4 or block.shape[-1] != 3:
        raise ValueError("infer_video_depth: frames must be [N, H, W, 3], got shape %r" % (tuple(block.shape),))
    if shape is not None and tuple(block.shape[1:3]) != tuple(shape):
        raise ValueError("infer_video_depth: every frame must have the first frame's size %r, got shape %r" % (tuple(shape), tuple(block.shape)))
    if block.dtype != np.uint8:
        ok = bool(block.size == 0 or (block.min() >= 0 and block.max() <= 255 and
                                      (np.issubdtype(block.dtype, np.integer) or np.array_equal(block, np.rint(block)))))
        if not ok:
            raise TypeError("infer_video_depth: frames must hold 8-bit values (uint8, or any dtype whose values are integers "
                            "within 0..255); got dtype %s with other values" % block.dtype)
        block = block.astype(np.uint8)
    return block


class _FrameFeed:
    """The source, drawn block by block; holds the blocks that are not uploaded yet."""

    def __init__(self, frames):
        if isinstance(frames, np.ndarray):
            # an array (or memory map) of the whole video: the same checks as infer_video_depth up front, then views of STEP frames -
            # a memory map is paged in run by run as the uploads reach it
            if frames.ndim != 4 or frames.shape[-1] != 3:
                raise ValueError("infer_video_depth: frames must be [N, H, W, 3], got shape %r" % (tuple(frames.shape),))
            self._it = (frames[i:i + STEP] for i in range(0, frames.shape[0], STEP))
        else:
            self._it = iter(frames)
        self.shape = None                        # (H0, W0), fixed by the first block
        self.drawn = 0
        self.blocks = collections.deque()        # (first frame, uint8 [m,H0,W0,3])

    def draw(self):
        """Draw one block; returns its frame count, or None when the source is exhausted."""
        while True:
            try:
                block = next(self._it)
            except StopIteration:
                return None
            block = _as_u8_block(block, self.shape)
            if block.shape[0] == 0:
                continue
            if self.shape is None:
                self.shape = tuple(block.shape[1:3])
            self.blocks.append((self.drawn, block))
            self.drawn += block.shape[0]
            return block.shape[0]

    def runs(self, f0, f1):
        """Frames f0 .. f1-1 as (first frame, array) pieces of the held blocks."""
        for base, block in self.blocks:
            lo, hi = max(f0, base), min(f1, base + block.shape[0])
            if lo < hi:
                yield lo, block[lo - base:hi - base]

    def uploaded_through(self, f):
        """Frames <= f are in HBM: blocks that end there are dropped."""
        while self.blocks and self.blocks[0][0] + self.blocks[0][1].shape[0] - 1 <= f:
            self.blocks.popleft()


class DepthStream:
    """Iterator of (first frame, float32 [c,H0,W0]) pieces; see VideoDepthAnything.infer_video_depth_stream."""

    def __init__(self, model, eng, frames, target_fps, input_size, fp32):
        self.n_frames = None
        self.depth_min = None
        self.depth_max = None
        self.fps = target_fps
        self._feed = _FrameFeed(frames)
        self._gen = self._run(eng, int(input_size), bool(fp32), bool(model.METRIC))

    def __iter__(self):
        return self

    def __next__(self):
        return next(self._gen)

    def close(self):
        """Stop early: joins the lanes, waits for what is in flight and restores the handle's options. Idempotent."""
        self._gen.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------------------------
    def _run(self, eng, input_size, fp32, metric):
        dev = eng.device
        keep = eng.options.get("enc_split", -1)           # as infer_video_depth: two windows in flight already fill the chip
        eng.set_option("enc_split", 0)
        streams = []                                      # everything that has to be joined on the way out
        compute = None
        try:
            with torch.cuda.device(dev):
                compute = torch.cuda.current_stream(dev)
                eng.set_option("dyn_sched", 0)            # one rank: no collective beside the GEMMs
                core = _Core(eng, self._feed, input_size, fp32, metric, compute, streams)
            while True:
                with torch.cuda.device(dev), torch.cuda.stream(compute):
                    piece = core.step()
                if piece is None:
                    break
                yield piece
            with torch.cuda.device(dev), torch.cuda.stream(compute):
                self.n_frames = core.planner.arrived
                lo, hi = core.minmax.cpu().tolist()       # (waits for the consumer stream: every chunk's reduction is behind it)
                self.depth_min, self.depth_max = np.float32(lo), np.float32(hi)
        finally:
            with torch.cuda.device(dev):
                if compute is not None:
                    for s in streams:
                        compute.wait_stream(s)
                    compute.synchronize()                 # no kernel of the handle is in flight when control returns
                eng.set_option("enc_split", keep)
        eng.check()                                       # (only reached when the stream ran to its end)


class _Core:
    """The single-rank schedule of infer_video_depth, one window per step()."""
    NSLOT = 2

    def __init__(self, eng, feed, input_size, fp32, metric, compute, streams):
        self.eng, self.feed, self.fp32, self.compute = eng, feed, fp32, compute
        self.planner = WindowPlanner()
        self.windows = {}                                 # decided, not yet issued: k -> source frames
        self.reserved = set()
        self.k = 0                                        # next window to issue
        self.pending = None                               # (pinned slot, first output frame, count) of the copy in flight
        self.state = "windows"
        if not self._decide(0):
            raise ValueError("empty video")               # (WindowPlanner.feed(end=True) raises it for a source without frames)
        dev = self.dev = eng.device
        H0, W0 = self.H0, self.W0 = feed.shape
        H, W = self.H, self.W = network_size(H0, W0, input_size)
        NSLOT = self.NSLOT
        self.ring = FrameRing()
        self.video = torch.empty((self.ring.capacity, H0, W0, 3), dtype=torch.uint8, device=dev)
        self.upload = torch.cuda.Stream(device=dev)
        self.lanes = [torch.cuda.Stream(device=dev) for _ in range(NSLOT)]
        self.copy_stream = torch.cuda.Stream(device=dev)
        streams += self.lanes + [self.upload, self.copy_stream]
        self.computed = [torch.cuda.Event() for _ in range(NSLOT)]     # slot's window is in send[s] (recorded on its lane)
        self.freed = [torch.cuda.Event() for _ in range(NSLOT)]        # the stitcher is done with the slot (recorded on `compute`)
        self.used = [False] * NSLOT
        self.xin = [torch.empty(1, INFER_LEN, 3, H, W, dtype=torch.float32, device=dev) for _ in range(NSLOT)]
        self.send = [torch.empty(INFER_LEN, H0, W0, dtype=torch.float32, device=dev) for _ in range(NSLOT)]
        self.st = DeviceStitcher(H0, W0, dev, metric)
        self.chunk = [torch.empty(FIRST, H0, W0, dtype=torch.float32, device=dev) for _ in range(2)]
        self.pinned = [torch.empty(FIRST, H0, W0, dtype=torch.float32, pin_memory=True) for _ in range(2)]
        self.done = [torch.cuda.Event() for _ in range(2)]
        self.minmax = torch.tensor([float("inf"), float("-inf")], dtype=torch.float32, device=dev)

    # ---- source -> plan -> ring
    def _decide(self, k):
        """Draw from the source until window k is decided or the source has ended; True if window k exists."""
        while self.planner.emitted <= k and not self.planner.ended:
            m = self.feed.draw()
            new = self.planner.feed(end=True) if m is None else self.planner.feed(m)
            for i, w in enumerate(new):
                self.windows[self.planner.emitted - len(new) + i] = w
        return k in self.windows

    def _ensure(self, k, s):
        """Queue the upload of window k's not-yet-resident frames into their ring slots (runs of consecutive frames of one source
        block = one copy each). s: the lane slot of the window being issued when this is a prefetch (k - 1's), else None."""
        if k in self.reserved or not self._decide(k):
            return
        todo, evicted_reader = self.ring.reserve(k, self.windows[k])
        self.reserved.add(k)
        if evicted_reader >= 0:
            # Slot reuse. The slots overwritten here were last read by the gather of a window <= k - 3 (RING_FRAMES is derived for
            # exactly that, scheduler.py). This is the prefetch under window k - 1 on lane slot s, and freed[s] was recorded by the
            # consumer behind the stitch of window k - 3 - behind its forward, behind its gather. The upload stream waits for that
            # event: the `freed` events order the reuse, not stream order on the lanes (uploads have their own stream).
            assert s is not None and evicted_reader <= k - 3, (k, evicted_reader)
            self.upload.wait_event(self.freed[s])
        with torch.cuda.stream(self.upload):
            i = 0
            while i < len(todo):
                j = i
                while j + 1 < len(todo) and todo[j + 1][0] == todo[j][0] + 1 and todo[j + 1][1] == todo[j][1] + 1:
                    j += 1
                f0, s0 = todo[i]
                for lo, run in self.feed.runs(f0, todo[j][0] + 1):
                    if not (run.flags.c_contiguous and run.flags.writeable):
                        run = np.array(run)              # a memory-mapped or strided source: page this run in
                    d0 = s0 + (lo - f0)
                    self.video[d0:d0 + run.shape[0]].copy_(torch.from_numpy(run), non_blocking=True)
                i = j + 1
        if todo:
            self.feed.uploaded_through(todo[-1][0])

    # ---- one window on its lane (infer_video_depth.window_depth)
    def _window_depth(self, k, s):
        self._ensure(k, None)
        lane = self.lanes[s]
        lane.wait_stream(self.upload)
        if self.used[s]:
            lane.wait_event(self.freed[s])
        self.used[s] = True
        win = self.windows.pop(k)
        H0, W0, H, W = self.H0, self.W0, self.H, self.W
        with torch.cuda.stream(lane):
            idx = torch.tensor(self.ring.slots(win), dtype=torch.int32, device=self.dev)
            if (H0, W0) == (H, W):
                ops.gather_normalize_u8(self.video, idx, self.xin[s], INFER_LEN, H0, W0)
            else:
                ops.gather_resize_normalize_u8(self.video, idx, self.xin[s], INFER_LEN, H0, W0, H, W)
            self.ring.issued(k, win)                      # the slot-consuming kernel is queued
            depth = self.eng.forward(self.xin[s], fp32=self.fp32, slot=s)
            ops.bilinear_plane(depth.view(INFER_LEN, H, W), self.send[s], INFER_LEN, H, W, H0, W0)
            self.computed[s].record(lane)
        self.reserved.discard(k)
        self._ensure(k + 1, s)                            # overlaps this window's compute

    # ---- finished chunks
    def _send(self, src, b, lo, cnt):
        """Trim to the video, fold the chunk into the running depth range, start its device-to-host copy."""
        if self.planner.ended:
            cnt = min(lo + cnt, self.planner.arrived) - lo
        if cnt <= 0:
            return None
        ops.minmax_accum(src, self.minmax, cnt * self.H0 * self.W0)
        self.copy_stream.wait_stream(self.compute)
        with torch.cuda.stream(self.copy_stream):
            self.pinned[b][:cnt].copy_(src[:cnt], non_blocking=True)
            self.done[b].record(self.copy_stream)
        return (b, lo, cnt)

    def _harvest(self, p):
        b, lo, cnt = p
        self.done[b].synchronize()
        # the chunk's window (and every earlier one) has finished: a window that left fp16's range is reported here, before its
        # frames - NaN by then - could be handed out
        self.eng.check(synchronize=False)
        return lo, self.pinned[b][:cnt].numpy().copy()    # the caller's own array; the pinned buffer is reused two chunks on

    def step(self):
        """Issue windows until a piece is ready; returns (first frame, depths) or None at the end."""
        while self.state == "windows":
            k = self.k
            if not self._decide(k):
                self.state = "last"
                break
            s = k % self.NSLOT
            self._window_depth(k, s)
            self.compute.wait_event(self.computed[s])
            cnt = self.st.push(self.send[s], self.chunk[k & 1])
            nxt = self._send(self.chunk[k & 1], k & 1, self.st.first_frame_of(k), cnt)
            self.freed[s].record(self.compute)
            self.k += 1
            out, self.pending = self.pending, nxt
            if out is not None:
                return self._harvest(out)
        if self.state == "last":
            self.state = "tail"
            out, self.pending = self.pending, None
            if out is not None:
                return self._harvest(out)
        if self.state == "tail":
            self.state = "end"
            p = self._send(self.st.tail, 0, self.st.tail_position(), INTERP_LEN)   # after the last window its tail is final too
            if p is not None:
                return self._harvest(p)
        return None
