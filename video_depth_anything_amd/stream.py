"""`VideoDepthAnything.infer_video_depth_stream`: infer_video_depth for a video of unknown length, in bounded memory.

The same kernels on the same lanes in the same order as the single-rank path of infer_video_depth (two windows in flight, the
next window's frames uploaded under the current one, the device stitcher, one device-to-host copy per finished chunk through a
pinned ring), so every output frame is bit-identical - by construction: both paths queue every window through lanes.WindowLanes.run,
every upload through lanes.upload_runs, every chunk through stitch.DeviceStitcher and lanes.HostCopyRing, inside one
lanes.video_session. This module holds only the schedule: decide, reserve, issue, stitch, harvest. What differs is what is kept:

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
from .config import INTERP_LEN
from .lanes import HostCopyRing, WindowLanes, as_u8_frames, check_frames, upload_runs, video_session
from .scheduler import STEP, FrameRing, WindowPlanner, _as_block, network_size, piece_position, tail_position
from .stitch import FIRST, DeviceStitcher


class _FrameFeed:
    """The source, drawn block by block; holds the blocks that are not uploaded yet."""

    def __init__(self, frames):
        if isinstance(frames, np.ndarray):
            # an array (or memory map) of the whole video: the same checks as infer_video_depth up front, then views of STEP frames -
            # a memory map is paged in run by run as the uploads reach it
            check_frames(frames)
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
            block = as_u8_frames(_as_block(block), self.shape)   # (a single [H0,W0,3] frame is a block of one)
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
        # one rank: no collective beside the GEMMs (dyn_sched 0). On every way out the lanes, the upload and the copy stream are
        # joined and the consumer stream is synchronised: no kernel of the handle is in flight when control returns
        with video_session(eng, 0, synchronize=True) as (compute, streams):
            with torch.cuda.device(dev):
                core = _Core(eng, self._feed, input_size, fp32, metric, streams)
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
        eng.check()                                       # (only reached when the stream ran to its end)


class _Core:
    """The single-rank schedule of infer_video_depth, one window per step()."""

    def __init__(self, eng, feed, input_size, fp32, metric, streams):
        self.eng, self.feed = eng, feed
        self.planner = WindowPlanner()
        self.windows = {}                                 # decided, not yet issued: k -> source frames
        self.reserved = set()
        self.k = 0                                        # next window to issue
        self.pending = None                               # (copy in flight, first output frame)
        self.state = "windows"
        if not self._decide(0):
            raise ValueError("empty video")               # (WindowPlanner.feed(end=True) raises it for a source without frames)
        dev = eng.device
        H0, W0 = feed.shape
        self.px = H0 * W0
        self.ring = FrameRing()
        self.video = torch.empty((self.ring.capacity, H0, W0, 3), dtype=torch.uint8, device=dev)
        self.upload = torch.cuda.Stream(device=dev)
        self.lanes = WindowLanes(eng, self.video, *network_size(H0, W0, input_size), fp32)
        self.st = DeviceStitcher(H0, W0, dev, metric)
        self.chunk = [torch.empty(FIRST, H0, W0, dtype=torch.float32, device=dev) for _ in range(2)]
        self.out = HostCopyRing(2, FIRST, H0, W0, dev)
        streams += self.lanes.lanes + [self.upload, self.out.copy_stream]
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
            self.upload.wait_event(self.lanes.freed[s])
        with torch.cuda.stream(self.upload):
            upload_runs(self.video, todo, self.feed.runs)
        if todo:
            self.feed.uploaded_through(todo[-1][0])

    # ---- one window on its lane
    def _window_depth(self, k, s):
        self._ensure(k, None)
        win = self.windows.pop(k)
        self.lanes.run(self.ring.slots(win), s, self.upload)
        # The slot-consuming kernel (the gather) is queued. FrameRing is host bookkeeping that asserts host state, and between the
        # gather inside run() and here no upload is queued and FrameRing is not asked anything (run() goes on to the forward, the
        # resize and the event, all on the lane): telling it now is the same as telling it right behind the gather.
        self.ring.issued(k, win)
        self.reserved.discard(k)
        self._ensure(k + 1, s)                            # overlaps this window's compute

    # ---- finished chunks
    def _send(self, src, lo, cnt):
        """Trim to the video, fold the chunk into the running depth range, start its device-to-host copy."""
        if self.planner.ended:
            cnt = min(lo + cnt, self.planner.arrived) - lo
        if cnt <= 0:
            return None
        ops.minmax_accum(src, self.minmax, cnt * self.px)
        return self.out.start(src, cnt), lo

    def _harvest(self, p):
        token, lo = p
        view = self.out.wait(token)
        # the chunk's window (and every earlier one) has finished: a window that left fp16's range is reported here, before its
        # frames - NaN by then - could be handed out
        self.eng.check(synchronize=False)
        return lo, view.numpy().copy()                    # the caller's own array; the pinned buffer is reused two chunks on

    def step(self):
        """Issue windows until a piece is ready; returns (first frame, depths) or None at the end."""
        while self.state == "windows":
            k = self.k
            if not self._decide(k):
                self.state = "last"
                break
            s = k % 2
            self._window_depth(k, s)
            self.lanes.ready(s)
            cnt = self.st.push(self.lanes.send[s], self.chunk[k & 1])
            nxt = self._send(self.chunk[k & 1], piece_position(k)[0], cnt)
            self.lanes.release(s)
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
            p = self._send(self.st.tail, tail_position(self.st.k), INTERP_LEN)   # after the last window its tail is final too
            if p is not None:
                return self._harvest(p)
        return None
