"""`VideoDepthAnything`: the drop-in class for the reference's model wrapper.

Same constructor arguments, `load_state_dict(sd, strict=True)`, `forward(x)` and
`infer_video_depth(frames, target_fps, input_size=518, device='cuda', fp32=False)` as
/root/reference/video_depth_anything/video_depth.py:37-63,89-93,161-254, so the four callers
(run.py:45-50, metric_depth/run.py:43-48, app.py:34-48, benchmark/infer/infer.py:36-58) can switch
by changing one import. All arithmetic runs in libvda_hip.so: the model is a `vda_model` handle of the C ABI
(handle.py -> csrc/host.hip), preprocessing / resize / stitch are per-kernel entry points.

Precision follows the reference: `infer_video_depth(..., fp32=False)` is its autocast path (fp16 MFMA operands, fp32
accumulation and residual streams), `fp32=True` its full-fp32 path (fp32 operands on fp32-input MFMA). A bare
`model(x)` takes the precision from the ambient `torch.autocast` state exactly as the reference's nn.Module would
(fp32 outside autocast, fp16 inside); pass `fp32=` to be explicit.
"""
import numpy as np
import torch

from .config import INFER_LEN, get_config
from .scheduler import network_size


class VideoDepthAnything:
    METRIC = False   # metric variant stitches with scale=1, shift=0 (metric_depth/.../video_depth.py:132)

    def __init__(self, encoder='vits', features=64, out_channels=[48, 96, 192, 384], use_bn=False, use_clstoken=False,
                 num_frames=32, pe='ape', **_unused):
        # num_block / out_channel / conv of the fork's constructor (video_depth.py:47-49) are accepted and unused, as there.
        self.encoder = encoder
        self.intermediate_layer_idx = {'vits': [2, 5, 8, 11], 'vitl': [4, 11, 17, 23]}
        # use_bn / pe='rope' (no released configuration sets them): BatchNorm folded into the fusion blocks' convs at pack time,
        # rotary embedding of q / k in the temporal attention; any other pe raises NotImplementedError as motion_module.py:226-227
        self.cfg = get_config(encoder, features, out_channels, num_frames, use_clstoken, use_bn, pe)
        self.engine = None
        self._device = torch.device('cuda' if torch.cuda.is_available() else 'cpu')
        self._sd = None
        # Multi-rank runs (torch.distributed initialised): ranks that should receive the stitched video. None = every rank
        # (each process returns the full sequence); e.g. (0,) lets the other ranks skip the stitch and its device-to-host
        # copies - they return (None, target_fps).
        self.result_ranks = None
        # What the ranks exchange per round: "windows" = whole windows all-gathered, every result rank stitches the video
        # (north_star's form); "keys" = 11 key frames per window all-gathered, the scale/shift chain on every rank, each rank
        # finalises its own windows and only final frames travel to the result ranks (scheduler.drive_windows_keys).
        # Both give bit-identical videos.
        self.exchange = "windows"

    # ---- nn.Module-like surface used by the callers -------------------------------------------
    def load_state_dict(self, state_dict, strict=True):
        from .weights import check_state_dict
        check_state_dict(self.cfg, state_dict, strict)
        self._sd = state_dict
        if self.engine is not None:
            self.engine.load_state_dict(state_dict, strict)
        return self

    def to(self, device):
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError("video_depth_anything_amd runs on an MI355X HIP device only (got device=%r)" % (device,))
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if self.engine is not None and device != self.engine.device:
            self.engine.close()                   # the handle is bound to one device: rebuild it on the new one
            self.engine = None
        self._device = device
        self._ensure_engine()
        return self

    def cuda(self):
        return self.to('cuda')

    def eval(self):
        return self

    def _ensure_engine(self):
        if self.engine is None:
            from .handle import ModelHandle       # imports the HIP library; fails loudly if it is missing
            self.engine = ModelHandle(self.cfg, self._device)
            if self._sd is not None:
                self.engine.load_state_dict(self._sd, True)
        return self.engine

    def python_engine(self):
        """The Python launch sequence over the per-kernel ABI (engine.py): the bit-exact cross-check of the handle."""
        from .engine import Engine
        if self.cfg.use_bn or self.cfg.pe != "ape":
            raise NotImplementedError("the Python launch sequence (engine.py) covers the released configurations only; "
                                      "use_bn / pe='rope' run through the handle (vda_forward)")
        e = Engine(self.cfg, self._ensure_engine().device)
        e.load_state_dict(self._sd, True)
        return e

    # ---- forward -----------------------------------------------------------------------------
    def forward(self, x, fp32=None):
        """x [B,T,3,H,W] (H, W multiples of 14, T <= 32) -> depth fp32 [B,T,H,W]."""
        if fp32 is None:
            fp32 = not torch.is_autocast_enabled()
        return self._ensure_engine().forward(x, fp32=bool(fp32))

    __call__ = forward

    # ---- video inference ---------------------------------------------------------------------
    def infer_video_depth(self, frames, target_fps, input_size=518, device='cuda', fp32=False):
        if torch.device(device).type != 'cuda':
            raise RuntimeError("video_depth_anything_amd runs on an MI355X HIP device only (got device=%r)" % (device,))
        return self._infer_video_depth(self._ensure_engine(), frames, target_fps, input_size, bool(fp32))

    def infer_video_depth_stream(self, frames, target_fps, input_size=518, device='cuda', fp32=False):
        """infer_video_depth for a video of unknown length, in bounded memory (stream.py):

            stream = model.infer_video_depth_stream(frames, target_fps)
            for first, depths in stream:      # depths: np.float32 [c, H0, W0] = frames first .. first + c - 1, the caller's own array
                ...
            stream.n_frames, stream.depth_min, stream.depth_max, stream.fps      # valid once exhausted

        frames: an [N,H,W,3] array or memory map (as infer_video_depth takes it), or any iterable of [H,W,3] frames or [m,H,W,3]
        blocks. The pieces are what the stitcher makes final - 24 frames, then 22 per window, then the 8-frame tail, trimmed to the
        video -, in order; concatenated they are bit-identical to infer_video_depth's result. A bad block raises infer_video_depth's
        ValueError / TypeError when it is drawn, a source without frames ValueError("empty video"), a window whose residual stream
        left fp16's range RuntimeError before any of its frames is handed out. stream.close() (also on garbage collection) stops
        early; on every way out the lanes are joined and the handle's options restored. One rank only."""
        import torch.distributed as dist
        from .stream import DepthStream
        if torch.device(device).type != 'cuda':
            raise RuntimeError("video_depth_anything_amd runs on an MI355X HIP device only (got device=%r)" % (device,))
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("infer_video_depth_stream runs on one rank: sharding a video of unknown length is not built; "
                                      "with torch.distributed initialised use infer_video_depth, which shards the windows of an array")
        return DepthStream(self, self._ensure_engine(), frames, target_fps, input_size, bool(fp32))

    def _infer_video_depth(self, eng, frames, target_fps, input_size, fp32):
        import torch.distributed as dist
        from .lanes import WindowLanes, as_u8_frames, check_frames, upload_runs, video_session
        from .scheduler import drive_windows, plan_windows, shard_windows
        from .stitch import all_gather, stitch_stream
        if not isinstance(frames, np.ndarray):
            frames = np.asarray(frames)
        check_frames(frames)
        n = frames.shape[0]
        if frames.dtype != np.uint8:
            u8 = np.empty(frames.shape, dtype=np.uint8)
            for i in range(0, n, 64):                            # chunked: a memory-mapped video is not paged in at once
                u8[i:i + 64] = as_u8_frames(frames[i:i + 64])
            frames = u8
        H0, W0 = frames.shape[1:3]
        H, W = network_size(H0, W0, input_size)
        dev = eng.device
        plan = plan_windows(n)
        world = dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1
        rank = dist.get_rank() if world > 1 else 0
        mine = list(shard_windows(len(plan), world, rank))
        wanted = self.result_ranks is None or rank in self.result_ranks

        # The uint8 frames THIS rank's windows read (frame 0, the previous window's key frame and its own 30 frames each -
        # SURVEY.md section 8e) live in HBM in a compact buffer, and each crosses PCIe once - not all up front: what the next
        # window needs is uploaded on a side stream while the current one computes.
        # `frames` may be a memory map (utils/dc_utils.read_video_frames on a .npy): only the runs a window needs are touched
        need = sorted({f for k in mine for f in plan[k]})
        slot_of = {f: i for i, f in enumerate(need)}
        resident = set()

        with video_session(eng, 1 if world > 1 else 0) as (_, streams), torch.cuda.device(dev):
            video = torch.empty((max(len(need), 1), H0, W0, 3), dtype=torch.uint8, device=dev)
            upload = torch.cuda.Stream(device=dev)
            lanes = WindowLanes(eng, video, H, W, fp32)
            streams += lanes.lanes
            send, acquire, ready, release = lanes.send, lanes.acquire, lanes.ready, lanes.release

            def ensure(k):
                """Queue the upload of window k's not-yet-resident frames (runs of consecutive frames = one copy each)."""
                if k is None:
                    return
                todo = sorted(f for f in set(plan[k]) if f not in resident)
                with torch.cuda.stream(upload):
                    upload_runs(video, [(f, slot_of[f]) for f in todo], lambda f0, f1: [(f0, frames[f0:f1])])
                resident.update(todo)

            def window_depth(k, s, keys=None):
                ensure(k)
                lanes.run([slot_of[f] for f in plan[k]], s, upload, keys)
                pos = mine.index(k)
                ensure(mine[pos + 1] if pos + 1 < len(mine) else None)          # overlaps this window's compute

            if self.exchange == "keys":
                from .scheduler import KEY_SLOTS, drive_windows_keys
                from .stitch import DeviceKeyOps, collect_pieces
                assert tuple(KEY_SLOTS) == (0, 1, 12) + tuple(range(INFER_LEN - 8, INFER_LEN))

                def gather_keys(s, out, inp):
                    lanes.behind(s, (lambda: all_gather(out, inp)) if world > 1 else (lambda: out[0].copy_(inp)))

                kops = DeviceKeyOps(send, H0, W0, dev, self.METRIC, world, rank, len(plan), self.result_ranks, window_depth, ready,
                                    release, gather_keys, acquire)
                pieces = drive_windows_keys(len(plan), world, rank, kops, self.result_ranks)
                if wanted:
                    depths = collect_pieces(pieces, n, H0, W0, dev, on_copied=kops.copied)
            else:
                # One process per GPU: rank r computes windows r, r + world, ... with no data-path collective; after each round
                # the finished windows are all-gathered (the one exchange of the path: RCCL over xGMI, on the slot's lane behind
                # its window, under the next round's compute - the lane's next window, two rounds on, queues behind a gather that
                # has long finished under the other lane's compute) and handed to the stitcher in window order, so only a two-slot
                # ring of gathered windows ever exists. Ranks without a window in the last round contribute an unused slot.
                recv = [torch.empty(world, INFER_LEN, H0, W0, dtype=torch.float32, device=dev) for _ in send] if world > 1 else None
                pieces = drive_windows(len(plan), world, rank, send, recv, window_depth,
                                       lambda s: lanes.behind(s, lambda: all_gather(recv[s], send[s])), ready, release)
                if wanted:
                    depths = stitch_stream(pieces, n, H0, W0, dev, metric=self.METRIC)
            if not wanted:
                for _ in pieces:                                                 # compute and exchange; no stitch, no D2H
                    pass
                depths = None
            eng.check()                                   # a window whose residual stream left fp16's range is an error, not a NaN video
            return depths, target_fps


class MetricVideoDepthAnything(VideoDepthAnything):
    """metric_depth/video_depth_anything/video_depth.py: ViT-L defaults, no scale/shift alignment."""
    METRIC = True

    def __init__(self, encoder='vitl', features=256, out_channels=[256, 512, 1024, 1024], use_bn=False, use_clstoken=False,
                 num_frames=32, pe='ape'):
        super().__init__(encoder, features, out_channels, use_bn, use_clstoken, num_frames, pe)
