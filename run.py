#!/usr/bin/env python
"""CLI with the reference's flags and defaults (/root/reference/run.py:24-34) over the MI355X engine.

Frame I/O is utils/dc_utils.py (same two helpers as the reference's): `--input_video` may be an .npy / .npz (key `frames`)
of uint8 [N,H,W,3] RGB frames, a directory of images, a GIF, a Motion-JPEG .avi (decoded on the device, csrc/mjpeg_decode.hip; with
`--stream` a window's frames at a time, so a long .avi runs in bounded memory), or a video file when decord or cv2 is importable;
frames larger than `--max_res` are scaled down on the device with cv2's 8-bit arithmetic (csrc/resize_u8.hip), with `--stream` a
block at a time (utils.dc_utils.read_video_blocks), so an HD .avi or .npy keeps its bounded memory; the
visualisations are mp4 through imageio when present and animated GIFs otherwise, or with `--mjpeg` Motion-JPEG .avi files that
need no encoder library (the JPEG coding runs on the device too, csrc/mjpeg.hip); `--save_npz` adds <name>_depths.npz
(key `depths`, read with np.load; on a GPU its deflate streams are made on the device, csrc/deflate.hip, instead of by zlib on one core); `--save_exr` adds <name>_depths_exr/frame_00000.exr ... (OpenEXR, channel Z, float32, ZIP; on a GPU the
files are made on the device, csrc/exr.hip, and no OpenEXR library is needed; video_depth_anything_amd.exr.read_exr reads them).
<name>_vis carries the reference's colours: depth is mapped through matplotlib's 256-entry inferno table, which ships in
video_depth_anything_amd/visualize.py (not through the polynomial fit utils/dc_utils.py keeps as save_video's default), and on a
GPU the mapping itself runs on the device (csrc/visualize.hip) - the same bytes as on the host.
`--metric` selects the metric-depth variant (metric_depth/run.py: ViT-L, no scale/shift alignment).
`--stream` runs infer_video_depth_stream instead: an .npy (a memory map) and, on a GPU, a Motion-JPEG .avi are fed to the stream block
by block, the depths go piece by piece into <name>_depths.npy on disk and the visualisation is made from that file block by block,
so neither such a video nor its depth is ever held in memory as one array - with one exception: without `--mjpeg`, <name>_src of an
input that had to be scaled or thinned is written from the scaled frames as one array (the mp4 / GIF writers take no blocks). Every
other kind of input is decoded whole by its decoder, once.
"""
import argparse
import itertools
import os
import struct

import numpy as np
import torch

from utils.dc_utils import read_video_blocks, read_video_frames, reads_in_blocks, save_video
from video_depth_anything_amd import deflate, exr, mjpeg
from video_depth_anything_amd.scale import scaled_size
from video_depth_anything_amd.visualize import inferno_table
from video_depth_anything_amd.video_depth import MetricVideoDepthAnything, VideoDepthAnything


class GrowingNpy:
    """A float32 .npy written piece by piece when the number of frames is not known up front: a fixed 128-byte header is reserved,
    the pieces are appended raw, and close() writes the header for the shape that arrived and returns the file memory-mapped."""
    HEADER = 128

    def __init__(self, path):
        self.path, self.n, self.frame_shape = path, 0, None
        self.f = open(path, "wb")
        self.f.write(b"\0" * self.HEADER)

    def append(self, piece):
        piece = np.ascontiguousarray(piece, dtype=np.float32)
        if self.frame_shape is None:
            self.frame_shape = tuple(piece.shape[1:])
        assert tuple(piece.shape[1:]) == self.frame_shape
        self.f.write(piece.tobytes())
        self.n += piece.shape[0]

    def close(self):
        d = "{'descr': %r, 'fortran_order': False, 'shape': %r, }" % (np.lib.format.dtype_to_descr(np.dtype(np.float32)), (self.n,) + self.frame_shape)
        pad = self.HEADER - 10 - len(d) - 1
        assert pad >= 0
        self.f.seek(0)
        self.f.write(b"\x93NUMPY\x01\x00" + struct.pack("<H", self.HEADER - 10) + (d + " " * pad + "\n").encode("latin1"))
        self.f.close()
        return np.load(self.path, mmap_mode="r")


def write_depth_stream(stream, path, n_frames=None):
    """Every piece of an infer_video_depth_stream into the .npy at `path`; returns it memory-mapped. n_frames known (an array
    source): np.lib.format.open_memmap of the final shape; unknown (an iterable): a growing file whose header is fixed up at the end."""
    sink = None
    for first, d in stream:
        if n_frames is None:
            sink = sink or GrowingNpy(path)
            sink.append(d)
        else:
            if sink is None:
                sink = np.lib.format.open_memmap(path, mode="w+", dtype=np.float32, shape=(n_frames,) + d.shape[1:])
            sink[first:first + d.shape[0]] = d
    if n_frames is None:
        return sink.close()
    sink.flush()
    return np.load(path, mmap_mode="r")


def write_src_from_source_jpegs(path, input_video, max_len, target_fps, max_res, fps, device):
    """<name>_src.avi as a copy of the source's own JPEGs: nothing is decoded or held. Only for a Motion-JPEG .avi that is decoded on
    the device and of which no frame was dropped or scaled (then those JPEGs ARE the frames the model saw); False otherwise."""
    if device is None or not (input_video.lower().endswith('.avi') and os.path.isfile(input_video) and mjpeg.is_mjpeg_avi(input_video)):
        return False
    jpegs = mjpeg.iter_avi(input_video, limit=max_len if max_len > 0 else None)
    src_fps, src_w, src_h = next(jpegs)
    if (target_fps >= 0 and max(round(src_fps / target_fps), 1) != 1) or scaled_size(src_h, src_w, max_res) != (src_h, src_w):
        return False
    mjpeg.write_avi(path, jpegs, fps, src_w, src_h)
    return True


def stream_input(source, device):
    """What run.py --stream feeds infer_video_depth_stream from source = (input_video, max_len, target_fps, max_res): (frames, fps,
    whole). An .npy and (on a device) a Motion-JPEG .avi come as read_video_blocks' iterator and whole is None: neither the file nor
    its scaled frames are ever held as one array. Every other source is decoded whole whichever way it is read, so it is read once,
    by read_video_frames, and whole is that array, kept for <name>_src."""
    if reads_in_blocks(source[0], device):
        blocks, fps = read_video_blocks(*source, device=device)
        return blocks, fps, None
    frames, fps = read_video_frames(*source, device=device)
    return frames, fps, frames


def frames_for_writer(source, device, whole):
    """The frames save_video writes <name>_src from after a stream: the array stream_input kept, else read_video_frames of the source
    once more. That is the memory map itself for an .npy of which nothing is scaled or dropped (save_video reads it a block at a
    time: still bounded). For an .npy or .avi that IS scaled or thinned it is the scaled video as one array: the mp4 / GIF writers
    take no blocks, so this is the one place where --stream without --mjpeg holds a whole (scaled) video."""
    return whole if whole is not None else read_video_frames(*source, device=device)[0]


def block_jpegs(blocks, quality, device):
    """The JPEGs of uint8 [m,H,W,3] blocks, a block at a time: coded on the device when there is one, by the host twin otherwise."""
    for b in blocks:
        yield from (mjpeg.encode_jpeg_numpy(b, quality) if device is None else mjpeg.encode_jpeg(b, quality, device))


def save_depths_npz(path, depths, device):
    """<name>_depths.npz, key `depths`, as np.savez_compressed writes it and np.load reads it. On a device the deflate streams are made
    there (csrc/deflate.hip) instead of by zlib on one core; `depths` may be the memory map --stream left, which is then read block by
    block. Without a device it IS np.savez_compressed."""
    return deflate.savez_compressed(path, device=device, depths=depths)


def save_depths_exr(exr_dir, depths, device):
    """<name>_depths_exr/frame_00000.exr ...: one OpenEXR file per frame, channel Z, float32, ZIP (run.py:64-76). On a device the ZIP
    blocks are made there (csrc/exr.hip), no OpenEXR library needed; `depths` may be the memory map --stream left, which is then read
    a block of frames at a time. Without a device: the OpenEXR library when it imports, as the reference; otherwise the host writer of
    exr.py, whose deflate streams are zlib's."""
    if device is None:
        try:
            import Imath
            import OpenEXR
        except ImportError:
            return exr.write_exr_sequence(depths, exr_dir, device=None)
        os.makedirs(exr_dir, exist_ok=True)
        paths = []
        for i, depth in enumerate(depths):
            header = OpenEXR.Header(depth.shape[1], depth.shape[0])
            header["channels"] = {"Z": Imath.Channel(Imath.PixelType(Imath.PixelType.FLOAT))}
            paths.append(f"{exr_dir}/frame_{i:05d}.exr")
            f = OpenEXR.OutputFile(paths[-1], header)
            f.writePixels({"Z": np.ascontiguousarray(depth, np.float32).tobytes()})
            f.close()
        return paths
    return exr.write_exr_sequence(depths, exr_dir, device=device)


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description='Video Depth Anything (MI355X)')
    parser.add_argument('--input_video', type=str, default='./assets/example_videos/davis_rollercoaster.mp4')
    parser.add_argument('--output_dir', type=str, default='./outputs')
    parser.add_argument('--input_size', type=int, default=518)
    parser.add_argument('--max_res', type=int, default=1280)
    parser.add_argument('--encoder', type=str, default='vitl', choices=['vits', 'vitl'])
    parser.add_argument('--max_len', type=int, default=-1, help='maximum length of the input video, -1 means no limit')
    parser.add_argument('--target_fps', type=int, default=-1, help='target fps of the input video, -1 means the original fps')
    parser.add_argument('--fp32', action='store_true', help='model infer with torch.float32, default is torch.float16')
    parser.add_argument('--grayscale', action='store_true', help='do not apply colorful palette')
    parser.add_argument('--save_npz', action='store_true', help='save depths as npz')
    parser.add_argument('--save_exr', action='store_true', help='save depths as exr')
    parser.add_argument('--metric', action='store_true', help='metric-depth checkpoint and stitching (metric_depth/run.py)')
    parser.add_argument('--stream', action='store_true', help='bounded memory: infer_video_depth_stream, depths written to <name>_depths.npy piece by piece')
    parser.add_argument('--mjpeg', action='store_true', help='write <name>_src.avi / <name>_vis.avi (Motion-JPEG, no encoder library) instead of mp4 / GIF')
    parser.add_argument('--mjpeg_quality', type=int, default=90, help='JPEG quality of --mjpeg, 1..100')
    parser.add_argument('--checkpoint', type=str, default=None, help='override ./checkpoints/<name>.pth; "synthetic" = seeded random weights')
    args = parser.parse_args()

    DEVICE = 'cuda' if torch.cuda.is_available() else 'cpu'
    model_configs = {
        'vits': {'encoder': 'vits', 'features': 64, 'out_channels': [48, 96, 192, 384]},
        'vitl': {'encoder': 'vitl', 'features': 256, 'out_channels': [256, 512, 1024, 1024]},
    }
    cls = MetricVideoDepthAnything if args.metric else VideoDepthAnything
    video_depth_anything = cls(**model_configs[args.encoder])
    ckpt = args.checkpoint or (f'./checkpoints/metric_video_depth_anything_{args.encoder}.pth' if args.metric
                               else f'./checkpoints/video_depth_anything_{args.encoder}.pth')
    if ckpt == "synthetic":
        from video_depth_anything_amd.weights import synthetic_state_dict
        sd = synthetic_state_dict(video_depth_anything.cfg, seed=0)
    else:
        sd = torch.load(ckpt, map_location='cpu', weights_only=True)
    video_depth_anything.load_state_dict(sd, strict=True)
    video_depth_anything = video_depth_anything.to(DEVICE).eval()

    # On a GPU a Motion-JPEG .avi is decoded on the device (csrc/mjpeg_decode.hip) instead of by decord / cv2 / PIL, and frames larger
    # than --max_res are scaled there (csrc/resize_u8.hip). With --stream an .npy and such an .avi are never held as a whole:
    # read_video_blocks hands the stream a window's new frames at a time, dropped frames skipped and large frames scaled block by block.
    io_device = DEVICE if DEVICE == 'cuda' else None
    source = (args.input_video, args.max_len, args.target_fps, args.max_res)
    if args.stream:
        frames, target_fps, whole = stream_input(source, io_device)
    else:
        frames, target_fps = read_video_frames(*source, device=io_device)                                  # run.py:53
    video_name = os.path.basename(args.input_video)
    os.makedirs(args.output_dir, exist_ok=True)
    stem = os.path.join(args.output_dir, os.path.splitext(video_name)[0])
    d_range = {}
    if args.stream:
        stream = video_depth_anything.infer_video_depth_stream(frames, target_fps, input_size=args.input_size, device=DEVICE, fp32=args.fp32)
        depths = write_depth_stream(stream, stem + '_depths.npy', len(whole) if whole is not None else None)
        fps = stream.fps
        d_range = dict(d_min=stream.depth_min, d_max=stream.depth_max)      # the stream kept the range: no second pass over the file
        # <name>_src shows the frames the model saw. A source that was read in blocks is read a second time: with --mjpeg still a
        # block at a time (or its own JPEGs are copied); for the mp4 / GIF writer see frames_for_writer
        if whole is None and args.mjpeg:
            frames = None
            if not write_src_from_source_jpegs(stem + '_src.avi', *source, fps, io_device):
                blocks = read_video_blocks(*source, device=io_device)[0]
                first = next(blocks)
                mjpeg.write_avi(stem + '_src.avi', block_jpegs(itertools.chain([first], blocks), args.mjpeg_quality, io_device), fps,
                                first.shape[2], first.shape[1])
        else:
            frames = frames_for_writer(source, io_device, whole)
    else:
        depths, fps = video_depth_anything.infer_video_depth(frames, target_fps, input_size=args.input_size, device=DEVICE, fp32=args.fp32)

    # run.py:57-62: <name>_src.mp4 and <name>_vis.mp4 (GIFs when no H.264 encoder is importable)
    vis_device = DEVICE if DEVICE == 'cuda' else None
    codec = dict(codec='mjpeg', quality=args.mjpeg_quality) if args.mjpeg else {}      # <name>_src.avi / <name>_vis.avi then
    if frames is not None:
        save_video(frames, stem + '_src.mp4', fps=fps, device=vis_device if args.mjpeg else None, **codec)
    vis_path = save_video(depths, stem + '_vis.mp4', fps=fps, is_depths=True, grayscale=args.grayscale, palette=inferno_table(),
                          device=vis_device, **d_range, **codec)
    if args.save_npz:
        save_depths_npz(stem + '_depths.npz', depths, io_device)
    if args.save_exr:
        save_depths_exr(stem + '_depths_exr', depths, io_device)
    print(f"{depths.shape[0]} frames -> {vis_path}" + (f", {stem}_depths.npz" if args.save_npz else "")
          + (f", {stem}_depths_exr/" if args.save_exr else ""))
