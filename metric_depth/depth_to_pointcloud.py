#!/usr/bin/env python
"""Metric depth of a video as one coloured point cloud per frame, with the reference's flags and defaults
(metric_depth/depth_to_pointcloud.py) over the MI355X engine: <output_dir>/point0000.ply, point0001.ply, ...

The reference builds every cloud on the host and writes it through open3d; here the vertex records are built on the device
(video_depth_anything_amd/pointcloud.py, csrc/pointcloud.hip) and a file is Open3D's binary header plus one copy, so open3d is not
needed. Added to the reference's flags: `--checkpoint` as in run.py ("synthetic" = seeded random weights), `--max-depth M` (keep
only pixels with 0 < depth <= M; the default keeps every pixel, as the reference does), `--float32` (15-byte records of floats
in place of Open3D's 27-byte records of doubles) and `--stream` (infer_video_depth_stream: each 22-frame piece's clouds are written
as the piece becomes final, so neither the depths nor the clouds of a long video are ever held whole). Frame I/O is
utils/dc_utils.py, as in run.py. The reference lists only `vitl` because only that metric checkpoint was released; `vits` is
accepted too.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from utils.dc_utils import read_video_frames  # noqa: E402
from video_depth_anything_amd.pointcloud import write_pointclouds  # noqa: E402
from video_depth_anything_amd.video_depth import MetricVideoDepthAnything  # noqa: E402

if __name__ == '__main__':
    parser = argparse.ArgumentParser(description='Video Depth Anything: metric depth to point clouds (MI355X)')
    parser.add_argument('--input_video', type=str, default='../assets/davis_rollercoaster.mp4')
    parser.add_argument('--output_dir', type=str, default='./outputs')
    parser.add_argument('--input_size', type=int, default=518)
    parser.add_argument('--max_res', type=int, default=1280)
    parser.add_argument('--encoder', type=str, default='vitl', choices=['vits', 'vitl'])
    parser.add_argument('--max_len', type=int, default=-1, help='maximum length of the input video, -1 means no limit')
    parser.add_argument('--target_fps', type=int, default=-1, help='target fps of the input video, -1 means the original fps')
    parser.add_argument('--fp32', action='store_true', help='model infer with torch.float32, default is torch.float16')
    parser.add_argument('--focal-length-x', default=470.4, type=float, help='Focal length along the x-axis.')
    parser.add_argument('--focal-length-y', default=470.4, type=float, help='Focal length along the y-axis.')
    parser.add_argument('--checkpoint', type=str, default=None, help='override ./checkpoints/metric_video_depth_anything_<enc>.pth; "synthetic" = seeded random weights')
    parser.add_argument('--max-depth', type=float, default=None, help='keep only pixels with 0 < depth <= this many metres (default: keep every pixel)')
    parser.add_argument('--float32', action='store_true', help='vertices as floats (15-byte records) instead of doubles (27 bytes, what Open3D writes)')
    parser.add_argument('--stream', action='store_true', help='bounded memory: infer_video_depth_stream, the clouds of each piece written as it becomes final')
    args = parser.parse_args()

    DEVICE = 'cuda' if torch.cuda.is_available() else 'cpu'
    model_configs = {
        'vits': {'encoder': 'vits', 'features': 64, 'out_channels': [48, 96, 192, 384]},
        'vitl': {'encoder': 'vitl', 'features': 256, 'out_channels': [256, 512, 1024, 1024]},
    }
    video_depth_anything = MetricVideoDepthAnything(**model_configs[args.encoder])
    ckpt = args.checkpoint or f'./checkpoints/metric_video_depth_anything_{args.encoder}.pth'
    if ckpt == "synthetic":
        from video_depth_anything_amd.weights import synthetic_state_dict
        sd = synthetic_state_dict(video_depth_anything.cfg, seed=0)
    else:
        sd = torch.load(ckpt, map_location='cpu', weights_only=True)
    video_depth_anything.load_state_dict(sd, strict=True)
    video_depth_anything = video_depth_anything.to(DEVICE).eval()

    # on a GPU a Motion-JPEG .avi is decoded there and frames larger than --max_res are scaled there (csrc/resize_u8.hip)
    frames, target_fps = read_video_frames(args.input_video, args.max_len, args.target_fps, args.max_res,
                                           device=DEVICE if DEVICE == 'cuda' else None)
    os.makedirs(args.output_dir, exist_ok=True)
    cloud = dict(fx=args.focal_length_x, fy=args.focal_length_y, max_depth=args.max_depth, dtype='float32' if args.float32 else 'float64',
                 device=DEVICE)
    counts = []
    if args.stream:
        stream = video_depth_anything.infer_video_depth_stream(frames, target_fps, input_size=args.input_size, device=DEVICE, fp32=args.fp32)
        for first, depths in stream:
            colours = frames[first:first + depths.shape[0]]
            counts += write_pointclouds(depths, colours, args.output_dir, first_index=first, **cloud)
    else:
        depths, fps = video_depth_anything.infer_video_depth(frames, target_fps, input_size=args.input_size, device=DEVICE, fp32=args.fp32)
        counts = write_pointclouds(depths, frames, args.output_dir, **cloud)
    print(f"{len(counts)} frames, {sum(counts)} points -> {os.path.join(args.output_dir, 'point0000.ply')} ...")
