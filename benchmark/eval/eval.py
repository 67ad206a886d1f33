#!/usr/bin/env python
"""Score the .npy depth that benchmark/infer/infer.py wrote against the benchmark's ground truth, on the device.

The second stage of the reference's benchmark with its flags (`--infer_path`, `--infer_type`, `--benchmark_path`, `--datasets`):
for every scene of every dataset in the dataset's JSON manifest, stack the scene's ground truth (divided by each frame's `factor`,
cropped to the dataset's window) and the predictions, score them with `evaluate_depth` (one scale / shift per scene, fitted in
disparity over every valid pixel; a prediction that is not at the cropped ground truth's size is resized to it on the device as
the reference resizes it, cv2.resize's INTER_LINEAR arithmetic - so infer.py's full-size output scores on scannet and nyuv2), and
append the mean over scenes to `<infer_path>/results.txt` as `metric: value` lines between the dataset's start and finish rules.

Differences from the reference's script: the arithmetic runs in HIP kernels (csrc/eval.hip, csrc/resize.hip) instead of host numpy
and cv2; predictions must be .npy; `--all_metrics` also writes squared_relative_difference, delta2_acc and delta3_acc.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from video_depth_anything_amd.evaluate import evaluate_depth, load_gt  # noqa: E402

# dataset flag -> (key in the manifest = directory, manifest file, max_depth_eval, max_eval_len, crop rows a:b, columns c:d)
DATASETS = {
    "kitti":       ("kitti",   "kitti_video.json",       80.0, 110, (0, 374, 0, 1242)),
    "kitti_500":   ("kitti",   "kitti_video_500.json",   80.0, 500, (0, 374, 0, 1242)),
    "sintel":      ("sintel",  "sintel_video.json",      70.0, 100, (0, 436, 0, 1024)),
    "nyuv2_500":   ("nyuv2",   "nyuv2_video_500.json",   10.0, 500, (45, 471, 41, 601)),
    "bonn":        ("bonn",    "bonn_video.json",        10.0, 110, (0, 480, 0, 640)),
    "bonn_500":    ("bonn",    "bonn_video_500.json",    10.0, 500, (0, 480, 0, 640)),
    "scannet":     ("scannet", "scannet_video.json",     10.0, 90,  (8, -8, 11, -11)),
    "scannet_500": ("scannet", "scannet_video_500.json", 10.0, 500, (8, -8, 11, -11)),
}
REPORTED = ("abs_relative_difference", "rmse_linear", "delta1_acc")
EXTRA = ("squared_relative_difference", "delta2_acc", "delta3_acc")


def infer_file(infer_path, name, image):
    return os.path.join(infer_path, name, os.path.splitext(image)[0] + ".npy")


def resized_note(resized):
    return "" if resized is None else ", predictions resized from {}x{} to {}x{}".format(*resized[0], *resized[1])


def score_scene(frames, infer_path, root, name, max_depth, max_eval_len, crop):
    """frames: the manifest's list of {image, gt_depth, factor}. Frames whose prediction file is missing are left out. Returns
    evaluate_depth's dict with "resized": (from size, to size) when the predictions were resized to the ground truth's, else None."""
    a, b, c, d = crop
    preds, gts = [], []
    for fr in frames[:max_eval_len]:
        p = infer_file(infer_path, name, fr["image"])
        if not os.path.exists(p):
            continue
        gts.append(load_gt(os.path.join(root, fr["gt_depth"]), fr["factor"])[a:b, c:d])
        preds.append(np.load(p).astype(np.float32))
    if not preds:
        raise FileNotFoundError(f"no prediction of this scene under {os.path.join(infer_path, name)}")
    gt = np.stack(gts, axis=0)
    if gt.dtype not in (np.float32, np.float64):
        gt = gt.astype(np.float64)
    pred = np.stack(preds, axis=0)
    r = evaluate_depth(pred, gt, max_depth, max_eval_len, resize=True)
    r["resized"] = (pred.shape[1:], gt.shape[1:]) if pred.shape[1:] != gt.shape[1:] else None
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--infer_path", type=str, default="")
    ap.add_argument("--infer_type", type=str, default="npy", help="only npy: the format benchmark/infer/infer.py writes")
    ap.add_argument("--benchmark_path", type=str, default="")
    ap.add_argument("--datasets", type=str, nargs="+", default=["kitti", "sintel", "bonn", "scannet"])
    ap.add_argument("--all_metrics", action="store_true", help="also write " + ", ".join(EXTRA))
    args = ap.parse_args()
    if args.infer_type != "npy":
        ap.error("--infer_type: only npy predictions are scored")
    unknown = [d for d in args.datasets if d not in DATASETS]
    if unknown:
        ap.error(f"unknown datasets {unknown}; known: {sorted(DATASETS)}")
    names = REPORTED + (EXTRA if args.all_metrics else ())
    rule = "-" * 50
    for flag in args.datasets:
        name, manifest, max_depth, max_eval_len, crop = DATASETS[flag]
        root = os.path.join(args.benchmark_path, name)
        with open(os.path.join(root, manifest)) as fs:
            scenes = json.load(fs)[name]
        with open(os.path.join(args.infer_path, "results.txt"), "a") as out:
            print(f"<{rule} {name} start {rule}>")
            out.write(f"<{rule} {name} start {rule}>\n")
            rows = []
            for scene in scenes:
                for key, frames in scene.items():
                    r = score_scene(frames, args.infer_path, root, name, max_depth, max_eval_len, crop)
                    rows.append([r[m] for m in names])
                    print(f"{name}/{key}: " + ", ".join(f"{m} {r[m]:.6f}" for m in names) + f" ({r['n_frames_used']} frames, {r['n_valid']} pixels" + resized_note(r["resized"]) + ")")
            mean = np.mean(np.array(rows, dtype=np.float64), axis=0)
            for m, v in zip(names, mean):
                print(f"{m}: {v:04f}")
                out.write(f"{m}: {v:04f}\n")
            out.write(f"<{rule} {name} finish {rule}>\n")


if __name__ == "__main__":
    main()
