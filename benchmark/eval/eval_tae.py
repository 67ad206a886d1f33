#!/usr/bin/env python
"""Score the temporal consistency (TAE) of the .npy depth that benchmark/infer/infer.py wrote, on the device.

The third stage of the reference's benchmark with its flags (`--infer_path`, `--benchmark_path`, `--datasets`, `--start_idx`,
`--end_idx`, `--eval_scenes_num`, `--hard_crop`): for each of the first `eval_scenes_num` scenes of the dataset's JSON manifest, take
frames `start_idx:end_idx`, stack the ground truth (divided by each frame's `factor`, cropped to the dataset's window), the
predictions, and each frame's `K` and `pose` from the manifest, score them with `evaluate_tae` (one scale / shift per scene, then
every neighbouring pair reprojected in both directions), and append the mean over scenes to `<infer_path>/results.txt` as
`<dataset>: <value>` between the dataset's start and finish rules.

Differences from the reference's script: the arithmetic runs in HIP kernels (csrc/tae.hip) instead of torch; only `scannet` is
known, and it is the default - the reference's default also names `sintel`, for which its script has no settings and crashes;
predictions must be .npy. As in the reference, `--hard_crop` cuts the dataset's window out of each prediction first, and a
prediction that is then not at the cropped ground truth's size is resized to it (cv2.resize's INTER_LINEAR arithmetic, on the
device: csrc/resize.hip) - so infer.py's full-size output scores with or without the flag. Frames whose prediction file is missing
are left out together with their K and pose, as in the reference.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from video_depth_anything_amd.evaluate import evaluate_tae, load_gt  # noqa: E402

# dataset flag -> (manifest file, max_depth_eval, crop rows a:b, columns c:d); no dataset here has masks
DATASETS = {"scannet": ("scannet_video.json", 10.0, (8, -8, 11, -11))}


def infer_file(infer_path, name, image):
    return os.path.join(infer_path, name, os.path.splitext(image)[0] + ".npy")


def score_scene(frames, infer_path, root, name, max_depth, crop, hard_crop):
    """frames: the manifest's list of {image, gt_depth, factor, K, pose}. Frames whose prediction file is missing are left out. Returns
    evaluate_tae's dict with "resized": (from size, to size) when the predictions were resized to the ground truth's, else None."""
    a, b, c, d = crop
    preds, gts, Ks, poses = [], [], [], []
    for fr in frames:
        p = infer_file(infer_path, name, fr["image"])
        if not os.path.exists(p):
            continue
        pred = np.load(p).astype(np.float32)
        preds.append(pred[a:b, c:d] if hard_crop else pred)
        gts.append(load_gt(os.path.join(root, fr["gt_depth"]), fr["factor"])[a:b, c:d])
        Ks.append(np.array(fr["K"], dtype=np.float64))
        poses.append(np.array(fr["pose"], dtype=np.float64))
    if len(preds) < 2:
        raise FileNotFoundError(f"fewer than two predictions of this scene under {os.path.join(infer_path, name)}")
    gt = np.stack(gts, axis=0)
    if gt.dtype not in (np.float32, np.float64):
        gt = gt.astype(np.float64)
    pred = np.stack(preds, axis=0)
    r = evaluate_tae(pred, gt, np.stack(Ks, axis=0), np.stack(poses, axis=0), max_depth, resize=True)
    r["resized"] = (pred.shape[1:], gt.shape[1:]) if pred.shape[1:] != gt.shape[1:] else None
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--infer_path", type=str, default="")
    ap.add_argument("--benchmark_path", type=str, default="")
    ap.add_argument("--datasets", type=str, nargs="+", default=["scannet"])
    ap.add_argument("--start_idx", type=int, default=0)
    ap.add_argument("--end_idx", type=int, default=180)
    ap.add_argument("--eval_scenes_num", type=int, default=20)
    ap.add_argument("--hard_crop", action="store_true", default=False, help="cut the dataset's window out of the predictions (before any resize)")
    args = ap.parse_args()
    unknown = [d for d in args.datasets if d not in DATASETS]
    if unknown:
        ap.error(f"unknown datasets {unknown}; known: {sorted(DATASETS)}")
    rule = "-" * 50
    for name in args.datasets:
        manifest, max_depth, crop = DATASETS[name]
        root = os.path.join(args.benchmark_path, name)
        with open(os.path.join(root, manifest)) as fs:
            scenes = json.load(fs)[name]
        with open(os.path.join(args.infer_path, "results.txt"), "a") as out:
            print(f"<{rule} {name} start {rule}>")
            out.write(f"<{rule} {name} start {rule}>\n")
            values = []
            for scene in scenes[:args.eval_scenes_num]:
                for key, frames in scene.items():
                    r = score_scene(frames[args.start_idx:args.end_idx], args.infer_path, root, name, max_depth, crop, args.hard_crop)
                    values.append(r["tae"])
                    print(f"{name}/{key}: tae {r['tae']:.6f} ({r['pair_counts'].shape[0] + 1} frames, scale {r['scale']:.6g}, shift {r['shift']:.6g}"
                          + ("" if r["resized"] is None else ", predictions resized from {}x{} to {}x{}".format(*r["resized"][0], *r["resized"][1])) + ")")
            mean = float(np.sum(np.array(values, dtype=np.float64)) / len(values))
            print(f"{name} :  tae  {mean}")
            out.write(f"{name}: {mean}\n")
            out.write(f"<{rule} {name} finish {rule}>\n")


if __name__ == "__main__":
    main()
