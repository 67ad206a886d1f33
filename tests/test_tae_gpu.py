"""evaluate_tae (csrc/tae.hip) on the MI355X against what the reference's eval_TAE computed on the four cases of
tests/golden/tae_metrics.npz, with the bounds of tests/test_tae_numpy.py; plus the properties a deterministic splat must have:
bit-identical repeats, chunking and host / device inputs, the 16-byte mask path, and the CLI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _tae_inputs import CASES, assert_matches, load_case

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (k, a[k], b[k])


@pytest.mark.parametrize("name", CASES)
def test_device_tae_matches_the_reference(golden_dir, name):
    """Case B is the one a splat that is not last-wins fails: its first-wins and nearest-wins values differ in the second digit."""
    from video_depth_anything_amd.evaluate import evaluate_tae
    pred, gt, K, poses, mask, max_depth, exp = load_case(golden_dir, name)
    assert_matches(evaluate_tae(pred, gt, K, poses, max_depth, mask=mask), exp, f"case {name}")


def test_chunks_inputs_and_repeats_are_bit_identical(golden_dir):
    from video_depth_anything_amd.evaluate import evaluate_tae
    pred, gt, K, poses, mask, max_depth, exp = load_case(golden_dir, "D")
    whole = evaluate_tae(pred, gt, K, poses, max_depth)
    assert_matches(whole, exp, "case D")
    same_bits(whole, evaluate_tae(pred, gt, K, poses, max_depth))                               # a repeat
    same_bits(whole, evaluate_tae(pred, gt, K, poses, max_depth, chunk_pairs=1))
    same_bits(whole, evaluate_tae(pred, gt, K, poses, max_depth, chunk_pairs=2))                # 5 pairs: a ragged last chunk
    dp, dg = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    same_bits(whole, evaluate_tae(dp, dg, torch.from_numpy(K), torch.from_numpy(poses).cuda(), max_depth))
    same_bits(whole, evaluate_tae(dp, gt, K, poses, max_depth, chunk_pairs=2))                  # one of each


def test_mask_on_the_16_byte_path_and_bool_masks(golden_dir):
    """Case C's masked planes have 903 pixels (the scalar path). Here: case B's 48 x 64 planes (16-byte loads, 4 mask bytes per load)
    with a seeded mask, against the host twin: counts exact, errors within the bound; a bool mask and a device mask give the same bits."""
    from video_depth_anything_amd.evaluate import evaluate_tae, evaluate_tae_numpy
    pred, gt, K, poses, _, max_depth, _ = load_case(golden_dir, "B")
    mask = (np.random.default_rng(5).random(pred.shape) < 0.6).astype(np.uint8) * 255
    mask[1, :, 7] = 0
    want = evaluate_tae_numpy(pred, gt, K, poses, max_depth, mask=mask)
    want["margins"] = None
    got = evaluate_tae(pred, gt, K, poses, max_depth, mask=mask)
    assert_matches(got, want, "case B with a mask")
    assert (got["pair_counts"] < load_case(golden_dir, "B")[6]["pair_counts"]).all()
    same_bits(got, evaluate_tae(pred, gt, K, poses, max_depth, mask=mask > 0))
    same_bits(got, evaluate_tae(pred, gt, K, poses, max_depth, mask=torch.from_numpy(mask > 0).cuda(), chunk_pairs=1))


def test_non_default_stream(golden_dir):
    from video_depth_anything_amd.evaluate import evaluate_tae
    pred, gt, K, poses, mask, max_depth, _ = load_case(golden_dir, "C")
    ref = evaluate_tae(pred, gt, K, poses, max_depth, mask=mask)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = evaluate_tae(pred, gt, K, poses, max_depth, mask=mask)
    s.synchronize()
    same_bits(ref, got)


def test_cli_scores_a_scene_with_a_missing_prediction(golden_dir, tmp_path):
    """benchmark/eval/eval_tae.py as a child process on a scannet-shaped directory built from case A: 53 x 75 ground truth and
    predictions that the scannet window 8:-8, 11:-11 cuts to case A's 37 x 53 (--hard_crop), K and pose in the manifest, frame 1's
    prediction missing. It reproduces evaluate_tae on the surviving frames; results.txt has the reference's form."""
    from video_depth_anything_amd.evaluate import evaluate_tae
    pred, gt, K, poses, _, max_depth, _ = load_case(golden_dir, "A")
    assert max_depth == 10.0 and pred.shape[1:] == (37, 53)
    bench, infer = tmp_path / "bench", tmp_path / "infer"
    frames = []
    for i in range(pred.shape[0]):
        rel = f"scene0/{i:03d}"
        for root, arr in ((bench / "scannet" / "gt", gt[i]), (infer / "scannet" / "rgb", pred[i])):
            if i == 1 and root.parent.parent == infer:
                continue
            os.makedirs(root / "scene0", exist_ok=True)
            np.save(root / f"{rel}.npy", np.pad(arr, ((8, 8), (11, 11)), constant_values=0.5))
        frames.append({"image": f"rgb/{rel}.jpg", "gt_depth": f"gt/{rel}.npy", "factor": 1.0, "K": K[i].tolist(), "pose": poses[i].tolist()})
    with open(bench / "scannet" / "scannet_video.json", "w") as f:
        json.dump({"scannet": [{"scene0": frames}]}, f)
    r = subprocess.run([sys.executable, os.path.join(REPO, "benchmark", "eval", "eval_tae.py"), "--infer_path", str(infer), "--benchmark_path", str(bench),
                        "--hard_crop"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    keep = [0, 2, 3]
    want = evaluate_tae(pred[keep], gt[keep], K[keep], poses[keep], max_depth)
    assert want["tae"] > 0 and want["pair_counts"][0].min() > 0
    lines = (infer / "results.txt").read_text().splitlines()
    rule = "-" * 50
    assert lines == [f"<{rule} scannet start {rule}>", f"scannet: {want['tae']}", f"<{rule} scannet finish {rule}>"], lines
