"""evaluate_depth (csrc/eval.hip) on the MI355X against what the reference's eval_depthcrafter computed on the four cases of
tests/golden/eval_metrics.npz, with the bounds of tests/test_eval_numpy.py; plus the properties a device reduction must have:
bit-identical repeats, host / device inputs, float32 / widened float64 gt, chunked feeding, a non-default stream, and the CLI."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _eval_inputs import assert_matches, load_case

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cases = {}


def case(golden_dir, name):
    """Loaded once per session and shared; nothing below writes into the arrays."""
    if name not in _cases:
        _cases[name] = load_case(golden_dir, name)
        for a in _cases[name][:2]:
            a.setflags(write=False)
    return _cases[name]


def run(golden_dir, name, **kw):
    from video_depth_anything_amd.evaluate import evaluate_depth
    pred, gt, max_depth, max_eval_len, exp = case(golden_dir, name)
    return evaluate_depth(pred, gt, max_depth, max_eval_len, **kw), exp


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), (k, a[k], b[k])


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_device_scorer_matches_the_reference(golden_dir, name):
    got, exp = run(golden_dir, name)
    assert_matches(got, exp, f"case {name}")


def test_repeat_is_bit_identical(golden_dir):
    for name in ("A", "D"):
        same_bits(run(golden_dir, name)[0], run(golden_dir, name)[0])


def test_device_tensors_and_host_arrays_agree_bit_for_bit(golden_dir):
    from video_depth_anything_amd.evaluate import evaluate_depth
    for name in ("A", "B"):                                             # A: a cropped (strided) float32 view; B: float64
        pred, gt, max_depth, max_eval_len, _ = case(golden_dir, name)
        host = evaluate_depth(pred, gt, max_depth, max_eval_len)
        dp, dg = torch.from_numpy(np.ascontiguousarray(pred)).cuda(), torch.from_numpy(np.ascontiguousarray(gt)).cuda()
        same_bits(host, evaluate_depth(dp, dg, max_depth, max_eval_len))
        same_bits(host, evaluate_depth(pred, dg, max_depth, max_eval_len))      # one of each


def test_float64_gt_widened_from_float32_gives_the_same_bits(golden_dir):
    from video_depth_anything_amd.evaluate import evaluate_depth
    for name in ("A", "C"):
        pred, gt, max_depth, max_eval_len, _ = case(golden_dir, name)
        assert gt.dtype == np.float32
        same_bits(evaluate_depth(pred, gt, max_depth, max_eval_len), evaluate_depth(pred, gt.astype(np.float64), max_depth, max_eval_len))


def test_chunked_feeding_stays_within_the_bounds(golden_dir):
    got, exp = run(golden_dir, "A", chunk_frames=1)
    assert_matches(got, exp, "case A, one frame per chunk")
    got, exp = run(golden_dir, "A", chunk_frames=2)                     # a ragged last chunk
    assert_matches(got, exp, "case A, two frames per chunk")
    got, exp = run(golden_dir, "B", chunk_frames=1)
    assert_matches(got, exp, "case B, one frame per chunk")


def test_non_default_stream(golden_dir):
    ref, exp = run(golden_dir, "A")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got, _ = run(golden_dir, "A")
    s.synchronize()
    same_bits(ref, got)


def test_no_valid_pixel_gives_nan_on_the_device():
    from video_depth_anything_amd.evaluate import METRICS, evaluate_depth
    r = evaluate_depth(np.ones((2, 3, 5), np.float32), np.zeros((2, 3, 5), np.float32), 10.0)
    assert r["n_frames_used"] == 0 and r["n_valid"] == 0
    assert all(math.isnan(r[k]) for k in METRICS + ("scale", "shift"))


def test_cli_scores_a_two_scene_manifest(golden_dir, tmp_path):
    """benchmark/eval/eval.py as a child process on .npy scenes from case A (float32 gt, factor 1) and case B (uint16 gt, factor
    1000, its first two frames): results.txt holds the scene mean of the fixture's numbers in the reference's format."""
    bench, infer = tmp_path / "bench", tmp_path / "infer"
    scenes, want = [], []
    raw_b = np.load(os.path.join(golden_dir, "eval_metrics.npz"))["B_gt_raw"]
    assert raw_b.dtype == np.uint16
    for name in ("A", "B"):
        pred, gt, max_depth, max_eval_len, exp = case(golden_dir, name)
        assert max_depth == 10.0                                        # bonn's max_depth_eval; its crop 0:480, 0:640 keeps these frames whole
        frames = []
        for i in range(min(pred.shape[0], max_eval_len)):
            rel = f"scene{name}/{i:03d}"
            for root, arr in ((bench / "bonn" / "gt", gt[i] if name == "A" else raw_b[i]), (infer / "bonn" / "rgb", pred[i])):
                os.makedirs(root / f"scene{name}", exist_ok=True)
                np.save(root / f"{rel}.npy", arr)
            frames.append({"image": f"rgb/{rel}.png", "gt_depth": f"gt/{rel}.npy", "factor": 1.0 if name == "A" else 1000.0})
        scenes.append({f"scene{name}": frames})
        want.append(exp)
    with open(bench / "bonn" / "bonn_video.json", "w") as f:
        json.dump({"bonn": scenes}, f)
    r = subprocess.run([sys.executable, os.path.join(REPO, "benchmark", "eval", "eval.py"), "--infer_path", str(infer), "--benchmark_path", str(bench),
                        "--datasets", "bonn"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = (infer / "results.txt").read_text().splitlines()
    rule = "-" * 50
    assert lines[0] == f"<{rule} bonn start {rule}>" and lines[-1] == f"<{rule} bonn finish {rule}>" and len(lines) == 5
    for line, m in zip(lines[1:4], ("abs_relative_difference", "rmse_linear", "delta1_acc")):
        mean = (want[0][m] + want[1][m]) / 2                            # each is > 1e-7 away from a rounding boundary of the 6th decimal
        assert line == f"{m}: {mean:04f}", (line, mean)
