"""resize_prediction (csrc/resize.hip) on the MI355X: bit for bit the host twin resize_prediction_numpy on every shape (the file is
built without fused multiply-add, so every rounding of the contract is the twin's), host / device inputs, a non-default stream,
repeats; the scorers' `resize=True` against their twins and against resizing up front; and the two CLIs on predictions at the
uncropped size.

The shapes cover what a launch can get wrong: every output row (11, 5, 3, 9, 19, 618, 621 pixels) is no multiple of a vector width
(2 or 4) except 618 = 2 * 309, and none is a multiple of the 256-thread block: 618 and 621 span three blocks with a ragged last
one; no n * H * W (264, 90, 24, 70, 108, 855, 573 504, 232 254) is a multiple of the block size either."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _eval_inputs
import _tae_inputs
from _resize_inputs import IDS, SHAPES, planes

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_twins = {}


def twin(n, src_hw, dst_hw):
    """The host twin's result, computed once per shape and shared."""
    from video_depth_anything_amd.evaluate import resize_prediction_numpy
    key = (n, src_hw, dst_hw)
    if key not in _twins:
        _twins[key] = torch.from_numpy(resize_prediction_numpy(planes(n, src_hw), dst_hw))
    return _twins[key]


def report_difference(got, want, what):
    """Which outputs differ and by how much: printed before the assertion so a failure says which rounding to look for."""
    diff = (got != want).nonzero()
    if diff.numel():
        worst = (got.double() - want.double()).abs().max().item()
        print(f"{what}: {diff.shape[0]} of {want.numel()} values differ, worst {worst:.3e}, first at {diff[0].tolist()}: "
              f"got {got[tuple(diff[0])].item()!r} want {want[tuple(diff[0])].item()!r}")


@pytest.mark.parametrize("n,src_hw,dst_hw", SHAPES, ids=IDS)
def test_device_resize_is_the_twin_bit_for_bit(n, src_hw, dst_hw):
    from video_depth_anything_amd.evaluate import resize_prediction
    src, want = planes(n, src_hw), twin(n, src_hw, dst_hw)
    out = resize_prediction(src, dst_hw)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (n,) + dst_hw
    got = out.cpu()
    report_difference(got, want, f"{src_hw} -> {dst_hw}")
    assert torch.equal(got, want)
    dev_in = torch.from_numpy(src).cuda()
    assert torch.equal(resize_prediction(dev_in, dst_hw).cpu(), want)           # a CUDA tensor as input
    assert torch.equal(resize_prediction(src, dst_hw).cpu(), want)              # a second run
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        on_stream = resize_prediction(src, dst_hw)
    s.synchronize()
    assert torch.equal(on_stream.cpu(), want)


def test_identity_size_is_the_upload():
    from video_depth_anything_amd.evaluate import resize_prediction
    src = planes(3, (5, 7))
    out = resize_prediction(src, (5, 7))
    assert out.is_cuda and torch.equal(out.cpu(), torch.from_numpy(src))
    dev_in = torch.from_numpy(src).cuda()
    assert resize_prediction(dev_in, (5, 7)).data_ptr() == dev_in.data_ptr()


def at_size(pred, size, seed):
    """A seeded prediction at another size than `pred` [N,H,W]: pred resized to `size`, with 1 % noise."""
    from video_depth_anything_amd.evaluate import resize_prediction_numpy
    other = resize_prediction_numpy(np.ascontiguousarray(pred), size)
    return other * np.random.default_rng(seed).uniform(0.99, 1.01, size=other.shape).astype(np.float32)


def other_size(pred, seed):
    """About 1.3 x 0.8 of pred's size."""
    N, H, W = pred.shape
    return at_size(pred, (int(H * 1.3) + 2, max(2, int(W * 0.8) - 1)), seed)


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.asarray(a[k], dtype=np.float64).tobytes() == np.asarray(b[k], dtype=np.float64).tobytes(), (k, a[k], b[k])


@pytest.mark.parametrize("name", ["A", "C"])
def test_evaluate_depth_resizes_first(golden_dir, name):
    from video_depth_anything_amd.evaluate import evaluate_depth, evaluate_depth_numpy, resize_prediction
    pred, gt, max_depth, max_eval_len, _ = _eval_inputs.load_case(golden_dir, name)
    small = other_size(pred, 11)
    want = evaluate_depth_numpy(small, gt, max_depth, max_eval_len, resize=True)
    got = evaluate_depth(small, gt, max_depth, max_eval_len, resize=True)
    _eval_inputs.assert_matches(got, want, f"case {name}, resized, against the twin")
    same_bits(got, evaluate_depth(resize_prediction(small, gt.shape[1:]), gt, max_depth, max_eval_len))
    same_bits(got, evaluate_depth(torch.from_numpy(small).cuda(), gt, max_depth, max_eval_len, resize=True))
    for chunk in (1, 2):                                                 # the bounds test_eval_gpu.py allows between chunkings
        got = evaluate_depth(small, gt, max_depth, max_eval_len, resize=True, chunk_frames=chunk)
        _eval_inputs.assert_matches(got, want, f"case {name}, resized, {chunk} frames per chunk")


@pytest.mark.parametrize("name", ["A", "C"])
def test_evaluate_tae_resizes_first(golden_dir, name):
    from video_depth_anything_amd.evaluate import evaluate_tae, evaluate_tae_numpy, resize_prediction
    pred, gt, K, poses, mask, max_depth, _ = _tae_inputs.load_case(golden_dir, name)
    small = other_size(pred, 12)
    want = evaluate_tae_numpy(small, gt, K, poses, max_depth, mask=mask, resize=True)
    want["margins"] = None
    got = evaluate_tae(small, gt, K, poses, max_depth, mask=mask, resize=True)
    _tae_inputs.assert_matches(got, want, f"case {name}, resized, against the twin")
    same_bits(got, evaluate_tae(resize_prediction(small, gt.shape[1:]), gt, K, poses, max_depth, mask=mask))
    for chunk in (1, 2):                                                 # test_tae_gpu.py: chunk_pairs never changes a bit
        same_bits(got, evaluate_tae(small, gt, K, poses, max_depth, mask=mask, resize=True, chunk_pairs=chunk))


def run_cli(script, infer, bench):
    r = subprocess.run([sys.executable, os.path.join(REPO, "benchmark", "eval", script), "--infer_path", str(infer), "--benchmark_path", str(bench),
                        "--datasets", "scannet"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout, (infer / "results.txt").read_text().splitlines()


def test_both_clis_score_predictions_at_the_uncropped_size(golden_dir, tmp_path):
    """A scannet-shaped tree built from TAE case A: 53 x 75 ground truth that the scannet window 8:-8, 11:-11 cuts to case A's 37 x 53,
    and predictions at the same full 53 x 75, as infer.py writes them. No --hard_crop: both scorers resize 53 x 75 to 37 x 53 and
    results.txt carries the host twins' values."""
    from video_depth_anything_amd.evaluate import evaluate_depth_numpy, evaluate_tae_numpy
    pred, gt, K, poses, _, max_depth, _ = _tae_inputs.load_case(golden_dir, "A")
    assert max_depth == 10.0 and pred.shape[1:] == (37, 53)
    full = at_size(pred, (53, 75), 13)
    assert full.shape[1:] == (53, 75) and full.dtype == np.float32
    bench, infer = tmp_path / "bench", tmp_path / "infer"
    frames = []
    for i in range(pred.shape[0]):
        rel = f"scene0/{i:03d}"
        for root, arr in ((bench / "scannet" / "gt", np.pad(gt[i], ((8, 8), (11, 11)), constant_values=0.5)), (infer / "scannet" / "rgb", full[i])):
            os.makedirs(root / "scene0", exist_ok=True)
            np.save(root / f"{rel}.npy", arr)
        frames.append({"image": f"rgb/{rel}.jpg", "gt_depth": f"gt/{rel}.npy", "factor": 1.0, "K": K[i].tolist(), "pose": poses[i].tolist()})
    with open(bench / "scannet" / "scannet_video.json", "w") as f:
        json.dump({"scannet": [{"scene0": frames}]}, f)
    rule = "-" * 50

    want = evaluate_depth_numpy(full, gt, max_depth, 90, resize=True)
    stdout, lines = run_cli("eval.py", infer, bench)
    assert "resized from 53x75 to 37x53" in stdout, stdout
    assert lines[0] == f"<{rule} scannet start {rule}>" and lines[-1] == f"<{rule} scannet finish {rule}>" and len(lines) == 5
    for line, m in zip(lines[1:4], ("abs_relative_difference", "rmse_linear", "delta1_acc")):
        key, value = line.split(": ")
        print(f"eval.py {key}: {value} want {want[m]!r}")
        assert key == m and abs(float(value) - want[m]) <= 1e-6, (line, want[m])

    want = evaluate_tae_numpy(full, gt, K, poses, max_depth, resize=True)
    assert want["tae"] > 0 and want["pair_counts"][0].min() > 0
    stdout, lines = run_cli("eval_tae.py", infer, bench)
    assert "resized from 53x75 to 37x53" in stdout, stdout
    assert lines[5] == f"<{rule} scannet start {rule}>" and lines[7] == f"<{rule} scannet finish {rule}>" and len(lines) == 8
    key, value = lines[6].split(": ")
    print(f"eval_tae.py {key}: {value} want {want['tae']!r}")
    assert key == "scannet" and abs(float(value) - want["tae"]) <= 1e-6, (lines[6], want["tae"])
