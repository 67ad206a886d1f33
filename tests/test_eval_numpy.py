"""evaluate_depth_numpy (the host twin of the device scorer) against what the reference's eval_depthcrafter computed on the
four cases of tests/golden/eval_metrics.npz (tools/gen_eval_golden.py). CPU only; needs neither the library nor a GPU."""
import math

import numpy as np
import pytest

from _eval_inputs import assert_matches, load_case


@pytest.mark.parametrize("case", ["A", "B", "C", "D"])
def test_numpy_twin_matches_the_reference(golden_dir, case):
    from video_depth_anything_amd.evaluate import evaluate_depth_numpy
    pred, gt, max_depth, max_eval_len, exp = load_case(golden_dir, case)
    assert gt.dtype == (np.float64 if case == "B" else np.float32)        # the two promotion routes of gt / factor
    assert_matches(evaluate_depth_numpy(pred, gt, max_depth, max_eval_len), exp, f"case {case}")


def test_case_a_drops_the_empty_frame_and_case_b_the_third(golden_dir):
    from video_depth_anything_amd.evaluate import evaluate_depth_numpy
    pred, gt, max_depth, max_eval_len, exp = load_case(golden_dir, "A")
    assert exp["n_frames_used"] == 4 and pred.shape[0] == 5
    pred, gt, max_depth, max_eval_len, exp = load_case(golden_dir, "B")
    full = evaluate_depth_numpy(pred, gt, max_depth, None)
    cut = evaluate_depth_numpy(pred, gt, max_depth, max_eval_len)
    assert cut["n_frames_used"] == 2 and full["n_frames_used"] == 3 and full["abs_relative_difference"] != cut["abs_relative_difference"]


def test_shape_mismatch_raises():
    from video_depth_anything_amd.evaluate import evaluate_depth, evaluate_depth_numpy
    pred, gt = np.ones((2, 4, 6), np.float32), np.ones((2, 4, 5), np.float32)
    for fn in (evaluate_depth_numpy, evaluate_depth):                     # both refuse before anything touches a device
        with pytest.raises(ValueError, match="resize"):
            fn(pred, gt, 10.0)


def test_no_valid_pixel_gives_nan():
    from video_depth_anything_amd.evaluate import METRICS, evaluate_depth_numpy
    r = evaluate_depth_numpy(np.ones((2, 3, 5), np.float32), np.zeros((2, 3, 5), np.float32), 10.0)
    assert r["n_frames_used"] == 0 and r["n_valid"] == 0
    assert all(math.isnan(r[k]) for k in METRICS + ("scale", "shift"))
