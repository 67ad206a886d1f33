"""evaluate_tae_numpy (the host twin of the device TAE scorer) against what the reference's eval_TAE computed on the four cases of
tests/golden/tae_metrics.npz (tools/gen_tae_golden.py). CPU only; needs neither the library nor a GPU."""
import os

import numpy as np
import pytest

from _tae_inputs import CASES, assert_matches, load_case


@pytest.mark.parametrize("case", CASES)
def test_numpy_twin_matches_the_reference(golden_dir, case):
    from video_depth_anything_amd.evaluate import evaluate_tae_numpy
    pred, gt, K, poses, mask, max_depth, exp = load_case(golden_dir, case)
    assert gt.dtype == (np.float64 if case == "B" else np.float32)        # the two promotion routes of gt / factor
    assert_matches(evaluate_tae_numpy(pred, gt, K, poses, max_depth, mask=mask), exp, f"case {case}")


def test_stored_guard_margins_hold(golden_dir):
    """The conditions on the inputs under which winners and counts are exact, as the fixture tool recorded them."""
    fix = np.load(os.path.join(golden_dir, "tae_metrics.npz"))
    half, mag, qz, gtm = fix["guards"]
    assert (half, mag, qz, gtm) == (1e-6, 1e6, 1e-6, 1e-9)
    for name in CASES:
        m = fix[f"{name}_margins"]            # half-integer distance, max |u|,|v|, min |Qz|, gt margin, determinant, clipped share
        assert m[0] > half and m[1] < mag and m[2] > qz and m[3] > gtm and m[4] != 0.0 and m[5] < 0.25, (name, m)


def test_the_cases_hold_what_they_were_built_for(golden_dir):
    fix = np.load(os.path.join(golden_dir, "tae_metrics.npz"))
    assert (fix["A_landed"][2] == 0).all() and (fix["A_pair_errors"][2] == 0).all()          # nothing lands: 0, still in the denominator
    assert fix["A_tae"] == fix["A_pair_errors"].sum() / 6 * 100
    assert fix["C_pair_counts"][0, 0] == 0 and fix["C_pair_counts"][1, 1] == 0 and fix["C_landed"].min() > 0     # blanked by the mask
    for k in ("A_variant_k_next", "B_variant_first", "B_variant_nearest", "C_variant_masks_swapped"):
        ref = fix[f"{k[0]}_tae"]
        assert abs(fix[k] - ref) > 1e-6 * ref, k


def test_last_wins_is_what_case_b_needs(golden_dir):
    """What the fixture tool measured for a first-wins and a nearest-wins (z-buffer) splat on case B is far outside the bound that
    the last-wins twin meets: a splat of another kind cannot pass case B."""
    from video_depth_anything_amd.evaluate import evaluate_tae_numpy
    pred, gt, K, poses, mask, max_depth, exp = load_case(golden_dir, "B")
    fix = np.load(os.path.join(golden_dir, "tae_metrics.npz"))
    got = evaluate_tae_numpy(pred, gt, K, poses, max_depth)["tae"]
    assert abs(got - exp["tae"]) <= 1e-12 * exp["tae"]
    for k in ("B_variant_first", "B_variant_nearest"):
        assert abs(fix[k] - got) > 1e-3 * exp["tae"], k


def test_k_may_be_one_matrix_for_all_frames(golden_dir):
    from video_depth_anything_amd.evaluate import evaluate_tae_numpy
    pred, gt, K, poses, mask, max_depth, exp = load_case(golden_dir, "C")
    assert (K == K[0]).all()
    a, b = evaluate_tae_numpy(pred, gt, K, poses, max_depth, mask=mask), evaluate_tae_numpy(pred, gt, K[0], poses, max_depth, mask=mask > 0)
    assert a["tae"] == b["tae"] and (a["pair_counts"] == b["pair_counts"]).all()


def test_bad_arguments_raise():
    from video_depth_anything_amd.evaluate import evaluate_tae, evaluate_tae_numpy
    pred, gt = np.ones((3, 4, 6), np.float32), np.ones((3, 4, 6), np.float32)
    K, poses = np.eye(3)[None].repeat(3, 0), np.eye(4)[None].repeat(3, 0)
    for fn in (evaluate_tae_numpy, evaluate_tae):                         # both refuse before anything touches a device
        with pytest.raises(ValueError, match="two"):
            fn(pred[:1], gt[:1], K[:1], poses[:1], 10.0)
        with pytest.raises(ValueError, match="resize"):
            fn(pred, gt[:, :, :5], K, poses, 10.0)
        with pytest.raises(ValueError, match="K must be"):
            fn(pred, gt, np.eye(4), poses, 10.0)
        with pytest.raises(ValueError, match="K "):
            fn(pred, gt, K[:2], poses, 10.0)
        with pytest.raises(ValueError, match="poses"):
            fn(pred, gt, K, poses[:, :3], 10.0)
        with pytest.raises(ValueError, match="poses"):
            fn(pred, gt, K, poses[:2], 10.0)
        with pytest.raises(ValueError, match="mask"):
            fn(pred, gt, K, poses, 10.0, mask=np.ones((3, 4, 5), np.uint8))
