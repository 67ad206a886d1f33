"""resize_prediction_numpy, the host twin of the device resize (csrc/resize.hip), against an independent yardstick, and the scorers'
`resize=True` on the host: no library, no GPU."""
import numpy as np
import pytest

import _eval_inputs
import _tae_inputs
from _resize_inputs import IDS, SHAPES, bound, planes, yardstick


def other_size(pred, seed):
    """A seeded prediction at another size than `pred` [N,H,W]: pred resized to about 1.3 x 0.8 of its size, with 1 % noise."""
    from video_depth_anything_amd.evaluate import resize_prediction_numpy
    N, H, W = pred.shape
    small = resize_prediction_numpy(np.ascontiguousarray(pred), (int(H * 1.3) + 2, max(2, int(W * 0.8) - 1)))
    noise = np.random.default_rng(seed).uniform(0.99, 1.01, size=small.shape).astype(np.float32)
    return small * noise


@pytest.mark.parametrize("n,src_hw,dst_hw", SHAPES, ids=IDS)
def test_twin_matches_the_yardstick(n, src_hw, dst_hw):
    from video_depth_anything_amd.evaluate import resize_prediction_numpy
    src = planes(n, src_hw)
    out = resize_prediction_numpy(src, dst_hw)
    assert out.dtype == np.float32 and out.shape == (n,) + dst_hw
    err = float(np.abs(out.astype(np.float64) - yardstick(src, dst_hw)).max())
    print(f"{src_hw} -> {dst_hw}: worst |out - yardstick| {err:.3e}, bound {bound(src):.3e}")
    assert err <= bound(src)
    lo, hi = float(src.min()), float(src.max())
    assert out.min() >= lo * (1 - 1e-6) and out.max() <= hi * (1 + 1e-6), (out.min(), lo, out.max(), hi)


@pytest.mark.parametrize("n,src_hw,dst_hw", SHAPES[:6], ids=IDS[:6])
def test_every_plane_is_resized_alone(n, src_hw, dst_hw):
    """The plane stride: plane k of the stack equals the resize of plane k on its own."""
    from video_depth_anything_amd.evaluate import resize_prediction_numpy
    src = planes(n, src_hw)
    out = resize_prediction_numpy(src, dst_hw)
    for k in range(n):
        assert np.array_equal(out[k], resize_prediction_numpy(src[k:k + 1], dst_hw)[0])


def test_identity_size_returns_the_values_exactly():
    from video_depth_anything_amd.evaluate import resize_prediction_numpy
    for n, hw, _ in SHAPES[:6]:
        src = planes(n, hw)
        assert np.array_equal(resize_prediction_numpy(src, hw), src)


def test_twin_refuses_bad_arguments():
    from video_depth_anything_amd.evaluate import resize_prediction_numpy
    with pytest.raises(ValueError, match="float32"):
        resize_prediction_numpy(np.ones((2, 3, 4), np.float64), (5, 6))
    with pytest.raises(ValueError, match="N,h,w"):
        resize_prediction_numpy(np.ones((3, 4), np.float32), (5, 6))
    with pytest.raises(ValueError, match="positive"):
        resize_prediction_numpy(np.ones((2, 3, 4), np.float32), (0, 6))


@pytest.mark.parametrize("name", ["A", "C"])
def test_evaluate_depth_numpy_resizes_first(golden_dir, name):
    from video_depth_anything_amd.evaluate import evaluate_depth_numpy, resize_prediction_numpy
    pred, gt, max_depth, max_eval_len, _ = _eval_inputs.load_case(golden_dir, name)
    small = other_size(pred, 11)
    assert small.shape[0] == gt.shape[0] and small.shape[1:] != gt.shape[1:]
    got = evaluate_depth_numpy(small, gt, max_depth, max_eval_len, resize=True)
    want = evaluate_depth_numpy(resize_prediction_numpy(small, gt.shape[1:]), gt, max_depth, max_eval_len)
    assert got.keys() == want.keys()
    for k in got:
        assert np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes(), (k, got[k], want[k])
    assert got["n_valid"] > 0 and np.isfinite(got["abs_relative_difference"])


@pytest.mark.parametrize("name", ["A", "C"])
def test_evaluate_tae_numpy_resizes_first(golden_dir, name):
    from video_depth_anything_amd.evaluate import evaluate_tae_numpy, resize_prediction_numpy
    pred, gt, K, poses, mask, max_depth, _ = _tae_inputs.load_case(golden_dir, name)
    small = other_size(pred, 12)
    assert small.shape[0] == gt.shape[0] and small.shape[1:] != gt.shape[1:]
    got = evaluate_tae_numpy(small, gt, K, poses, max_depth, mask=mask, resize=True)
    want = evaluate_tae_numpy(resize_prediction_numpy(small, gt.shape[1:]), gt, K, poses, max_depth, mask=mask)
    assert got.keys() == want.keys()
    for k in got:
        assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), (k, got[k], want[k])
    assert np.isfinite(got["tae"]) and got["pair_counts"].sum() > 0


def test_a_mismatch_without_resize_and_a_frame_count_mismatch_raise():
    """`resize=False` keeps the refusal and its wording; another N raises whatever `resize` is."""
    from video_depth_anything_amd.evaluate import evaluate_depth_numpy, evaluate_tae_numpy
    pred, gt = np.ones((3, 4, 6), np.float32), np.ones((3, 5, 7), np.float32)
    K, poses = np.eye(3), np.stack([np.eye(4)] * 3)
    with pytest.raises(ValueError, match="resize"):
        evaluate_depth_numpy(pred, gt, 10.0)
    with pytest.raises(ValueError, match="resize"):
        evaluate_depth_numpy(pred, gt, 10.0, resize=False)
    with pytest.raises(ValueError, match="number of frames"):
        evaluate_depth_numpy(pred[:2], gt, 10.0, resize=True)
    with pytest.raises(ValueError):
        evaluate_depth_numpy(pred[:2], gt, 10.0)
    with pytest.raises(ValueError, match="resize"):
        evaluate_tae_numpy(pred, gt, K, poses, 10.0)
    with pytest.raises(ValueError, match="resize"):
        evaluate_tae_numpy(pred, gt, K, poses, 10.0, resize=False)
    with pytest.raises(ValueError, match="number of frames"):
        evaluate_tae_numpy(pred[:2], gt, K, poses, 10.0, resize=True)
    with pytest.raises(ValueError, match="mask"):
        evaluate_tae_numpy(pred, gt, K, poses, 10.0, mask=np.ones(pred.shape, np.uint8), resize=True)       # the mask is at gt's size
