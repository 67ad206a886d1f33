"""staging.py on the CPU: the block-size formula, the device rule and its error texts, and the scorers' one_device. Nothing here
touches a device: torch.device is only parsed."""
import pytest
import torch

from video_depth_anything_amd import staging


def test_frames_per_block_edges():
    f = staging.frames_per_block
    assert f(10, 100, 99) == 1                  # the budget is below one frame: still one
    assert f(10, 100, 0) == 1
    assert f(10, 100, 300) == 3                 # an exact fit
    assert f(10, 100, 399) == 3
    assert f(2, 100, 1000) == 2                 # fewer frames than fit
    assert f(1, 100, 1000) == 1 and f(1, 100, 1) == 1
    assert f(10, 100, 1000) == 10 and f(10, 100, 1001) == 10


@pytest.mark.parametrize("who,twin,text", [
    ("deflate", "deflate_numpy", "deflate: needs a cuda device, got 'cpu'; deflate_numpy is the host twin"),
    ("exr", "encode_exr_numpy", "exr: needs a cuda device, got 'cpu'; encode_exr_numpy is the host twin"),
    ("mjpeg", "encode_jpeg_numpy", "mjpeg: needs a cuda device, got 'cpu'; encode_jpeg_numpy is the host twin"),
    ("visualize", "colorize_numpy", "visualize: needs a cuda device, got 'cpu'; colorize_numpy is the host twin"),
    ("resize_frames", "resize_frames_numpy", "resize_frames: needs a cuda device, got 'cpu'; resize_frames_numpy is the host twin"),
    ("pointcloud", None, "pointcloud: needs a cuda device, got 'cpu'"),
])
def test_cuda_device_refuses_the_host_in_the_callers_words(who, twin, text):
    with pytest.raises(ValueError) as e:
        staging.cuda_device("cpu", who, twin)
    assert str(e.value) == text
    with pytest.raises(ValueError) as e:
        staging.cuda_device(torch.device("cpu"), who, twin)
    assert str(e.value) == text.replace("'cpu'", "device(type='cpu')")


def test_cuda_device_parses_without_touching_a_device():
    assert staging.cuda_device(None, "x") == torch.device("cuda")
    assert staging.cuda_device("cuda", "x") == torch.device("cuda")
    assert staging.cuda_device("cuda:1", "x") == torch.device("cuda", 1)
    assert staging.cuda_device(torch.device("cuda:1"), "x", "y") == torch.device("cuda", 1)


def test_the_writers_raise_those_texts():
    """The callers hand in the names the six texts are made of."""
    import numpy as np
    from video_depth_anything_amd import deflate, exr, mjpeg, pointcloud, scale, visualize
    calls = [(lambda: deflate.deflate(np.zeros(8, np.uint8), device="cpu"), "deflate: needs a cuda device, got 'cpu'; deflate_numpy is the host twin"),
             (lambda: exr.encode_exr(np.zeros((1, 4, 4), np.float32), device="cpu"), "exr: needs a cuda device, got 'cpu'; encode_exr_numpy is the host twin"),
             (lambda: mjpeg.encode_jpeg(np.zeros((1, 8, 8, 3), np.uint8), device="cpu"), "mjpeg: needs a cuda device, got 'cpu'; encode_jpeg_numpy is the host twin"),
             (lambda: mjpeg.decode_jpeg([b"\xff\xd8"], device="cpu"), "mjpeg: needs a cuda device, got 'cpu'; decode_jpeg_numpy is the host twin"),
             (lambda: visualize.colorize(np.zeros((1, 3, 5), np.float32), device="cpu"), "visualize: needs a cuda device, got 'cpu'; colorize_numpy is the host twin"),
             (lambda: scale.resize_frames(np.ones((2, 3, 4, 3), np.uint8), 5, 6, device="cpu"),
              "resize_frames: needs a cuda device, got 'cpu'; resize_frames_numpy is the host twin"),
             (lambda: pointcloud.unproject(np.ones((1, 3, 5), np.float32), np.zeros((1, 3, 5, 3), np.uint8), 5.0, 5.0, device="cpu"),
              "pointcloud: needs a cuda device, got 'cpu'"),
             (lambda: mjpeg.encode_jpeg(torch.zeros(1, 8, 8, 3, dtype=torch.uint8)), "mjpeg: encode_jpeg takes a cuda tensor or a numpy array; encode_jpeg_numpy is the host twin"),
             (lambda: visualize.colorize(torch.zeros(1, 3, 5)), "visualize: colorize takes a cuda tensor or a numpy array; colorize_numpy is the host twin"),
             (lambda: scale.resize_frames(torch.ones(2, 3, 4, 3, dtype=torch.uint8), 5, 6),
              "resize_frames: takes a cuda tensor or a numpy array; resize_frames_numpy is the host twin")]
    for call, text in calls:
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text


def test_placement():
    import numpy as np
    with pytest.raises(ValueError) as e:
        staging.placement(torch.zeros(3), "cuda", "visualize", "colorize_numpy", "colorize")
    assert str(e.value) == "visualize: colorize takes a cuda tensor or a numpy array; colorize_numpy is the host twin"
    with pytest.raises(ValueError) as e:
        staging.placement(torch.zeros(3), None, "resize_frames", "resize_frames_numpy")
    assert str(e.value) == "resize_frames: takes a cuda tensor or a numpy array; resize_frames_numpy is the host twin"
    assert staging.placement(np.zeros(3), None, "x", "y") == (False, torch.device("cuda"))
    assert staging.placement(np.zeros(3), "cuda:1", "x", "y") == (False, torch.device("cuda", 1))
    with pytest.raises(ValueError, match="x: needs a cuda device, got 'cpu'; y is the host twin"):
        staging.placement(np.zeros(3), "cpu", "x", "y")


def test_one_device_without_a_tensor_on_a_device():
    host = torch.zeros(2)
    assert staging.one_device((host, host), "cuda", "evaluate_depth") == torch.device("cuda")
    assert staging.one_device((host, None, host), "cuda:1", "evaluate_tae") == torch.device("cuda", 1)
    assert staging.one_device((None, None), torch.device("cuda"), "w") == torch.device("cuda")
    assert staging.one_device((), "cuda", "w") == torch.device("cuda")
    with pytest.raises(ValueError) as e:
        staging.one_device((host, None), "cpu", "evaluate_depth")
    assert str(e.value) == "evaluate_depth: needs one cuda device, got 'cpu' / []"


def test_the_scorers_take_one_device_from_staging():
    from video_depth_anything_amd import evaluate, losses
    assert losses.one_device is staging.one_device and evaluate.one_device is staging.one_device
