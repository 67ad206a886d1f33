"""The resize's C entry point (csrc/resize.hip, include/vda.h) and the device scorers' `resize=` argument refuse bad arguments
before any launch: no GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from video_depth_anything_amd import build
    build.build()
    from video_depth_anything_amd import _lib
    return _lib.lib


@pytest.fixture(scope="module")
def ptrs():
    """(two distinct 16-byte aligned host addresses, the first + 2): never dereferenced, every call below is refused first."""
    buf = (ctypes.c_char * 256)()
    base = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    return buf, ctypes.c_void_p(base), ctypes.c_void_p(base + 64), ctypes.c_void_p(base + 2)


def refused(lib, rc, word):
    msg = lib.vda_last_error()
    assert rc != 0 and word in msg, (rc, msg)


def test_symbol_is_exported_with_the_declared_signature(lib):
    from video_depth_anything_amd import _lib
    assert hasattr(lib, "vda_resize_linear_f32")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vda.h")).read(), flags=re.S)
    decl = re.search(r"int\s+vda_resize_linear_f32\s*\(([^)]*)\)\s*;", text)
    assert decl, "include/vda.h does not declare vda_resize_linear_f32"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["const float* in", "float* out", "int n", "int h", "int w", "int H", "int W", "vda_stream_t stream"]
    res, args = _lib.SIGNATURES["vda_resize_linear_f32"]
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p]


def test_the_abi_number_stays(lib):
    assert lib.vda_abi_version() == 8


def test_resize_refuses(lib, ptrs):
    _, p, q, odd = ptrs
    f = lib.vda_resize_linear_f32
    refused(lib, f(None, q, 1, 2, 3, 4, 5, None), b"null")
    refused(lib, f(p, None, 1, 2, 3, 4, 5, None), b"null")
    for sizes in ((0, 2, 3, 4, 5), (1, 0, 3, 4, 5), (1, 2, 0, 4, 5), (1, 2, 3, 0, 5), (1, 2, 3, 4, 0), (-1, 2, 3, 4, 5)):
        refused(lib, f(p, q, *sizes, None), b"bad size")
    refused(lib, f(p, p, 1, 2, 3, 4, 5, None), b"in == out")
    refused(lib, f(odd, q, 1, 2, 3, 4, 5, None), b"misaligned")
    refused(lib, f(p, odd, 1, 2, 3, 4, 5, None), b"misaligned")
    refused(lib, f(p, q, 1 << 20, 2, 3, 1 << 12, 5, None), b"too large")                # n * H = 2^32 rows
    refused(lib, f(p, q, 1, 2, 3, 4, (1 << 30) + 1, None), b"too large")


def test_python_layer_refuses_host_tensors_and_bad_shapes(lib):
    """ops.resize_linear takes device tensors only: a host tensor is an error, not a silent copy or a CPU path."""
    import torch
    from video_depth_anything_amd import ops
    with pytest.raises(ValueError, match="cuda"):
        ops.resize_linear(torch.ones(2, 3, 4), torch.ones(2, 5, 6))


def test_device_scorers_refuse_before_any_device_work(lib):
    """`resize=False` keeps the refusal and its wording; another N raises with `resize=True` too; so does a non-cuda device."""
    from video_depth_anything_amd.evaluate import evaluate_depth, evaluate_tae, resize_prediction
    pred, gt = np.ones((3, 4, 6), np.float32), np.ones((3, 5, 7), np.float32)
    K, poses = np.eye(3), np.stack([np.eye(4)] * 3)
    with pytest.raises(ValueError, match="resize"):
        evaluate_depth(pred, gt, 10.0)
    with pytest.raises(ValueError, match="resize"):
        evaluate_depth(pred, gt, 10.0, resize=False)
    with pytest.raises(ValueError, match="number of frames"):
        evaluate_depth(pred[:2], gt, 10.0, resize=True)
    with pytest.raises(ValueError, match="resize"):
        evaluate_tae(pred, gt, K, poses, 10.0)
    with pytest.raises(ValueError, match="resize"):
        evaluate_tae(pred, gt, K, poses, 10.0, resize=False)
    with pytest.raises(ValueError, match="number of frames"):
        evaluate_tae(pred[:2], gt, K, poses, 10.0, resize=True)
    with pytest.raises(ValueError, match="float32"):
        resize_prediction(pred.astype(np.float64), (5, 7))
    with pytest.raises(ValueError, match="cuda"):
        resize_prediction(pred, (5, 7), device="cpu")
