"""The loss entry points (csrc/losses.hip, include/vda.h) refuse bad arguments before any launch, and the Python layer refuses what
it must before it touches a device: no GPU needed."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from video_depth_anything_amd import build
    build.build()
    from video_depth_anything_amd import _lib
    return _lib.lib


@pytest.fixture(scope="module")
def ptrs():
    """(an 8-byte aligned host address, the same + 4, the same + 1): never dereferenced, every call below is refused first."""
    buf = (ctypes.c_char * 256)()
    base = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    return buf, ctypes.c_void_p(base), ctypes.c_void_p(base + 4), ctypes.c_void_p(base + 1)


def refused(lib, rc, word):
    msg = lib.vda_last_error()
    assert rc != 0 and word in msg, (rc, msg)


def test_abi_version_is_unchanged(lib):
    assert lib.vda_abi_version() == 8


def test_lsq_partial_refuses(lib, ptrs):
    _, p, odd, byte = ptrs
    f = lib.vda_loss_lsq_partial
    refused(lib, f(None, p, p, 1, 100, 0, p, p, 1, None), b"null")
    refused(lib, f(p, None, p, 1, 100, 0, p, p, 1, None), b"null")
    refused(lib, f(p, p, None, 1, 100, 0, None, p, 1, None), b"null")
    refused(lib, f(p, p, None, 1, 100, 0, p, None, 1, None), b"null")
    refused(lib, f(p, p, p, 0, 100, 0, p, p, 1, None), b"n=0")
    refused(lib, f(p, p, p, 65536, 100, 0, p, p, 1, None), b"bad size")
    refused(lib, f(p, p, p, 1, 0, 0, p, p, 1, None), b"bad size")
    refused(lib, f(p, p, p, 1, 100, 0, p, p, 0, None), b"block count")
    refused(lib, f(p, p, p, 1, 100, 0, p, p, 4097, None), b"block count")
    refused(lib, f(p, p, p, 60000, 100, 0, p, p, 4096, None), b"too many partial rows")
    refused(lib, f(p, p, p, 1, 100, 3, p, p, 1, None), b"pass")
    refused(lib, f(p, p, p, 1, 100, -1, p, p, 1, None), b"pass")
    refused(lib, f(byte, p, p, 1, 100, 0, p, p, 1, None), b"misaligned")
    refused(lib, f(p, byte, p, 1, 100, 0, p, p, 1, None), b"misaligned")
    refused(lib, f(p, p, p, 1, 100, 0, odd, p, 1, None), b"misaligned")
    refused(lib, f(p, p, p, 1, 100, 0, p, odd, 1, None), b"misaligned")


def test_lsq_finish_refuses(lib, ptrs):
    _, p, odd, _ = ptrs
    f = lib.vda_loss_lsq_finish
    refused(lib, f(None, 1, 1, 0, 1e-8, p, p, None), b"null")
    refused(lib, f(p, 1, 1, 0, 1e-8, None, p, None), b"null")
    refused(lib, f(p, 1, 1, 2, 1e-8, p, None, None), b"null")                    # the result is needed in pass 2 only
    refused(lib, f(p, 0, 1, 0, 1e-8, p, p, None), b"n=0")
    refused(lib, f(p, 1, 0, 0, 1e-8, p, p, None), b"block count")
    refused(lib, f(p, 1, 4097, 0, 1e-8, p, p, None), b"block count")
    refused(lib, f(p, 1, 1, 3, 1e-8, p, p, None), b"pass")
    refused(lib, f(odd, 1, 1, 0, 1e-8, p, p, None), b"misaligned")
    refused(lib, f(p, 1, 1, 0, 1e-8, odd, p, None), b"misaligned")
    refused(lib, f(p, 1, 1, 2, 1e-8, p, odd, None), b"misaligned")


def test_median_refuses(lib, ptrs):
    _, p, _, byte = ptrs
    f = lib.vda_loss_median
    refused(lib, f(None, p, p, 1, 100, p, None), b"null")
    refused(lib, f(p, p, p, 1, 100, None, None), b"null")
    refused(lib, f(p, p, p, 0, 100, p, None), b"n=0")
    refused(lib, f(p, p, p, 1, 0, p, None), b"bad size")
    refused(lib, f(p, p, p, 65536, 100, p, None), b"bad size")
    refused(lib, f(p, p, p, 1, 1 << 31, p, None), b"too large")
    refused(lib, f(byte, p, p, 1, 100, p, None), b"misaligned")
    refused(lib, f(p, byte, p, 1, 100, p, None), b"misaligned")
    refused(lib, f(p, p, p, 1, 100, byte, None), b"misaligned")


def test_mad_refuses(lib, ptrs):
    _, p, odd, byte = ptrs
    f = lib.vda_loss_mad_scale_partial
    refused(lib, f(None, p, p, 1, 100, p, p, 1, None), b"null")
    refused(lib, f(p, None, p, 1, 100, p, p, 1, None), b"null")
    refused(lib, f(p, p, p, 1, 100, None, p, 1, None), b"null")
    refused(lib, f(p, p, p, 1, 100, p, None, 1, None), b"null")
    refused(lib, f(p, p, p, 0, 100, p, p, 1, None), b"n=0")
    refused(lib, f(p, p, p, 1, 0, p, p, 1, None), b"bad size")
    refused(lib, f(p, p, p, 1, 100, p, p, 4097, None), b"block count")
    refused(lib, f(p, p, p, 1, 100, byte, p, 1, None), b"misaligned")
    refused(lib, f(p, p, p, 1, 100, p, odd, 1, None), b"misaligned")
    f = lib.vda_loss_mad_scale_finish
    refused(lib, f(None, 1, 1, 1e-8, p, p, None), b"null")
    refused(lib, f(p, 1, 1, 1e-8, None, p, None), b"null")
    refused(lib, f(p, 1, 1, 1e-8, p, None, None), b"null")
    refused(lib, f(p, 0, 1, 1e-8, p, p, None), b"n=0")
    refused(lib, f(p, 1, 0, 1e-8, p, p, None), b"block count")
    refused(lib, f(odd, 1, 1, 1e-8, p, p, None), b"misaligned")
    refused(lib, f(p, 1, 1, 1e-8, p, odd, None), b"misaligned")
    f = lib.vda_loss_mad_rows
    refused(lib, f(None, p, p, 1, 4, 5, p, p, None), b"null")
    refused(lib, f(p, None, p, 1, 4, 5, p, p, None), b"null")
    refused(lib, f(p, p, p, 1, 4, 5, None, p, None), b"null")
    refused(lib, f(p, p, p, 1, 4, 5, p, None, None), b"null")
    refused(lib, f(p, p, p, 0, 4, 5, p, p, None), b"n=0")
    refused(lib, f(p, p, p, 1, 0, 5, p, p, None), b"bad size")
    refused(lib, f(p, p, p, 1, 4, 0, p, p, None), b"bad size")
    refused(lib, f(p, p, p, 5000, 1000, 5, p, p, None), b"too many image rows")
    refused(lib, f(byte, p, p, 1, 4, 5, p, p, None), b"misaligned")
    refused(lib, f(p, p, p, 1, 4, 5, odd, p, None), b"misaligned")
    refused(lib, f(p, p, p, 1, 4, 5, p, odd, None), b"misaligned")
    f = lib.vda_loss_mad_finish
    refused(lib, f(None, 1, 4, p, None), b"null")
    refused(lib, f(p, 1, 4, None, None), b"null")
    refused(lib, f(p, 0, 4, p, None), b"n=0")
    refused(lib, f(p, 1, 0, p, None), b"bad size")
    refused(lib, f(p, 5000, 1000, p, None), b"too many image rows")
    refused(lib, f(odd, 1, 4, p, None), b"misaligned")
    refused(lib, f(p, 1, 4, odd, None), b"misaligned")


def test_tgm_refuses(lib, ptrs):
    _, p, odd, byte = ptrs
    f = lib.vda_loss_tgm_partial
    refused(lib, f(None, p, p, 1, 2, 100, p, 1, None), b"null")
    refused(lib, f(p, None, p, 1, 2, 100, p, 1, None), b"null")
    refused(lib, f(p, p, p, 1, 2, 100, None, 1, None), b"null")
    refused(lib, f(p, p, p, 0, 2, 100, p, 1, None), b"n=0")
    refused(lib, f(p, p, p, 1, 1, 100, p, 1, None), b"N >= 2")                   # a single frame has no pair: the caller returns NaN
    refused(lib, f(p, p, p, 70000, 2, 100, p, 1, None), b"bad size")
    refused(lib, f(p, p, p, 1, 2, 0, p, 1, None), b"bad size")
    refused(lib, f(p, p, p, 1, 2, 100, p, 0, None), b"block count")
    refused(lib, f(p, p, p, 1, 2, 100, p, 4097, None), b"block count")
    refused(lib, f(byte, p, p, 1, 2, 100, p, 1, None), b"misaligned")
    refused(lib, f(p, p, p, 1, 2, 100, odd, 1, None), b"misaligned")
    f = lib.vda_loss_tgm_finish
    refused(lib, f(None, 1, 2, 1, p, None), b"null")
    refused(lib, f(p, 1, 2, 1, None, None), b"null")
    refused(lib, f(p, 0, 2, 1, p, None), b"n=0")
    refused(lib, f(p, 1, 1, 1, p, None), b"N >= 2")
    refused(lib, f(p, 1, 2, 0, p, None), b"block count")
    refused(lib, f(odd, 1, 2, 1, p, None), b"misaligned")
    refused(lib, f(p, 1, 2, 1, odd, None), b"misaligned")


def test_python_layer_refuses_before_touching_a_device(lib):
    from video_depth_anything_amd import losses
    f32, f64 = np.zeros((1, 2, 3, 4), np.float32), np.zeros((1, 2, 3, 4), np.float64)
    for fn in (losses.ssi_loss, losses.tgm_loss, losses.validation_loss):
        with pytest.raises(ValueError, match="float32"):
            fn(f64, f32)
        with pytest.raises(ValueError, match="float32"):
            fn(f32, f32.astype(np.float16))
        with pytest.raises(ValueError, match="shape"):
            fn(f32, f32[:, :1])
        with pytest.raises(ValueError, match="shape"):
            fn(f32[0], f32[0])
        with pytest.raises(ValueError, match="mask"):
            fn(f32, f32, np.zeros((1, 2, 1, 3, 4), bool))
        with pytest.raises(ValueError, match="mask"):
            fn(f32, f32, np.zeros((1, 2, 3, 4), np.float32))
    with pytest.raises(ValueError, match="variant"):
        losses.ssi_loss(f32, f32, variant="mse")
    with pytest.raises(ValueError, match="cuda"):
        losses.ssi_loss(f32, f32, device="cpu")
    with pytest.raises(ValueError, match="float32"):
        losses._masked_median(f64)


def test_ops_layer_refuses_host_tensors(lib):
    """ops.loss_* take device tensors only: a host tensor is an error, not a silent copy or a CPU path."""
    import torch
    from video_depth_anything_amd import ops
    x = torch.ones(1, 2, 3, 4)
    with pytest.raises(ValueError, match="cuda"):
        ops.loss_tgm(x, x, None, torch.zeros(8, dtype=torch.float64), 1, torch.zeros(8, dtype=torch.float64))
    with pytest.raises(ValueError, match="cuda"):
        ops.loss_median(x, None, None, torch.zeros(2))


def test_loss_modules_are_inference_only(lib):
    import torch
    from utils import loss as loss_da
    from utils import loss_MiDas
    assert loss_da.Loss_tgm is loss_MiDas.Loss_tgm
    x = torch.zeros(1, 2, 1, 3, 4, requires_grad=True)
    y = torch.zeros(1, 2, 1, 3, 4)
    m = torch.ones(1, 2, 3, 4)
    for mod in (loss_MiDas.Loss_ssi(), loss_da.Loss_ssi(eps=1e-6), loss_MiDas.Loss_tgm()):
        with pytest.raises(RuntimeError, match="inference-only"):
            mod(x, y, m)
    assert loss_da.Loss_ssi(eps=1e-6).eps == 1e-6 and loss_MiDas.Loss_ssi().eps == 1e-8
