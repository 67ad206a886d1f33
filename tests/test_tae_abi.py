"""The TAE scorer's C entry points (csrc/tae.hip, include/vda.h) refuse bad arguments before any launch: no GPU needed."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from video_depth_anything_amd import build
    build.build()
    from video_depth_anything_amd import _lib
    return _lib.lib


@pytest.fixture(scope="module")
def ptrs():
    """(an 8-byte aligned host address, the same + 4, the same + 2): never dereferenced, every call below is refused first."""
    buf = (ctypes.c_char * 256)()
    base = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    return buf, ctypes.c_void_p(base), ctypes.c_void_p(base + 4), ctypes.c_void_p(base + 2)


def refused(lib, rc, word):
    msg = lib.vda_last_error()
    assert rc != 0 and word in msg, (rc, msg)


def test_splat_refuses(lib, ptrs):
    _, p, odd, odd2 = ptrs
    f = lib.vda_tae_splat
    for hole in range(4):                                               # pred, fit, cam, winner
        a = [p, p, p, p]
        a[hole] = None
        refused(lib, f(a[0], 1, 4, 5, 10.0, a[1], a[2], a[3], None), b"null")
    refused(lib, f(p, 0, 4, 5, 10.0, p, p, p, None), b"n=0")
    refused(lib, f(p, 32768, 4, 5, 10.0, p, p, p, None), b"bad size")
    refused(lib, f(p, 1, 0, 5, 10.0, p, p, p, None), b"bad size")
    refused(lib, f(p, 1, 4, -1, 10.0, p, p, p, None), b"bad size")
    refused(lib, f(p, 1, 65536, 32768, 10.0, p, p, p, None), b"too large")         # H * W = 2^31
    refused(lib, f(p, 1, 2147483647, 1, 10.0, p, p, p, None), b"too large")        # H * W = 2^31 - 1: index + 1 needs bit 31
    refused(lib, f(p, 1, 4, 5, 10.0, odd, p, p, None), b"misaligned")
    refused(lib, f(p, 1, 4, 5, 10.0, p, odd, p, None), b"misaligned")
    refused(lib, f(odd2, 1, 4, 5, 10.0, p, p, p, None), b"misaligned")
    refused(lib, f(p, 1, 4, 5, 10.0, p, p, odd2, None), b"misaligned")


def test_compare_refuses(lib, ptrs):
    _, p, odd, odd2 = ptrs
    f = lib.vda_tae_compare
    for hole in range(5):                                               # pred, fit, cam, winner, partial (mask may be null)
        a = [p, p, p, p, p]
        a[hole] = None
        refused(lib, f(a[0], None, 1, 4, 5, 10.0, a[1], a[2], a[3], a[4], 0, 1, None), b"null")
    refused(lib, f(p, p, 0, 4, 5, 10.0, p, p, p, p, 0, 1, None), b"n=0")
    refused(lib, f(p, p, 1, 65536, 32768, 10.0, p, p, p, p, 0, 1, None), b"too large")
    refused(lib, f(p, p, 1, 4, 5, 10.0, p, p, p, p, 0, 0, None), b"block count")
    refused(lib, f(p, p, 1, 4, 5, 10.0, p, p, p, p, 0, 4097, None), b"block count")
    refused(lib, f(p, p, 1, 4, 5, 10.0, p, p, p, p, -1, 1, None), b"pair offset")
    refused(lib, f(p, p, 1000, 4, 5, 10.0, p, p, p, p, 0, 4096, None), b"too many partial rows")
    refused(lib, f(p, p, 1, 4, 5, 10.0, p, p, p, odd, 0, 1, None), b"misaligned")
    refused(lib, f(p, p, 1, 4, 5, 10.0, odd, p, p, p, 0, 1, None), b"misaligned")
    refused(lib, f(p, p, 1, 4, 5, 10.0, p, p, odd2, p, 0, 1, None), b"misaligned")


def test_finish_refuses(lib, ptrs):
    _, p, odd, _ = ptrs
    f = lib.vda_tae_finish
    refused(lib, f(None, 1, 1, p, None), b"null")
    refused(lib, f(p, 1, 1, None, None), b"null")
    refused(lib, f(p, 0, 1, p, None), b"n=0")
    refused(lib, f(p, 1, 0, p, None), b"bad sizes")
    refused(lib, f(p, 1, 4097, p, None), b"bad sizes")
    refused(lib, f(p, 1000, 4096, p, None), b"bad sizes")
    refused(lib, f(odd, 1, 1, p, None), b"misaligned")
    refused(lib, f(p, 1, 1, odd, None), b"misaligned")


def test_abi_version_is_unchanged(lib):
    assert lib.vda_abi_version() == 8                                    # the vda_tae_* entry points are additive


def test_python_layer_refuses_host_tensors(lib):
    """ops.tae_* take device tensors only: a host tensor is an error, not a silent copy or a CPU path."""
    import torch
    from video_depth_anything_amd import ops
    pred, f64 = torch.ones(2, 3, 4), torch.zeros(64, dtype=torch.float64)
    win = torch.zeros(2, 3, 4, dtype=torch.int32)
    with pytest.raises(ValueError, match="cuda"):
        ops.tae_splat(pred, 10.0, f64, f64, win)
    with pytest.raises(ValueError, match="cuda"):
        ops.tae_compare(pred, None, 10.0, f64, f64, win, f64, 0, 1)
    with pytest.raises(ValueError, match="cuda"):
        ops.tae_finish(f64, 1, 1, f64)
