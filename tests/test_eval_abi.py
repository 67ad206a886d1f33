"""The scorer's C entry points (csrc/eval.hip, include/vda.h) refuse bad arguments before any launch: no GPU needed."""
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
    """(an 8-byte aligned host address, the same + 4): never dereferenced, every call below is refused first."""
    buf = (ctypes.c_char * 256)()
    base = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    return buf, ctypes.c_void_p(base), ctypes.c_void_p(base + 4)


def refused(lib, rc, word):
    msg = lib.vda_last_error()
    assert rc != 0 and word in msg, (rc, msg)


def test_lsq_partial_refuses(lib, ptrs):
    _, p, odd = ptrs
    f = lib.vda_eval_lsq_partial
    refused(lib, f(None, p, 0, 100, 10.0, p, 0, 1, None), b"null")
    refused(lib, f(p, None, 0, 100, 10.0, p, 0, 1, None), b"null")
    refused(lib, f(p, p, 0, 100, 10.0, None, 0, 1, None), b"null")
    refused(lib, f(p, p, 0, 0, 10.0, p, 0, 1, None), b"n=0")
    refused(lib, f(p, p, 0, 100, 10.0, p, 0, 4097, None), b"block count")
    refused(lib, f(p, p, 0, 100, 10.0, p, 0, 0, None), b"block count")
    refused(lib, f(p, p, 0, 100, 10.0, p, -1, 1, None), b"row offset")
    refused(lib, f(p, p, 2, 100, 10.0, p, 0, 1, None), b"gt_is_f64")
    refused(lib, f(p, p, 0, 100, 10.0, odd, 0, 1, None), b"misaligned")
    refused(lib, f(p, odd, 1, 100, 10.0, p, 0, 1, None), b"misaligned")          # fp64 gt at a 4-byte address


def test_lsq_finish_refuses(lib, ptrs):
    _, p, odd = ptrs
    f = lib.vda_eval_lsq_finish
    refused(lib, f(None, 1, p, None), b"null")
    refused(lib, f(p, 1, None, None), b"null")
    refused(lib, f(p, 0, p, None), b"n=0")
    refused(lib, f(odd, 1, p, None), b"misaligned")
    refused(lib, f(p, 1, odd, None), b"misaligned")


def test_metric_partial_refuses(lib, ptrs):
    _, p, odd = ptrs
    f = lib.vda_eval_metric_partial
    refused(lib, f(None, p, 0, 1, 100, 10.0, p, p, 0, 1, None), b"null")
    refused(lib, f(p, None, 0, 1, 100, 10.0, p, p, 0, 1, None), b"null")
    refused(lib, f(p, p, 0, 1, 100, 10.0, None, p, 0, 1, None), b"null")
    refused(lib, f(p, p, 0, 1, 100, 10.0, p, None, 0, 1, None), b"null")
    refused(lib, f(p, p, 0, 0, 100, 10.0, p, p, 0, 1, None), b"n=0")
    refused(lib, f(p, p, 0, 1, 0, 10.0, p, p, 0, 1, None), b"bad size")
    refused(lib, f(p, p, 0, 1, 100, 10.0, p, p, 0, 4097, None), b"block count")
    refused(lib, f(p, p, 0, 1, 100, 10.0, p, p, -1, 1, None), b"frame offset")
    refused(lib, f(p, p, 0, 60000, 100, 10.0, p, p, 60000, 4096, None), b"too many partial rows")
    refused(lib, f(p, p, 0, 1, 100, 10.0, p, odd, 0, 1, None), b"misaligned")
    refused(lib, f(p, p, 0, 1, 100, 10.0, odd, p, 0, 1, None), b"misaligned")


def test_metric_finish_refuses(lib, ptrs):
    _, p, odd = ptrs
    f = lib.vda_eval_metric_finish
    refused(lib, f(None, 1, 1, p, None), b"null")
    refused(lib, f(p, 1, 1, None, None), b"null")
    refused(lib, f(p, 0, 1, p, None), b"n=0")
    refused(lib, f(p, 1, 4097, p, None), b"bad sizes")
    refused(lib, f(odd, 1, 1, p, None), b"misaligned")
    refused(lib, f(p, 1, 1, odd, None), b"misaligned")


def test_python_layer_refuses_host_tensors(lib):
    """ops.eval_* take device tensors only: a host tensor is an error, not a silent copy or a CPU path."""
    import torch
    from video_depth_anything_amd import ops
    x = torch.ones(2, 3, 4)
    with pytest.raises(ValueError, match="cuda"):
        ops.eval_lsq_partial(x, x, 10.0, torch.zeros(5, dtype=torch.float64), 0, 1)
