"""The 8-bit resize's C entry point (csrc/resize_u8.hip, include/vda.h) and its Python layer (ops.resize_linear_u8,
scale.resize_frames) refuse bad arguments before any launch: no GPU needed."""
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
    """(two distinct host addresses): never dereferenced, every call below is refused first."""
    buf = (ctypes.c_char * 256)()
    base = ctypes.addressof(buf)
    return buf, ctypes.c_void_p(base + 1), ctypes.c_void_p(base + 66)


def refused(lib, rc, word):
    msg = lib.vda_last_error()
    assert rc != 0 and word in msg, (rc, msg)


def test_symbol_is_exported_with_the_declared_signature(lib):
    from video_depth_anything_amd import _lib
    assert hasattr(lib, "vda_resize_linear_u8")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vda.h")).read(), flags=re.S)
    decl = re.search(r"int\s+vda_resize_linear_u8\s*\(([^)]*)\)\s*;", text)
    assert decl, "include/vda.h does not declare vda_resize_linear_u8"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["const uint8_t* in", "uint8_t* out", "int n", "int h", "int w", "int c", "int H", "int W", "vda_stream_t stream"]
    res, args = _lib.SIGNATURES["vda_resize_linear_u8"]
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 6 + [ctypes.c_void_p]


def test_the_abi_number_stays(lib):
    assert lib.vda_abi_version() == 8


def test_the_file_is_built_without_contraction():
    from video_depth_anything_amd import build
    assert "-ffp-contract=off" in build.PER_FILE["resize_u8.hip"]


def test_resize_refuses(lib, ptrs):
    _, p, q = ptrs
    f = lib.vda_resize_linear_u8
    refused(lib, f(None, q, 1, 2, 3, 3, 4, 5, None), b"null")
    refused(lib, f(p, None, 1, 2, 3, 3, 4, 5, None), b"null")
    for sizes in ((0, 2, 3, 3, 4, 5), (1, 0, 3, 3, 4, 5), (1, 2, 0, 3, 4, 5), (1, 2, 3, 3, 0, 5), (1, 2, 3, 3, 4, 0), (-1, 2, 3, 3, 4, 5)):
        refused(lib, f(p, q, *sizes, None), b"bad size")
    for c in (0, 2, 4, -3):
        refused(lib, f(p, q, 1, 2, 3, c, 4, 5, None), b"bad size")
    refused(lib, f(p, p, 1, 2, 3, 3, 4, 5, None), b"in == out")
    refused(lib, f(p, q, 1 << 20, 2, 3, 3, 1 << 12, 5, None), b"too large")             # n * H = 2^32 rows
    refused(lib, f(p, q, 1 << 20, 1 << 12, 3, 1, 2, 5, None), b"too large")             # n * h = 2^32 rows
    refused(lib, f(p, q, 1, 2, 3, 1, 4, (1 << 30) + 1, None), b"too large")             # an output row of 2^30 + 1 bytes
    refused(lib, f(p, q, 1, 2, (1 << 30) + 1, 1, 4, 5, None), b"too large")             # a source row of 2^30 + 1 bytes
    refused(lib, f(p, q, 1, 2, 3, 3, 4, (1 << 30) // 3 + 1, None), b"too large")        # 3 bytes a pixel: 2^30 + 2 bytes


def test_python_layer_refuses_host_tensors_and_other_types(lib):
    """No silent CPU path: ops.resize_linear_u8 and scale.resize_frames take device memory (or numpy frames to stage), uint8 only."""
    import torch
    from video_depth_anything_amd import ops
    from video_depth_anything_amd.scale import resize_frames
    with pytest.raises(ValueError, match="cuda"):
        ops.resize_linear_u8(torch.ones(2, 3, 4, 3, dtype=torch.uint8), torch.ones(2, 5, 6, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="cuda"):
        resize_frames(torch.ones(2, 3, 4, 3, dtype=torch.uint8), 5, 6)
    with pytest.raises(ValueError, match="cuda"):
        resize_frames(np.ones((2, 3, 4, 3), np.uint8), 5, 6, device="cpu")
    with pytest.raises(TypeError, match="uint8"):
        resize_frames(np.ones((2, 3, 4, 3), np.float32), 5, 6)
    with pytest.raises(TypeError, match="uint8"):
        resize_frames(torch.ones(2, 3, 4, 3), 5, 6)
    with pytest.raises(ValueError, match="N,h,w"):
        resize_frames(np.ones((2, 3, 4, 4), np.uint8), 5, 6)
    with pytest.raises(ValueError, match="positive"):
        resize_frames(np.ones((2, 3, 4, 3), np.uint8), 5, 0)
