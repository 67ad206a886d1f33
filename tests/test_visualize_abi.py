"""The visualisation entry point of the C ABI (csrc/visualize.hip, include/vda.h) refuses bad arguments before any launch, each by
the name of the argument, and the Python layer refuses what it cannot map: no GPU needed."""
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
    """Distinct 16-byte aligned host addresses and misaligned ones: never dereferenced, every call below is refused first."""
    buf = (ctypes.c_char * 512)()
    base = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    at = lambda off: ctypes.c_void_p(base + off)
    return buf, dict(depth=at(0), minmax=at(64), lut=at(128), out=at(192)), at


def refused(lib, rc, *words):
    msg = lib.vda_last_error()
    assert rc != 0 and all(w in msg for w in words), (rc, msg)


def declared(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vda.h")).read(), flags=re.S)
    decl = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert decl, f"include/vda.h does not declare {name}"
    return decl.group(1), [" ".join(p.split()) for p in decl.group(2).split(",")]


def test_symbol_is_exported_with_the_declared_signature(lib):
    from video_depth_anything_amd import _lib
    vp = ctypes.c_void_p
    assert hasattr(lib, "vda_depth_vis_u8")
    assert declared("vda_depth_vis_u8") == ("int", ["const float* depth", "long long n", "const float* minmax", "const uint8_t* lut",
                                                    "uint8_t* out", "vda_stream_t stream"])
    assert _lib.SIGNATURES["vda_depth_vis_u8"] == (ctypes.c_int, [vp, ctypes.c_longlong, vp, vp, vp, vp])


def test_the_abi_number_stays(lib):
    assert lib.vda_abi_version() == 8


def call(lib, ptrs, **over):
    a = dict(ptrs[1], n=5883)
    a.update(over)
    return lib.vda_depth_vis_u8(a["depth"], a["n"], a["minmax"], a["lut"], a["out"], None)


def test_depth_vis_refuses(lib, ptrs):
    at = ptrs[2]
    for name in ("depth", "minmax", "out"):
        refused(lib, call(lib, ptrs, **{name: None}), name.encode(), b"null")
        refused(lib, call(lib, ptrs, **{name: None, "lut": None}), name.encode(), b"null")     # gray refuses the same
    for n in (0, -1, -(1 << 40)):
        refused(lib, call(lib, ptrs, n=n), b"n=", b"bad size")
    for off in (1, 2, 3):
        refused(lib, call(lib, ptrs, depth=at(off)), b"depth", b"4-byte aligned")
        refused(lib, call(lib, ptrs, minmax=at(64 + off)), b"minmax", b"4-byte aligned")


def test_python_layer_refuses(lib):
    import torch
    from video_depth_anything_amd import ops
    from video_depth_anything_amd.visualize import colorize
    for bad in (np.zeros((1, 3, 5), np.float64), np.zeros((1, 3, 5), np.float16), np.zeros((1, 3, 5), np.uint8),
                torch.zeros(1, 3, 5, dtype=torch.float64), torch.zeros(1, 3, 5, dtype=torch.float16)):
        with pytest.raises(ValueError, match="float32"):
            colorize(bad)
    with pytest.raises(ValueError, match=r"\[N,H,W\]"):
        colorize(np.zeros(7, np.float32))
    with pytest.raises(ValueError, match="palette"):
        colorize(np.zeros((1, 3, 5), np.float32), palette=np.zeros((255, 3), np.uint8))
    # a host tensor or a host device is an error, not a silent CPU path: colorize_numpy is the host twin
    with pytest.raises(ValueError, match="cuda"):
        colorize(torch.zeros(1, 3, 5))
    with pytest.raises(ValueError, match="cuda"):
        colorize(np.zeros((1, 3, 5), np.float32), device="cpu")
    with pytest.raises(ValueError, match="cuda"):
        ops.depth_vis(torch.zeros(15), torch.zeros(2), None, torch.zeros(15, dtype=torch.uint8))
