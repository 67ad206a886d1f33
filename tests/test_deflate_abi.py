"""The deflate entry points of the C ABI (csrc/deflate.hip, include/vda.h): exported with the declared signatures, the size functions
are the documented formulas, bad arguments are refused before any launch, each by its own message: no GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 16384


@pytest.fixture(scope="module")
def lib():
    from video_depth_anything_amd import build
    build.build()
    from video_depth_anything_amd import _lib
    return _lib.lib


@pytest.fixture(scope="module")
def args(lib):
    """Well-formed arguments for 40 000 bytes at 16-byte aligned HOST addresses that are never dereferenced (every call below is
    refused first)."""
    buf = (ctypes.c_char * 1024)()
    base = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    at = lambda off: ctypes.c_void_p(base + off)
    n = 40000
    a = dict(data=at(0), n=n, final=1, workspace=at(64), workspace_bytes=lib.vda_deflate_workspace_bytes(n), out=at(128),
             out_capacity=lib.vda_deflate_out_bytes(n), length=at(192), crcs=at(256))
    return buf, a, at


def call(lib, args, **over):
    a = dict(args[1])
    a.update(over)
    return lib.vda_deflate_u8(a["data"], a["n"], a["final"], a["workspace"], a["workspace_bytes"], a["out"], a["out_capacity"], a["length"], a["crcs"], None)


def refused(lib, rc, *words):
    msg = lib.vda_last_error()
    assert rc != 0 and all(w in msg for w in words), (rc, msg)


def declared(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vda.h")).read(), flags=re.S)
    decl = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert decl, f"include/vda.h does not declare {name}"
    return decl.group(1), [" ".join(p.split()) for p in decl.group(2).split(",")]


def test_symbols_are_exported_with_the_declared_signatures(lib):
    from video_depth_anything_amd import _lib
    vp, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    for name in ("vda_deflate_workspace_bytes", "vda_deflate_out_bytes"):
        assert hasattr(lib, name)
        assert declared(name) == ("size_t", ["size_t n"])
        assert _lib.SIGNATURES[name] == (sz, [sz])
    assert hasattr(lib, "vda_deflate_u8")
    assert declared("vda_deflate_u8") == ("int", ["const uint8_t* in", "size_t n", "int final", "void* workspace", "size_t workspace_bytes", "uint8_t* out",
                                                  "size_t out_capacity", "long long* length", "uint32_t* crcs", "vda_stream_t stream"])
    assert _lib.SIGNATURES["vda_deflate_u8"] == (i, [vp, sz, i, vp, sz, vp, sz, vp, vp, vp])


def test_the_abi_number_stays(lib):
    assert lib.vda_abi_version() == 8


def test_the_bounds_are_the_documented_ones(lib):
    from video_depth_anything_amd import deflate
    up16 = lambda v: (v + 15) // 16 * 16
    for n in (0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 40000, 8 * 518 * 518 * 4, (1 << 32) + 5, 1 << 44):
        chunks = max(1, -(-n // CHUNK))
        assert lib.vda_deflate_out_bytes(n) == n + 5 * chunks == deflate.out_bytes(n)
        assert lib.vda_deflate_workspace_bytes(n) == chunks * 16400 + up16(4 * chunks) + up16(8 * chunks)
    assert lib.vda_deflate_out_bytes((1 << 44) + 1) == 0 and lib.vda_deflate_workspace_bytes((1 << 44) + 1) == 0


def test_encode_refuses(lib, args):
    at = args[2]
    for name, word in (("data", b"in"), ("workspace", b"workspace"), ("out", b"out"), ("length", b"length"), ("crcs", b"crcs")):
        refused(lib, call(lib, args, **{name: None}), word, b"null")
    refused(lib, call(lib, args, n=(1 << 44) + 1), b"bad size", str((1 << 44) + 1).encode())
    for v in (2, -1):
        refused(lib, call(lib, args, final=v), b"final=" + str(v).encode())
    refused(lib, call(lib, args, workspace=at(64 + 8)), b"workspace", b"16-byte aligned")
    refused(lib, call(lib, args, length=at(192 + 4)), b"length", b"8-byte aligned")
    refused(lib, call(lib, args, crcs=at(256 + 2)), b"crcs", b"4-byte aligned")
    a = args[1]
    refused(lib, call(lib, args, workspace_bytes=a["workspace_bytes"] - 1), b"workspace capacity", str(a["workspace_bytes"]).encode())
    refused(lib, call(lib, args, out_capacity=a["out_capacity"] - 1), b"out capacity", str(a["out_capacity"]).encode())
    # an empty input needs no input pointer, but everything else
    refused(lib, call(lib, args, data=None, n=0, out=None), b"out", b"null")


def test_python_layer_refuses(lib):
    import torch
    from video_depth_anything_amd import deflate, ops
    with pytest.raises(ValueError, match="deflate_numpy"):
        deflate.deflate(torch.zeros(8, dtype=torch.uint8))                    # a host tensor is an error, not a silent CPU path
    with pytest.raises(ValueError, match="deflate_numpy"):
        deflate.deflate(np.zeros(8, np.uint8), device="cpu")
    with pytest.raises(ValueError, match="multiple of 16384"):
        deflate.deflate(np.zeros(8, np.uint8), block_bytes=1000)
    with pytest.raises(ValueError, match="cuda"):
        z = torch.zeros(64, dtype=torch.uint8)
        ops.deflate(z, True, z, z, torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32))
