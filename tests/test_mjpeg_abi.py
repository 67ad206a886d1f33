"""The Motion-JPEG entry points of the C ABI (csrc/mjpeg.hip, include/vda.h) refuse bad arguments before any launch, each by its own
message, and the Python layer refuses what it cannot encode: no GPU needed."""
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
def args(lib):
    """Well-formed arguments for 2 frames of 17 x 23 x 3 at 16-byte aligned HOST addresses that are never dereferenced (every call
    below is refused first), with real host tables."""
    buf = (ctypes.c_char * 1024)()
    base = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    at = lambda off: ctypes.c_void_p(base + off)
    qt = np.full(128, 7, np.uint16)
    a = dict(frames=at(0), n=2, h=17, w=23, channels=3, qtables=qt.ctypes.data_as(ctypes.c_void_p), workspace=at(64),
             workspace_bytes=lib.vda_mjpeg_workspace_bytes(2, 17, 23, 3), out=at(128), out_capacity=lib.vda_mjpeg_out_bytes(2, 17, 23, 3),
             lengths=at(192))
    return (buf, qt), a, at


def call(lib, args, **over):
    a = dict(args[1])
    a.update(over)
    return lib.vda_mjpeg_encode_u8(a["frames"], a["n"], a["h"], a["w"], a["channels"], a["qtables"], a["workspace"], a["workspace_bytes"],
                                   a["out"], a["out_capacity"], a["lengths"], None)


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
    for name in ("vda_mjpeg_workspace_bytes", "vda_mjpeg_out_bytes"):
        assert hasattr(lib, name)
        assert declared(name) == ("size_t", ["int n", "int h", "int w", "int channels"])
        assert _lib.SIGNATURES[name] == (sz, [i, i, i, i])
    assert hasattr(lib, "vda_mjpeg_encode_u8")
    assert declared("vda_mjpeg_encode_u8") == ("int", ["const uint8_t* frames", "int n", "int h", "int w", "int channels", "const uint16_t* qtables",
                                                       "void* workspace", "size_t workspace_bytes", "uint8_t* out", "size_t out_capacity",
                                                       "long long* lengths", "vda_stream_t stream"])
    assert _lib.SIGNATURES["vda_mjpeg_encode_u8"] == (i, [vp, i, i, i, i, vp, vp, sz, vp, sz, vp, vp])


def test_the_abi_number_stays(lib):
    assert lib.vda_abi_version() == 8


def test_the_bounds_are_the_documented_ones(lib):
    # bh = 3, nb = 3 * 3: 416 bytes a block after stuffing, 2 per interval for RSTm, 2 per frame for EOI
    assert lib.vda_mjpeg_out_bytes(2, 17, 23, 3) == 2 * (3 * (9 * 416 + 2) + 2)
    assert lib.vda_mjpeg_out_bytes(1, 8, 8, 1) == 416 + 2 + 2
    assert lib.vda_mjpeg_workspace_bytes(2, 17, 23, 3) == 2 * 3 * 9 * (128 + 208 + 416) + 32 + 16
    for bad in ((0, 8, 8, 3), (1, 0, 8, 3), (1, 8, 0, 3), (1, 8, 8, 2), (1, 65536, 8, 3), (1, 8, 65536, 1), (-1, 8, 8, 3)):
        assert lib.vda_mjpeg_out_bytes(*bad) == 0 and lib.vda_mjpeg_workspace_bytes(*bad) == 0


def test_encode_refuses(lib, args):
    at = args[2]
    for name in ("frames", "qtables", "workspace", "out", "lengths"):
        refused(lib, call(lib, args, **{name: None}), name.encode(), b"null")
    for name in ("n", "h", "w"):
        for v in (0, -3):
            refused(lib, call(lib, args, **{name: v}), b"bad size", name.encode() + b"=" + str(v).encode())
    refused(lib, call(lib, args, h=65536), b"bad size", b"65535")
    refused(lib, call(lib, args, w=70000), b"bad size", b"65535")
    for ch in (0, 2, 4, -1):
        refused(lib, call(lib, args, channels=ch), b"channels=" + str(ch).encode())
    for where, v in ((0, 0), (63, 256), (64, 0), (127, 1000)):
        qt = np.full(128, 7, np.uint16)
        qt[where] = v
        refused(lib, call(lib, args, qtables=qt.ctypes.data_as(ctypes.c_void_p)), b"qtables[" + str(where).encode() + b"]=" + str(v).encode())
    gray_ok = np.full(128, 7, np.uint16)
    gray_ok[64:] = 0                       # a gray frame has no chrominance table: entries 64.. are not read
    refused(lib, call(lib, args, channels=1, qtables=gray_ok.ctypes.data_as(ctypes.c_void_p), workspace_bytes=0), b"workspace capacity")
    refused(lib, call(lib, args, workspace=at(64 + 8)), b"workspace", b"16-byte aligned")
    refused(lib, call(lib, args, lengths=at(192 + 4)), b"lengths", b"8-byte aligned")
    a = args[1]
    refused(lib, call(lib, args, workspace_bytes=a["workspace_bytes"] - 1), b"workspace capacity", str(a["workspace_bytes"]).encode())
    refused(lib, call(lib, args, out_capacity=a["out_capacity"] - 1), b"out capacity", str(a["out_capacity"]).encode())
    refused(lib, call(lib, args, n=(1 << 31) - 1, h=16, w=8), b"bad size", b"workgroups")   # past 2^31 - 1 workgroups: refused before the capacities are looked at


def test_python_layer_refuses(lib):
    import torch
    from video_depth_anything_amd import mjpeg, ops
    for fn in (mjpeg.encode_jpeg, mjpeg.encode_jpeg_numpy):
        for bad in (np.zeros((1, 8, 8, 3), np.float32), np.zeros((1, 8, 8, 3), np.int8), np.zeros((1, 8, 8), np.uint16)):
            with pytest.raises(TypeError, match="uint8"):
                fn(bad)
        for bad in (np.zeros((8, 8), np.uint8), np.zeros((1, 8, 8, 4), np.uint8), np.zeros((1, 2, 8, 8, 3), np.uint8), np.zeros((0, 8, 8, 3), np.uint8)):
            with pytest.raises(ValueError, match=r"\[N,H,W,3\]"):
                fn(bad)
        for q in (0, 101, -5, 50.0, None):
            with pytest.raises(ValueError, match="quality"):
                fn(np.zeros((1, 8, 8, 3), np.uint8), quality=q)
    with pytest.raises(TypeError, match="uint8"):
        mjpeg.encode_jpeg(torch.zeros(1, 8, 8, 3))
    # a host tensor or a host device is an error, not a silent CPU path: encode_jpeg_numpy is the host twin
    with pytest.raises(ValueError, match="encode_jpeg_numpy"):
        mjpeg.encode_jpeg(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="encode_jpeg_numpy"):
        mjpeg.encode_jpeg(np.zeros((1, 8, 8, 3), np.uint8), device="cpu")
    with pytest.raises(ValueError, match="cuda"):
        z = torch.zeros(64, dtype=torch.uint8)
        ops.mjpeg_encode(torch.zeros(1, 8, 8, dtype=torch.uint8), np.ones((1, 64), np.uint16), z, z, torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="4 GiB|fps"):
        mjpeg.write_avi(os.devnull, [], 0, 8, 8)
