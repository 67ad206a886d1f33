"""The Motion-JPEG decoder's entry points of the C ABI (csrc/mjpeg_decode.hip, include/vda.h) refuse bad arguments before any
launch, each by its own message, and the Python layer refuses what it cannot decode: no GPU needed. The device addresses below
are host addresses that are never dereferenced (every call is refused first); the host tables are real."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDER = ("scan", "scan_bytes", "intervals", "n_intervals", "tables", "qtables", "n", "h", "w", "components", "hs", "vs", "workspace",
         "workspace_bytes", "out", "out_capacity", "status")


@pytest.fixture(scope="module")
def lib():
    from video_depth_anything_amd import build
    build.build()
    from video_depth_anything_amd import _lib
    return _lib.lib


@pytest.fixture(scope="module")
def args(lib):
    """Well-formed arguments for 2 frames of 17 x 23 x 3 in 4:2:0 (2 x 2 MCUs), an interval per frame."""
    from video_depth_anything_amd import mjpeg
    buf = (ctypes.c_char * 1024)()
    base = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    at = lambda off: ctypes.c_void_p(base + off)
    qt = np.full(192, 7, np.uint16)
    iv = np.array([[0, 0, 100, 0, 4], [1, 100, 60, 0, 4]], np.int32)
    tables = np.zeros((), mjpeg.TABLES_DTYPE)
    a = dict(scan=at(0), scan_bytes=160, intervals=iv.ctypes.data_as(ctypes.c_void_p), n_intervals=2, tables=tables.ctypes.data_as(ctypes.c_void_p),
             qtables=qt.ctypes.data_as(ctypes.c_void_p), n=2, h=17, w=23, components=3, hs=2, vs=2, workspace=at(64),
             workspace_bytes=lib.vda_mjpeg_decode_workspace_bytes(2, 17, 23, 3, 2, 2, 2), out=at(128), out_capacity=2 * 17 * 23 * 3, status=at(192))
    return (buf, qt, iv, tables), a, at


def call(lib, args, **over):
    a = dict(args[1])
    a.update(over)
    return lib.vda_mjpeg_decode_u8(*[a[k] for k in ORDER], None)


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
    assert hasattr(lib, "vda_mjpeg_decode_workspace_bytes") and hasattr(lib, "vda_mjpeg_decode_u8")
    assert declared("vda_mjpeg_decode_workspace_bytes") == ("size_t", ["int n", "int h", "int w", "int components", "int hs", "int vs", "int intervals"])
    assert _lib.SIGNATURES["vda_mjpeg_decode_workspace_bytes"] == (sz, [i] * 7)
    assert declared("vda_mjpeg_decode_u8") == ("int", ["const uint8_t* scan", "size_t scan_bytes", "const int* intervals", "int n_intervals",
                                                       "const void* tables", "const uint16_t* qtables", "int n", "int h", "int w", "int components",
                                                       "int hs", "int vs", "void* workspace", "size_t workspace_bytes", "uint8_t* out",
                                                       "size_t out_capacity", "int* status", "vda_stream_t stream"])
    assert _lib.SIGNATURES["vda_mjpeg_decode_u8"] == (i, [vp, sz, vp, i, vp, vp, i, i, i, i, i, i, vp, sz, vp, sz, vp, vp])


def test_the_abi_number_stays(lib):
    assert lib.vda_abi_version() == 8


def test_the_tables_record_is_the_headers_struct():
    """mjpeg.TABLES_DTYPE is MjdTables of csrc/mjpeg_decode_core.h, field by field."""
    from video_depth_anything_amd import mjpeg
    text = open(os.path.join(REPO, "video_depth_anything_amd", "csrc", "mjpeg_decode_core.h")).read()
    assert re.search(r"struct MjdHuff \{\s*uint16_t look\[256\];\s*int32_t maxcode\[18\];\s*int32_t valoff\[18\];\s*uint8_t vals\[256\];\s*\};", text)
    assert re.search(r"struct MjdTables \{\s*MjdHuff dc\[3\], ac\[3\];\s*uint8_t zigzag\[64\];\s*\};", text)
    assert mjpeg.HUFF_DTYPE.itemsize == 912 and [mjpeg.HUFF_DTYPE.fields[k][1] for k in ("look", "maxcode", "valoff", "vals")] == [0, 512, 584, 656]
    assert mjpeg.TABLES_DTYPE.itemsize == 6 * 912 + 64 and mjpeg.TABLES_DTYPE.fields["ac"][1] == 3 * 912 and mjpeg.TABLES_DTYPE.fields["zigzag"][1] == 6 * 912
    for code, name in ((1, "BAD_CODE"), (2, "BAD_SIZE"), (3, "RUN_PAST_63"), (4, "INTERVAL_SHORT"), (5, "INTERVAL_COUNT"), (6, "DC_RANGE"), (7, "NO_EOI")):
        assert re.search(rf"MJD_{name} = {code},", text) and code in mjpeg.DECODE_STATUS


def test_the_workspace_bound_is_the_documented_one(lib):
    up16 = lambda v: (v + 15) & ~15
    # 4:2:0, 17 x 23: 2 x 2 MCUs of 4 + 1 + 1 blocks; 192 bytes a block behind the interval table and the tables
    assert lib.vda_mjpeg_decode_workspace_bytes(2, 17, 23, 3, 2, 2, 5) == up16(5 * 20) + up16(6 * 912 + 64) + 2 * 24 * 192
    assert lib.vda_mjpeg_decode_workspace_bytes(1, 8, 8, 1, 1, 1, 1) == 32 + 5536 + 192
    assert lib.vda_mjpeg_decode_workspace_bytes(1, 8, 8, 3, 2, 1, 1) == 32 + 5536 + 4 * 192          # 4:2:2: the MCU is 16 x 8
    for bad in ((0, 8, 8, 3, 1, 1, 1), (1, 0, 8, 3, 1, 1, 1), (1, 8, 0, 3, 1, 1, 1), (1, 8, 8, 2, 1, 1, 1), (1, 65536, 8, 3, 1, 1, 1), (1, 8, 8, 3, 1, 2, 1),
                (1, 8, 8, 1, 2, 2, 1), (1, 8, 8, 3, 4, 1, 1), (1, 8, 8, 3, 1, 1, -1)):
        assert lib.vda_mjpeg_decode_workspace_bytes(*bad) == 0


def test_decode_refuses(lib, args):
    at = args[2]
    for name in ("scan", "intervals", "tables", "qtables", "workspace", "out", "status"):
        refused(lib, call(lib, args, **{name: None}), name.encode(), b"null")
    for name in ("n", "h", "w"):
        for v in (0, -3):
            refused(lib, call(lib, args, **{name: v}), b"bad size", name.encode() + b"=" + str(v).encode())
    refused(lib, call(lib, args, h=65536), b"bad size", b"65535")
    refused(lib, call(lib, args, w=70000), b"bad size", b"65535")
    for ch in (0, 2, 4, -1):
        refused(lib, call(lib, args, components=ch), b"components=" + str(ch).encode())
    for hs, vs in ((1, 2), (2, 4), (4, 1), (0, 1), (3, 3)):
        refused(lib, call(lib, args, hs=hs, vs=vs), b"bad sampling", f"hs={hs} vs={vs}".encode())
    refused(lib, call(lib, args, components=1), b"bad sampling", b"hs=2 vs=2")                      # one component is 1 x 1
    refused(lib, call(lib, args, scan_bytes=1 << 31), b"scan_bytes=2147483648")
    refused(lib, call(lib, args, scan_bytes=(1 << 31) - 15), b"scan_bytes=2147483633", b"2^31 - 16")
    for v in (0, -1):
        refused(lib, call(lib, args, n_intervals=v), b"n_intervals=" + str(v).encode())
    refused(lib, call(lib, args, n=(1 << 31) - 1, h=64, w=64), b"bad size", b"workgroups")
    refused(lib, call(lib, args, workspace=at(64 + 8)), b"workspace", b"16-byte aligned")
    refused(lib, call(lib, args, status=at(192 + 2)), b"status", b"4-byte aligned")
    a = args[1]
    refused(lib, call(lib, args, workspace_bytes=a["workspace_bytes"] - 1), b"workspace capacity", str(a["workspace_bytes"]).encode())
    refused(lib, call(lib, args, out_capacity=a["out_capacity"] - 1), b"out capacity", str(a["out_capacity"]).encode())
    for where, v in ((0, 0), (63, 256), (64, 0), (191, 1000)):
        qt = np.full(192, 7, np.uint16)
        qt[where] = v
        refused(lib, call(lib, args, qtables=qt.ctypes.data_as(ctypes.c_void_p)), b"qtables[" + str(where).encode() + b"]=" + str(v).encode())


def test_decode_validates_the_interval_table(lib, args):
    """On the host side of the call, before anything is launched: the frame, the bytes and the MCUs of every interval exist."""
    good = args[0][2]
    for row, col, v, words in ((0, 0, -1, (b"interval 0", b"frame -1 of 2")), (1, 0, 2, (b"interval 1", b"frame 2 of 2")),
                               (0, 1, -4, (b"interval 0", b"bytes -4 + 100")), (1, 2, 61, (b"interval 1", b"bytes 100 + 61", b"160")),
                               (1, 1, (1 << 31) - 1, (b"interval 1", b"outside the scan")), (0, 2, -1, (b"interval 0", b"bytes 0 + -1")),
                               (0, 3, -1, (b"interval 0", b"MCUs -1 + 4")), (1, 4, 5, (b"interval 1", b"MCUs 0 + 5", b"frame's 4")),
                               (1, 3, 1, (b"interval 1", b"MCUs 1 + 4")), (0, 4, (1 << 31) - 1, (b"interval 0", b"outside the frame"))):
        iv = good.copy()
        iv[row, col] = v
        refused(lib, call(lib, args, intervals=iv.ctypes.data_as(ctypes.c_void_p)), *words)


def test_python_layer_refuses(lib):
    import torch
    from video_depth_anything_amd import mjpeg, ops
    with pytest.raises(ValueError, match="decode_jpeg_numpy"):
        mjpeg.decode_jpeg([b"\xff\xd8"], device="cpu")
    with pytest.raises(ValueError, match="no frames"):
        mjpeg.decode_jpeg([])
    z = torch.zeros(64, dtype=torch.uint8)
    iv, tables, qt = np.zeros((1, 5), np.int32), np.zeros((), mjpeg.TABLES_DTYPE), np.ones((1, 64), np.uint16)
    with pytest.raises(ValueError, match="cuda"):
        ops.mjpeg_decode(z, iv, tables, qt, 1, 1, z, torch.zeros(1, 8, 8, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32))
