"""The point-cloud entry points of the C ABI (csrc/pointcloud.hip, include/vda.h) refuse bad arguments before any launch, and the
Python layer refuses host tensors: no GPU needed."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, H, W = 2, 7, 37
FX, FY, CX, CY = 470.4, 391.7, 18.5, 3.5
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def lib():
    from video_depth_anything_amd import build
    build.build()
    from video_depth_anything_amd import _lib
    return _lib.lib


@pytest.fixture(scope="module")
def ptrs():
    """Distinct 16-byte aligned host addresses and two misaligned ones: never dereferenced, every call below is refused first."""
    buf = (ctypes.c_char * 512)()
    base = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    at = lambda off: ctypes.c_void_p(base + off)
    return buf, dict(depth=at(0), rgb=at(64), records=at(128), counts=at(192), workspace=at(256)), at(2), at(128 + 8)


def refused(lib, rc, word):
    msg = lib.vda_last_error()
    assert rc != 0 and word in msg, (rc, msg)


def declared(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vda.h")).read(), flags=re.S)
    decl = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert decl, f"include/vda.h does not declare {name}"
    return decl.group(1), [" ".join(p.split()) for p in decl.group(2).split(",")]


def test_symbols_are_exported_with_the_declared_signatures(lib):
    from video_depth_anything_amd import _lib
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    for name in ("vda_pointcloud_frame_stride", "vda_pointcloud_workspace_bytes", "vda_pointcloud_f32"):
        assert hasattr(lib, name)
    assert declared("vda_pointcloud_frame_stride") == ("size_t", ["int h", "int w", "int record_f32"])
    assert _lib.SIGNATURES["vda_pointcloud_frame_stride"] == (ctypes.c_size_t, [i, i, i])
    assert declared("vda_pointcloud_workspace_bytes") == ("size_t", ["int n", "int h", "int w"])
    assert _lib.SIGNATURES["vda_pointcloud_workspace_bytes"] == (ctypes.c_size_t, [i, i, i])
    assert declared("vda_pointcloud_f32") == ("int", [
        "const float* depth", "const uint8_t* rgb", "void* records", "int* counts", "void* workspace", "size_t workspace_bytes",
        "int n", "int h", "int w", "double fx", "double fy", "double cx", "double cy", "float max_depth", "int record_f32", "vda_stream_t stream"])
    res, args = _lib.SIGNATURES["vda_pointcloud_f32"]
    assert res is ctypes.c_int
    assert args == [vp] * 5 + [ctypes.c_size_t, i, i, i, d, d, d, d, ctypes.c_float, i, vp]


def test_the_abi_number_stays(lib):
    assert lib.vda_abi_version() == 8


def test_frame_stride_and_workspace(lib):
    for h, w in ((1, 1), (3, 5), (7, 37), (23, 45), (720, 1280)):
        for f32, size in ((0, 27), (1, 15)):
            s = lib.vda_pointcloud_frame_stride(h, w, f32)
            assert s % 16 == 0 and h * w * size <= s < h * w * size + 16
        assert lib.vda_pointcloud_workspace_bytes(4, h, w) > 0
    assert lib.vda_pointcloud_frame_stride(0, 5, 0) == 0 and lib.vda_pointcloud_frame_stride(3, 5, 2) == 0
    assert lib.vda_pointcloud_workspace_bytes(0, 3, 5) == 0


def call(lib, ptrs, **over):
    a = dict(ptrs[1], workspace_bytes=None, n=N, h=H, w=W, fx=FX, fy=FY, cx=CX, cy=CY, max_depth=0.0, record_f32=0)
    a.update(over)
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = max(lib.vda_pointcloud_workspace_bytes(N, H, W), 1)
    return lib.vda_pointcloud_f32(a["depth"], a["rgb"], a["records"], a["counts"], a["workspace"], a["workspace_bytes"], a["n"], a["h"], a["w"],
                                  a["fx"], a["fy"], a["cx"], a["cy"], a["max_depth"], a["record_f32"], None)


def test_pointcloud_refuses(lib, ptrs):
    _, _, odd, half = ptrs
    for name in ("depth", "rgb", "records", "counts", "workspace"):
        refused(lib, call(lib, ptrs, **{name: None}), b"null")
    for sizes in (dict(n=0), dict(h=0), dict(w=0), dict(n=-1), dict(h=-3)):
        refused(lib, call(lib, ptrs, **sizes), b"bad size")
    for bad in (0.0, INF, -INF, NAN):
        refused(lib, call(lib, ptrs, fx=bad), b"focal")
        refused(lib, call(lib, ptrs, fy=bad), b"focal")
        if bad != 0.0:
            refused(lib, call(lib, ptrs, cx=bad), b"principal")
            refused(lib, call(lib, ptrs, cy=bad), b"principal")
    for bad in (-1.0, NAN, -INF):
        refused(lib, call(lib, ptrs, max_depth=bad), b"max_depth")
    for bad in (-1, 2, 27):
        refused(lib, call(lib, ptrs, record_f32=bad), b"record type")
    refused(lib, call(lib, ptrs, workspace_bytes=lib.vda_pointcloud_workspace_bytes(N, H, W) - 1), b"workspace too small")
    refused(lib, call(lib, ptrs, workspace_bytes=0), b"workspace too small")
    for name in ("depth", "counts", "workspace"):
        refused(lib, call(lib, ptrs, **{name: odd}), b"misaligned")
    refused(lib, call(lib, ptrs, records=half), b"misaligned")                 # 8-byte aligned is not enough for the records
    huge = ctypes.c_size_t(-1).value
    refused(lib, call(lib, ptrs, h=1 << 16, w=1 << 15, workspace_bytes=huge), b"too large")      # h * w = 2^31 pixels
    refused(lib, call(lib, ptrs, h=(1 << 15) + 1, w=1 << 15, workspace_bytes=huge), b"too large")   # just over 2^30
    refused(lib, call(lib, ptrs, n=1 << 20, h=1 << 10, w=1 << 10, workspace_bytes=huge), b"too large")   # 2^32 workgroups


def test_python_layer_refuses_host_tensors(lib):
    """ops.pointcloud takes device tensors only: a host tensor is an error, not a silent copy or a CPU path."""
    import torch
    from video_depth_anything_amd import ops
    depth, rgb = torch.ones(1, 3, 5), torch.zeros(1, 3, 5, 3, dtype=torch.uint8)
    records, counts = torch.zeros(ops.pointcloud_frame_stride(3, 5, False), dtype=torch.uint8), torch.zeros(1, dtype=torch.int32)
    workspace = torch.zeros(ops.pointcloud_workspace_bytes(1, 3, 5), dtype=torch.uint8)
    with pytest.raises(ValueError, match="cuda"):
        ops.pointcloud(depth, rgb, records, counts, workspace, FX, FY, 2.5, 1.5)
    from video_depth_anything_amd.pointcloud import unproject
    with pytest.raises(ValueError, match="cuda"):
        unproject(depth.numpy(), rgb.numpy(), FX, FY, device="cpu")
