"""The EXR entry points of the C ABI (csrc/exr.hip, include/vda.h): exported with the declared signatures, the size functions are the
documented formulas, bad arguments are refused before any launch, each by its own message: no GPU needed."""
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
    """Well-formed arguments for 3 frames of 37 x 518 at aligned HOST addresses that are never dereferenced (every call below is
    refused first)."""
    buf = (ctypes.c_char * 1024)()
    base = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    at = lambda off: ctypes.c_void_p(base + off)
    a = dict(depth=at(0), frames=3, h=37, w=518, frame_stride=37 * 518, header_bytes=277, workspace=at(64),
             workspace_bytes=lib.vda_exr_workspace_bytes(3, 37, 518), payload=at(129), payload_capacity=lib.vda_exr_payload_bytes(3, 37, 518),
             offsets=at(192))
    return buf, a, at


def call(lib, args, **over):
    a = dict(args[1])
    a.update(over)
    return lib.vda_exr_zip_f32(a["depth"], a["frames"], a["h"], a["w"], a["frame_stride"], a["header_bytes"], a["workspace"], a["workspace_bytes"],
                               a["payload"], a["payload_capacity"], a["offsets"], None)


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
    vp, i, ll, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_size_t
    for name in ("vda_exr_workspace_bytes", "vda_exr_payload_bytes"):
        assert hasattr(lib, name)
        assert declared(name) == ("size_t", ["int frames", "int h", "int w"])
        assert _lib.SIGNATURES[name] == (sz, [i, i, i])
    assert hasattr(lib, "vda_exr_zip_f32")
    assert declared("vda_exr_zip_f32") == ("int", ["const float* depth", "int frames", "int h", "int w", "long long frame_stride", "long long header_bytes",
                                                   "void* workspace", "size_t workspace_bytes", "uint8_t* payload", "size_t payload_capacity",
                                                   "long long* offsets", "vda_stream_t stream"])
    assert _lib.SIGNATURES["vda_exr_zip_f32"] == (i, [vp, i, i, i, ll, ll, vp, sz, vp, sz, vp, vp])


def test_the_abi_number_stays(lib):
    assert lib.vda_abi_version() == 8


def chunks_of(h, w):
    """Chunks and blocks of one frame: a block of `rows` scanlines is ceil(4 w rows / 16384) chunks."""
    nb = -(-h // 16)
    return sum(-(-4 * w * min(16, h - 16 * b) // CHUNK) for b in range(nb)), nb


def test_the_bounds_are_the_documented_ones(lib):
    up16 = lambda v: (v + 15) // 16 * 16
    for frames, h, w in ((1, 1, 1), (1, 16, 64), (1, 16, 256), (2, 17, 257), (3, 37, 518), (32, 518, 518), (7, 1080, 1920), (1, 65535, 65535),
                         (2, 15, 4097), (5, 16, 4096), (1000, 518, 518)):
        per_frame, nb = chunks_of(h, w)
        chunks, blocks = frames * per_frame, frames * nb
        assert lib.vda_exr_payload_bytes(frames, h, w) == frames * (8 * nb + 8 * nb + 4 * w * h)
        assert lib.vda_exr_workspace_bytes(frames, h, w) == chunks * 16400 + 2 * up16(4 * chunks) + 16 * chunks + 2 * up16(4 * blocks) + up16(8 * blocks)
    for frames, h, w in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, 65536, 4), (1, 4, 65536), (2049, 65535, 65535)):
        assert lib.vda_exr_payload_bytes(frames, h, w) == 0 and lib.vda_exr_workspace_bytes(frames, h, w) == 0
    # the largest frame is 1 048 560 chunks: 2048 of them are one grid of at most 2^31 - 1 workgroups, 2049 are not
    assert chunks_of(65535, 65535)[0] * 2048 <= 2 ** 31 - 1 < chunks_of(65535, 65535)[0] * 2049
    assert lib.vda_exr_workspace_bytes(2048, 65535, 65535) > 0


def test_encode_refuses(lib, args):
    at, a = args[2], args[1]
    for name, word in (("depth", b"depth"), ("workspace", b"workspace"), ("payload", b"payload"), ("offsets", b"offsets")):
        refused(lib, call(lib, args, **{name: None}), word, b"null")
    for name in ("frames", "h", "w"):
        for v in (0, -3):
            refused(lib, call(lib, args, **{name: v}), b"bad size", name.encode() + b"=" + str(v).encode())
    refused(lib, call(lib, args, h=65536), b"too large", b"h=65536")
    refused(lib, call(lib, args, w=65536), b"too large", b"w=65536")
    refused(lib, call(lib, args, frames=2049, h=65535, w=65535, frame_stride=65535 * 65535), b"too large", b"chunks")
    refused(lib, call(lib, args, frame_stride=37 * 518 - 1), b"frame_stride", str(37 * 518 - 1).encode())
    refused(lib, call(lib, args, header_bytes=-1), b"header_bytes=-1")
    for off in (1, 2, 3):
        refused(lib, call(lib, args, depth=at(off)), b"depth", b"4-byte aligned")
    refused(lib, call(lib, args, workspace=at(64 + 8)), b"workspace", b"16-byte aligned")
    refused(lib, call(lib, args, offsets=at(192 + 4)), b"offsets", b"8-byte aligned")
    refused(lib, call(lib, args, workspace_bytes=a["workspace_bytes"] - 1), b"workspace capacity", str(a["workspace_bytes"]).encode())
    refused(lib, call(lib, args, payload_capacity=a["payload_capacity"] - 1), b"payload capacity", str(a["payload_capacity"]).encode())


def test_python_layer_refuses(lib):
    import torch
    from video_depth_anything_amd import exr, ops
    with pytest.raises(ValueError, match="encode_exr_numpy"):
        exr.encode_exr(torch.zeros(1, 4, 4))                                  # a host tensor is an error, not a silent CPU path
    with pytest.raises(ValueError, match="encode_exr_numpy"):
        exr.encode_exr(np.zeros((1, 4, 4), np.float32), device="cpu")
    with pytest.raises(ValueError, match="cuda"):
        z = torch.zeros(64, dtype=torch.uint8)
        ops.exr_zip(torch.zeros(1, 4, 4), 277, z, z, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"\[h, w\]"):
        exr.encode_exr_numpy(np.zeros((2, 3, 4), np.float32))
