"""unproject / write_pointclouds (csrc/pointcloud.hip) on the MI355X: the device's record bytes are the host twin
unproject_numpy's bytes, exactly, for both record types.

A workgroup of the kernel covers 256 consecutive pixels of a frame (PC_T in csrc/pointcloud.hip, TILE in _pointcloud_inputs.py), so
the shapes are the smallest that meet each hazard: one pixel; 7 x 37 = 259, one workgroup plus 3; 16 x 16, exactly one; 33 x 31 with
an odd width and a ragged tail; two frames whose H * W * 27 is no multiple of 4; three frames of nine whole workgroups. Every call
writes into a buffer pre-filled with 0xA5 that is followed by 64 sentinel bytes: nothing past a frame's records may change."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _pointcloud_inputs import DTYPES, FX, FY, IDS, MAX_DEPTH, PATTERNS, RECORD_SIZE, SHAPES, TILE, case, keep_mask, with_pattern

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL, SENTINEL = 0xA5, 64
_twins = {}


def twin(key, depths, frames, **kw):
    """The host twin's bytes, computed once per case and shared."""
    from video_depth_anything_amd.pointcloud import unproject_numpy
    if key not in _twins:
        _twins[key] = unproject_numpy(depths, frames, FX, FY, **kw)
    return _twins[key]


def run_device(depths, frames, max_depth=None, dtype="float64", cx=None, cy=None):
    """One call of ops.pointcloud into a 0xA5 buffer with a sentinel behind it: (record bytes per frame, counts, the whole buffer).
    Checked here: nothing outside a frame's count * record_size bytes was written, the sentinel least of all."""
    from video_depth_anything_amd import ops
    n, h, w = depths.shape
    f32 = dtype == "float32"
    stride = ops.pointcloud_frame_stride(h, w, f32)
    assert stride % 16 == 0 and stride >= h * w * RECORD_SIZE[dtype]
    buf = torch.full((n * stride + SENTINEL,), FILL, dtype=torch.uint8, device="cuda")
    counts = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    workspace = torch.full((ops.pointcloud_workspace_bytes(n, h, w),), FILL, dtype=torch.uint8, device="cuda")
    ops.pointcloud(torch.from_numpy(depths).cuda(), torch.from_numpy(frames).cuda(), buf, counts, workspace, FX, FY,
                   w / 2.0 if cx is None else cx, h / 2.0 if cy is None else cy, max_depth, f32)
    torch.cuda.synchronize()
    whole, counts = buf.cpu().numpy(), counts.cpu().tolist()
    assert (whole[n * stride:] == FILL).all(), "the sentinel behind the last slot was written"
    out = []
    for i, c in enumerate(counts):
        assert 0 <= c <= h * w
        used = c * RECORD_SIZE[dtype]
        out.append(whole[i * stride:i * stride + used])
        assert (whole[i * stride + used:(i + 1) * stride] == FILL).all(), f"frame {i}: bytes behind its {c} records were written"
    return out, counts, whole


def report_difference(got, want, what):
    """Where the bytes differ: printed before the assertion so that a failure says which record and which byte of it."""
    if got.size != want.size:
        print(f"{what}: {got.size} bytes, want {want.size}")
        return
    diff = np.flatnonzero(got != want)
    if diff.size:
        print(f"{what}: {diff.size} of {want.size} bytes differ, first at byte {diff[0]}, last at {diff[-1]}: "
              f"got {got[diff[0]]:#04x} want {want[diff[0]]:#04x}")


def assert_frames_equal(got, want, what):
    assert len(got) == len(want)
    for i, (g, t) in enumerate(zip(got, want)):
        report_difference(g, t, f"{what}, frame {i}")
        assert g.tobytes() == t.tobytes(), f"{what}, frame {i}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,h,w", SHAPES, ids=IDS)
def test_keeping_every_pixel_is_the_twin_byte_for_byte(n, h, w, dtype):
    """The default: counts are H * W and NaN, Inf, zeros and negatives pass through with the twin's bits."""
    depths, frames = case(n, h, w)
    got, counts, whole = run_device(depths, frames, None, dtype)
    assert counts == [h * w] * n
    assert_frames_equal(got, twin((n, h, w, dtype, None), depths, frames, dtype=dtype), f"{(n, h, w)} {dtype}")
    _, counts2, whole2 = run_device(depths, frames, None, dtype)             # a second run: identical bytes and counts
    assert counts2 == counts and whole2.tobytes() == whole.tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", PATTERNS)
def test_max_depth_keeps_in_order(kind, dtype):
    """max_depth = 10 on every shape with the kept set chosen by overwriting depths (_pointcloud_inputs.with_pattern)."""
    for n, h, w in SHAPES:
        depths, frames = case(n, h, w)
        d = with_pattern(depths, kind)
        mask = keep_mask(d).reshape(n, -1)
        if kind == "alternating" and h * w >= 3 * TILE:
            # the workgroups' first bytes fall on different residues modulo 4 and modulo 16
            per_tile = [int(mask[0][k:k + TILE].sum()) for k in range(0, h * w, TILE)]
            first = np.cumsum([0] + per_tile[:-1]) * RECORD_SIZE[dtype]
            assert len(set((first % 4).tolist())) > 1 and len(set((first % 16).tolist())) > 2, first
        got, counts, whole = run_device(d, frames, MAX_DEPTH, dtype)
        assert counts == mask.sum(1).tolist(), (kind, (n, h, w))
        if kind == "none":
            assert counts == [0] * n
        if kind == "all":
            assert counts == [h * w] * n
        if kind == "last":
            assert counts == [1] * n
        assert_frames_equal(got, twin((n, h, w, dtype, kind), d, frames, max_depth=MAX_DEPTH, dtype=dtype), f"{kind} {(n, h, w)} {dtype}")
        if (n, h, w) == SHAPES[-1]:
            _, counts2, whole2 = run_device(d, frames, MAX_DEPTH, dtype)      # two runs give identical bytes and counts
            assert counts2 == counts and whole2.tobytes() == whole.tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_default_principal_point(dtype):
    from video_depth_anything_amd.pointcloud import unproject_numpy
    depths, frames = case(2, 23, 45)
    for max_depth in (None, MAX_DEPTH):
        got, _, _ = run_device(depths, frames, max_depth, dtype, cx=20.25, cy=-3.5)
        assert_frames_equal(got, unproject_numpy(depths, frames, FX, FY, cx=20.25, cy=-3.5, max_depth=max_depth, dtype=dtype), f"cx, cy, {max_depth}")


def test_unproject_takes_host_arrays_and_device_tensors():
    from video_depth_anything_amd.pointcloud import unproject
    depths, frames = case(2, 23, 45)
    for dtype in DTYPES:
        for max_depth in (None, MAX_DEPTH):
            want = twin((2, 23, 45, dtype, "as_is" if max_depth else None), depths, frames, max_depth=max_depth, dtype=dtype)
            got = unproject(depths, frames, FX, FY, max_depth=max_depth, dtype=dtype)
            assert all(isinstance(g, np.ndarray) and g.dtype == np.uint8 for g in got)
            assert_frames_equal(got, want, f"host arrays {dtype} {max_depth}")
            on_device = unproject(torch.from_numpy(depths).cuda(), torch.from_numpy(frames).cuda(), FX, FY, max_depth=max_depth, dtype=dtype)
            assert_frames_equal(on_device, want, f"device tensors {dtype} {max_depth}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_files_do_not_depend_on_block_frames(dtype, tmp_path):
    from video_depth_anything_amd.pointcloud import frame_name, ply_header, read_ply, unproject_numpy, write_pointclouds
    depths, frames = case(5, 23, 45)
    for max_depth in (None, MAX_DEPTH):
        want = unproject_numpy(depths, frames, FX, FY, max_depth=max_depth, dtype=dtype)
        for block in (1, 3, 8):
            out = tmp_path / f"{max_depth}_{block}"
            counts = write_pointclouds(depths, frames, out, FX, FY, max_depth=max_depth, dtype=dtype, block_frames=block)
            assert sorted(os.listdir(out)) == [frame_name(i) for i in range(5)] == [f"point000{i}.ply" for i in range(5)]
            assert counts == [t.size // RECORD_SIZE[dtype] for t in want]
            for i in range(5):
                blob = (out / frame_name(i)).read_bytes()
                assert blob == ply_header(counts[i], dtype).encode() + want[i].tobytes(), (max_depth, block, i)
        points, colors = read_ply(out / frame_name(4))
        assert points.shape == (counts[4], 3) and colors.shape == (counts[4], 3)


def test_cli_writes_the_models_depth(tmp_path):
    """metric_depth/depth_to_pointcloud.py end to end on the frames test_run_cli_synthetic uses (30 of 70 x 84, two pieces of the
    stream): one file per frame with H * W vertices, Z the metric model's own depth bit for bit, the colours the frames; --stream
    writes the same files."""
    from video_depth_anything_amd.pointcloud import frame_name, ply_header, read_ply
    from video_depth_anything_amd.video_depth import MetricVideoDepthAnything
    from video_depth_anything_amd.weights import synthetic_state_dict
    frames = np.random.default_rng(9).integers(0, 256, (30, 70, 84, 3), dtype=np.uint8)
    src = tmp_path / "clip.npz"
    np.savez(src, frames=frames, fps=24)
    blobs = {}
    for flag in ([], ["--stream"]):
        out = tmp_path / ("streamed" if flag else "whole")
        r = subprocess.run([sys.executable, os.path.join(REPO, "metric_depth", "depth_to_pointcloud.py"), "--input_video", str(src), "--output_dir",
                            str(out), "--encoder", "vits", "--input_size", "70", "--checkpoint", "synthetic"] + flag,
                           capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        assert sorted(os.listdir(out)) == [frame_name(i) for i in range(30)]
        blobs[bool(flag)] = [(out / frame_name(i)).read_bytes() for i in range(30)]
    assert blobs[True] == blobs[False]

    m = MetricVideoDepthAnything(encoder="vits", features=64, out_channels=[48, 96, 192, 384])
    m.load_state_dict(synthetic_state_dict(m.cfg, seed=0), strict=True)
    depths, _ = m.to("cuda").eval().infer_video_depth(frames, 24, input_size=70, device="cuda")
    assert depths.shape == (30, 70, 84) and depths.dtype == np.float32
    header = ply_header(70 * 84).encode()
    for i in range(30):
        assert blobs[False][i].startswith(header) and len(blobs[False][i]) == len(header) + 70 * 84 * 27
        points, colors = read_ply(tmp_path / "whole" / frame_name(i))
        assert points.dtype == np.float64 and points[:, 2].tobytes() == depths[i].astype(np.float64).tobytes(), i
        assert colors.tobytes() == frames[i].tobytes(), i
        if i == 0:                                                     # the reference's defaults: fx = fy = 470.4, cx = 42, cy = 35
            z = depths[0].astype(np.float64)
            x = ((np.arange(84, dtype=np.float64) - 42.0) / 470.4)[None, :] * z
            y = ((np.arange(70, dtype=np.float64) - 35.0) / 470.4)[:, None] * z
            assert points[:, 0].tobytes() == x.tobytes() and points[:, 1].tobytes() == y.tobytes()
