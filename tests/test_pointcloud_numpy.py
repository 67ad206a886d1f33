"""The host side of the point-cloud export (video_depth_anything_amd/pointcloud.py): the twin unproject_numpy against a case worked
out by hand and against an independent restatement of the reference's expressions, the two record layouts, the keep rule, the
header and the file round trip. No GPU and no shared library: the module is loaded from its file."""
import importlib.util
import os

import numpy as np
import pytest

from _pointcloud_inputs import DTYPES, FX, FY, IDS, MAX_DEPTH, PATTERNS, RECORD_SIZE, SHAPES, case, keep_mask, with_pattern

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_BITS = 0x7ff8000000000000


@pytest.fixture(scope="module")
def pc():
    spec = importlib.util.spec_from_file_location("_pointcloud_under_test", os.path.join(REPO, "video_depth_anything_amd", "pointcloud.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def fields(pc, raw, dtype):
    return np.frombuffer(raw.tobytes(), dtype=pc.record_dtype(dtype))


def test_the_twin_on_a_case_worked_out_by_hand(pc):
    """2 x 3, fx = fy = 1, cx = 1.5, cy = 1.0 and depths that are powers of two: every product is exact."""
    depth = np.array([[[1.0, 2.0, 4.0], [0.5, 8.0, 0.25]]], np.float32)
    rgb = np.arange(18, dtype=np.uint8).reshape(1, 2, 3, 3) * 15
    want_x = [-1.5, -1.0, 2.0, -0.75, -4.0, 0.125]          # (c - 1.5) * z
    want_y = [-1.0, -2.0, -4.0, 0.0, 0.0, 0.0]              # (r - 1.0) * z
    want_z = [1.0, 2.0, 4.0, 0.5, 8.0, 0.25]
    for dtype in DTYPES:
        (raw,) = pc.unproject_numpy(depth, rgb, 1.0, 1.0, dtype=dtype)
        assert raw.dtype == np.uint8 and raw.size == 6 * RECORD_SIZE[dtype]
        rec = fields(pc, raw, dtype)
        assert rec["x"].tolist() == want_x and rec["y"].tolist() == want_y and rec["z"].tolist() == want_z
        assert not np.signbit(rec["y"][3:]).any()                           # (+0) * z = +0 in row 1
        assert np.stack([rec["red"], rec["green"], rec["blue"]], -1).tolist() == rgb.reshape(-1, 3).tolist()
    # the packed layout, byte for byte, of the first float64 record: doubles at 0 / 8 / 16, r g b at 24 / 25 / 26
    (raw,) = pc.unproject_numpy(depth, rgb, 1.0, 1.0)
    assert raw[:27].tobytes() == np.array([-1.5, -1.0, 1.0], "<f8").tobytes() + bytes([0, 15, 30])
    (raw,) = pc.unproject_numpy(depth, rgb, 1.0, 1.0, dtype="float32")
    assert raw[15:30].tobytes() == np.array([-1.0, -2.0, 2.0], "<f4").tobytes() + bytes([45, 60, 75])


def restated(depth, rgb, fx, fy):
    """The reference's own expressions (np.meshgrid of integer aranges, promoted to float64 by `width / 2` and the float32 depth by
    np.multiply) for one frame: points float64 [H*W, 3]. Shares no code with the twin."""
    height, width = depth.shape
    x, y = np.meshgrid(np.arange(width), np.arange(height))
    x = (x - width / 2) / fx
    y = (y - height / 2) / fy
    z = np.array(depth)
    with np.errstate(invalid="ignore"):
        points = np.stack((np.multiply(x, z), np.multiply(y, z), z), axis=-1).reshape(-1, 3)
    assert points.dtype == np.float64
    return points, np.array(rgb).reshape(-1, 3)


def canonical(points):
    """The contract's one departure from what a host computes: a NaN coordinate is the quiet NaN 0x7ff8000000000000 whatever sign
    the host's FPU gave it (0 * Inf is -NaN on x86). Every other value is compared bit for bit."""
    bits = np.ascontiguousarray(points).view(np.uint64).copy()
    bits[np.isnan(points)] = NAN_BITS
    return bits


@pytest.mark.parametrize("n,h,w", SHAPES, ids=IDS)
def test_the_twin_is_the_reference_expression_bit_for_bit(pc, n, h, w):
    depths, frames = case(n, h, w)
    got = pc.unproject_numpy(depths, frames, FX, FY)
    got32 = pc.unproject_numpy(depths, frames, FX, FY, dtype="float32")
    assert len(got) == len(got32) == n
    for i in range(n):
        points, colors = restated(depths[i], frames[i], FX, FY)
        rec = fields(pc, got[i], "float64")
        mine = np.stack([rec["x"], rec["y"], rec["z"]], -1)
        assert np.array_equal(canonical(mine), canonical(points))
        assert np.array_equal(np.stack([rec["red"], rec["green"], rec["blue"]], -1), colors)
        # NaN and Inf depths pass through: Z has the depth's own value, bit for bit after the exact widening
        assert mine[:, 2].tobytes() == depths[i].astype(np.float64).tobytes()
        # the float32 record is the float64 result rounded once; its Z is the depth's own bits
        rec32 = fields(pc, got32[i], "float32")
        with np.errstate(over="ignore"):
            assert rec32["x"].tobytes() == rec["x"].astype(np.float32).tobytes() and rec32["y"].tobytes() == rec["y"].astype(np.float32).tobytes()
        assert rec32["z"].tobytes() == depths[i].tobytes()
        assert np.array_equal(np.stack([rec32["red"], rec32["green"], rec32["blue"]], -1), colors)


def test_a_generated_nan_is_the_positive_quiet_nan(pc):
    depth = np.full((1, 2, 2), np.inf, np.float32)            # cx = cy = 1.0: column 1 and row 1 have factor 0
    (raw,) = pc.unproject_numpy(depth, np.zeros((1, 2, 2, 3), np.uint8), FX, FY)
    rec = fields(pc, raw, "float64")
    assert rec["x"].view(np.uint64).tolist() == [0xfff0000000000000, NAN_BITS, 0xfff0000000000000, NAN_BITS]
    assert rec["y"].view(np.uint64).tolist() == [0xfff0000000000000, 0xfff0000000000000, NAN_BITS, NAN_BITS]


def test_the_colour_round_trip_is_the_identity():
    """The reference stores colour / 255.0 and Open3D's writer maps it back with round(clamp(c, 0, 1) * 255)."""
    c = np.arange(256, dtype=np.uint8)
    back = np.round(np.clip(c / 255.0, 0.0, 1.0) * 255.0)
    assert np.array_equal(back, c.astype(np.float64))


def test_non_default_principal_point(pc):
    depths, frames = case(1, 3, 5)
    (raw,) = pc.unproject_numpy(depths, frames, FX, FY, cx=1.25, cy=-0.75)
    rec = fields(pc, raw, "float64")
    z = depths[0].astype(np.float64)
    with np.errstate(invalid="ignore"):
        x = ((np.arange(5, dtype=np.float64) - 1.25) / FX)[None, :] * z
        y = ((np.arange(3, dtype=np.float64) + 0.75) / FY)[:, None] * z
    assert np.array_equal(canonical(rec["x"]), canonical(x.ravel())) and np.array_equal(canonical(rec["y"]), canonical(y.ravel()))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_keep_rule(pc, dtype):
    """0 < z <= max_depth: zero, negatives, NaN, Inf and anything beyond are dropped, z == max_depth stays; order is row-major."""
    depth = np.array([[[0.0, -1.0, np.nan, np.inf, 10.0, np.nextafter(np.float32(10), np.float32(11)), 1e-30, 3.0]]], np.float32)
    rgb = np.arange(24, dtype=np.uint8).reshape(1, 1, 8, 3)
    (raw,) = pc.unproject_numpy(depth, rgb, FX, FY, max_depth=MAX_DEPTH, dtype=dtype)
    rec = fields(pc, raw, dtype)
    assert rec["z"].tolist() == [10.0, float(np.float32(1e-30)), 3.0] and rec["red"].tolist() == [12, 18, 21]
    (everything,) = pc.unproject_numpy(depth, rgb, FX, FY, dtype=dtype)
    assert fields(pc, everything, dtype).size == 8                                   # the default keeps every pixel
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_depth"):
            pc.unproject_numpy(depth, rgb, FX, FY, max_depth=bad)
    for n, h, w in SHAPES:
        depths, frames = case(n, h, w)
        for kind in PATTERNS:
            d = with_pattern(depths, kind)
            kept = pc.unproject_numpy(d, frames, FX, FY, max_depth=MAX_DEPTH, dtype=dtype)
            full = pc.unproject_numpy(d, frames, FX, FY, dtype=dtype)
            for i in range(n):
                mask = keep_mask(d[i]).ravel()
                assert kept[i].tobytes() == fields(pc, full[i], dtype)[mask].tobytes()       # numpy's records[keep]
                if kind == "none":
                    assert kept[i].size == 0
                if kind == "all":
                    assert kept[i].size == h * w * RECORD_SIZE[dtype]
                if kind == "last":
                    assert kept[i].size == RECORD_SIZE[dtype]


def test_bad_arguments_are_refused(pc):
    depths, frames = case(1, 3, 5)
    with pytest.raises(ValueError, match="dtype"):
        pc.unproject_numpy(depths, frames, FX, FY, dtype="float16")
    with pytest.raises(ValueError, match="float32"):
        pc.unproject_numpy(depths.astype(np.float64), frames, FX, FY)
    with pytest.raises(ValueError, match=r"\[n,H,W,3\]"):
        pc.unproject_numpy(depths, frames[:, :, :4], FX, FY)
    for fx in (0.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="focal"):
            pc.unproject_numpy(depths, frames, fx, FY)
    with pytest.raises(ValueError, match="principal"):
        pc.unproject_numpy(depths, frames, FX, FY, cx=float("nan"))


def test_the_header_text(pc):
    assert pc.ply_header(921600) == ("ply\n"
                                     "format binary_little_endian 1.0\n"
                                     "comment Created by Open3D\n"
                                     "element vertex 921600\n"
                                     "property double x\n"
                                     "property double y\n"
                                     "property double z\n"
                                     "property uchar red\n"
                                     "property uchar green\n"
                                     "property uchar blue\n"
                                     "end_header\n")
    assert pc.ply_header(0, "float32") == ("ply\n"
                                           "format binary_little_endian 1.0\n"
                                           "comment Created by Open3D\n"
                                           "element vertex 0\n"
                                           "property float x\n"
                                           "property float y\n"
                                           "property float z\n"
                                           "property uchar red\n"
                                           "property uchar green\n"
                                           "property uchar blue\n"
                                           "end_header\n")
    assert pc.frame_name(7) == "point0007.ply" and pc.frame_name(12345) == "point12345.ply"


@pytest.mark.parametrize("dtype", DTYPES)
def test_write_then_read(pc, dtype, tmp_path):
    depths, frames = case(2, 23, 45)
    for max_depth in (None, MAX_DEPTH):
        for i, raw in enumerate(pc.unproject_numpy(depths, frames, FX, FY, max_depth=max_depth, dtype=dtype)):
            path = tmp_path / pc.frame_name(i)
            count = pc.write_ply(path, raw, dtype)
            assert count * RECORD_SIZE[dtype] == raw.size
            assert os.path.getsize(path) == len(pc.ply_header(count, dtype)) + count * RECORD_SIZE[dtype]
            assert path.read_bytes() == pc.ply_header(count, dtype).encode() + raw.tobytes()
            points, colors = pc.read_ply(path)
            rec = fields(pc, raw, dtype)
            assert points.dtype == np.dtype(dtype) and points.shape == (count, 3) and colors.dtype == np.uint8 and colors.shape == (count, 3)
            assert points.tobytes() == np.stack([rec["x"], rec["y"], rec["z"]], -1).tobytes()
            assert colors.tobytes() == np.stack([rec["red"], rec["green"], rec["blue"]], -1).tobytes()
    empty = tmp_path / "empty.ply"
    assert pc.write_ply(empty, np.zeros(0, np.uint8), dtype) == 0 and pc.read_ply(empty)[0].shape == (0, 3)
    with pytest.raises(ValueError, match="whole number"):
        pc.write_ply(tmp_path / "bad.ply", np.zeros(RECORD_SIZE[dtype] + 1, np.uint8), dtype)


def test_read_refuses_what_it_did_not_write(pc, tmp_path):
    depths, frames = case(1, 3, 5)
    (raw,) = pc.unproject_numpy(depths, frames, FX, FY)
    good = pc.ply_header(15).encode() + raw.tobytes()
    foreign = {
        "ascii.ply": good.replace(b"binary_little_endian", b"ascii"),
        "big.ply": good.replace(b"binary_little_endian", b"binary_big_endian"),
        "normals.ply": good.replace(b"property uchar red\n", b"property double nx\nproperty uchar red\n"),
        "faces.ply": good.replace(b"end_header\n", b"element face 0\nproperty list uchar int vertex_indices\nend_header\n"),
        "comment.ply": good.replace(b"Created by Open3D", b"Created by something else"),
        "short.ply": good[:-1],
        "long.ply": good + b"\0",
        "nothing.ply": b"not a ply file\n",
        "headless.ply": b"ply\nformat binary_little_endian 1.0\n",
    }
    for name, blob in foreign.items():
        (tmp_path / name).write_bytes(blob)
        with pytest.raises(ValueError):
            pc.read_ply(tmp_path / name)
    (tmp_path / "good.ply").write_bytes(good)
    assert pc.read_ply(tmp_path / "good.ply")[0].shape == (15, 3)
