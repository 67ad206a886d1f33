"""Metric depth as coloured point clouds: one binary PLY per frame, as the reference's metric_depth/depth_to_pointcloud.py writes
them through Open3D, with the vertex records built on the device (csrc/pointcloud.hip).

The contract. For frame i, pixel (row r, column c), z = depths[i, r, c] (float32) and colour frames[i, r, c, :] (uint8), in fp64
with every operation rounded once:

    X = ((c - cx) / fx) * z        cx defaults to W / 2.0 (x.5 for an odd W)
    Y = ((r - cy) / fy) * z        cy defaults to H / 2.0
    Z = z

the division first and the product second - numpy's `(x - width / 2) / fx` followed by `np.multiply(x, z)`. An X or Y that is NaN
(z is NaN, or 0 * Inf on the centre column or row) is the quiet NaN 0x7ff8000000000000: IEEE leaves the sign of a generated NaN to
the machine (x86 makes it negative, the GPU positive), so the contract fixes it. The reference divides the colours by 255.0 and
Open3D's writer maps them back with round(clamp(c, 0, 1) * 255), which is the identity on all 256 byte values: a record's colour
bytes are the frame's.

Records are packed and little-endian: "float64" (Open3D's own layout) is 27 bytes, doubles X, Y, Z at 0 / 8 / 16 and r, g, b at
24 / 25 / 26; "float32" is 15 bytes, floats at 0 / 4 / 8 (X and Y the fp64 results rounded once, Z the depth itself) and r, g, b at
12 / 13 / 14. `max_depth=None` keeps every pixel with its value untouched, as the reference does; `max_depth=m` (m > 0, rounded to
float32 like the depth it is compared with) keeps a pixel iff 0 < z <= m, in row-major order: numpy's `records[keep]`.

`unproject_numpy` is the host twin: no GPU, the same bytes as `unproject`.
"""
import os
import re

import numpy as np

RECORD_SIZE = {"float64": 27, "float32": 15}
_PLY_TYPE = {"float64": "double", "float32": "float"}
_NP_TYPE = {"float64": "<f8", "float32": "<f4"}
CANONICAL_NAN = np.float64(np.nan)                   # 0x7ff8000000000000


def record_dtype(dtype="float64"):
    """The packed numpy record of one vertex (itemsize 27 or 15)."""
    _record_size(dtype)
    f = _NP_TYPE[dtype]
    return np.dtype([("x", f), ("y", f), ("z", f), ("red", "u1"), ("green", "u1"), ("blue", "u1")])


def _record_size(dtype):
    if dtype not in RECORD_SIZE:
        raise ValueError(f"pointcloud: dtype must be 'float64' or 'float32', got {dtype!r}")
    return RECORD_SIZE[dtype]


def _intrinsics(h, w, fx, fy, cx, cy, max_depth):
    fx, fy = float(fx), float(fy)
    cx = w / 2.0 if cx is None else float(cx)
    cy = h / 2.0 if cy is None else float(cy)
    if not (np.isfinite(fx) and np.isfinite(fy) and fx != 0.0 and fy != 0.0):
        raise ValueError(f"pointcloud: focal lengths must be finite and not zero, got fx={fx} fy={fy}")
    if not (np.isfinite(cx) and np.isfinite(cy)):
        raise ValueError(f"pointcloud: the principal point must be finite, got cx={cx} cy={cy}")
    if max_depth is not None:
        max_depth = float(np.float32(max_depth))
        if not max_depth > 0.0:
            raise ValueError(f"pointcloud: max_depth must be None (keep every pixel) or > 0, got {max_depth}")
    return fx, fy, cx, cy, max_depth


def _check_shapes(depth_shape, depth_dtype, frame_shape, frame_dtype):
    if len(depth_shape) != 3 or 0 in depth_shape or tuple(frame_shape) != tuple(depth_shape) + (3,):
        raise ValueError(f"pointcloud: depths {tuple(depth_shape)} and frames {tuple(frame_shape)} must be [n,H,W] and [n,H,W,3]")
    if str(depth_dtype).replace("torch.", "") != "float32" or str(frame_dtype).replace("torch.", "") != "uint8":
        raise ValueError(f"pointcloud: depths must be float32 and frames uint8, got {depth_dtype} and {frame_dtype}")


# ---------------------------------------------------------------------------------------------------------------- the host twin
def unproject_numpy(depths, frames, fx, fy, cx=None, cy=None, max_depth=None, dtype="float64", device=None):
    """The record bytes of every frame on the host: a list of n uint8 arrays of count * record_size bytes. `device` is ignored."""
    rs = _record_size(dtype)
    depths, frames = np.asarray(depths), np.asarray(frames)
    _check_shapes(depths.shape, depths.dtype, frames.shape, frames.dtype)
    n, h, w = depths.shape
    fx, fy, cx, cy, max_depth = _intrinsics(h, w, fx, fy, cx, cy, max_depth)
    xfac = (np.arange(w, dtype=np.float64) - cx) / fx          # one subtraction and one division per column ...
    yfac = (np.arange(h, dtype=np.float64) - cy) / fy          # ... and per row
    out = []
    for i in range(n):
        z32 = np.asarray(depths[i])
        z = z32.astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            x, y = xfac[None, :] * z, yfac[:, None] * z        # one product per coordinate
        x[np.isnan(x)] = CANONICAL_NAN
        y[np.isnan(y)] = CANONICAL_NAN
        rec = np.empty(h * w, dtype=record_dtype(dtype))
        with np.errstate(over="ignore"):
            rec["x"], rec["y"] = x.ravel(), y.ravel()          # "float32": rounded once here
        rec["z"] = z32.ravel()                                 # float32 -> float64 is exact, float32 -> float32 keeps the bits
        rgb = np.asarray(frames[i]).reshape(-1, 3)
        rec["red"], rec["green"], rec["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
        if max_depth is not None:
            flat = z32.ravel()
            with np.errstate(invalid="ignore"):
                rec = rec[(flat > 0) & (flat <= np.float32(max_depth))]
        b = np.frombuffer(rec.tobytes(), dtype=np.uint8)
        assert b.size == rec.size * rs
        out.append(b)
    return out


# ------------------------------------------------------------------------------------------------------------------ PLY files
def ply_header(count, dtype="float64"):
    """Open3D's binary header for a cloud with points and colours (restated from its published writer), LF line ends."""
    _record_size(dtype)
    t = _PLY_TYPE[dtype]
    return ("ply\nformat binary_little_endian 1.0\ncomment Created by Open3D\n"
            f"element vertex {int(count)}\nproperty {t} x\nproperty {t} y\nproperty {t} z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")


def _as_bytes(records, dtype):
    rs = _record_size(dtype)
    records = np.ascontiguousarray(records).view(np.uint8).reshape(-1)
    if records.size % rs:
        raise ValueError(f"pointcloud: {records.size} bytes are no whole number of {rs}-byte records")
    return records, records.size // rs


def write_ply(path, records, dtype="float64"):
    """The header and the record bytes (uint8, as unproject returns them) as one file; returns the number of vertices."""
    records, count = _as_bytes(records, dtype)
    with open(path, "wb") as f:
        f.write(ply_header(count, dtype).encode("ascii"))
        f.write(memoryview(records))
    return count


def read_ply(path):
    """(points [N,3] float64 or float32, colors uint8 [N,3]) of a file with exactly one of the two layouts of ply_header; anything
    else (another property list, ascii, big endian, faces, a truncated body) is refused."""
    with open(path, "rb") as f:
        blob = f.read()
    end = blob.find(b"end_header\n")
    if not blob.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    header = blob[:end + len(b"end_header\n")].decode("ascii", errors="replace")
    m = re.search(r"^element vertex (\d+)$", header, flags=re.M)
    dtype = next((d for d in RECORD_SIZE if m and header == ply_header(int(m.group(1)), d)), None)
    if dtype is None:
        raise ValueError(f"{path}: not one of the two layouts this module writes (binary little endian, x y z as double or float, "
                         f"red green blue as uchar); header:\n{header}")
    count, body = int(m.group(1)), blob[len(header):]
    if len(body) != count * RECORD_SIZE[dtype]:
        raise ValueError(f"{path}: {count} vertices of {RECORD_SIZE[dtype]} bytes announced, {len(body)} bytes found")
    rec = np.frombuffer(body, dtype=record_dtype(dtype))
    points = np.stack([rec["x"], rec["y"], rec["z"]], axis=-1)
    colors = np.stack([rec["red"], rec["green"], rec["blue"]], axis=-1)
    return points, colors


def frame_name(i):
    return 'point' + str(i).zfill(4) + '.ply'                  # depth_to_pointcloud.py:68


# ------------------------------------------------------------------------------------------------------------------ the device
class _Unprojector:
    """The device buffers for blocks of at most `frames` frames of h x w, and the launch."""

    def __init__(self, frames, h, w, fx, fy, cx, cy, max_depth, dtype, device):
        import torch
        from . import ops, staging
        self.ops, self.torch = ops, torch
        self.rs = _record_size(dtype)
        self.f32 = dtype == "float32"
        self.h, self.w = h, w
        self.fx, self.fy, self.cx, self.cy, self.max_depth = _intrinsics(h, w, fx, fy, cx, cy, max_depth)
        self.device = staging.cuda_device(device, "pointcloud")
        self.stride = ops.pointcloud_frame_stride(h, w, self.f32)
        with torch.cuda.device(self.device):
            self.records = torch.empty(frames * self.stride, dtype=torch.uint8, device=self.device)
            self.counts = torch.empty(frames, dtype=torch.int32, device=self.device)
            self.workspace = torch.empty(ops.pointcloud_workspace_bytes(frames, h, w), dtype=torch.uint8, device=self.device)

    def upload(self, block, dtype):
        torch = self.torch
        if not isinstance(block, torch.Tensor):
            block = torch.from_numpy(np.ascontiguousarray(block))
        return block.to(self.device, dtype=dtype).contiguous()

    def launch(self, depth, rgb):
        """depth [m,h,w] and rgb [m,h,w,3] on the device, m <= frames: the records and counts of the first m slots."""
        self.ops.pointcloud(depth, rgb, self.records, self.counts, self.workspace, self.fx, self.fy, self.cx, self.cy, self.max_depth, self.f32)


def _device_of(depths, frames, device):
    """The device the cuda tensors among depths and frames share; `device` when neither is on one."""
    import torch
    from . import staging
    on_dev = [t for t in (depths, frames) if isinstance(t, torch.Tensor) and t.is_cuda]
    return staging.one_device(on_dev, device, "pointcloud") if on_dev else device


def unproject(depths, frames, fx, fy, cx=None, cy=None, max_depth=None, dtype="float64", device="cuda"):
    """The record bytes of every frame, built on the device: a list of n uint8 numpy arrays of count * record_size bytes, the same
    bytes as unproject_numpy. depths float32 [n,H,W] and frames uint8 [n,H,W,3] are numpy arrays or CUDA tensors."""
    import torch
    _check_shapes(depths.shape, depths.dtype, frames.shape, frames.dtype)
    n, h, w = depths.shape
    dev = _device_of(depths, frames, device)
    u = _Unprojector(n, h, w, fx, fy, cx, cy, max_depth, dtype, dev)
    with torch.cuda.device(u.device):
        u.launch(u.upload(depths, torch.float32), u.upload(frames, torch.uint8))
        counts = u.counts.cpu().tolist()
        return [u.records[i * u.stride:i * u.stride + c * u.rs].cpu().numpy() for i, c in enumerate(counts)]


def write_pointclouds(depths, frames, out_dir, fx, fy, cx=None, cy=None, max_depth=None, dtype="float64", block_frames=8, device="cuda",
                      first_index=0):
    """point0000.ply, point0001.ply, ... in out_dir, one per frame (frame i of this call is file first_index + i); returns the
    vertex counts. Works block_frames frames at a time: the files of one block are written from one of two pinned host buffers while
    the device works on the next block, so depths and frames may be memory maps of a video that does not fit in memory. The files
    do not depend on block_frames."""
    import torch
    _check_shapes(depths.shape, depths.dtype, frames.shape, frames.dtype)
    n, h, w = depths.shape
    B = max(1, min(int(block_frames), n))
    u = _Unprojector(B, h, w, fx, fy, cx, cy, max_depth, dtype, _device_of(depths, frames, device))
    os.makedirs(out_dir, exist_ok=True)
    host = [torch.empty(B * u.stride, dtype=torch.uint8).pin_memory() for _ in range(2)]
    host_counts = [torch.empty(B, dtype=torch.int32).pin_memory() for _ in range(2)]
    landed = [torch.cuda.Event() for _ in range(2)]
    all_counts = []

    def fetch(k, m):
        """Block k's counts and record bytes into pinned buffer k % 2, asynchronously; `landed` marks the end of the copies."""
        if u.max_depth is None:
            host_counts[k % 2][:m].fill_(h * w)                      # known without asking the device
        else:
            host_counts[k % 2][:m].copy_(u.counts[:m], non_blocking=True)
            torch.cuda.current_stream().synchronize()
        for i, c in enumerate(host_counts[k % 2][:m].tolist()):
            span = slice(i * u.stride, i * u.stride + c * u.rs)
            host[k % 2][span].copy_(u.records[span], non_blocking=True)
        landed[k % 2].record()

    def write(k, start, m):
        landed[k % 2].synchronize()
        buf = host[k % 2].numpy()
        for i, c in enumerate(host_counts[k % 2][:m].tolist()):
            write_ply(os.path.join(out_dir, frame_name(first_index + start + i)), buf[i * u.stride:i * u.stride + c * u.rs], dtype)
            all_counts.append(c)

    with torch.cuda.device(u.device):
        pending = None
        for k, start in enumerate(range(0, n, B)):
            m = min(B, n - start)
            u.launch(u.upload(depths[start:start + m], torch.float32), u.upload(frames[start:start + m], torch.uint8))
            if u.max_depth is None:
                fetch(k, m)                   # everything of block k is queued before block k - 1's files are written
            if pending is not None:
                write(*pending)
            if u.max_depth is not None:
                fetch(k, m)                   # needs the counts: block k's kernels ran while block k - 1's files were written
            pending = (k, start, m)
        write(*pending)
    return all_counts
