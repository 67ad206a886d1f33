"""Seeded inputs shared by the point-cloud tests (tests/test_pointcloud_numpy.py, tests/test_pointcloud_gpu.py): made once per shape
and read-only.

Depths are float32 in (0, 20) with exact zeros, negatives, NaN and +Inf sprinkled in (one of each per dozen pixels, where the frame
has that many) and +Inf on the centre pixel, where the default principal point of an even size makes the column or row factor
exactly 0 and the product 0 * Inf. Colours are random uint8 and include 0 and 255. fx = 470.4 and fy = 391.7: every division is
inexact."""
import numpy as np

FX, FY = 470.4, 391.7
MAX_DEPTH = 10.0
TILE = 256                                   # pixels of one workgroup of csrc/pointcloud.hip (PC_T)
# 7 x 37 = 259 is one workgroup plus 3, 16 x 16 exactly one, 33 x 31 has an odd width and a ragged tail, (2,23,45) has two frames
# whose H * W * 27 is no multiple of 4 (slots are independent), (3,36,64) has nine whole workgroups per frame
SHAPES = [(1, 1, 1), (1, 3, 5), (1, 7, 37), (1, 16, 16), (1, 33, 31), (2, 23, 45), (3, 36, 64)]
IDS = ["{}x{}x{}".format(*s) for s in SHAPES]
DTYPES = ["float64", "float32"]
RECORD_SIZE = {"float64": 27, "float32": 15}
PATTERNS = ["as_is", "none", "all", "alternating", "hole", "last"]
_cases = {}


def case(n, h, w):
    """(depths float32 [n,h,w], frames uint8 [n,h,w,3])."""
    key = (n, h, w)
    if key not in _cases:
        rng = np.random.default_rng(100000 * n + 1000 * h + w)
        d = rng.uniform(0.01, 20.0, size=key).astype(np.float32)
        flat = d.reshape(-1)
        order = rng.permutation(flat.size)
        for j, v in enumerate((0.0, -1.5, np.nan, np.inf)):
            flat[order[j::12]] = v                       # for a tiny frame the later values win
        if h * w > 1:
            d[:, h // 2, w // 2] = np.inf
        rgb = rng.integers(0, 256, size=key + (3,), dtype=np.uint8)
        if h * w > 1:
            rgb[:, 0, 0], rgb[:, -1, -1] = (0, 255, 0), (255, 0, 255)
        d.setflags(write=False), rgb.setflags(write=False)
        _cases[key] = (d, rgb)
    return _cases[key]


def with_pattern(depths, kind):
    """A copy of `depths` overwritten so that max_depth = 10 keeps a chosen set of pixels (kept: 0 < z <= 10).
    as_is: the seeded depths, about half of them kept at random. none: nothing. all: everything (z == max_depth among them).
    alternating: every other pixel, less k + 1 of them in workgroup k, so that the workgroups' output offsets fall on different
    residues modulo 4 and 16 (exactly every other pixel would put each on a multiple of 128 * 27 = 216 * 16 bytes).
    hole: the range of one whole workgroup in the middle dropped (the second, where a frame has three). last: the last pixel only."""
    n, h, w = depths.shape
    d = np.array(depths)
    flat = d.reshape(n, -1)
    kept = np.float32(0.5) + (np.arange(h * w) % 19).astype(np.float32) * np.float32(0.5)      # 0.5 .. 9.5
    dropped = np.array([0.0, -2.0, np.nan, np.inf, 10.000001, 15.0], np.float32)[np.arange(h * w) % 6]
    if kind == "as_is":
        return d
    if kind == "none":
        flat[:] = dropped
    elif kind == "all":
        flat[:] = kept
        flat[:, ::3] = MAX_DEPTH
    elif kind == "alternating":
        p = np.arange(h * w)
        keep = p % 2 == 0
        keep &= ~((p % TILE) < 2 * (p // TILE + 1))
        flat[:] = np.where(keep, kept, dropped)
    elif kind == "hole":
        flat[:] = kept
        lo = TILE if h * w >= 3 * TILE else 0
        flat[:, lo:lo + TILE] = dropped[lo:lo + TILE]
    elif kind == "last":
        flat[:] = dropped
        flat[:, -1] = 7.25
    else:
        raise ValueError(kind)
    return d


def keep_mask(depths):
    with np.errstate(invalid="ignore"):
        return (depths > 0) & (depths <= np.float32(MAX_DEPTH))
