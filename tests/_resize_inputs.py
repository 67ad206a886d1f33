"""Shapes, inputs and the independent yardstick shared by the resize tests (tests/test_resize_numpy.py, tests/test_resize_gpu.py)."""
import numpy as np

# (planes, (h, w), (H, W))
SHAPES = [
    (3, (5, 7), (8, 11)),                   # up, non-integer ratio
    (3, (13, 17), (6, 5)),                  # down by more than 2: taps skip pixels
    (2, (1, 1), (4, 3)),                    # one-pixel axes: every column and row clamped
    (2, (3, 1), (7, 5)),
    (3, (4, 6), (4, 9)),                    # one axis is the identity
    (3, (16, 20), (15, 19)),                # near-identity ratio: coordinates land near integers
    (2, (480, 640), (464, 618)),            # scannet's own sizes: the fp32 rounding of coordinates up to 640 matters
    (2, (374, 1242), (187, 621)),           # kitti's size halved: coordinates are exact half-integers
]
IDS = ["{}x{}-to-{}x{}".format(*a, *b) for _, a, b in SHAPES]
_inputs = {}


def planes(n, hw):
    """Seeded, finite, uniform in [0.1, 20]; made once per shape and read-only."""
    key = (n,) + tuple(hw)
    if key not in _inputs:
        rng = np.random.default_rng(1000 * hw[0] + hw[1])
        a = rng.uniform(0.1, 20.0, size=key).astype(np.float32)
        a.setflags(write=False)
        _inputs[key] = a
    return _inputs[key]


def yardstick(src, size):
    """Bilinear interpolation with replicated borders at the exact fp64 coordinates (d + 0.5) * n_src / n_dst - 0.5, by
    scipy.ndimage.map_coordinates on the float64 planes: shares no code and no rounding with the twin."""
    from scipy.ndimage import map_coordinates
    n, h, w = src.shape
    H, W = size
    ys = (np.arange(H, dtype=np.float64) + 0.5) * h / H - 0.5
    xs = (np.arange(W, dtype=np.float64) + 0.5) * w / W - 0.5
    grid = np.meshgrid(ys, xs, indexing="ij")
    return np.stack([map_coordinates(p.astype(np.float64), grid, order=1, mode="nearest") for p in src])


def bound(src):
    """|out - yardstick| <= 2 * 2^-24 * max(h, w) * (max src - min src) + 2^-20 * max |src|. First term: the fp32 rounding of a
    coordinate is at most 2^-24 * |coordinate| and moves the weight by that much, on each axis. Second term: at most eight fp32
    roundings of values no larger than the largest tap give 8 * 2^-24 = 2^-21; doubled."""
    n, h, w = src.shape
    return 2.0 * 2.0 ** -24 * max(h, w) * float(src.max() - src.min()) + 2.0 ** -20 * float(np.abs(src).max())
