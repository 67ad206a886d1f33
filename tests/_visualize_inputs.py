"""Seeded inputs shared by the visualisation tests (tests/test_visualize_numpy.py, tests/test_visualize_gpu.py) and by
tools/gen_vis_golden.py, which runs the reference's save_video on cases A-C and records what its writer received in
tests/golden/vis_frames.npz. Made once and read-only.

A: random depth in [0.3, 7.3], 3 x 37 x 53: a frame of 1961 pixels starts at no multiple of 4 bytes in either output.
B: the boundary ramp, [2, 16, 32]: every integer k in 0..255 and nextafter(k, -inf) for k >= 1, padded with repeats; the range is
   [0, 255], so every quotient boundary k / 255 is hit exactly and just below, and every table row is used (255 at the maximum only).
C: a narrow metric-style range, values in [5, 5.001], 2 x 9 x 11: span is 1e-3 and the subtraction cancels most of the bits.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vis_frames.npz")
CASES = ["A", "B", "C"]
# sizes of the flat kernel tests: below one group of four, 5 883 = 3 * 37 * 53, and past one pass of the capped grid
# (csrc/visualize.hip: 2048 workgroups x 256 threads x 4 pixels = 2^21 pixels, less a head of up to 3)
ONE_PASS = 2048 * 256 * 4
SMALL_SIZES = [1, 2, 3, 5, 7, 5883]
LARGE_SIZES = [(1 << 20) + 3, ONE_PASS + 7]
_made = {}


def _frozen(a):
    a.setflags(write=False)
    return a


def case_a():
    return np.random.default_rng(0).uniform(0.3, 7.3, (3, 37, 53)).astype(np.float32)


def case_b():
    k = np.arange(256, dtype=np.float32)
    below = np.nextafter(k[1:], np.float32(-np.inf), dtype=np.float32)
    vals = np.concatenate([k, below])                                   # 511 values
    vals = np.concatenate([vals, vals, vals[:2]])                       # 1024: padded with repeats
    return vals.reshape(2, 16, 32)


def case_c():
    d = np.random.default_rng(2).uniform(5.0, 5.001, (2, 9, 11)).astype(np.float32)
    d[0, 0, 0], d[1, -1, -1] = 5.0, 5.001                               # the ends of the range themselves
    return d


def case(name):
    """The float32 [N,H,W] depth of case A, B or C."""
    if name not in _made:
        _made[name] = _frozen({"A": case_a, "B": case_b, "C": case_c}[name]())
    return _made[name]


def flat(n, seed=7):
    """n float32 pixels in [0.3, 7.3] with both ends present (for n >= 2): the range does not depend on the seed."""
    key = ("flat", n, seed)
    if key not in _made:
        d = np.random.default_rng(seed).uniform(0.3, 7.3, n).astype(np.float32)
        d[0] = 0.3
        d[-1] = 7.3 if n > 1 else 0.3
        _made[key] = _frozen(d)
    return _made[key]


def specials():
    """37 pixels for a GIVEN range [1, 3]: NaN, +-inf, values outside the range on both sides, the ends, -0.0, and plain ones."""
    key = "specials"
    if key not in _made:
        d = np.linspace(0.5, 3.5, 37).astype(np.float32)
        d[[0, 5, 11, 17, 23, 29, 36]] = [np.nan, np.inf, -np.inf, 1.0, 3.0, -0.0, 1e30]
        d[2], d[3] = np.nextafter(np.float32(1.0), np.float32(0)), np.nextafter(np.float32(3.0), np.float32(4))
        _made[key] = _frozen(d)
    return _made[key]


SPECIALS_RANGE = (1.0, 3.0)


def specials_levels():
    """What the contract says of specials() in [1, 3], written out by hand for the special pixels (the rest are checked against
    the twin): NaN -> 0, +inf -> 255, -inf -> 0, the minimum -> 0, the maximum -> 255, below -> 0, above -> 255."""
    return {0: 0, 5: 255, 11: 0, 17: 0, 23: 255, 29: 0, 36: 255, 2: 0, 3: 255, 1: 0, 35: 255}


def random_table(seed=11):
    """A palette that is not inferno: every byte of every row is told apart."""
    key = ("table", seed)
    if key not in _made:
        _made[key] = _frozen(np.random.default_rng(seed).integers(0, 256, (256, 3), dtype=np.uint8))
    return _made[key]


def golden():
    if "golden" not in _made:
        _made["golden"] = {k: _frozen(v) for k, v in np.load(GOLDEN).items()}
    return _made["golden"]
