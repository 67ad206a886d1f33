"""Seeded small frames shared by the CPU and GPU tests of the Motion-JPEG encoder, and the host twin's streams for them (computed
once per process). The shapes are the smallest that reach every path: one block; both edges ragged with two frames of different
compressed length; ten one-MCU restart intervals, so that the RSTm counter wraps past 7; several intervals of 17 MCUs over three
frames, the last tile column inside a workgroup's third chunk of 8 tiles; gray."""
import functools

import numpy as np

SHAPES = [(1, 8, 8, 3), (2, 17, 23, 3), (1, 80, 8, 3), (3, 40, 136, 3), (2, 24, 40)]
CONTENTS = ["flat", "ramp", "noise", "checker", "impulses"]
QUALITIES = [50, 90, 100]
CASES = [(s, c, q) for s in SHAPES for c in CONTENTS for q in QUALITIES]


def case_id(case):
    shape, content, q = case
    return "x".join(map(str, shape)) + f"-{content}-q{q}"


@functools.lru_cache(maxsize=None)
def frames(shape, content):
    """uint8 frames of `shape` ([N,H,W,3] or [N,H,W]); read-only."""
    from video_depth_anything_amd import visualize
    # (the single block's seed is picked so that its noise has a stuffed FF at quality 100: test_mjpeg_numpy.py asserts it)
    rng = np.random.default_rng(0 if shape == SHAPES[0] else sum(shape) * 131 + CONTENTS.index(content))
    n, h, w = shape[:3]
    gray = len(shape) == 3
    if content == "flat":                                   # white, then darker per frame: the first DC difference of a row is the largest there is
        out = np.empty(shape, np.uint8)
        for i in range(n):
            out[i] = 255 - 40 * i
    elif content == "ramp":                                 # a diagonal depth ramp through the reference's colour table, shifted per frame
        d = (np.add.outer(np.arange(h), np.arange(w))[None] + 3.0 * np.arange(n)[:, None, None]).astype(np.float32)
        out = visualize.colorize_numpy(d, grayscale=gray)
    elif content == "noise":
        out = rng.integers(0, 256, shape, dtype=np.uint8)
    elif content == "checker":                              # 0 / 255 from pixel to pixel: the largest AC coefficient there is
        c = ((np.add.outer(np.arange(h), np.arange(w)) + np.arange(n)[:, None, None]) & 1).astype(np.uint8) * 255
        out = c if gray else np.repeat(c[..., None], 3, axis=-1)
    else:                                                   # a few single bright or dark pixels on mid-gray ground
        out = np.full(shape, 120, np.uint8)
        for _ in range(max(2, n * h * w // 48)):
            i, y, x = rng.integers(n), rng.integers(h), rng.integers(w)
            out[i, y, x] = rng.choice([0, 255], size=() if gray else (3,))
    out = np.ascontiguousarray(out)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(shape, content, quality):
    """(list of JPEG bytes, coverage record) of the host twin."""
    from video_depth_anything_amd import mjpeg
    cover = mjpeg.new_coverage()
    return mjpeg.encode_jpeg_numpy(frames(shape, content), quality, coverage=cover), cover


def psnr(a, b):
    mse = np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)
    return np.inf if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)
