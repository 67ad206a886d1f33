"""Seeded uint8 frames for the 8-bit resize tests (tests/test_resize_u8_numpy.py, tests/test_resize_u8_gpu.py)."""
import numpy as np


def frames(n, h, w, c=3, seed=0):
    """uint8 [n,h,w,3] (c = 3) or [n,h,w] (c = 1) of noise: every frame differs, so a wrong plane index shows."""
    shape = (n, h, w) + ((3,) if c == 3 else ())
    return np.random.default_rng([seed, n, h, w, c]).integers(0, 256, size=shape, dtype=np.uint8)


def checkerboard(n, h, w, c=3):
    """0 / 255 alternating per pixel: the largest steps the intermediate sums can see."""
    board = (((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1) * 255).astype(np.uint8)
    x = np.broadcast_to(board[None, :, :, None], (n, h, w, 3)) if c == 3 else np.broadcast_to(board[None], (n, h, w))
    return np.ascontiguousarray(x)


def clip(n, h, w):
    """A smooth moving scene that JPEG codes well: uint8 [n,h,w,3]."""
    y, x = np.mgrid[0:h, 0:w]
    out = np.empty((n, h, w, 3), np.uint8)
    for i in range(n):
        out[i, ..., 0] = (x * 3 + i * 11) % 256
        out[i, ..., 1] = (y * 5 + i * 7) % 256
        out[i, ..., 2] = ((x + y) * 2 + i * 29) % 256
    return out
