"""Frames larger than `max_res` scaled down as the reference's cv2 branch scales them (utils/dc_utils.py there:
cv2.resize(frame, (width, height)) on uint8 frames), on the device (csrc/resize_u8.hip).

The contract is `resize_frames_numpy`: cv2's INTER_LINEAR for 8-bit images restated from its published algorithm (OpenCV
modules/imgproc/src/resize.cpp, resizeGeneric_ with HResizeLinear<uchar,int,short> / VResizeLinear<uchar,int,short>). The source
coordinates and the two border rules are evaluate.resize_prediction_numpy's (one fp64 expression rounded once to float32; columns
zero the weight at the border, rows clamp the indices); everything behind them is integer arithmetic:

  weights   a0 = 1.f - fx, a1 = fx, b0 = 1.f - fy, b1 = fy, each the 16-bit integer rint(a * 2048.f), half to even, saturated
  columns   T = S[x0] * a0 + S[x1] * a1                                                 int32, at most 255 * 2048
  rows      out = (((b0 * (T0 >> 4)) >> 16) + ((b1 * (T1 >> 4)) >> 16) + 2) >> 2        nothing negative, nothing wraps

so the device reproduces it byte for byte. Equal sizes give the input back; an exact halving of both axes gives
(p00 + p01 + p10 + p11 + 2) >> 2. cv2 is not importable here: parity with a cv2 build is not pinned.
"""
import numpy as np

from . import staging
from .evaluate import _axis_taps

COEF_ONE = 2048                              # cv2's INTER_RESIZE_COEF_SCALE = 1 << 11
_BLOCK_BYTES = 1 << 26                       # source bytes staged at a time by resize_frames' numpy path


def scaled_size(h, w, max_res):
    """(H, W) of an h x w frame under `max_res`, the reference's cv2-branch rule: scale = max_res / max(h, w), each side rounded
    (python's round: a .5 goes to the even neighbour). (h, w) itself when nothing is to be scaled."""
    if max_res > 0 and max(h, w) > max_res:
        scale = max_res / max(h, w)
        return round(h * scale), round(w * scale)
    return h, w


def _coefficients(a):
    """cv2's saturate_cast<short>(a * 2048.f) of a float32 array: rint (half to even), saturated."""
    return np.clip(np.rint(a * np.float32(COEF_ONE)), -32768, 32767).astype(np.int32)


def _check(frames, H, W, who):
    shape, dtype = tuple(frames.shape), str(frames.dtype).replace("torch.", "")
    if dtype != "uint8":
        raise TypeError(f"{who}: frames must be uint8, got {frames.dtype}")
    if len(shape) not in (3, 4) or (len(shape) == 4 and shape[3] != 3) or 0 in shape or H < 1 or W < 1:
        raise ValueError(f"{who}: frames must be a non-empty [N,h,w,3] or [N,h,w] and the size positive, got {shape} to {(H, W)}")


def resize_frames_numpy(frames, H, W):
    """uint8 [N,h,w,3] (or [N,h,w]) -> uint8 [N,H,W,3] (or [N,H,W]): the contract, in numpy integers, a frame at a time."""
    frames = frames if isinstance(frames, np.ndarray) else np.asarray(frames)
    H, W = int(H), int(W)
    _check(frames, H, W, "resize_frames_numpy")
    h, w = frames.shape[1:3]
    one = np.float32(1.0)
    x0, fx = _axis_taps(w, W)
    fx = np.where((x0 < 0) | (x0 >= w - 1), np.float32(0.0), fx)           # columns: the weight is zeroed at the border ...
    x0 = np.clip(x0, 0, w - 1)
    x1 = np.minimum(x0 + 1, w - 1)                                          # ... and only tap x0 is read at the right one
    sy, fy = _axis_taps(h, H)                                               # rows: the fraction stays, the indices are clamped
    y0, y1 = np.clip(sy, 0, h - 1), np.clip(sy + 1, 0, h - 1)
    tail = (1,) * (frames.ndim - 3)                                         # the channel axis, when there is one
    a0, a1 = _coefficients(one - fx).reshape((1, W) + tail), _coefficients(fx).reshape((1, W) + tail)
    b0, b1 = _coefficients(one - fy).reshape((H, 1) + tail), _coefficients(fy).reshape((H, 1) + tail)
    out = np.empty((frames.shape[0], H, W) + frames.shape[3:], np.uint8)
    for i, f in enumerate(frames):
        s = f.astype(np.int32)
        t = s[:, x0] * a0 + s[:, x1] * a1                                   # [h,W(,3)]
        v = (((b0 * (t[y0] >> 4)) >> 16) + ((b1 * (t[y1] >> 4)) >> 16) + 2) >> 2
        assert v.min() >= 0 and v.max() <= 255
        out[i] = v
    return out


def resize_frames(frames, H, W, device="cuda"):
    """resize_frames_numpy's bytes from the device (vda_resize_linear_u8). A cuda uint8 tensor gives a cuda tensor on its device and
    stream. A numpy array or memory map gives a numpy array: the frames are staged a block at a time on `device`, so only a block of
    the source is ever on the device. Anything but uint8, a host tensor or a device that is not cuda is an error: there is no CPU
    path behind this name."""
    import torch
    if not isinstance(frames, (torch.Tensor, np.ndarray)):
        frames = np.asarray(frames)
    H, W = int(H), int(W)
    _check(frames, H, W, "resize_frames")
    is_tensor, dev = staging.placement(frames, device, "resize_frames", "resize_frames_numpy")
    from . import ops
    n, (h, w), tail = frames.shape[0], frames.shape[1:3], tuple(frames.shape[3:])
    with torch.cuda.device(dev):
        b = n if is_tensor else staging.frames_per_block(n, h * w * (3 if tail else 1), _BLOCK_BYTES)      # frames per call
        dev_out = torch.empty((b, H, W) + tail, dtype=torch.uint8, device=dev)
        if is_tensor:
            ops.resize_linear_u8(frames.contiguous(), dev_out)
            return dev_out
        out = np.empty((n, H, W) + tail, np.uint8)
        for i, m, x in staging.Staged(b, (h, w) + tail, torch.uint8, dev).blocks(frames):
            ops.resize_linear_u8(x, dev_out[:m])
            out[i:i + m] = dev_out[:m].cpu().numpy()
        return out
