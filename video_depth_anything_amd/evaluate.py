"""Score a depth video against ground truth: the second stage of the reference's benchmark
(benchmark/eval/eval.py:67-122 and metric.py there) on the device.

    valid   = (gt > 1e-3) & (gt < max_depth)
    x       = clip(pred, 1e-3)                                        float32
    scale, shift = argmin || scale * x + shift - 1 / (gt + 1e-8) ||   fp64, over every valid pixel of the whole video
    p       = clip(1 / clip(scale * x + shift, 1e-3), 1e-3, max_depth)
    per frame with a valid pixel: abs_rel, sq_rel, rmse, delta1..3; each metric is the mean over those frames

`evaluate_depth` runs that as two streaming reductions of csrc/eval.hip (vda_eval_*): fp64 partial rows, a fixed combination
order, no atomics, scale and shift never leave the device between the passes, one small device-to-host copy at the end.
`evaluate_depth_numpy` restates the same arithmetic on the host for the CPU-side tests (as scheduler.py carries a numpy
stitcher); `evaluate_depth` never calls it - there is no CPU path.

dtype rules (they decide the last bits): a float32 ground truth stays float32 and is widened exactly; an integer ground truth
divided by its factor is float64. So `gt` may be float32 or float64 and is never narrowed. The validity comparisons happen in
gt's own type, as numpy compares an array with a python scalar. The delta ratios are float32 count / n, everything else fp64.

`resize_prediction` is the reference's answer to a prediction that is not at the ground truth's size (eval.py: get_infer's
cv2.resize(infer, (W, H)); eval_tae.py after its optional hard crop): cv2's INTER_LINEAR for float32 on the device (csrc/resize.hip,
vda_resize_linear_f32; the contract is in DESIGN.md 6c). Both scorers apply it with `resize=True`, to the raw prediction before
anything else, chunk by chunk. `resize_prediction_numpy` is its host twin for the CPU tests, bit for bit.

`evaluate_tae` is the benchmark's third stage (benchmark/eval/eval_tae.py there), the temporal alignment error: the same fit, then
for every pair of neighbouring frames and both directions the aligned depth of one frame is unprojected with K, moved with the
relative pose, splatted LAST-WINS into the other frame's grid and compared with that frame's aligned depth (csrc/tae.hip,
vda_tae_*; the contract is in DESIGN.md 6d). `evaluate_tae_numpy` is its host twin for the CPU tests.
"""
import numpy as np

from .staging import cuda_device, one_device

METRICS = ("abs_relative_difference", "squared_relative_difference", "rmse_linear", "delta1_acc", "delta2_acc", "delta3_acc")
EVAL_T = 256                 # threads per block of the two passes (csrc/eval.hip EV_T)
LSQ_MAX_BLOCKS = 1024        # pass 1: blocks per call
METRIC_MAX_BLOCKS = 64       # pass 2: blocks per frame
_D1, _D2, _D3 = 1.25, 1.25 ** 2, 1.25 ** 3


def _axis_taps(n_src, n_dst):
    """One axis of cv2's INTER_LINEAR for float32: (floor of the source coordinate as int64, its fraction as float32), before any
    border rule. The coordinate is fp64 and rounded once to float32."""
    scale = 1.0 / (float(n_dst) / float(n_src))
    c = ((np.arange(n_dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    fl = np.floor(c)
    return fl.astype(np.int64), c - fl


def resize_prediction_numpy(pred, size):
    """Host twin of resize_prediction: the same operations in numpy float32 (fp64 only for the coordinates), the same bits.
    pred float32 [N,h,w], size (H, W) -> float32 [N,H,W]. For tests; not a product path."""
    pred = np.asarray(pred)
    H, W = (int(v) for v in size)
    if pred.dtype != np.float32 or pred.ndim != 3 or pred.size == 0 or H < 1 or W < 1:
        raise ValueError(f"resize_prediction_numpy: pred must be a non-empty float32 [N,h,w] and size positive, got {pred.dtype} {pred.shape} to {(H, W)}")
    h, w = pred.shape[1:]
    if (H, W) == (h, w):
        return pred
    one = np.float32(1.0)
    x0, fx = _axis_taps(w, W)
    fx = np.where((x0 < 0) | (x0 >= w - 1), np.float32(0.0), fx)           # columns: the weight is zeroed at the border ...
    x0 = np.clip(x0, 0, w - 1)
    x1 = np.minimum(x0 + 1, w - 1)                                          # ... and only tap x0 is read at the right one
    sy, fy = _axis_taps(h, H)                                               # rows: the fraction stays, the indices are clamped
    y0, y1 = np.clip(sy, 0, h - 1), np.clip(sy + 1, 0, h - 1)
    a0, a1 = one - fx, fx
    b0, b1 = (one - fy)[:, None], fy[:, None]
    hor = pred[:, :, x0] * a0 + pred[:, :, x1] * a1                         # [N,h,W]: three float32 roundings
    out = hor[:, y0] * b0 + hor[:, y1] * b1
    assert out.dtype == np.float32
    return out


def resize_prediction(pred, size, device="cuda"):
    """`pred` (float32 [N,h,w], a numpy array or a CUDA tensor) resized to size = (H, W) as the reference's scorers resize a
    prediction, cv2.resize(infer, (W, H)): INTER_LINEAR on float32, in one kernel (csrc/resize.hip). Returns a CUDA tensor [N,H,W];
    size == (h, w) returns the input unchanged apart from the upload, as the reference calls cv2 only on a mismatch. Runs on the
    current stream of the device."""
    import torch
    from . import ops

    if not isinstance(pred, torch.Tensor):
        pred = torch.from_numpy(np.asarray(pred))
    H, W = (int(v) for v in size)
    if pred.dtype != torch.float32 or pred.ndim != 3 or pred.numel() == 0 or H < 1 or W < 1:
        raise ValueError(f"resize_prediction: pred must be a non-empty float32 [N,h,w] and size positive, got {pred.dtype} {tuple(pred.shape)} to {(H, W)}")
    dev = pred.device if pred.is_cuda else cuda_device(device, "resize_prediction")
    with torch.cuda.device(dev):
        x = pred.to(dev).contiguous()
        if (H, W) == tuple(x.shape[1:]):
            return x
        out = torch.empty((x.shape[0], H, W), dtype=torch.float32, device=dev)
        ops.resize_linear(x, out)
    return out


def _check_pair(pred, gt, max_eval_len, resize=False):
    """Common argument checks; returns (pred[:L], gt[:L]), both [N,H,W] - of one shape, or with `resize` of one N."""
    if pred.ndim != 3 or gt.ndim != 3:
        raise ValueError(f"evaluate_depth: pred and gt must be [N,H,W], got {tuple(pred.shape)} and {tuple(gt.shape)}")
    if max_eval_len is not None:
        pred, gt = pred[:max_eval_len], gt[:max_eval_len]
    if resize and pred.shape[0] != gt.shape[0]:
        raise ValueError(f"evaluate_depth: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ in the number of frames")
    if tuple(pred.shape) != tuple(gt.shape) and not resize:
        raise ValueError(f"evaluate_depth: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ in shape. The reference resizes a "
                         "mismatched prediction with cv2.resize; resizing is not part of this scorer - write the prediction at the "
                         "(cropped) ground-truth size")
    if pred.shape[0] == 0 or pred.shape[1] * pred.shape[2] == 0 or gt.shape[1] * gt.shape[2] == 0:
        raise ValueError("evaluate_depth: empty video")
    return pred, gt


def _result(fit, res):
    out = {k: float(v) for k, v in zip(METRICS, res[:6])}
    out["scale"], out["shift"] = float(fit[0]), float(fit[1])
    out["n_valid"], out["n_frames_used"] = int(fit[2]), int(res[6])
    return out


def evaluate_depth_numpy(pred, gt, max_depth, max_eval_len=None, resize=False):
    """Host twin of evaluate_depth: the same arithmetic in numpy, normal equations in fp64. For tests; not a product path."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    if pred.dtype != np.float32 or gt.dtype not in (np.float32, np.float64):
        raise ValueError(f"evaluate_depth_numpy: pred must be float32 and gt float32 or float64, got {pred.dtype} and {gt.dtype}")
    pred, gt = _check_pair(pred, gt, max_eval_len, resize)
    pred = resize_prediction_numpy(pred, gt.shape[1:])                  # the identity unless `resize` let a mismatch through
    hi = gt.dtype.type(max_depth)
    valid = (gt > gt.dtype.type(1e-3)) & (gt < hi)
    xc = np.clip(pred, np.float32(1e-3), None)
    g = gt.astype(np.float64)
    x = xc[valid].astype(np.float64)
    y = 1.0 / (g[valid] + 1e-8)
    n = float(x.size)
    a01, a00, b1, b0 = x.sum(), (x * x).sum(), y.sum(), (x * y).sum()
    det = a00 * n - a01 * a01
    nan = float("nan")
    scale, shift = ((n * b0 - a01 * b1) / det, (a00 * b1 - a01 * b0) / det) if (n >= 2 and det != 0.0) else (nan, nan)
    with np.errstate(all="ignore"):
        aligned = np.clip(scale * xc.astype(np.float64) + shift, 1e-3, None)
        p = np.clip(1.0 / aligned, 1e-3, float(max_depth))
        gs = np.where(valid, g, 1.0)
        d = np.where(valid, p - gs, 0.0)
        r = np.maximum(p / gs, gs / p)
    nf = valid.sum((1, 2))
    used = nf > 0
    if not used.any():
        return _result((scale, shift, n), [nan] * 6 + [0])
    nu = nf[used].astype(np.float64)
    res = [((np.abs(d) / gs).sum((1, 2))[used] / nu).mean(), ((d * d) / gs).sum((1, 2))[used] / nu, np.sqrt((d * d).sum((1, 2))[used] / nu).mean()]
    res[1] = res[1].mean()
    for thr in (_D1, _D2, _D3):
        cnt = ((r < thr) & valid).sum((1, 2))[used]
        res.append((cnt.astype(np.float32) / nf[used].astype(np.float32)).astype(np.float64).mean())
    return _result((scale, shift, n), res + [int(used.sum())])


# ---------------------------------------------------------------------------------------------- host steps the device scorers share
def _as_tensor(a, name, dtypes, what):
    import torch

    if not isinstance(a, torch.Tensor):
        a = torch.from_numpy(np.asarray(a))
    if a.dtype not in dtypes:
        raise ValueError(f"{what}: {name} must be {' or '.join(str(d) for d in dtypes)}, got {a.dtype}")
    return a


def _chunk_feeds(pred, gt, dev, size):
    """(pred_chunk, gt_chunk): frames lo .. hi-1 on the device, the prediction at gt's `size` (deterministic: the same bits every pass)."""
    on_device = lambda t, lo, hi: t[lo:hi].to(dev, non_blocking=False).contiguous()  # noqa: E731
    return (lambda lo, hi: resize_prediction(on_device(pred, lo, hi), size)), (lambda lo, hi: on_device(gt, lo, hi))


def _fit_chunks(N, step, px):
    """Pass 1's calls over N frames, `step` at a time: (lo, hi, blocks); a block leaves one partial row of 5 doubles."""
    return [(lo, min(lo + step, N), min(LSQ_MAX_BLOCKS, -(-min(step, N - lo) * px // EVAL_T))) for lo in range(0, N, step)]


def _fit_scale_shift(ops, chunks, pred_chunk, gt_chunk, max_depth, work, fit):
    """Pass 1 over `chunks` (their rows one after the other in `work`) and its finisher: fit = {scale, shift, n_valid} on the device.
    `ops` is the kernel binding module its caller has imported already (a relative import per call costs microseconds)."""
    row = 0
    for lo, hi, nb in chunks:
        ops.eval_lsq_partial(pred_chunk(lo, hi), gt_chunk(lo, hi), max_depth, work, row, nb)
        row += nb
    ops.eval_lsq_finish(work, row, fit)


def evaluate_depth(pred, gt, max_depth, max_eval_len=None, device="cuda", chunk_frames=None, resize=False):
    """Metrics of `pred` (float32 [N,H,W]) against `gt` (float32 or float64 [N,H,W]) on the device; numpy arrays or CUDA tensors.
    Device-resident tensors are used in place; host arrays are uploaded `chunk_frames` frames at a time (all at once when None), once
    per pass. With `resize`, a prediction [N,h,w] at another size is resized to gt's grid first (resize_prediction), chunk by chunk
    in both passes: the resized video is never resident as a whole and never returns to the host. Returns a dict: the six METRICS,
    scale, shift, n_valid, n_frames_used. Runs on the current stream of the device."""
    import torch
    from . import ops

    pred = _as_tensor(pred, "pred", (torch.float32,), "evaluate_depth")
    gt = _as_tensor(gt, "gt", (torch.float32, torch.float64), "evaluate_depth")
    pred, gt = _check_pair(pred, gt, max_eval_len, resize)
    dev = one_device((pred, gt), device, "evaluate_depth")
    N, H, W = gt.shape
    px = H * W
    step = N if chunk_frames is None else int(chunk_frames)
    if step <= 0:
        raise ValueError("evaluate_depth: chunk_frames must be positive")
    chunks = _fit_chunks(N, step, px)
    bpf = min(METRIC_MAX_BLOCKS, -(-px // EVAL_T))
    max_depth = float(max_depth)

    with torch.cuda.device(dev):
        work = torch.empty(max(5 * sum(nb for _, _, nb in chunks), 7 * N * bpf), dtype=torch.float64, device=dev)
        out = torch.empty(10, dtype=torch.float64, device=dev)          # fit {scale, shift, n_valid} | result[7]
        fit, res = out[:3], out[3:]
        pred_chunk, gt_chunk = _chunk_feeds(pred, gt, dev, (H, W))
        _fit_scale_shift(ops, chunks, pred_chunk, gt_chunk, max_depth, work, fit)
        for lo, hi, _ in chunks:
            ops.eval_metric_partial(pred_chunk(lo, hi), gt_chunk(lo, hi), max_depth, fit, work, lo, bpf)
        ops.eval_metric_finish(work, N, bpf, res)
        host = out.cpu().numpy()                                        # the one device-to-host copy (synchronises)
    return _result(host[:3], host[3:])


# ---------------------------------------------------------------------------------------------- temporal alignment error
TAE_MAX_BLOCKS = 64          # compare pass: blocks per (pair, direction) plane
TAE_PX_PER_BLOCK = 4 * EVAL_T
TAE_FIT_FRAMES = 8           # frames per call of the fit's pass 1: fixed, so that scale / shift do not depend on chunk_pairs


def _host64(a, name, tail):
    """K / poses as float64 numpy, whatever they came as; K [3,3] is left for the caller to broadcast."""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    a = np.asarray(a, dtype=np.float64)
    if a.shape[-2:] != tail or a.ndim not in ((2, 3) if name == "K" else (3,)):
        raise ValueError(f"evaluate_tae: {name} must be [N,{tail[0]},{tail[1]}]" + (" or [3,3]" if name == "K" else "") + f", got {a.shape}")
    return a


def _check_tae(pred, gt, K, poses, mask, resize=False):
    """Argument checks shared by evaluate_tae and its twin; returns the cameras of _tae_cameras. The mask is at gt's size."""
    if resize and pred.ndim == 3 and gt.ndim == 3 and pred.shape[0] != gt.shape[0]:
        raise ValueError(f"evaluate_tae: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ in the number of frames")
    mismatch = tuple(pred.shape) != tuple(gt.shape) and not (resize and pred.ndim == 3 and gt.ndim == 3)
    if pred.ndim != 3 or gt.ndim != 3 or mismatch:
        raise ValueError(f"evaluate_tae: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} must be equal [N,H,W]. The reference resizes a "
                         "mismatched prediction with cv2.resize; resizing is not part of this scorer - write the prediction at the "
                         "(cropped) ground-truth size")
    N = pred.shape[0]
    if N < 2 or pred.shape[1] * pred.shape[2] == 0 or gt.shape[1] * gt.shape[2] == 0:
        raise ValueError(f"evaluate_tae: needs at least two non-empty frames, got {tuple(pred.shape)} (the reference divides by 2 (N - 1))")
    if mask is not None and tuple(mask.shape) != tuple(gt.shape):
        raise ValueError(f"evaluate_tae: mask {tuple(mask.shape)} and gt {tuple(gt.shape)} differ in shape")
    K, poses = _host64(K, "K", (3, 3)), _host64(poses, "poses", (4, 4))
    if K.ndim == 2:
        K = np.broadcast_to(K, (N, 3, 3))
    if K.shape[0] != N or poses.shape[0] != N:
        raise ValueError(f"evaluate_tae: {N} frames but K {K.shape} and poses {poses.shape}")
    return _tae_cameras(K, poses)


def _tae_cameras(K, poses):
    """fp64 [N-1, 28] as vda_tae_* take it: fx, fy, cx, cy of K[i] (the reference reads K[i] for both directions), rows 0..2 of
    T21 = inv(pose[i+1]) @ pose[i], rows 0..2 of T12 = inv(T21) - on the host, in exactly these two steps (eval_tae.py:169,203)."""
    cam = np.empty((poses.shape[0] - 1, 28), dtype=np.float64)
    for i in range(cam.shape[0]):
        T21 = np.linalg.inv(poses[i + 1]) @ poses[i]
        T12 = np.linalg.inv(T21)
        cam[i, :4] = K[i, 0, 0], K[i, 1, 1], K[i, 0, 2], K[i, 1, 2]
        cam[i, 4:16], cam[i, 16:] = T21[:3].ravel(), T12[:3].ravel()
    return cam


def _tae_result(fit, res, npairs):
    return {"tae": float(res[0]), "scale": float(fit[0]), "shift": float(fit[1]), "n_valid": int(fit[2]),
            "pair_errors": np.array(res[1:1 + 2 * npairs], dtype=np.float64).reshape(npairs, 2),
            "pair_counts": np.array(res[1 + 2 * npairs:1 + 4 * npairs]).astype(np.int64).reshape(npairs, 2)}


def evaluate_tae_numpy(pred, gt, K, poses, max_depth, mask=None, resize=False):
    """Host twin of evaluate_tae: the same arithmetic in vectorised numpy (last-wins through np.maximum.at on source indices).
    For tests; not a product path."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    if pred.dtype != np.float32 or gt.dtype not in (np.float32, np.float64):
        raise ValueError(f"evaluate_tae_numpy: pred must be float32 and gt float32 or float64, got {pred.dtype} and {gt.dtype}")
    mask = None if mask is None else np.asarray(mask) != 0
    cam = _check_tae(pred, gt, K, poses, mask, resize)
    pred = resize_prediction_numpy(pred, gt.shape[1:])                  # the identity unless `resize` let a mismatch through
    fit = evaluate_depth_numpy(pred, gt, max_depth)
    N, H, W = pred.shape
    with np.errstate(all="ignore"):
        x = np.clip(pred, np.float32(1e-3), None).astype(np.float64)
        d = np.clip(1.0 / np.clip(fit["scale"] * x + fit["shift"], 1e-3, None), 1e-3, float(max_depth)).reshape(N, -1)
    ys, xs = (a.ravel().astype(np.float64) for a in np.indices((H, W)))
    src_index = np.arange(H * W, dtype=np.int64)
    err, cnt = np.zeros((N - 1, 2)), np.zeros((N - 1, 2), dtype=np.int64)
    for i in range(N - 1):
        fx, fy, cx, cy = cam[i, :4]
        for direction in (0, 1):
            m = cam[i, 4 + 12 * direction:16 + 12 * direction]
            src, dst = d[i + direction], d[i + 1 - direction]
            with np.errstate(all="ignore"):
                X, Y = (xs - cx) * src / fx, (ys - cy) * src / fy
                Qx, Qy, Qz = (X * m[4 * r] + Y * m[4 * r + 1] + src * m[4 * r + 2] + m[4 * r + 3] for r in range(3))
                u, v = np.rint(Qx * fx / Qz + cx), np.rint(Qy * fy / Qz + cy)
                inside = (u >= 0) & (u < W) & (v >= 0) & (v < H)
            winner = np.zeros(H * W, dtype=np.int64)
            np.maximum.at(winner, (v[inside] * W + u[inside]).astype(np.int64), src_index[inside] + 1)
            proj = np.where(winner > 0, Qz[np.maximum(winner, 1) - 1], 0.0)
            use = (proj > 0) & (dst > 0)
            if mask is not None:
                use &= mask[i + 1 - direction].ravel()
            cnt[i, direction] = use.sum()
            if cnt[i, direction]:
                err[i, direction] = (np.abs(dst[use] - proj[use]) / dst[use]).mean()
    tae = err.sum() / (2 * (N - 1)) * 100.0
    return {"tae": float(tae), "scale": fit["scale"], "shift": fit["shift"], "n_valid": fit["n_valid"], "pair_errors": err, "pair_counts": cnt}


def evaluate_tae(pred, gt, K, poses, max_depth, mask=None, device="cuda", chunk_pairs=None, resize=False):
    """Temporal alignment error of `pred` (float32 [N,H,W]) on the device. gt (float32 or float64 [N,H,W]) only takes part in the
    scale / shift fit, which is evaluate_depth's; K [N,3,3] or [3,3] and poses [N,4,4] (camera to world) go through the host; mask
    (bool or uint8 [N,H,W], optional) excludes target pixels. pred, gt and mask may be numpy arrays or CUDA tensors: device-resident
    tensors are used in place, host arrays are uploaded a few frames at a time. `chunk_pairs` bounds the winner planes (8 bytes per
    pixel and pair; all pairs at once when None); the result does not depend on it. With `resize`, a prediction [N,h,w] at another
    size is resized to gt's grid first (resize_prediction), a few frames at a time wherever frames are fed. Returns a dict: tae, scale,
    shift, n_valid, pair_errors and pair_counts [N-1, 2] (column 0: frame i into i+1). Runs on the current stream of the device."""
    import torch
    from . import ops

    pred = _as_tensor(pred, "pred", (torch.float32,), "evaluate_tae")
    gt = _as_tensor(gt, "gt", (torch.float32, torch.float64), "evaluate_tae")
    mask = None if mask is None else _as_tensor(mask, "mask", (torch.bool, torch.uint8), "evaluate_tae")
    cam_host = _check_tae(pred, gt, K, poses, mask, resize)
    dev = one_device((pred, gt, mask), device, "evaluate_tae")
    N, H, W = gt.shape
    px, P = H * W, N - 1
    if px >= 2 ** 31 - 1:
        raise ValueError(f"evaluate_tae: a frame of {H} x {W} is too large (a pixel index + 1 must fit 31 bits)")
    step = P if chunk_pairs is None else int(chunk_pairs)
    if step <= 0:
        raise ValueError("evaluate_tae: chunk_pairs must be positive")
    fit_chunks = _fit_chunks(N, TAE_FIT_FRAMES, px)
    bpp = min(TAE_MAX_BLOCKS, -(-px // TAE_PX_PER_BLOCK))
    max_depth = float(max_depth)

    with torch.cuda.device(dev):
        work = torch.empty(max(5 * sum(nb for _, _, nb in fit_chunks), 4 * P * bpp), dtype=torch.float64, device=dev)
        out = torch.empty(3 + 1 + 4 * P, dtype=torch.float64, device=dev)       # fit {scale, shift, n_valid} | tae, errors, counts
        fit, res = out[:3], out[3:]
        cam = torch.from_numpy(cam_host).to(dev)
        winner = torch.empty((2 * min(step, P), H, W), dtype=torch.int32, device=dev)
        pred_chunk, gt_chunk = _chunk_feeds(pred, gt, dev, (H, W))
        _fit_scale_shift(ops, fit_chunks, pred_chunk, gt_chunk, max_depth, work, fit)
        for lo in range(0, P, step):
            hi = min(lo + step, P)                                              # pairs lo .. hi-1 touch frames lo .. hi
            p = pred_chunk(lo, hi + 1)
            m = None if mask is None else mask[lo:hi + 1].to(dev).contiguous().to(torch.uint8)
            ops.tae_splat(p, max_depth, fit, cam[lo:hi], winner)
            ops.tae_compare(p, m, max_depth, fit, cam[lo:hi], winner, work, lo, bpp)
        ops.tae_finish(work, P, bpp, res)
        host = out.cpu().numpy()                                                # the one device-to-host copy (synchronises)
    return _tae_result(host[:3], host[3:], P)


def load_gt(path, factor):
    """One ground-truth frame: `.npy` as stored, anything else as a 16-bit image (cv2 when importable, else PIL), divided by
    `factor` with numpy's own promotion: float32 / python float stays float32, an integer array becomes float64."""
    if path.endswith(".npy"):
        raw = np.load(path)
    else:
        try:
            import cv2
            raw = np.array(cv2.imread(path, -1))
        except ImportError:
            from PIL import Image
            raw = np.asarray(Image.open(path))
            if raw.dtype == np.int32:                                   # PIL opens 16-bit PNG as mode I (int32); values are 0..65535
                raw = raw.astype(np.uint16)
    return raw / factor
