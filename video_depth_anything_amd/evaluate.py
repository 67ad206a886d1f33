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
"""
import numpy as np

METRICS = ("abs_relative_difference", "squared_relative_difference", "rmse_linear", "delta1_acc", "delta2_acc", "delta3_acc")
EVAL_T = 256                 # threads per block of the two passes (csrc/eval.hip EV_T)
LSQ_MAX_BLOCKS = 1024        # pass 1: blocks per call
METRIC_MAX_BLOCKS = 64       # pass 2: blocks per frame
_D1, _D2, _D3 = 1.25, 1.25 ** 2, 1.25 ** 3


def _check_pair(pred, gt, max_eval_len):
    """Common argument checks; returns (pred[:L], gt[:L]) with pred.shape == gt.shape == [N,H,W]."""
    if pred.ndim != 3 or gt.ndim != 3:
        raise ValueError(f"evaluate_depth: pred and gt must be [N,H,W], got {tuple(pred.shape)} and {tuple(gt.shape)}")
    if max_eval_len is not None:
        pred, gt = pred[:max_eval_len], gt[:max_eval_len]
    if tuple(pred.shape) != tuple(gt.shape):
        raise ValueError(f"evaluate_depth: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ in shape. The reference resizes a "
                         "mismatched prediction with cv2.resize; resizing is not part of this scorer - write the prediction at the "
                         "(cropped) ground-truth size")
    if pred.shape[0] == 0 or pred.shape[1] * pred.shape[2] == 0:
        raise ValueError("evaluate_depth: empty video")
    return pred, gt


def _result(fit, res):
    out = {k: float(v) for k, v in zip(METRICS, res[:6])}
    out["scale"], out["shift"] = float(fit[0]), float(fit[1])
    out["n_valid"], out["n_frames_used"] = int(fit[2]), int(res[6])
    return out


def evaluate_depth_numpy(pred, gt, max_depth, max_eval_len=None):
    """Host twin of evaluate_depth: the same arithmetic in numpy, normal equations in fp64. For tests; not a product path."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    if pred.dtype != np.float32 or gt.dtype not in (np.float32, np.float64):
        raise ValueError(f"evaluate_depth_numpy: pred must be float32 and gt float32 or float64, got {pred.dtype} and {gt.dtype}")
    pred, gt = _check_pair(pred, gt, max_eval_len)
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


def evaluate_depth(pred, gt, max_depth, max_eval_len=None, device="cuda", chunk_frames=None):
    """Metrics of `pred` (float32 [N,H,W]) against `gt` (float32 or float64 [N,H,W]) on the device; numpy arrays or CUDA tensors.
    Device-resident tensors are used in place; host arrays are uploaded `chunk_frames` frames at a time (all at once when None), once
    per pass. Returns a dict: the six METRICS, scale, shift, n_valid, n_frames_used. Runs on the current stream of the device."""
    import torch
    from . import ops

    def as_tensor(a, name, dtypes):
        if not isinstance(a, torch.Tensor):
            a = torch.from_numpy(np.asarray(a))
        if a.dtype not in dtypes:
            raise ValueError(f"evaluate_depth: {name} must be {' or '.join(str(d) for d in dtypes)}, got {a.dtype}")
        return a

    pred = as_tensor(pred, "pred", (torch.float32,))
    gt = as_tensor(gt, "gt", (torch.float32, torch.float64))
    pred, gt = _check_pair(pred, gt, max_eval_len)
    on_dev = [t.device for t in (pred, gt) if t.is_cuda]
    dev = on_dev[0] if on_dev else torch.device(device)
    if dev.type != "cuda" or any(d != dev for d in on_dev):
        raise ValueError(f"evaluate_depth: needs one cuda device, got {device!r} / {[str(d) for d in on_dev]}")
    N, H, W = pred.shape
    px = H * W
    step = N if chunk_frames is None else int(chunk_frames)
    if step <= 0:
        raise ValueError("evaluate_depth: chunk_frames must be positive")
    chunks = [(lo, min(lo + step, N)) for lo in range(0, N, step)]
    nblk = [min(LSQ_MAX_BLOCKS, -(-(hi - lo) * px // EVAL_T)) for lo, hi in chunks]
    bpf = min(METRIC_MAX_BLOCKS, -(-px // EVAL_T))
    max_depth = float(max_depth)

    with torch.cuda.device(dev):
        work = torch.empty(max(5 * sum(nblk), 7 * N * bpf), dtype=torch.float64, device=dev)
        out = torch.empty(10, dtype=torch.float64, device=dev)          # fit {scale, shift, n_valid} | result[7]
        fit, res = out[:3], out[3:]

        def on_device(t, lo, hi):
            return t[lo:hi].to(dev, non_blocking=False).contiguous()

        row = 0
        for (lo, hi), nb in zip(chunks, nblk):
            ops.eval_lsq_partial(on_device(pred, lo, hi), on_device(gt, lo, hi), max_depth, work, row, nb)
            row += nb
        ops.eval_lsq_finish(work, row, fit)
        for lo, hi in chunks:
            ops.eval_metric_partial(on_device(pred, lo, hi), on_device(gt, lo, hi), max_depth, fit, work, lo, bpf)
        ops.eval_metric_finish(work, N, bpf, res)
        host = out.cpu().numpy()                                        # the one device-to-host copy (synchronises)
    return _result(host[:3], host[3:])


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
