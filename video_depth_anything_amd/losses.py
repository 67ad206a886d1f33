"""The reference's validation losses on the device: what its train.py (validation pass, eval() under no_grad) ranks checkpoints by,

    val_loss = ratio_tgm * Loss_tgm(pred, y, mask) + ratio_ssi * Loss_ssi(pred, y, mask)          (configs/config.yaml: 10 and 1)

as inference-time arithmetic - no gradient is involved. `ssi_loss`, `tgm_loss` and `validation_loss` run it as the streaming fp64
reductions of csrc/losses.hip (vda_loss_*): nothing returns to the host between the passes and one small device-to-host copy ends
the call, where the reference loops over B * N frames in Python and synchronises 2 B (N - 1) times per batch in Loss_tgm alone.
`*_numpy` restate the same arithmetic on the host in fp64 for the CPU-side tests; the device functions never call them - there is no
CPU path. The contract is in DESIGN.md 6g; in short, with every float32 value widened exactly and all arithmetic fp64:

  pred, y : float32 [B,N,H,W] ([B,N,1,H,W] is squeezed, as the reference does); mask : bool / uint8 [B,N,H,W], 0 = excluded, None =
            all valid. Finite inputs only: a NaN under a masked-out pixel poisons the reference's sums and is outside the contract.
  ssi "lsq" utils/loss_MiDas.py, the one train.py imports. Per frame, n = max(valid pixels, 1): means mu_d, mu_y over the valid
            pixels; num = sum (d - mu_d)(y - mu_y), den = sum (d - mu_d)^2 (the CENTRED two-pass form: raw moments cancel);
            s = num / (den + eps), t = mu_y - s mu_d; frame loss = sum (s d + t - y)^2 / n. The mean over all B N frames; a frame
            without a valid pixel contributes 0 and still counts.
  ssi "mad" utils/loss.py, the Depth-Anything form. Per frame and tensor: med = the LOWER median of the valid values (element
            (n - 1) // 2 of the sorted values, torch.median's rule), sc = mean |v - med| + eps (no valid pixel: med = 0, sc = eps);
            rho = ((pred - med_p) / sc_p - (y - med_y) / sc_y)^2 on valid pixels. That file normalises PER IMAGE ROW -
            rho.sum(-1) / max(mask.sum(-1), 1) - so the result is the mean over all B N H rows and a row without a valid pixel
            counts as 0. The quirk is kept: it is what that file computes.
  tgm       per clip b and pair (i, i + 1): valid = mask_i & mask_{i+1}; static = valid & (|y_{i+1} - y_i| < 0.05), the difference
            and the comparison in fp64 against the double 0.05; a pair with no valid or no static pixel is skipped; otherwise
            pair = sum_static | |d_{i+1} - d_i| - |y_{i+1} - y_i| | / n_static. Clip value = sum of pairs / (N - 1), skipped pairs
            staying in the divisor; the mean over clips. N = 1 gives NaN, as the reference's 0 / 0 does.
"""
import numpy as np

from .staging import one_device

VARIANTS = ("lsq", "mad")
LOSS_T = 256                 # threads per block of the reductions (csrc/losses.hip LS_T)
LOSS_MAX_BLOCKS = 64         # blocks per plane


# ---------------------------------------------------------------------------------------------- argument checks (host side, no GPU)
def _shape_checks(pred, y, mask, what):
    """pred / y / mask as handed in (numpy arrays or tensors: only .shape, .ndim and .dtype are read). Returns the squeezed shape."""
    def squeezed(a):
        s = tuple(a.shape)
        return s[:2] + s[3:] if len(s) == 5 and s[2] == 1 else s

    f32 = {"float32", "torch.float32"}
    if str(pred.dtype) not in f32 or str(y.dtype) not in f32:
        raise ValueError(f"{what}: pred and y must be float32, got {pred.dtype} and {y.dtype}")
    sp, sy = squeezed(pred), squeezed(y)
    if len(sp) != 4 or sp != sy:
        raise ValueError(f"{what}: pred and y must be one shape [B,N,H,W] or [B,N,1,H,W], got {tuple(pred.shape)} and {tuple(y.shape)}")
    if min(sp) < 1:
        raise ValueError(f"{what}: empty input {sp}")
    if mask is not None:
        if str(mask.dtype) not in {"bool", "uint8", "torch.bool", "torch.uint8"}:
            raise ValueError(f"{what}: mask must be bool or uint8, got {mask.dtype}")
        if tuple(mask.shape) != sp:
            raise ValueError(f"{what}: mask {tuple(mask.shape)} must be [B,N,H,W] = {sp}")
    return sp


def _check_variant(variant):
    if variant not in VARIANTS:
        raise ValueError(f"variant must be one of {VARIANTS}, got {variant!r}")


def _host(pred, y, mask, what):
    pred, y = np.asarray(pred), np.asarray(y)
    mask = None if mask is None else np.asarray(mask)
    shape = _shape_checks(pred, y, mask, what)
    m = np.ones(shape, dtype=bool) if mask is None else mask != 0
    return pred.reshape(shape).astype(np.float64), y.reshape(shape).astype(np.float64), m, pred.reshape(shape), y.reshape(shape)


# ---------------------------------------------------------------------------------------------- numpy twins
def _keys(v):
    """Order-preserving uint32 keys of float32 values: the sign bit flipped for non-negative values, all bits for negative ones."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def _values(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def _masked_median_numpy(x, mask=None):
    """Lower median of the valid values of every [H,W] plane of float32 x [..,H,W]: float32 [..], 0 where no pixel is valid. The
    order is that of the keys (-0 before +0), so the result is one input element, bit for bit."""
    x = np.asarray(x)
    if x.dtype != np.float32 or x.ndim < 2:
        raise ValueError(f"_masked_median_numpy: x must be float32 [..,H,W], got {x.dtype} {x.shape}")
    lead = x.shape[:-2]
    xf = x.reshape(-1, x.shape[-2] * x.shape[-1])
    mf = np.ones(xf.shape, dtype=bool) if mask is None else (np.asarray(mask) != 0).reshape(xf.shape)
    out = np.zeros(xf.shape[0], dtype=np.float32)
    for f in range(xf.shape[0]):
        k = _keys(xf[f][mf[f]])
        if k.size:
            r = (k.size - 1) // 2
            out[f] = _values(np.partition(k, r)[r:r + 1])[0]
    return out.reshape(lead)


def _ssi_frames_numpy(pred, y, mask, variant, eps):
    d, g, m, d32, g32 = _host(pred, y, mask, "ssi_loss_numpy")
    B, N, H, W = d.shape
    if variant == "lsq":
        d, g, m = d.reshape(B * N, -1), g.reshape(B * N, -1), m.reshape(B * N, -1)
        n = np.maximum(m.sum(1), 1).astype(np.float64)
        mu_d, mu_y = np.where(m, d, 0.0).sum(1) / n, np.where(m, g, 0.0).sum(1) / n
        dd, dy = d - mu_d[:, None], g - mu_y[:, None]
        num, den = np.where(m, dd * dy, 0.0).sum(1), np.where(m, dd * dd, 0.0).sum(1)
        s = num / (den + eps)
        t = mu_y - s * mu_d
        r = (s[:, None] * d + t[:, None]) - g
        per = np.where(m, r * r, 0.0).sum(1) / n
        return per.mean(), per.reshape(B, N)
    med_d, med_y = _masked_median_numpy(d32, m).astype(np.float64), _masked_median_numpy(g32, m).astype(np.float64)
    cnt = m.sum((2, 3))

    def scale(v, med):
        dev = np.where(m, np.abs(v - med[:, :, None, None]), 0.0).sum((2, 3))
        return np.where(cnt > 0, dev / np.maximum(cnt, 1), 0.0) + eps

    sc_d, sc_y = scale(d, med_d), scale(g, med_y)
    diff = (d - med_d[:, :, None, None]) / sc_d[:, :, None, None] - (g - med_y[:, :, None, None]) / sc_y[:, :, None, None]
    rows = np.where(m, diff * diff, 0.0).sum(-1) / np.maximum(m.sum(-1), 1)            # [B,N,H]: that file's per-row rule
    return rows.mean(), rows.mean(-1)


def ssi_loss_numpy(pred, y, mask=None, variant="lsq", eps=1e-8):
    """Host twin of ssi_loss in numpy fp64. For tests; not a product path."""
    _check_variant(variant)
    return float(_ssi_frames_numpy(pred, y, mask, variant, float(eps))[0])


def _tgm_pairs_numpy(pred, y, mask):
    d, g, m, _, _ = _host(pred, y, mask, "tgm_loss_numpy")
    B, N = d.shape[:2]
    pairs = np.full((B, max(N - 1, 0)), np.nan)
    n_static = np.zeros((B, max(N - 1, 0)), dtype=np.int64)
    for b in range(B):
        for i in range(N - 1):
            valid = m[b, i] & m[b, i + 1]
            gy = np.abs(g[b, i + 1] - g[b, i])
            static = valid & (gy < 0.05)
            n_static[b, i] = static.sum()
            if valid.any() and n_static[b, i]:
                pairs[b, i] = np.abs(np.abs(d[b, i + 1] - d[b, i]) - gy)[static].sum() / n_static[b, i]
    with np.errstate(all="ignore"):
        clips = np.where(np.isnan(pairs), 0.0, pairs).sum(1) / np.float64(N - 1)
    return float(clips.mean()), pairs, n_static


def tgm_loss_numpy(pred, y, mask=None):
    """Host twin of tgm_loss in numpy fp64. For tests; not a product path."""
    return _tgm_pairs_numpy(pred, y, mask)[0]


def _combine(ssi, per_frame, tgm, pairs, n_static, ratio_ssi, ratio_tgm):
    return {"loss": float(ratio_tgm) * tgm + float(ratio_ssi) * ssi, "ssi": ssi, "tgm": tgm, "ssi_per_frame": per_frame,
            "tgm_per_pair": pairs, "n_static": n_static}


def validation_loss_numpy(pred, y, mask=None, ratio_ssi=1.0, ratio_tgm=10.0, variant="lsq", eps=1e-8):
    """Host twin of validation_loss in numpy fp64. For tests; not a product path."""
    _check_variant(variant)
    ssi, per_frame = _ssi_frames_numpy(pred, y, mask, variant, float(eps))
    tgm, pairs, n_static = _tgm_pairs_numpy(pred, y, mask)
    return _combine(float(ssi), per_frame, tgm, pairs, n_static, ratio_ssi, ratio_tgm)


# ---------------------------------------------------------------------------------------------- the device path
def _as_tensor(a):
    """A host array as a tensor that shares its memory (a read-only array is copied: torch cannot wrap one)."""
    import torch

    if isinstance(a, torch.Tensor):
        return a
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy())


def _device_inputs(pred, y, mask, device, what):
    """Checked on the host first (no GPU is touched before a ValueError); returns contiguous device tensors [B,N,H,W] (mask uint8 or
    None) and their device."""
    import torch

    shape = _shape_checks(pred, y, mask, what)
    ts = [_as_tensor(pred), _as_tensor(y)] + ([] if mask is None else [_as_tensor(mask)])
    dev = one_device(ts, device, what)
    with torch.cuda.device(dev):
        ts = [t.detach().to(dev).reshape(shape).contiguous() for t in ts]
        m = None
        if mask is not None:
            m = ts[2].view(torch.uint8) if ts[2].dtype == torch.bool else ts[2]
    return ts[0], ts[1], m, dev


def _bpp(px):
    return min(LOSS_MAX_BLOCKS, -(-px // LOSS_T))


def _run(pred, y, mask, variant, eps, device, want_ssi, want_tgm, what):
    """Queues the wanted losses on the current stream of the device and makes the one device-to-host copy. Returns
    (ssi block [1 + F] or None, tgm block [1 + 2 P] or None, (B, N))."""
    import torch
    from . import ops

    _check_variant(variant)
    pred, y, mask, dev = _device_inputs(pred, y, mask, device, what)
    B, N, H, W = pred.shape
    F, P, bpp = B * N, B * (N - 1), _bpp(H * W)
    want_tgm = want_tgm and N >= 2
    n_ssi, n_tgm = (1 + F if want_ssi else 0), (1 + 2 * P if want_tgm else 0)
    if n_ssi + n_tgm == 0:
        return None, None, (B, N)
    with torch.cuda.device(dev):
        out = torch.empty(n_ssi + n_tgm, dtype=torch.float64, device=dev)
        work = torch.empty(3 * F * bpp, dtype=torch.float64, device=dev)
        if want_ssi:
            stats = torch.empty(ops.LOSS_STATS * F, dtype=torch.float64, device=dev)
            if variant == "lsq":
                for step in (0, 1, 2):
                    ops.loss_lsq_pass(pred, y, mask, step, eps, stats, work, bpp, out[:n_ssi] if step == 2 else None)
            else:
                med = torch.empty(2 * F, dtype=torch.float32, device=dev)
                rows = torch.empty(2 * F * H, dtype=torch.float64, device=dev)
                ops.loss_median(pred, y, mask, med)
                ops.loss_mad(pred, y, mask, eps, med, stats, work, bpp, rows, out[:n_ssi])
        if want_tgm:
            ops.loss_tgm(pred, y, mask, work, bpp, out[n_ssi:])
        host = out.cpu().numpy()                                        # the one device-to-host copy (synchronises)
    return (host[:n_ssi] if want_ssi else None), (host[n_ssi:] if want_tgm else None), (B, N)


def ssi_loss(pred, y, mask=None, variant="lsq", eps=1e-8, device="cuda"):
    """The scale-and-shift-invariant loss of `pred` against `y` (module docstring) as a Python float. pred, y (float32) and mask
    (bool / uint8 or None) may be numpy arrays or CUDA tensors in any mix: device-resident tensors are used in place, host arrays are
    uploaded. Runs on the current stream of the device; one device-to-host copy at the end."""
    ssi, _, _ = _run(pred, y, mask, variant, float(eps), device, True, False, "ssi_loss")
    return float(ssi[0])


def tgm_loss(pred, y, mask=None, device="cuda"):
    """The temporal gradient matching loss (module docstring) as a Python float; NaN for N = 1. Inputs as for ssi_loss."""
    _, tgm, _ = _run(pred, y, mask, "lsq", 1e-8, device, False, True, "tgm_loss")
    return float("nan") if tgm is None else float(tgm[0])


def validation_loss(pred, y, mask=None, ratio_ssi=1.0, ratio_tgm=10.0, variant="lsq", eps=1e-8, device="cuda"):
    """The number the reference's validation pass ranks checkpoints by, ratio_tgm * tgm + ratio_ssi * ssi, with its parts:
    {'loss', 'ssi', 'tgm', 'ssi_per_frame' [B,N], 'tgm_per_pair' [B,N-1] (NaN where the pair was skipped), 'n_static' [B,N-1]}.
    With the "mad" variant a frame's entry of ssi_per_frame is the mean over its image rows. Inputs as for ssi_loss; both losses are
    queued on the current stream and one device-to-host copy ends the call."""
    ssi, tgm, (B, N) = _run(pred, y, mask, variant, float(eps), device, True, True, "validation_loss")
    P = B * (N - 1)
    if tgm is None:
        t, pairs, n_static = float("nan"), np.full((B, 0), np.nan), np.zeros((B, 0), dtype=np.int64)
    else:
        t, pairs, n_static = float(tgm[0]), tgm[1:1 + P].reshape(B, N - 1).copy(), tgm[1 + P:].astype(np.int64).reshape(B, N - 1)
    return _combine(float(ssi[0]), ssi[1:].reshape(B, N).copy(), t, pairs, n_static, ratio_ssi, ratio_tgm)


def _masked_median(x, mask=None, device="cuda"):
    """The device's exact masked lower medians of float32 x [..,H,W] (numpy or CUDA tensor): numpy float32 [..], 0 where no pixel is
    valid. What the "mad" variant uses, exposed so that a test can hold it against _masked_median_numpy bit for bit."""
    import torch
    from . import ops

    if str(x.dtype) not in {"float32", "torch.float32"} or x.ndim < 2 or min(tuple(x.shape)) < 1:
        raise ValueError(f"_masked_median: x must be a non-empty float32 [..,H,W], got {x.dtype} {tuple(x.shape)}")
    if mask is not None and (tuple(mask.shape) != tuple(x.shape) or str(mask.dtype) not in {"bool", "uint8", "torch.bool", "torch.uint8"}):
        raise ValueError(f"_masked_median: mask must be bool / uint8 of x's shape {tuple(x.shape)}, got {mask.dtype} {tuple(mask.shape)}")
    lead = tuple(x.shape[:-2])
    shape = (1, max(int(np.prod(lead)), 1)) + tuple(x.shape[-2:])
    xt = _as_tensor(x)
    mt = None if mask is None else _as_tensor(mask)
    dev = xt.device if xt.is_cuda else torch.device(device)
    with torch.cuda.device(dev):
        xt = xt.detach().to(dev).reshape(shape).contiguous()
        if mt is not None:
            mt = mt.to(dev).reshape(shape).contiguous()
            mt = mt.view(torch.uint8) if mt.dtype == torch.bool else mt
        med = torch.empty(shape[1], dtype=torch.float32, device=dev)
        ops.loss_median(xt, None, mt, med)
        return med.cpu().numpy().reshape(lead)
