"""Drop-in for the reference's utils/loss_MiDas.py as its train.py imports it (`from utils.loss_MiDas import Loss_ssi, Loss_tgm`),
for the VALIDATION pass only: the arithmetic runs on the device in fp64 (video_depth_anything_amd/losses.py, csrc/losses.hip) and
the modules return a 0-dim float32 tensor on pred's device, so `ratio_tgm * loss_tgm(pred, y, mask) + ratio_ssi * loss_ssi(pred,
y, mask)` runs unchanged. Inference only: an input that requires grad is refused (there is no backward), and nothing is printed.
Loss_ssi here is the least-squares (MiDaS) form; the Depth-Anything form is utils/loss.py."""
import numpy as np
import torch
import torch.nn as nn

from video_depth_anything_amd import losses

_VARIANT = "lsq"


def _no_grad_inputs(name, *tensors):
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise RuntimeError(f"{name}: an input requires grad, but this module is inference-only (the validation pass runs under "
                               "torch.no_grad(); training losses are out of scope)")


def _mask(masks):
    if masks is None:
        return None
    return masks != 0 if isinstance(masks, torch.Tensor) else np.asarray(masks) != 0          # the reference's masks.bool()


def _scalar(value, like):
    dev = like.device if isinstance(like, torch.Tensor) else "cpu"
    return torch.tensor(np.float32(value), dtype=torch.float32, device=dev)


class Loss_ssi(nn.Module):
    """forward(pred, y, masks): pred, y float32 [B,N,1,H,W] or [B,N,H,W], masks [B,N,H,W] (any dtype, nonzero = valid)."""

    def __init__(self, eps=1e-8):
        super().__init__()
        self.eps = eps

    def forward(self, pred, y, masks):
        _no_grad_inputs("Loss_ssi", pred, y)
        return _scalar(losses.ssi_loss(pred, y, _mask(masks), variant=_VARIANT, eps=self.eps), pred)


class Loss_tgm(nn.Module):
    """forward(pred, y, masks): as Loss_ssi; NaN for N = 1, as the reference's 0 / 0."""

    def forward(self, pred, y, masks):
        _no_grad_inputs("Loss_tgm", pred, y)
        return _scalar(losses.tgm_loss(pred, y, _mask(masks)), pred)
