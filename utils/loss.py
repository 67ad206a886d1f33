"""Drop-in for the reference's utils/loss.py (`from utils.loss import Loss_ssi, Loss_tgm`), for validation only: Loss_ssi is the
Depth-Anything form - a masked lower median and mean absolute deviation per frame, normalised PER IMAGE ROW as that file does - and
Loss_tgm is the one of utils/loss_MiDas.py (the two files define the same one). The arithmetic runs on the device in fp64
(video_depth_anything_amd/losses.py); a 0-dim float32 tensor on pred's device comes back. Inference only, nothing is printed."""
import torch.nn as nn

from utils.loss_MiDas import Loss_tgm, _mask, _no_grad_inputs, _scalar  # noqa: F401  (Loss_tgm is re-exported)
from video_depth_anything_amd import losses


class Loss_ssi(nn.Module):
    """forward(pred, y, masks): pred, y float32 [B,N,1,H,W] or [B,N,H,W], masks [B,N,H,W] (any dtype, nonzero = valid)."""

    def __init__(self, eps=1e-8):
        super().__init__()
        self.eps = eps

    def forward(self, pred, y, masks):
        _no_grad_inputs("Loss_ssi", pred, y)
        return _scalar(losses.ssi_loss(pred, y, _mask(masks), variant="mad", eps=self.eps), pred)
