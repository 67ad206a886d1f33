"""fp64 reference of option "oc1_mix" (include/vda.h): refinenet1's out_conv (1x1), the 2x align_corners upsample and output_conv1 (3x3, pad 1)
as ONE channel-mixing GEMM on the half-resolution grid (z, 9 x Fh channels) and a gather-and-add pass.

    z[b, y, x, tap, co] = sum_ci Wz[tap, co, ci] r[b, y, x, ci] + bz[tap, co],   Wz[tap] = W1[:, :, tap] . Wo,  bz[tap] = W1[:, :, tap] . bo
    o1[b, Y, X, co]     = b1[co] + sum over taps (ky, kx) with q = (Y + ky - 1, X + kx - 1) inside the 2h x 2w map of
                          sum_j a_j(q) z[b, s_j(q), tap, co]

Everything is numpy float64, NHWC; `target` is torch's own conv2d(interpolate(conv1x1(r)))."""
import numpy as np

TILE_ROWS = 16          # csrc/oc1_mix.hip: a workgroup's strip of output rows, and its 256 / (Fhp / 8) output columns


def tile_cols(Fhp):
    return 256 // (Fhp // 8)


# 1x1, 1x2, 2x1: scale 0 along an axis of one pixel (every sample lands on pixel 0); (9, 35): 18 x 70 outputs = two strips of 16 rows and
# two tiles of 64 columns at Fhp = 32 (five of 16 at Fhp = 128), neither dividing evenly
GRIDS = [(1, 1), (1, 2), (2, 1), (2, 3), (5, 7), (9, 35)]


def compose(W1, Wo, bo):
    """W1 [Fh, Fe, 3, 3], Wo [Fe, Fe], bo [Fe] -> Wz [9, Fh, Fe], bz [9, Fh]."""
    W1 = np.asarray(W1, np.float64).reshape(W1.shape[0], W1.shape[1], 9)
    Wo, bo = np.asarray(Wo, np.float64).reshape(W1.shape[1], W1.shape[1]), np.asarray(bo, np.float64)
    return np.einsum("omt,mi->toi", W1, Wo), np.einsum("omt,m->to", W1, bo)


def pack(Wz, bz, Fhp):
    """The GEMM's operands: rows (tap, cout) with cout padded to Fhp by zero rows -> [9 * Fhp, Fe], [9 * Fhp]."""
    _, Fh, Fe = Wz.shape
    W, b = np.zeros((9, Fhp, Fe)), np.zeros((9, Fhp))
    W[:, :Fh], b[:, :Fh] = Wz, bz
    return W.reshape(9 * Fhp, Fe), b.reshape(9 * Fhp)


def corners(n):
    """For q in [0, 2n): (lower source index, upper source index, fraction) of F.interpolate(scale_factor=2, align_corners=True)."""
    q = np.arange(2 * n, dtype=np.float64)
    s = q * ((n - 1) / (2 * n - 1)) if n > 1 else np.zeros(2 * n)
    a = np.minimum(np.floor(s).astype(np.int64), n - 1)
    return a, np.minimum(a + 1, n - 1), s - a


def gather(z, b1=None):
    """z [B, h, w, 9, C] -> [B, 2h, 2w, C]: per tap the interpolation of its plane, shifted by the tap's offset, zero outside the map."""
    B, h, w, _, C = z.shape
    H, W = 2 * h, 2 * w
    ya, yb, fy = corners(h)
    xa, xb, fx = corners(w)
    out = np.zeros((B, H, W, C))
    for ky in range(3):
        for kx in range(3):
            p = z[:, :, :, 3 * ky + kx]
            rows = p[:, ya] * (1 - fy)[None, :, None, None] + p[:, yb] * fy[None, :, None, None]            # [B, H, w, C]
            up = rows[:, :, xa] * (1 - fx)[None, None, :, None] + rows[:, :, xb] * fx[None, None, :, None]    # [B, H, W, C]: U_tap[q]
            # o1[Y, X] += U_tap[Y + ky - 1, X + kx - 1] where that lies inside
            Y0, Y1, X0, X1 = max(0, 1 - ky), min(H, H + 1 - ky), max(0, 1 - kx), min(W, W + 1 - kx)
            out[:, Y0:Y1, X0:X1] += up[:, Y0 + ky - 1:Y1 + ky - 1, X0 + kx - 1:X1 + kx - 1]
    return out if b1 is None else out + np.asarray(b1, np.float64)


def mix(r, W1, Wo, bo, b1):
    """r [B, h, w, Fe] -> (o1 [B, 2h, 2w, Fh], z [B, h, w, 9, Fh]) by the composed form."""
    Wz, bz = compose(W1, Wo, bo)
    z = np.einsum("byxi,toi->byxto", np.asarray(r, np.float64), Wz) + bz
    return gather(z, b1), z


def target(r, W1, Wo, bo, b1):
    """torch: conv2d(interpolate(conv1x1(r), scale_factor=2, mode='bilinear', align_corners=True), W1, padding=1) + b1, NHWC float64."""
    import torch
    import torch.nn.functional as F
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    x = t(r).permute(0, 3, 1, 2)
    Fe = x.shape[1]
    c = F.conv2d(x, t(Wo).reshape(Fe, Fe, 1, 1), t(bo))
    up = F.interpolate(c, scale_factor=2, mode="bilinear", align_corners=True)
    return F.conv2d(up, t(W1), t(b1), padding=1).permute(0, 2, 3, 1).numpy()


def inputs(B, h, w, Fe, Fh, seed):
    """Random operands at the scale the head runs at (weights ~ 1 / sqrt(fan-in))."""
    g = np.random.default_rng(seed)
    r = g.standard_normal((B, h, w, Fe))
    W1 = g.standard_normal((Fh, Fe, 3, 3)) / np.sqrt(9 * Fe)
    Wo = g.standard_normal((Fe, Fe)) / np.sqrt(Fe)
    return r, W1, Wo, 0.1 * g.standard_normal(Fe), 0.1 * g.standard_normal(Fh)
