"""Reference composer for the folded ConvTranspose2d(k == stride) + bias-free 3x3 / pad 1 conv (include/vda.h, VDA_EPI_CONVT_FOLD_F16).

Everything here is fp64 torch on the CPU and follows the algebra literally; tests/test_convt_fold_numpy.py holds it against
conv2d(conv_transpose2d(x)) and tests/test_convt_fold_gpu.py holds the device pack and the folded GEMM against it."""
import torch
import torch.nn.functional as F

F64 = torch.float64


def split(q, k):
    """q = py + ky - 1 in [-1, k] -> (d = floor(q / k), ConvTranspose phase q - k*d)."""
    d = q // k
    return d, q - d * k


def compose(wt, bt, wr):
    """wt [Ci,Cm,k,k], bt [Cm], wr [Co,Cm,3,3] -> Wc [k*k, 3, 3, Co, Ci] and Bc [k*k, 3, 3, Co], indexed [phase][dy+1][dx+1]."""
    wt, bt, wr = wt.to(F64), bt.to(F64), wr.to(F64)
    Ci, Cm, k, _ = wt.shape
    Co = wr.shape[0]
    Wc = torch.zeros(k * k, 3, 3, Co, Ci, dtype=F64)
    Bc = torch.zeros(k * k, 3, 3, Co, dtype=F64)
    for py in range(k):
        for px in range(k):
            for ky in range(3):
                for kx in range(3):
                    (dy, ry), (dx, rx) = split(py + ky - 1, k), split(px + kx - 1, k)
                    Wc[py * k + px, dy + 1, dx + 1] += wr[:, :, ky, kx] @ wt[:, :, ry, rx].T
                    Bc[py * k + px, dy + 1, dx + 1] += wr[:, :, ky, kx] @ bt
    return Wc, Bc


def tap_blocks(Wc_or_k):
    """Number of (phase, tap) blocks a phase can reach: from the geometry alone (int k) or the non-zero blocks of a composed Wc."""
    if isinstance(Wc_or_k, int):
        k = Wc_or_k
        return len({(py, px, split(py + ky - 1, k)[0], split(px + kx - 1, k)[0]) for py in range(k) for px in range(k) for ky in range(3) for kx in range(3)})
    return int((Wc_or_k.abs().sum(dim=(3, 4)) != 0).sum())


def class_bias(Bc):
    """Bc [k*k, 3, 3, Co] -> [k*k, 9, Co]: for border class 3*cy + cx (0 first, 1 interior, 2 last) the sum over the taps inside the image."""
    P, Co = Bc.shape[0], Bc.shape[-1]
    out = torch.zeros(P, 9, Co, dtype=F64)
    inside = {0: (1, 2), 1: (0, 1, 2), 2: (0, 1)}          # tap index d + 1: class 0 has no d = -1, class 2 no d = +1
    for cy in range(3):
        for cx in range(3):
            for ty in inside[cy]:
                for tx in inside[cx]:
                    out[:, cy * 3 + cx] += Bc[:, ty, tx]
    return out


def pack(Wc, cin_pad=None):
    """Wc [k*k, 3, 3, Co, Ci] -> the GEMM's W [k*k*Co rows (phase, co)][9*cin_pad (tap, ci)], zero padded."""
    P, _, _, Co, Ci = Wc.shape
    cin_pad = Ci if cin_pad is None else cin_pad
    o = torch.zeros(P, Co, 3, 3, cin_pad, dtype=F64)
    o[..., :Ci] = Wc.permute(0, 3, 1, 2, 4)
    return o.reshape(P * Co, 9 * cin_pad)


def apply(t, Wc, Bc, k):
    """The folded pair on t [B,Ci,H,W] -> [B,Co,k*H,k*W]: per phase, the taps inside the grid contribute weight AND bias."""
    t = t.to(F64)
    B, Ci, H, W = t.shape
    Co = Wc.shape[3]
    out = torch.zeros(B, Co, k * H, k * W, dtype=F64)
    for py in range(k):
        for px in range(k):
            for y in range(H):
                for x in range(W):
                    acc = torch.zeros(B, Co, dtype=F64)
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            if 0 <= y + dy < H and 0 <= x + dx < W:
                                acc += t[:, :, y + dy, x + dx] @ Wc[py * k + px, dy + 1, dx + 1].T + Bc[py * k + px, dy + 1, dx + 1]
                    out[:, :, k * y + py, k * x + px] = acc
    return out


def border_class(i, n, phase, k):
    """The class whose table row is right for grid index i of n and phase row / column `phase`: on a 1-wide grid first and last
    coincide, and phase 0 (the only one that reaches d = -1) takes 'first', phase k - 1 (the only one that reaches d = +1) 'last'."""
    if i == 0 and phase == 0:
        return 0
    if i == n - 1 and phase == k - 1:
        return 2
    return 1


def apply_by_class(t, Wc, Bc, k):
    """The same through the class-bias table, as the kernels evaluate it: taps outside the grid read zeros, the bias comes by class."""
    t = t.to(F64)
    B, Ci, H, W = t.shape
    Co = Wc.shape[3]
    cb = class_bias(Bc)
    tp = F.pad(t, (1, 1, 1, 1))
    out = torch.zeros(B, Co, k * H, k * W, dtype=F64)
    for py in range(k):
        for px in range(k):
            w = Wc[py * k + px].permute(2, 3, 0, 1)                      # [Co, Ci, 3, 3] over (dy, dx)
            o = F.conv2d(tp, w)
            for y in range(H):
                for x in range(W):
                    o[:, :, y, x] += cb[py * k + px, 3 * border_class(y, H, py, k) + border_class(x, W, px, k)]
            out[:, :, py::k, px::k] = o
    return out


def unfused(t, wt, bt, wr, k):
    return F.conv2d(F.conv_transpose2d(t.to(F64), wt.to(F64), bt.to(F64), stride=k), wr.to(F64), padding=1)


def exact_inputs(k, Ci, Co, B, H, W, seed, cm=None):
    """Small-integer operands for the bit-exact GPU cases: t, wt in {-1, 0, 1} (sparse), bt in [-2, 2], wr with at most three +-1
    entries per (tap, output channel). Every composed weight, every intermediate and every result is then a small integer."""
    g = torch.Generator().manual_seed(seed)
    Cm = Ci if cm is None else cm
    r = lambda shape, lo, hi: torch.randint(lo, hi + 1, shape, generator=g).to(F64)
    t = r((B, Ci, H, W), -1, 1) * (torch.rand((B, Ci, H, W), generator=g, dtype=F64) < 0.25)
    wt = r((Ci, Cm, k, k), -1, 1) * (torch.rand((Ci, Cm, k, k), generator=g, dtype=F64) < 0.25)
    bt = r((Cm,), -2, 2)
    wr = torch.zeros(Co, Cm, 3, 3, dtype=F64)
    for co in range(Co):
        for tap in range(9):
            idx = torch.randint(0, Cm, (3,), generator=g)
            wr[co, idx, tap // 3, tap % 3] = r((3,), 0, 1) * 2 - 1
    return t, wt, bt, wr
