"""Thin tensor -> pointer wrappers over the C ABI (include/vda.h).

torch is used for device memory and the current HIP stream only; every op here
is one call into libvda_hip.so and nothing else. Shapes are validated twice:
here (tensor metadata the C side cannot see) and in the library (geometry).

Two operand precisions share these wrappers, selected by the dtype of the activation tensors handed in: fp16
(the *_f16 entry points: the reference's autocast path) and fp32 (the *_f32 twins: its fp32=True path).
"""
import ctypes as C

import torch

import os
import sys

from . import _lib
from ._lib import GemmArgs, lib
from ._lib import check as _check

_TRACE = os.environ.get("VDA_TRACE_SYNC") == "1"     # debug: sync + log after every launch (finds a faulting kernel)


def check(rc, what=""):
    _check(rc, what)
    if _TRACE:
        sys.stderr.write(f"[vda] {what} ...")
        sys.stderr.flush()
        torch.cuda.synchronize()
        sys.stderr.write(" ok\n")
        sys.stderr.flush()

F16, F32 = torch.float16, torch.float32


def _stream(t=None):
    """The current stream of the device the operands live on (NOT of whichever device happens to be current)."""
    dev = t.device if t is not None else None
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _act(t, name):
    if t is None:
        return
    if not t.is_cuda or t.dtype not in (F16, F32) or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous cuda fp16 / fp32 activation, got {t.dtype} {t.device} contiguous={t.is_contiguous()}")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _req(t, dtype, name):
    if t is None:
        return
    if not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{name}: expected contiguous cuda {dtype}, got {t.dtype} {t.device} contiguous={t.is_contiguous()}")


def _same_device(what, *tensors):
    if len({t.device for t in tensors if t is not None}) != 1:
        raise ValueError(f"{what}: the operands live on different devices")


def _host_array(a, dtype, size, name, what, form=None):
    """`a` must be a contiguous host numpy array of `dtype` and `size`: the number of entries, or the shape with None for any
    extent. `form` words the error where "array of size entries" does not."""
    import numpy as np
    ok = isinstance(a, np.ndarray) and a.dtype == dtype and a.flags.c_contiguous
    got, want = ((a.size,), (size,)) if ok and isinstance(size, int) else (getattr(a, "shape", ()), size)
    if not ok or len(got) != len(want) or any(w not in (None, g) for g, w in zip(got, want)):
        raise ValueError(f"{what}: {name} must be {form or f'a contiguous host {np.dtype(dtype).name} array of {size} entries'}")


_zero_pages = {}


def zero_page(device):
    z = _zero_pages.get(device)
    if z is None:
        z = torch.zeros(256, dtype=torch.uint8, device=device)
        _zero_pages[device] = z
    return z


def gemm(A, W, out, epi, *, M, N, K, lda=None, ldc=None, bias=None, res=None, res2=None, gamma=None, pos=None,
         relu_in=False, conv=None, P=0, convt=None, out2=None, stats=None, sched=None, stats_ld=0, tile_rows=0):
    """out = epilogue(A[M,K] W[N,K]^T). conv = (B,H,W,Cin,Ho,Wo,stride) switches A to the
    implicit 3x3 window of an NHWC tensor; convt = (k, h, w, Cout) for VDA_EPI_CONVT_F16 and, with conv on the same h x w grid,
    for VDA_EPI_CONVT_FOLD_F16 (W, bias = fold_convt_weight's Wf, Bc)."""
    _act(A, "A"), _req(W, A.dtype, "W"), _req(bias, F32, "bias"), _req(gamma, F32, "gamma"), _req(pos, F32, "pos")
    fn, fname = (lib.vda_gemm_f32, "vda_gemm_f32") if A.dtype == F32 else (lib.vda_gemm_f16, "vda_gemm_f16")
    a = GemmArgs()
    a.A, a.W, a.bias, a.out = _p(A), _p(W), _p(bias), _p(out)
    a.res, a.res2, a.gamma, a.pos = _p(res), _p(res2), _p(gamma), _p(pos)
    _req(stats, F32, "stats")
    a.out2, a.stats, a.sched = _p(out2), _p(stats), _p(sched)
    a.zero_page = _p(zero_page(A.device))
    a.M, a.N, a.K = M, N, K
    a.lda = K if lda is None else lda
    a.ldc = N if ldc is None else ldc
    a.a_mode = _lib.A_DENSE if conv is None else _lib.A_CONV3X3
    a.epilogue = epi
    a.relu_in = int(relu_in)
    if conv is not None:
        a.cB, a.cH, a.cW, a.cCin, a.cHo, a.cWo, a.cStride = conv
    a.P = P
    a.stats_ld, a.tile_rows = stats_ld, tile_rows      # a row range of a larger GEMM (vda_gemm_row_range's rules)
    if convt is not None:
        a.tK, a.tH, a.tW, a.tCout = convt
    if W.numel() < N * K:
        raise ValueError("W smaller than N*K")
    check(fn(C.byref(a), _stream(A)), f"{fname} M={M} N={N} K={K} epi={epi} conv={conv} lda={a.lda} ldc={a.ldc}" if _TRACE else fname)


def split_stats(x, hi, lo, stat, eps, rows, D, center=False):
    """fp32 rows -> the two fp16 planes of the split residual stream (x = hi + lo) and stat[r] = (mean, rstd).
    center=True: hi + lo = x - mean(x), stat[r] = (0, rstd) (the model's entry: the stream relative to each token's mean)."""
    _req(x, F32, "x"), _req(hi, F16, "hi"), _req(lo, F16, "lo"), _req(stat, F32, "stat")
    fn = lib.vda_split_center_stats_f32 if center else lib.vda_split_stats_f32
    check(fn(_p(x), _p(hi), _p(lo), _p(stat), eps, rows, D, _stream(x)), "vda_split_stats_f32")


def ln_stats_finalize(partial, stat, eps, rows, np_, overflow=None):
    """partial[np, r, 2] (sum, centred sum of squares per 64 columns) -> stat[r] = (mean, rstd)."""
    _req(partial, F32, "partial"), _req(stat, F32, "stat")
    check(lib.vda_ln_stats_finalize(_p(partial), _p(stat), eps, rows, np_, _p(overflow), _stream(partial)), "vda_ln_stats_finalize")


def layernorm_split(hi, lo, out, w, b, eps, rows, D, group=0, skip=0):
    """LayerNorm of x = hi + lo (fp32 statistics) -> fp16."""
    _req(hi, F16, "hi"), _req(lo, F16, "lo"), _req(out, F16, "out"), _req(w, F32, "w"), _req(b, F32, "b")
    check(lib.vda_layernorm_split_f16(_p(hi), _p(lo), _p(out), _p(w), _p(b), eps, rows, D, group, skip, _stream(hi)), "vda_layernorm_split_f16")


def layernorm_split_check(hi, lo, out, w, b, eps, rows, D, group=0, skip=0, overflow=None):
    """layernorm_split, and overflow[0] (int32, None = not asked) = 1 when a row it normalises holds a saturated element."""
    _req(hi, F16, "hi"), _req(lo, F16, "lo"), _req(out, F16, "out"), _req(w, F32, "w"), _req(b, F32, "b"), _req(overflow, torch.int32, "overflow")
    check(lib.vda_layernorm_split_check_f16(_p(hi), _p(lo), _p(out), _p(w), _p(b), eps, rows, D, group, skip, _p(overflow), _stream(hi)),
          "vda_layernorm_split_check_f16")


def fold_ln_weight(W, bias, ln_w, ln_b, Wf, c1, c2, N, K):
    """Wf = fp16(W * ln_w[None, :]), c1 = Wf.float().sum(1), c2 = bias + W @ ln_b (pack time)."""
    for t, n in ((W, "W"), (bias, "bias"), (ln_w, "ln_w"), (ln_b, "ln_b"), (c1, "c1"), (c2, "c2")):
        _req(t, F32, n)
    _req(Wf, F16, "Wf")
    check(lib.vda_fold_ln_weight(_p(W), _p(bias), _p(ln_w), _p(ln_b), _p(Wf), _p(c1), _p(c2), N, K, _stream(W)), "vda_fold_ln_weight")


def fold_convt_weight(wt, bt, wr, cin_pad=None):
    """ConvTranspose2d(k == stride) weight wt [Ci,Cm,k,k] and bias bt [Cm] composed with the bias-free 3x3 conv weight wr [Co,Cm,3,3]
    behind it, on the device (vda_fold_convt_weight): (Wf fp16 [k*k*Co, 9*cin_pad], Bc fp32 [k*k, 9, Co]) for VDA_EPI_CONVT_FOLD_F16."""
    _req(wt, F32, "wt"), _req(bt, F32, "bt"), _req(wr, F32, "wr")
    Ci, Cm, k, _ = wt.shape
    Co = wr.shape[0]
    if wr.shape[1] != Cm or bt.numel() != Cm or tuple(wr.shape[2:]) != (3, 3) or wt.shape[3] != k:
        raise ValueError("fold_convt_weight: wt [Ci,Cm,k,k], bt [Cm], wr [Co,Cm,3,3]")
    cin_pad = Ci if cin_pad is None else cin_pad
    wf = torch.empty(k * k * Co, 9 * cin_pad, dtype=F16, device=wt.device)
    bc = torch.empty(k * k, 9, Co, dtype=F32, device=wt.device)
    check(lib.vda_fold_convt_weight(_p(wt), _p(bt), _p(wr), _p(wf), _p(bc), k, Ci, Cm, Co, cin_pad, _stream(wt)), "vda_fold_convt_weight")
    return wf, bc


def fold_oc1_weight(w1, wo, bo, cout_pad=None, ldz=None):
    """output_conv1's weight w1 [Fh,Fe,3,3] composed with refinenet1's out_conv (wo [Fe,Fe,1,1], bo [Fe]) on the device
    (vda_fold_oc1_weight): (Wz fp16 [ldz, Fe] with rows (tap, cout), zero from 9*cout_pad on, bz fp32 [ldz]) for the z GEMM of option
    oc1_mix. ldz: z's row, default vda_oc1_mix_ldz(cout_pad)."""
    _req(w1, F32, "w1"), _req(wo, F32, "wo"), _req(bo, F32, "bo")
    Fh, Fe = w1.shape[0], w1.shape[1]
    if tuple(w1.shape[2:]) != (3, 3) or wo.numel() != Fe * Fe or bo.numel() != Fe:
        raise ValueError("fold_oc1_weight: w1 [Fh,Fe,3,3], wo [Fe,Fe(,1,1)], bo [Fe]")
    Fhp = Fh if cout_pad is None else cout_pad
    ldz = lib.vda_oc1_mix_ldz(Fhp) if ldz is None else ldz
    wz = torch.empty(ldz, Fe, dtype=F16, device=w1.device)
    bz = torch.empty(ldz, dtype=F32, device=w1.device)
    check(lib.vda_fold_oc1_weight(_p(w1), _p(wo), _p(bo), _p(wz), _p(bz), Fh, Fe, Fhp, ldz, _stream(w1)), "vda_fold_oc1_weight")
    return wz, bz


def oc1_mix_combine(z, bias, out, B, h, w, Fhp, ldz=None):
    """out [B,2h,2w,Fhp] = bias + the sum over the 3x3 taps inside the map of the 2x align_corners interpolation of z [B,h,w,ldz]'s
    tap plane (vda_oc1_mix_combine_f16; ldz defaults to 9*Fhp)."""
    ldz = 9 * Fhp if ldz is None else ldz
    _req(z, F16, "z"), _req(out, F16, "out"), _req(bias, F32, "bias")
    if z.numel() < B * h * w * ldz or out.numel() < B * 4 * h * w * Fhp or (bias is not None and bias.numel() < Fhp):
        raise ValueError("oc1_mix_combine buffers too small")
    check(lib.vda_oc1_mix_combine_f16(_p(z), _p(bias), _p(out), B, h, w, Fhp, ldz, _stream(z)), "vda_oc1_mix_combine_f16")


def mlp_permute_w2(w2, w2p, D, hidden):
    """fc2's weight [D, hidden] with its hidden columns in the order the fused MLP kernel's register-resident activations have."""
    _req(w2, F16, "w2"), _req(w2p, F16, "w2p")
    check(lib.vda_mlp_permute_w2_f16(_p(w2), _p(w2p), D, hidden, _stream(w2)), "vda_mlp_permute_w2_f16")


def mlp_fused(hi_in, stats, w1, c1, c2, w2p, b2, gamma, hi, lo, part, M, D, hidden, stats_ld=None):
    """hi + lo += gamma * (fc2(GELU(fc1(LayerNorm(hi + lo)))) + b2) in one kernel (vda_mlp_fused_f16: see include/vda.h)."""
    for t, n in ((hi_in, "hi_in"), (w1, "w1"), (w2p, "w2p"), (hi, "hi"), (lo, "lo")):
        _req(t, F16, n)
    for t, n in ((stats, "stats"), (c1, "c1"), (c2, "c2"), (b2, "b2"), (gamma, "gamma"), (part, "part")):
        _req(t, F32, n)
    check(lib.vda_mlp_fused_f16(_p(hi_in), _p(stats), _p(w1), _p(c1), _p(c2), _p(w2p), _p(b2), _p(gamma), _p(hi), _p(lo), _p(part), M, D, hidden,
                                M if stats_ld is None else stats_ld, _stream(hi)), "vda_mlp_fused_f16")


def layernorm(x, out, w, b, eps, rows, D, group=0, skip=0, pe=None, pe_rows_per_step=0, pe_steps=0):
    _req(x, F32, "x"), _act(out, "out"), _req(w, F32, "w"), _req(b, F32, "b"), _req(pe, F32, "pe")
    fn = lib.vda_layernorm_f32_f32 if out.dtype == F32 else lib.vda_layernorm_f32_f16
    check(fn(_p(x), _p(out), _p(w), _p(b), eps, rows, D, group, skip, _p(pe), pe_rows_per_step, pe_steps, _stream(x)), "vda_layernorm")


def layernorm_residual(x, y, gamma, out, w, b, eps, rows, D, group=0, skip=0):
    """x += gamma * y (x fp32 in place, y fp16), out = LayerNorm(x) fp16."""
    _req(x, F32, "x"), _req(y, F16, "y"), _req(gamma, F32, "gamma"), _req(out, F16, "out"), _req(w, F32, "w"), _req(b, F32, "b")
    if x.numel() < rows * D or y.numel() < rows * D:
        raise ValueError("layernorm_residual buffers too small")
    check(lib.vda_layernorm_residual_f32_f16(_p(x), _p(y), _p(gamma), _p(out), _p(w), _p(b), eps, rows, D, group, skip, _stream(x)),
          "vda_layernorm_residual_f32_f16")


def groupnorm(x, out, w, b, eps, frames, hw, Cc, groups, partial, chunks):
    _act(x, "x"), _req(out, x.dtype, "out"), _req(w, F32, "w"), _req(b, F32, "b"), _req(partial, F32, "partial")
    if partial.numel() < frames * chunks * groups * 2:
        raise ValueError("groupnorm workspace too small")
    fn = lib.vda_groupnorm_nhwc_f32 if x.dtype == F32 else lib.vda_groupnorm_nhwc_f16
    check(fn(_p(x), _p(out), _p(w), _p(b), eps, frames, hw, Cc, groups, _p(partial), chunks, _stream(x)), "vda_groupnorm_nhwc")


def attention(qkv, out, B, N, heads):
    _act(qkv, "qkv"), _req(out, qkv.dtype, "out")
    if qkv.numel() < B * N * 3 * heads * 64 or out.numel() < B * N * heads * 64:
        raise ValueError("attention buffers too small")
    fn = lib.vda_attention_f32 if qkv.dtype == F32 else lib.vda_attention_f16
    check(fn(_p(qkv), _p(out), B, N, heads, _stream(qkv)), "vda_attention")


def temporal_attention(qkv, out, T, hw, Cc, heads=8):
    _act(qkv, "qkv"), _req(out, qkv.dtype, "out")
    if qkv.numel() < T * hw * 3 * Cc or out.numel() < T * hw * Cc:
        raise ValueError("temporal attention buffers too small")
    fn = lib.vda_temporal_attention_f32 if qkv.dtype == F32 else lib.vda_temporal_attention_f16
    check(fn(_p(qkv), _p(out), T, hw, Cc, heads, _stream(qkv)), "vda_temporal_attention")


def rope_qk(qkv, T, hw, Cc):
    """pe='rope': rotate the q and k thirds of qkv [T*hw, 3*C] in place (motion_module/attention.py:403-429)."""
    _act(qkv, "qkv")
    if qkv.numel() < T * hw * 3 * Cc:
        raise ValueError("rope_qk buffer too small")
    fn = lib.vda_rope_qk_f32 if qkv.dtype == F32 else lib.vda_rope_qk_f16
    check(fn(_p(qkv), T, hw, Cc, _stream(qkv)), "vda_rope_qk")


def bilinear_nhwc(x, out, B, h, w, H, W, Cc, add=None):
    _act(x, "x"), _req(out, x.dtype, "out"), _req(add, x.dtype, "add")
    fn = lib.vda_bilinear_nhwc_f32 if x.dtype == F32 else lib.vda_bilinear_nhwc_f16
    check(fn(_p(x), _p(out), _p(add), B, h, w, H, W, Cc, _stream(x)), "vda_bilinear_nhwc")


def bilinear_plane(x, out, B, h, w, H, W, relu=False):
    _req(x, F32, "x"), _req(out, F32, "out")
    check(lib.vda_bilinear_plane_f32(_p(x), _p(out), B, h, w, H, W, 1 if relu else 0, _stream(x)), "vda_bilinear_plane_f32")


def patchify(x, out, B, H, W, Kpad):
    _req(x, F32, "x"), _act(out, "out")
    fn = lib.vda_patchify_f32_f32 if out.dtype == F32 else lib.vda_patchify_f32_f16
    check(fn(_p(x), _p(out), B, H, W, Kpad, _stream(x)), "vda_patchify")


def pos_embed_resample(pe, out, g, ph, pw, D):
    """dinov2.py:185-210: pe fp32 [1 + g*g, D] -> out fp32 [1 + ph*pw, D]."""
    _req(pe, F32, "pe"), _req(out, F32, "out")
    if pe.numel() < (1 + g * g) * D or out.numel() < (1 + ph * pw) * D:
        raise ValueError("pos_embed_resample buffers too small")
    check(lib.vda_pos_embed_resample_f32(_p(pe), _p(out), g, ph, pw, D, _stream(pe)), "vda_pos_embed_resample_f32")


def cls_rows(tok, cls, pos, B, P, D):
    _req(tok, F32, "tok"), _req(cls, F32, "cls"), _req(pos, F32, "pos")
    check(lib.vda_cls_rows_f32(_p(tok), _p(cls), _p(pos), B, P, D, _stream(tok)), "vda_cls_rows_f32")


def readout_concat(tok, out, frames, P, D):
    """[frames*(P+1), D] (cls first) -> [frames*P, 2D] = cat(patch token, the frame's cls token)."""
    _act(tok, "tok"), _req(out, tok.dtype, "out")
    if tok.numel() < frames * (P + 1) * D or out.numel() < frames * P * 2 * D:
        raise ValueError("readout_concat buffers too small")
    fn = lib.vda_readout_concat_f32 if tok.dtype == F32 else lib.vda_readout_concat_f16
    check(fn(_p(tok), _p(out), frames, P, D, _stream(tok)), "vda_readout_concat")


def head_out(x, w, bias, out, rows, Cpad):
    _act(x, "x"), _req(w, F32, "w"), _req(out, F32, "out")
    fn = lib.vda_head_out_f32_f32 if x.dtype == F32 else lib.vda_head_out_f16_f32
    check(fn(_p(x), _p(w), float(bias), _p(out), rows, Cpad, _stream(x)), "vda_head_out")


def depth_tail(x, w2, b2, w3, b3, out, B, h, w, H, W, Cc):
    """[resize h x w -> H x W] + conv3x3(C->32)+ReLU + conv1x1(32->1)+ReLU, NHWC fp16 in, fp32 [B,H,W] out."""
    _req(x, F16, "x"), _req(w2, F16, "w2"), _req(b2, F32, "b2"), _req(w3, F32, "w3"), _req(out, F32, "out")
    if x.numel() < B * h * w * Cc or out.numel() < B * H * W or w2.numel() < 32 * 9 * Cc:
        raise ValueError("depth_tail buffers too small")
    check(lib.vda_depth_tail_f16(_p(x), _p(w2), _p(b2), _p(w3), float(b3), _p(out), _p(zero_page(x.device)), B, h, w, H, W, Cc,
                                 _stream(x)), "vda_depth_tail_f16")


def conv3x3_up2(x, w, bias, out, B, h, wd, Cc, N, ldc):
    """out [B,2h,2w,ldc] = conv3x3(bilinear 2x, align_corners, of x [B,h,wd,C]) + bias: output_conv1 over refinenet1's upsample."""
    _req(x, F16, "x"), _req(w, F16, "w"), _req(out, F16, "out")
    if bias is not None:
        _req(bias, F32, "bias")
    if x.numel() < B * h * wd * Cc or out.numel() < B * 4 * h * wd * ldc or w.numel() < N * 9 * Cc:
        raise ValueError("conv3x3_up2 buffers too small")
    check(lib.vda_conv3x3_up2_f16(_p(x), _p(w), _p(bias) if bias is not None else None, _p(out), B, h, wd, Cc, N, ldc, _stream(x)),
          "vda_conv3x3_up2_f16")


def normalize_u8(frames, out, n, H, W):
    _req(frames, torch.uint8, "frames"), _req(out, F32, "out")
    check(lib.vda_normalize_u8_f32(_p(frames), _p(out), n, H, W, _stream(frames)), "vda_normalize_u8_f32")


def gather_normalize_u8(video, idx, out, n, H, W):
    _req(video, torch.uint8, "video"), _req(idx, torch.int32, "idx"), _req(out, F32, "out")
    if idx.numel() < n or out.numel() < n * 3 * H * W:
        raise ValueError("gather_normalize buffers too small")
    check(lib.vda_gather_normalize_u8_f32(_p(video), _p(idx), _p(out), n, video.shape[0], H, W, _stream(video)), "vda_gather_normalize_u8_f32")


def gather_resize_normalize_u8(video, idx, out, n, H0, W0, H, W):
    """Window gather + bicubic resize to the network size + normalise: uint8 [N,H0,W0,3] -> fp32 [n,3,H,W]."""
    _req(video, torch.uint8, "video"), _req(idx, torch.int32, "idx"), _req(out, F32, "out")
    if idx.numel() < n or out.numel() < n * 3 * H * W or video.numel() < video.shape[0] * H0 * W0 * 3:
        raise ValueError("gather_resize_normalize buffers too small")
    check(lib.vda_gather_resize_normalize_u8_f32(_p(video), _p(idx), _p(out), n, video.shape[0], H0, W0, H, W, _stream(video)),
          "vda_gather_resize_normalize_u8_f32")


LSQ_BLOCKS = 256


def lsq_scale_shift(pred, target, workspace, scale_shift):
    """scale_shift[0..1] (device fp32) = least-squares fit target ~ scale*pred + shift over all elements."""
    _req(pred, F32, "pred"), _req(target, F32, "target"), _req(workspace, torch.float64, "workspace"), _req(scale_shift, F32, "scale_shift")
    if pred.numel() != target.numel() or workspace.numel() < 4 * LSQ_BLOCKS or scale_shift.numel() < 2:
        raise ValueError("lsq_scale_shift: mismatched sizes")
    check(lib.vda_lsq_scale_shift_f32(_p(pred), _p(target), pred.numel(), _p(workspace), LSQ_BLOCKS, _p(scale_shift), _stream(pred)),
          "vda_lsq_scale_shift_f32")


def stitch_window(win, scale_shift, chunk, tail, ref1, px, wts):
    """Affine + clamp + cross-fade + append of one window (k > 0); see include/vda.h."""
    for t, nm in ((win, "win"), (scale_shift, "scale_shift"), (chunk, "chunk"), (tail, "tail"), (ref1, "ref1"), (wts, "wts")):
        _req(t, F32, nm)
    if win.numel() < 32 * px or chunk.numel() < 22 * px or tail.numel() < 8 * px or ref1.numel() < px or wts.numel() < 16:
        raise ValueError("stitch_window buffers too small")
    check(lib.vda_stitch_window_f32(_p(win), _p(scale_shift), _p(chunk), _p(tail), _p(ref1), px, _p(wts), _stream(win)), "vda_stitch_window_f32")


def affine_clamp(x, scale_shift, out):
    """out = max(x * scale + shift, 0) elementwise (the stitch's alignment of a frame), device scale_shift[2]."""
    _req(x, F32, "x"), _req(scale_shift, F32, "scale_shift"), _req(out, F32, "out")
    if out.numel() < x.numel() or scale_shift.numel() < 2:
        raise ValueError("affine_clamp buffers too small")
    check(lib.vda_affine_clamp_f32(_p(x), _p(scale_shift), _p(out), x.numel(), _stream(x)), "vda_affine_clamp_f32")


def minmax_accum(x, minmax, n=None):
    """minmax[0] = min(minmax[0], x[:n].min()), minmax[1] = max(minmax[1], x[:n].max()) over the first n elements of x (all of them
    when n is None); minmax: device fp32 [2], started at (+inf, -inf) by the caller. Exact; see include/vda.h."""
    _req(x, F32, "x"), _req(minmax, F32, "minmax")
    n = x.numel() if n is None else int(n)
    if n <= 0 or n > x.numel() or minmax.numel() < 2:
        raise ValueError("minmax_accum: bad sizes")
    check(lib.vda_minmax_accum_f32(_p(x), n, _p(minmax), _stream(x)), "vda_minmax_accum_f32")


# ---- benchmark scorer (csrc/eval.hip; evaluate.py lays the partial rows out) ------------------------------------------------
def _eval_pair(pred, gt, what):
    _req(pred, F32, "pred")
    if gt.dtype not in (F32, torch.float64):
        raise ValueError(f"{what}: gt must be float32 or float64, got {gt.dtype}")
    _req(gt, gt.dtype, "gt")
    if pred.shape != gt.shape or pred.device != gt.device or pred.numel() == 0:
        raise ValueError(f"{what}: pred {tuple(pred.shape)} on {pred.device} and gt {tuple(gt.shape)} on {gt.device} do not match")
    return int(gt.dtype == torch.float64)


def eval_lsq_partial(pred, gt, max_depth, workspace, row_offset, nblk):
    """Pass 1 of the scorer over all elements of pred / gt: nblk rows of 5 doubles at workspace[5 * row_offset ...]."""
    f64 = _eval_pair(pred, gt, "eval_lsq_partial")
    _req(workspace, torch.float64, "workspace")
    if row_offset < 0 or nblk <= 0 or workspace.numel() < 5 * (row_offset + nblk):
        raise ValueError("eval_lsq_partial: workspace too small")
    check(lib.vda_eval_lsq_partial(_p(pred), _p(gt), f64, pred.numel(), float(max_depth), _p(workspace), row_offset, nblk, _stream(pred)),
          "vda_eval_lsq_partial")


def eval_lsq_finish(workspace, nrows, fit):
    """fit[0..2] (device fp64) = {scale, shift, n_valid} from the first nrows rows of pass 1."""
    _req(workspace, torch.float64, "workspace"), _req(fit, torch.float64, "fit")
    if nrows <= 0 or workspace.numel() < 5 * nrows or fit.numel() < 3:
        raise ValueError("eval_lsq_finish: bad sizes")
    check(lib.vda_eval_lsq_finish(_p(workspace), nrows, _p(fit), _stream(workspace)), "vda_eval_lsq_finish")


def eval_metric_partial(pred, gt, max_depth, fit, workspace, frame_offset, blocks_per_frame):
    """Pass 2 of the scorer over pred / gt [n,H,W]: 7 doubles per (frame, block) at workspace[7 * frame_offset * blocks_per_frame ...]."""
    f64 = _eval_pair(pred, gt, "eval_metric_partial")
    _req(workspace, torch.float64, "workspace"), _req(fit, torch.float64, "fit")
    if pred.dim() != 3:
        raise ValueError("eval_metric_partial: pred must be [n,H,W]")
    n, px = pred.shape[0], pred.shape[1] * pred.shape[2]
    if frame_offset < 0 or blocks_per_frame <= 0 or workspace.numel() < 7 * (frame_offset + n) * blocks_per_frame or fit.numel() < 3:
        raise ValueError("eval_metric_partial: workspace too small")
    check(lib.vda_eval_metric_partial(_p(pred), _p(gt), f64, n, px, float(max_depth), _p(fit), _p(workspace), frame_offset, blocks_per_frame,
                                      _stream(pred)), "vda_eval_metric_partial")


def eval_metric_finish(workspace, nframes, blocks_per_frame, result):
    """result[0..6] (device fp64) = {abs_rel, sq_rel, rmse, delta1, delta2, delta3, frames used} from pass 2's rows."""
    _req(workspace, torch.float64, "workspace"), _req(result, torch.float64, "result")
    if nframes <= 0 or blocks_per_frame <= 0 or workspace.numel() < 7 * nframes * blocks_per_frame or result.numel() < 7:
        raise ValueError("eval_metric_finish: bad sizes")
    check(lib.vda_eval_metric_finish(_p(workspace), nframes, blocks_per_frame, _p(result), _stream(workspace)), "vda_eval_metric_finish")


# ---- temporal alignment error (csrc/tae.hip; evaluate.py cuts the pairs into chunks and lays the partial rows out) ------------
def _tae_planes(pred, fit, cam, winner, what):
    """Checks shared by the two passes; returns (pairs, H, W) of pred [pairs + 1, H, W]."""
    _req(pred, F32, "pred"), _req(fit, torch.float64, "fit"), _req(cam, torch.float64, "cam"), _req(winner, torch.int32, "winner")
    if pred.dim() != 3 or pred.shape[0] < 2 or pred.shape[1] * pred.shape[2] == 0:
        raise ValueError(f"{what}: pred must be [pairs + 1, H, W], got {tuple(pred.shape)}")
    n, H, W = pred.shape[0] - 1, pred.shape[1], pred.shape[2]
    if fit.numel() < 2 or cam.numel() < 28 * n or winner.numel() < 2 * n * H * W:
        raise ValueError(f"{what}: fit, cam or winner too small for {n} pairs of {H} x {W}")
    return n, H, W


def tae_splat(pred, max_depth, fit, cam, winner):
    """Clears winner (int32 [2 * pairs, H, W]) and splats both directions of every neighbouring pair of pred [pairs + 1, H, W]
    into it: winner[plane, v, u] = 1 + the largest source index that lands on (v, u). cam: fp64 [pairs, 28] (include/vda.h)."""
    n, H, W = _tae_planes(pred, fit, cam, winner, "tae_splat")
    check(lib.vda_tae_splat(_p(pred), n, H, W, float(max_depth), _p(fit), _p(cam), _p(winner), _stream(pred)), "vda_tae_splat")


def tae_compare(pred, mask, max_depth, fit, cam, winner, workspace, pair_offset, blocks_per_plane):
    """Compares each plane's splat with the target frame: 2 doubles per (plane, block) at workspace[4 * pair_offset *
    blocks_per_plane ...]. mask: uint8 of pred's shape (0 = excluded) or None."""
    n, H, W = _tae_planes(pred, fit, cam, winner, "tae_compare")
    _req(workspace, torch.float64, "workspace"), _req(mask, torch.uint8, "mask")
    if mask is not None and mask.shape != pred.shape:
        raise ValueError(f"tae_compare: mask {tuple(mask.shape)} and pred {tuple(pred.shape)} differ in shape")
    if pair_offset < 0 or blocks_per_plane <= 0 or workspace.numel() < 4 * (pair_offset + n) * blocks_per_plane:
        raise ValueError("tae_compare: workspace too small")
    check(lib.vda_tae_compare(_p(pred), _p(mask), n, H, W, float(max_depth), _p(fit), _p(cam), _p(winner), _p(workspace), pair_offset,
                              blocks_per_plane, _stream(pred)), "vda_tae_compare")


def tae_finish(workspace, npairs, blocks_per_plane, result):
    """result (device fp64 [1 + 4 * npairs]) = {tae, error per plane, count per plane} from the compare pass's rows."""
    _req(workspace, torch.float64, "workspace"), _req(result, torch.float64, "result")
    if npairs <= 0 or blocks_per_plane <= 0 or workspace.numel() < 4 * npairs * blocks_per_plane or result.numel() < 1 + 4 * npairs:
        raise ValueError("tae_finish: bad sizes")
    check(lib.vda_tae_finish(_p(workspace), npairs, blocks_per_plane, _p(result), _stream(workspace)), "vda_tae_finish")


# ---- a prediction resized to the ground truth's grid (csrc/resize.hip) ---------------------------------------------------------
def resize_linear(x, out):
    """out [n,H,W] = x [n,h,w] resized with cv2's INTER_LINEAR arithmetic for float32 (include/vda.h); both device fp32, distinct."""
    _req(x, F32, "x"), _req(out, F32, "out")
    if x.dim() != 3 or out.dim() != 3 or x.shape[0] != out.shape[0] or x.numel() == 0 or out.numel() == 0 or x.device != out.device:
        raise ValueError(f"resize_linear: x {tuple(x.shape)} on {x.device} and out {tuple(out.shape)} on {out.device} must be [n,h,w] and [n,H,W]")
    (n, h, w), (H, W) = x.shape, out.shape[1:]
    check(lib.vda_resize_linear_f32(_p(x), _p(out), n, h, w, H, W, _stream(x)), "vda_resize_linear_f32")


# ---- frames scaled to max_res (csrc/resize_u8.hip) -------------------------------------------------------------------------------
def resize_linear_u8(x, out):
    """out [n,H,W,3] or [n,H,W] = x [n,h,w,3] or [n,h,w] resized with cv2's INTER_LINEAR arithmetic for 8-bit images
    (include/vda.h); both device uint8, contiguous (any byte offset), distinct, of one rank."""
    _req(x, torch.uint8, "x"), _req(out, torch.uint8, "out")
    if (x.dim() not in (3, 4) or out.dim() != x.dim() or x.shape[0] != out.shape[0] or x.numel() == 0 or out.numel() == 0
            or x.device != out.device or (x.dim() == 4 and (x.shape[3] != 3 or out.shape[3] != 3))):
        raise ValueError(f"resize_linear_u8: x {tuple(x.shape)} on {x.device} and out {tuple(out.shape)} on {out.device} must be "
                         "[n,h,w,3] and [n,H,W,3], or [n,h,w] and [n,H,W]")
    (n, h, w), (H, W) = x.shape[:3], out.shape[1:3]
    check(lib.vda_resize_linear_u8(_p(x), _p(out), n, h, w, 3 if x.dim() == 4 else 1, H, W, _stream(x)), "vda_resize_linear_u8")


# ---- metric depth unprojected to PLY vertex records (csrc/pointcloud.hip) -------------------------------------------------------
def pointcloud_frame_stride(h, w, record_f32):
    """Bytes of one frame's slot in the record buffer: h * w records of 15 (record_f32) or 27 bytes, rounded up to 16."""
    return int(lib.vda_pointcloud_frame_stride(h, w, int(bool(record_f32))))


def pointcloud_workspace_bytes(n, h, w):
    return int(lib.vda_pointcloud_workspace_bytes(n, h, w))


def pointcloud(depth, rgb, records, counts, workspace, fx, fy, cx, cy, max_depth=None, record_f32=False):
    """records (device uint8, n slots of pointcloud_frame_stride bytes) and counts (device int32 [n]) = the PLY vertex records of
    depth [n,h,w] (device fp32) coloured by rgb [n,h,w,3] (device uint8): include/vda.h. max_depth None keeps every pixel."""
    _req(depth, F32, "depth"), _req(rgb, torch.uint8, "rgb"), _req(records, torch.uint8, "records"), _req(counts, torch.int32, "counts")
    _req(workspace, torch.uint8, "workspace")
    if depth.dim() != 3 or depth.numel() == 0 or tuple(rgb.shape) != tuple(depth.shape) + (3,):
        raise ValueError(f"pointcloud: depth {tuple(depth.shape)} and rgb {tuple(rgb.shape)} must be [n,h,w] and [n,h,w,3]")
    _same_device("pointcloud", depth, rgb, records, counts, workspace)
    n, h, w = depth.shape
    if counts.numel() < n or records.numel() < n * pointcloud_frame_stride(h, w, record_f32):
        raise ValueError(f"pointcloud: counts ({counts.numel()}) or records ({records.numel()} bytes) too small for {n} frames of {h} x {w}")
    check(lib.vda_pointcloud_f32(_p(depth), _p(rgb), _p(records), _p(counts), _p(workspace), workspace.numel(), n, h, w, float(fx), float(fy),
                                 float(cx), float(cy), 0.0 if max_depth is None else float(max_depth), int(bool(record_f32)), _stream(depth)),
          "vda_pointcloud_f32")


# ---- depth mapped to visualisation bytes (csrc/visualize.hip) -------------------------------------------------------------------
def depth_vis(depth, minmax, lut, out, n=None):
    """out (device uint8) = the first n pixels of depth (device fp32; all of them when n is None) mapped through minmax (device fp32
    [2], as minmax_accum leaves it) to levels 0..255, n bytes - or, with lut (device uint8 [256,3]), to lut rows, 3 n bytes packed
    RGB: include/vda.h. depth and out may be views at any element / byte offset of a larger buffer."""
    _req(depth, F32, "depth"), _req(minmax, F32, "minmax"), _req(lut, torch.uint8, "lut"), _req(out, torch.uint8, "out")
    n = depth.numel() if n is None else int(n)
    if n <= 0 or n > depth.numel() or minmax.numel() < 2 or out.numel() < n * (1 if lut is None else 3):
        raise ValueError(f"depth_vis: bad sizes (n={n} of {depth.numel()} pixels, minmax {minmax.numel()}, out {out.numel()} bytes)")
    if lut is not None and tuple(lut.shape) != (256, 3):
        raise ValueError(f"depth_vis: lut must be [256,3], got {tuple(lut.shape)}")
    _same_device("depth_vis", depth, minmax, out, lut)
    check(lib.vda_depth_vis_u8(_p(depth), n, _p(minmax), _p(lut), _p(out), _stream(depth)), "vda_depth_vis_u8")


# ---- frames as baseline JPEG scans (csrc/mjpeg.hip; mjpeg.py is the contract and owns the header and the container) ------------
def mjpeg_workspace_bytes(n, h, w, channels):
    return int(lib.vda_mjpeg_workspace_bytes(n, h, w, channels))


def mjpeg_out_bytes(n, h, w, channels):
    """The capacity mjpeg_encode's `out` needs for n frames: no stream of that shape is longer."""
    return int(lib.vda_mjpeg_out_bytes(n, h, w, channels))


def mjpeg_encode(frames, qtables, workspace, out, lengths):
    """out (device uint8) = the JPEG scans (entropy-coded data + EOI) of frames (device uint8 [n,h,w,3] RGB or [n,h,w] gray) back
    to back, lengths (device int64 [n]) their sizes: include/vda.h. qtables: HOST numpy uint16 [2,64] ([1,64] for gray), natural order."""
    import numpy as np
    _req(frames, torch.uint8, "frames"), _req(workspace, torch.uint8, "workspace"), _req(out, torch.uint8, "out"), _req(lengths, torch.int64, "lengths")
    if frames.dim() not in (3, 4) or (frames.dim() == 4 and frames.shape[3] != 3) or frames.numel() == 0:
        raise ValueError(f"mjpeg_encode: frames must be [n,h,w,3] or [n,h,w] and not empty, got {tuple(frames.shape)}")
    n, h, w = frames.shape[:3]
    ch = 3 if frames.dim() == 4 else 1
    _host_array(qtables, np.uint16, 64 * (2 if ch == 3 else 1), "qtables", "mjpeg_encode")
    if lengths.numel() < n:
        raise ValueError(f"mjpeg_encode: lengths holds {lengths.numel()} entries, needs {n}")
    _same_device("mjpeg_encode", frames, workspace, out, lengths)
    check(lib.vda_mjpeg_encode_u8(_p(frames), n, h, w, ch, qtables.ctypes.data_as(C.c_void_p), _p(workspace), workspace.numel(), _p(out), out.numel(),
                                  _p(lengths), _stream(frames)), "vda_mjpeg_encode_u8")


# ---- baseline JPEG scans back to pixels (csrc/mjpeg_decode.hip; mjpeg.py parses the headers and is the contract) ----------------
def mjpeg_decode_workspace_bytes(n, h, w, components, hs, vs, intervals):
    return int(lib.vda_mjpeg_decode_workspace_bytes(n, h, w, components, hs, vs, intervals))


def mjpeg_decode(scan, intervals, tables, qtables, hs, vs, workspace, out, status):
    """out (device uint8 [n,h,w,3] or [n,h,w]) = the pixels of the n frames whose scans lie back to back in scan (device uint8),
    status (device int32 [n]) their decode status: include/vda.h. HOST numpy: intervals int32 [k,5], tables one
    mjpeg.TABLES_DTYPE record, qtables uint16 [components,64] in natural order."""
    import numpy as np
    from .mjpeg import TABLES_DTYPE
    _req(scan, torch.uint8, "scan"), _req(workspace, torch.uint8, "workspace"), _req(out, torch.uint8, "out"), _req(status, torch.int32, "status")
    if out.dim() not in (3, 4) or (out.dim() == 4 and out.shape[3] != 3) or out.numel() == 0:
        raise ValueError(f"mjpeg_decode: out must be [n,h,w,3] or [n,h,w] and not empty, got {tuple(out.shape)}")
    n, h, w = out.shape[:3]
    ch = 3 if out.dim() == 4 else 1
    _host_array(intervals, np.int32, (None, 5), "intervals", "mjpeg_decode", "a contiguous host int32 array [k,5]")
    _host_array(tables, TABLES_DTYPE, 1, "tables", "mjpeg_decode", "one host record of mjpeg.TABLES_DTYPE")
    _host_array(qtables, np.uint16, 64 * ch, "qtables", "mjpeg_decode")
    if status.numel() < n:
        raise ValueError(f"mjpeg_decode: status holds {status.numel()} entries, needs {n}")
    _same_device("mjpeg_decode", scan, workspace, out, status)
    tables = np.ascontiguousarray(tables)
    check(lib.vda_mjpeg_decode_u8(_p(scan), scan.numel(), intervals.ctypes.data_as(C.c_void_p), intervals.shape[0], tables.ctypes.data_as(C.c_void_p),
                                  qtables.ctypes.data_as(C.c_void_p), n, h, w, ch, hs, vs, _p(workspace), workspace.numel(), _p(out), out.numel(),
                                  _p(status), _stream(scan)), "vda_mjpeg_decode_u8")


# ---- raw deflate of a device buffer (csrc/deflate.hip; deflate.py is the contract and owns the .npz container) --------------------
def deflate_workspace_bytes(n):
    return int(lib.vda_deflate_workspace_bytes(n))


def deflate_out_bytes(n):
    """The capacity deflate's `out` needs for n input bytes: no stream of them is longer."""
    return int(lib.vda_deflate_out_bytes(n))


def deflate(data, final, workspace, out, length, crcs):
    """data uint8 [n] (n may be 0; any byte offset of a larger tensor) -> out uint8 [>= deflate_out_bytes(n)]: the raw deflate stream,
    length int64 [1] its size, crcs int32 [>= max(1, ceil(n / 16384))] the CRC-32 of every 16384-byte chunk of the INPUT (as
    unsigned bits); workspace: deflate_workspace_bytes(n) bytes. final=False leaves a byte-aligned piece that a later call continues."""
    for t, name in ((data, "data"), (workspace, "workspace"), (out, "out")):
        _req(t, torch.uint8, name)
    _req(length, torch.int64, "length"), _req(crcs, torch.int32, "crcs")
    if data.dim() != 1:
        raise ValueError(f"deflate: data must be one axis of bytes, got {tuple(data.shape)}")
    n = data.numel()
    if length.numel() < 1 or crcs.numel() < max(1, -(-n // 16384)):
        raise ValueError(f"deflate: length holds {length.numel()} entries (needs 1), crcs {crcs.numel()} (needs {max(1, -(-n // 16384))})")
    _same_device("deflate", data, workspace, out, length, crcs)
    check(lib.vda_deflate_u8(_p(data), n, 1 if final else 0, _p(workspace), workspace.numel(), _p(out), out.numel(), _p(length), _p(crcs),
                             _stream(out)), "vda_deflate_u8")


# ---- OpenEXR ZIP files from float32 depth (csrc/exr.hip; exr.py is the contract and owns the header and the files) --------------
def exr_workspace_bytes(frames, h, w):
    return int(lib.vda_exr_workspace_bytes(frames, h, w))


def exr_payload_bytes(frames, h, w):
    """The capacity exr_zip's `payload` needs: every block raw, frames * (16 ceil(h / 16) + 4 w h)."""
    return int(lib.vda_exr_payload_bytes(frames, h, w))


def exr_zip(depth, header_bytes, workspace, payload, offsets):
    """depth fp32 [frames, h, w] whose frames are dense (any stride between frames, any dword offset of a larger tensor) -> payload
    uint8 [>= exr_payload_bytes]: per frame the offset table and the blocks of an OpenEXR ZIP file whose header is `header_bytes` long;
    offsets int64 [frames + 1]: frame f's payload is payload[offsets[f]:offsets[f + 1]]. workspace: exr_workspace_bytes bytes."""
    if not isinstance(depth, torch.Tensor) or not depth.is_cuda or depth.dtype != F32 or depth.dim() != 3 or depth.numel() == 0:
        raise ValueError(f"exr_zip: depth must be a cuda fp32 tensor [frames, h, w], got {getattr(depth, 'dtype', type(depth))} "
                         f"{tuple(getattr(depth, 'shape', ()))} {getattr(depth, 'device', None)}")
    n, h, w = depth.shape
    if depth.stride(2) != 1 or depth.stride(1) != w or (n > 1 and depth.stride(0) < h * w):
        raise ValueError(f"exr_zip: the frames of depth must be dense, got strides {depth.stride()} for {tuple(depth.shape)}")
    _req(workspace, torch.uint8, "workspace"), _req(payload, torch.uint8, "payload"), _req(offsets, torch.int64, "offsets")
    if offsets.numel() < n + 1:
        raise ValueError(f"exr_zip: offsets holds {offsets.numel()} entries, needs {n + 1}")
    _same_device("exr_zip", depth, workspace, payload, offsets)
    check(lib.vda_exr_zip_f32(_p(depth), n, h, w, depth.stride(0) if n > 1 else h * w, int(header_bytes), _p(workspace), workspace.numel(),
                              _p(payload), payload.numel(), _p(offsets), _stream(payload)), "vda_exr_zip_f32")


# ---- validation losses (csrc/losses.hip; losses.py lays the buffers out) --------------------------------------------------------
LOSS_STATS = 8               # doubles per frame in `stats` (include/vda.h)


def _loss_planes(pred, y, mask, what):
    """Checks shared by the loss passes; pred / y device fp32 of one shape with at least two axes [.., H, W], mask uint8 or None.
    Returns (frames, H, W)."""
    _req(pred, F32, "pred"), _req(y, F32, "y"), _req(mask, torch.uint8, "mask")
    if pred.dim() < 3 or pred.shape != y.shape or pred.numel() == 0 or (mask is not None and mask.shape != pred.shape):
        raise ValueError(f"{what}: pred {tuple(pred.shape)}, y {tuple(y.shape)} and mask "
                         f"{None if mask is None else tuple(mask.shape)} must be one non-empty [..,H,W]")
    _same_device(what, pred, y, mask)
    H, W = pred.shape[-2:]
    return pred.numel() // (H * W), H, W


def _f64_room(t, n, name, what):
    _req(t, torch.float64, name)
    if t.numel() < n:
        raise ValueError(f"{what}: {name} holds {t.numel()} doubles, needs {n}")


def loss_lsq_pass(pred, y, mask, step, eps, stats, workspace, bpp, result=None):
    """Pass `step` (0 means, 1 centred sums, 2 residual) of the least-squares SSI loss and its finisher (include/vda.h)."""
    F, H, W = _loss_planes(pred, y, mask, "loss_lsq_pass")
    _f64_room(stats, LOSS_STATS * F, "stats", "loss_lsq_pass"), _f64_room(workspace, 3 * F * bpp, "workspace", "loss_lsq_pass")
    if step == 2:
        _f64_room(result, 1 + F, "result", "loss_lsq_pass")
    check(lib.vda_loss_lsq_partial(_p(pred), _p(y), _p(mask), F, H * W, step, _p(stats), _p(workspace), bpp, _stream(pred)), "vda_loss_lsq_partial")
    check(lib.vda_loss_lsq_finish(_p(workspace), F, bpp, step, float(eps), _p(stats), _p(result), _stream(pred)), "vda_loss_lsq_finish")


def loss_median(x, y, mask, med):
    """med (device fp32 [F] or, with y, [2 F]) = the exact masked lower medians of x's (and y's) planes."""
    F, H, W = _loss_planes(x, x if y is None else y, mask, "loss_median")
    _req(med, F32, "med")
    if med.numel() < (1 if y is None else 2) * F or med.device != x.device:
        raise ValueError(f"loss_median: med holds {med.numel()} floats on {med.device}, needs {(1 if y is None else 2) * F} on {x.device}")
    check(lib.vda_loss_median(_p(x), _p(y), _p(mask), F, H * W, _p(med), _stream(x)), "vda_loss_median")


def loss_mad(pred, y, mask, eps, med, stats, workspace, bpp, rows, result):
    """The median / mean-deviation SSI loss after loss_median: scales, per-image-row sums and the finisher (include/vda.h)."""
    F, H, W = _loss_planes(pred, y, mask, "loss_mad")
    _req(med, F32, "med")
    if med.numel() < 2 * F:
        raise ValueError("loss_mad: med too small")
    _f64_room(stats, LOSS_STATS * F, "stats", "loss_mad"), _f64_room(workspace, 3 * F * bpp, "workspace", "loss_mad")
    _f64_room(rows, 2 * F * H, "rows", "loss_mad"), _f64_room(result, 1 + F, "result", "loss_mad")
    s = _stream(pred)
    check(lib.vda_loss_mad_scale_partial(_p(pred), _p(y), _p(mask), F, H * W, _p(med), _p(workspace), bpp, s), "vda_loss_mad_scale_partial")
    check(lib.vda_loss_mad_scale_finish(_p(workspace), F, bpp, float(eps), _p(med), _p(stats), s), "vda_loss_mad_scale_finish")
    check(lib.vda_loss_mad_rows(_p(pred), _p(y), _p(mask), F, H, W, _p(stats), _p(rows), s), "vda_loss_mad_rows")
    check(lib.vda_loss_mad_finish(_p(rows), F, H, _p(result), s), "vda_loss_mad_finish")


def loss_tgm(pred, y, mask, workspace, bpp, result):
    """The temporal gradient matching loss of pred / y [B,N,H,W] (N >= 2): result = {tgm, per pair [B (N-1)], n_static [B (N-1)]}."""
    _loss_planes(pred, y, mask, "loss_tgm")
    if pred.dim() != 4 or pred.shape[1] < 2:
        raise ValueError(f"loss_tgm: pred must be [B,N,H,W] with N >= 2, got {tuple(pred.shape)}")
    B, N, H, W = pred.shape
    P = B * (N - 1)
    _f64_room(workspace, 3 * P * bpp, "workspace", "loss_tgm"), _f64_room(result, 1 + 2 * P, "result", "loss_tgm")
    check(lib.vda_loss_tgm_partial(_p(pred), _p(y), _p(mask), B, N, H * W, _p(workspace), bpp, _stream(pred)), "vda_loss_tgm_partial")
    check(lib.vda_loss_tgm_finish(_p(workspace), B, N, bpp, _p(result), _stream(pred)), "vda_loss_tgm_finish")


# ---------------------------------------------------------------------------
# Weight layouts the kernels expect (done once at load time, on the host or device)
# ---------------------------------------------------------------------------
def pad_to(n, m=64):
    return (n + m - 1) // m * m


def pack_linear(w, n_pad=None, k_pad=None, dtype=F16):
    """[N,K] fp32 -> `dtype` [Npad,Kpad], zero padded."""
    N, K = w.shape
    n_pad = N if n_pad is None else n_pad
    k_pad = K if k_pad is None else k_pad
    o = torch.zeros(n_pad, k_pad, dtype=dtype, device=w.device)
    o[:N, :K] = w.to(dtype)
    return o


def pack_conv3x3(w, cout_pad=None, cin_pad=None, dtype=F16):
    """Conv2d weight [Cout,Cin,3,3] -> `dtype` [Coutpad, 9*Cinpad] with K ordered (ky,kx,ci)."""
    Co, Ci = w.shape[:2]
    cout_pad = Co if cout_pad is None else cout_pad
    cin_pad = Ci if cin_pad is None else cin_pad
    o = torch.zeros(cout_pad, 3, 3, cin_pad, dtype=dtype, device=w.device)
    o[:Co, :, :, :Ci] = w.permute(0, 2, 3, 1).to(dtype)
    return o.reshape(cout_pad, 9 * cin_pad).contiguous()


def pack_convt(w, bias, cpad, dtype=F16):
    """ConvTranspose2d (k == stride) weight [Cin,Cout,k,k] -> `dtype` [(ky,kx,co) = k*k*cpad, cpad(ci)],
    bias expanded to the same row order."""
    Ci, Co, k, _ = w.shape
    o = torch.zeros(k, k, cpad, cpad, dtype=dtype, device=w.device)
    o[:, :, :Co, :Ci] = w.permute(2, 3, 1, 0).to(dtype)
    bb = torch.zeros(k, k, cpad, dtype=F32, device=w.device)
    bb[:, :, :Co] = bias.to(F32)
    return o.reshape(k * k * cpad, cpad).contiguous(), bb.reshape(-1).contiguous()


def pack_geglu(w, bias, dtype=F16):
    """GEGLU proj [8C, C]: rows [value(4C) | gate(4C)] -> interleaved [16 value | 16 gate] per 32 rows."""
    two_n, K = w.shape
    n = two_n // 2
    assert n % 16 == 0
    wv, wg = w[:n].reshape(n // 16, 16, K), w[n:].reshape(n // 16, 16, K)
    wi = torch.stack((wv, wg), dim=1).reshape(two_n, K)
    bv, bg = bias[:n].reshape(n // 16, 16), bias[n:].reshape(n // 16, 16)
    bi = torch.stack((bv, bg), dim=1).reshape(two_n)
    return wi.to(dtype).contiguous(), bi.to(F32).contiguous()
