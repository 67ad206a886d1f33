/*
 * vda.h — C ABI of libvda_hip.so, the MI355X (gfx950) kernel library behind
 * VideoDepthAnything.forward / infer_video_depth.
 *
 * The reference has no FFI boundary: it is pure Python/PyTorch and every entry
 * point below replaces an ATen / xformers op site on its hot path
 * (SURVEY.md §2.2, K1-K20). The reference call site each one stands in for is
 * cited per function, paths relative to the reference's video_depth_anything/.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is a DEVICE pointer unless
 *    the name says host; no torch types, no ownership transfer;
 *  - every function enqueues on `stream` (a hipStream_t passed as void*) and
 *    returns immediately: 0 = ok, non-zero = refused (bad shape/alignment; the
 *    text is available from vda_last_error()); nothing is launched on refusal;
 *  - activations are token-major / NHWC; the *_f16 entry points take fp16 ("h") activations and fp16 MFMA operands with
 *    fp32 accumulation (the reference's autocast path, video_depth.py:203-205 with fp32=False); the *_f32 twins take
 *    fp32 activations and fp32 MFMA operands (exact fp32 products: the reference's fp32=True path, run.py:31);
 *  - the per-kernel entry points are not thread-safe per stream and do no allocation or synchronisation inside
 *    (graph-capturable); the handle API at the end of this file owns memory and says where it allocates.
 */
#ifndef VDA_H
#define VDA_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* vda_stream_t;

const char* vda_last_error(void);
int vda_abi_version(void);

/* ---------------------------------------------------------------- GEMM / conv
 * out = epilogue( A[M,K] * W[N,K]^T ), fp16 operands, fp32 accumulate (MFMA).
 * Replaces nn.Linear / 1x1 Conv2d / 3x3 Conv2d / ConvTranspose2d(k==stride):
 *   dinov2_layers/attention.py:51,60   dinov2_layers/mlp.py:36-40
 *   dinov2_layers/patch_embed.py:76    dpt.py:60-90,117-121   util/blocks.py:20-32,79-84,160
 *   motion_module/motion_module.py:113,120,242-250,290   motion_module/attention.py:333,383
 */
enum vda_a_mode {
    VDA_A_DENSE = 0,      /* A row m at A + m*lda (fp16) */
    VDA_A_CONV3X3 = 1     /* implicit GEMM: A row m = output pixel (b,oy,ox), K = (ky,kx,ci) over an NHWC fp16 input, pad 1 */
};

enum vda_epilogue {
    VDA_EPI_BIAS_F16 = 0,        /* out_h[m,n] = acc + bias[n]                                   */
    VDA_EPI_BIAS_GELU_F16 = 1,   /* out_h = gelu_erf(acc + bias)                 mlp.py:36-37    */
    VDA_EPI_BIAS_RELU_F16 = 2,   /* out_h = relu(acc + bias)                     blocks.py:79-83 */
    VDA_EPI_SCALE_RES_F32 = 3,   /* out_f[m,n] = res_f[m,n] + gamma[n]*(acc + bias[n])  block.py:105-106, layer_scale.py:28 (gamma NULL = 1) */
    VDA_EPI_RES_F16 = 4,         /* out_h = acc + bias + res_h[m,n] (+ res2_h[m,n])  blocks.py:91,145; motion_module.py:123 */
    VDA_EPI_GEGLU_F16 = 5,       /* W rows interleaved [16 value | 16 gate]: out_h[m, n/2] = (acc_v+b_v) * gelu(acc_g+b_g)  attention.py:383-384 */
    VDA_EPI_PATCH_F32 = 6,       /* out_f[(m/P)*(P+1) + 1 + m%P, n] = acc + bias[n] + pos[(1 + m%P)*N + n]   dinov2.py:218-219 */
    VDA_EPI_CONVT_F16 = 7,       /* W rows ordered (ky,kx,co): pixel-shuffle scatter of a k==stride ConvTranspose2d  dpt.py:71-82 */
    VDA_EPI_BIAS_F32 = 8,        /* out_f[m,n] = acc + bias[n] */
    VDA_EPI_SCALE_RES_F32_H = 9, /* out_h[m,n] = (fp16)(res_f[m,n] + gamma[n]*(acc + bias[n])): leaves an fp32 residual stream */
    /* ---- LayerNorm folded into the GEMMs either side of it (block.py:105-106 + :56/:68 of the next sub-block), fp16 path only.
     * The fp32 residual stream x is kept as TWO fp16 planes, x = hi + lo with hi = fp16(x), lo = fp16(x - hi) (22+ significant
     * bits): the hi plane IS the A operand of the GEMM that consumes LayerNorm(x), so no LayerNorm pass touches memory. */
    VDA_EPI_SCALE_RES_SPLIT = 10,/* x' = (res_h + res2_h) - c[m] + gamma[n]*(acc + bias[n]); out_h = fp16(x'), out2_h = fp16(x' - out_h) (in
                                    place over res / res2 is allowed); stats[n/64, m, :] = (sum, centred sum of squares) of x' over the 64
                                    columns n/64*64.. (fp32; N % 64 == 0): vda_ln_stats_finalize turns them into (mean, rstd) rows.
                                    c[m] = pos[2m] when pos != NULL (the [M, 2] (mean, rstd) rows of the LayerNorm in front of this
                                    branch: the stream is RE-CENTRED, i.e. kept relative to each token's own mean - every reader of it
                                    is a LayerNorm, invariant to a per-row shift - so the fp16 operand plane rounds relative to the
                                    token's spread, not its offset), 0 when pos == NULL (zero_page must then be set) */
    VDA_EPI_LN_BIAS_F16 = 11,    /* A = hi plane, W = W*diag(ln_w) (vda_fold_ln_weight): out_h = rstd[m]*(acc - mean[m]*gamma[n]) + bias[n]
                                    with (mean, rstd) = stats[m, 0:2], gamma = c1 = row sums of the folded W, bias = c2 = b + W.ln_b */
    VDA_EPI_LN_GELU_F16 = 12,    /* the same followed by gelu_erf (mlp.fc1) */
    /* ---- ConvTranspose2d(k == stride) folded into the bias-free 3x3 conv behind it (dpt.py:71-82 + dpt_temporal.py:78-79), fp16 path,
     * VDA_A_CONV3X3 only. A = the ConvTranspose's INPUT (NHWC, the "tap grid": cH x cW = tH x tW, stride 1), W = vda_fold_convt_weight's
     * Wf: row n = (py*k + px)*tCout + co is output phase (py, px) = the k x k sub-pixel of an input pixel, K = (dy, dx, ci) over the 3x3
     * neighbourhood of the tap grid; the blocks of taps a phase does not reach are zero and the kernels skip them (a phase reaches at
     * most 2 x 2 taps). bias = vda_fold_convt_weight's Bc [k*k][9][tCout] (REQUIRED): the ConvTranspose's bias seen through the conv's
     * zero padding, by the pixel's border class 3*cy + cx (0 = first row / column, 1 = interior, 2 = last).
     * out_h[((b*tH + y)*k + py) * tW*k + x*k + px, co] = acc + Bc[py*k + px][class(y, x)][co]; the accumulators start at zero. */
    VDA_EPI_CONVT_FOLD_F16 = 13
};

typedef struct vda_gemm_args {
    const void* A;          /* fp16: dense [M,lda] or NHWC input [B,H,W,Cin] */
    const void* W;          /* fp16 [N,K], K contiguous */
    const float* bias;      /* [N] or NULL */
    void* out;
    const void* res;        /* residual (type per epilogue) or NULL */
    const void* res2;       /* second fp16 residual for VDA_EPI_RES_F16 or NULL */
    const float* gamma;     /* [N] LayerScale or NULL */
    const float* pos;       /* VDA_EPI_PATCH_F32: pos-embed [(P+1), N]; VDA_EPI_SCALE_RES_SPLIT: NULL or re-centring rows [M, 2] */
    const void* zero_page;  /* >= 256 B of zeros (conv padding source) */
    int32_t M, N, K;
    int32_t lda, ldc;       /* in elements */
    int32_t a_mode, epilogue;
    int32_t relu_in;        /* apply relu to A elements on load (blocks.py:78) */
    /* VDA_A_CONV3X3 */
    int32_t cB, cH, cW, cCin, cHo, cWo, cStride;
    /* VDA_EPI_PATCH_F32: P patches per frame. VDA_EPI_CONVT_F16 / VDA_EPI_CONVT_FOLD_F16: k, input h, w, Cout */
    int32_t P, tK, tH, tW, tCout;
    void* out2;             /* VDA_EPI_SCALE_RES_SPLIT: lo plane of the result */
    float* stats;           /* VDA_EPI_SCALE_RES_SPLIT: out, [N/64, M, 2] partial row statistics;
                               VDA_EPI_LN_*: in, [M, 2] (mean, rstd) */
    int32_t* sched;         /* NULL, or eight int32 counters ZEROED before the launch (one per XCD): the 8-phase kernel then draws its
                               tiles dynamically - a launch that shares the GPU with another kernel degrades by the CUs it lost,
                               not by a whole shift of tiles. Other kernels ignore it. Results do not depend on it. */
    int32_t stats_ld;       /* VDA_EPI_SCALE_RES_SPLIT: rows per column block of the stats array (0 = M): lets a caller run a GEMM as
                               several row ranges (pointers advanced, M = rows of the range) into one [N/64, stats_ld, 2] array */
    int32_t tile_rows;      /* 0 = the planner's choice; 192 = 192-row tiles where the kernel family has them (the remainder
                               launch of a row split); any other value: a part of a split made by hand. Results do not depend on it. */
} vda_gemm_args;

int vda_gemm_f16(const vda_gemm_args* args, vda_stream_t stream);
/* fp32-operand twin (v_mfma_f32_32x32x2_f32, exact fp32): A, W, res, res2 and out are fp32; K % 16 == 0, conv Cin % 16 == 0.
 * The epilogue ids keep their meaning (what is fused); every "_F16" output / residual is fp32 here. */
int vda_gemm_f32(const vda_gemm_args* args, vda_stream_t stream);
/* Tuning / A-B hook (process-wide): -1 (default) picks the kernel per shape; 0 = 128-row tiles; 1 / 2 = 256x256 / 256x128 tiles on
 * 32x32x16 MFMA; 3 / 4 = the same tiles on 16x16x32 MFMA, one barrier per K tile; 5 = 256x256 8-phase two-group schedule (what -1
 * uses for wide N), 5 + 16*flags = the same with debug switches (gemm8p_kernel.h: 1 early next-tile prefetch, 2 clock stamps,
 * 4 / 8 prefetch placement, 16 no start stagger), 5 + 32*s = K-loop schedule s; 7 = patch-in-LDS direct 3x3 conv where it
 * applies; 8 = 192x128 tiles on six waves; 9 = 256x128 8-phase; 10 = 192x384 tiles on twelve waves where N is a multiple of 384
 * (an A/B form: not what -1 picks, see gemm.hip); 5 + 16*64 = 8-phase on 192x256 tiles where built. Environment: VDA_CONV_LDS, VDA_GEMM_8P128, VDA_GEMM_BIG_MIN_N,
 * VDA_GEMM_STAGGER, VDA_GEMM_BM192 (defaults 1, 0, 192, 0, 1). */
int vda_gemm_set_variant(int v);
/* Diagnostic switches of the 8-phase kernel (0 = none; never set by the model). Bit 0: clock stamps - thread 0 of every workgroup
 * writes (s_memtime, s_memrealtime) at tile start / K-loop start / K-loop end / tile end of its first 16 tiles into args.pos as
 * int64 [workgroups][16][4][2] (an epilogue that does not use pos; the in-kernel clock is d(memtime) / d(memrealtime) x 100 MHz:
 * tools/gemm_clock.py). Bit 1: L2-blocked tile order (an XCD keeps four column panels for the whole launch). Bit 2 (with bit 0): the
 * shader clock at the top of the first 32 K tiles of each workgroup's second tile, int64 [workgroups][32] behind the tile stamps. */
int vda_gemm_set_debug(int flags);
/* Cap on the workgroups the persistent GEMM / conv kernels launch (0 = one per CU, the default; a multiple of 8): lets two
 * independent launch sequences on two streams take half the chip each instead of queueing behind each other's full grids. */
int vda_set_max_wgs(int n);
/* What vda_gemm_f16 would run, as a value: vda_gemm_f16 = validate, vda_gemm_plan, launch each record. The planner launches nothing,
 * follows no operand pointer (a shape with NULL operands plans) and needs no GPU when ncu is given. One record = one kernel launch. */
enum vda_gemm_family {
    VDA_GEMM_FAM_128 = 0,       /* gemm_kernel: 128-row tiles, any size, any epilogue */
    VDA_GEMM_FAM_256 = 1,       /* gemm256_kernel: 256-row tiles, one barrier per K tile, 32x32x16 MFMA (variants 1 / 2 only) */
    VDA_GEMM_FAM_256S = 2,      /* gemm256s_kernel: the same on 16x16x32 MFMA; also 192 x 128 and 192 x 384 tiles */
    VDA_GEMM_FAM_8P = 3,        /* gemm8p_kernel: 8-phase two-group schedule, 256 x 256 / 256 x 128 / 192 x 256 tiles */
    VDA_GEMM_FAM_CONV_LDS = 4   /* patch-in-LDS direct 3x3 convolution (bn = 32 or 64 output channels per pass) */
};
typedef struct vda_gemm_launch {
    int32_t r0, rows;           /* the rows [r0, r0 + rows) of the GEMM this launch computes */
    int32_t family;             /* vda_gemm_family */
    int32_t bm, bn, per_cu;     /* tile and persistent workgroups per CU (bm = 0: VDA_GEMM_FAM_CONV_LDS) */
    int32_t ksched;             /* K-loop schedule of the 8-phase kernel as its name reports it (1 = default) */
    int32_t dyn;                /* the dynamic-draw instantiation (args.sched set, 8-phase kernel, default schedule) */
    int32_t options;            /* vda_gemm_args.relu_in as the kernel sees it: bit 0 + the planner's option bits (vda_common.h) */
    int32_t tile_rows;          /* vda_gemm_args.tile_rows of the launch */
    int32_t a_mode, epilogue;   /* (of the call: with the above, everything a kernel's name is made of) */
} vda_gemm_launch;
typedef struct vda_gemm_plan_t {
    int32_t n;                  /* 1, or 2 for a row split */
    vda_gemm_launch rec[2];     /* in row order; together they cover [0, M) exactly once */
} vda_gemm_plan_t;
/* m_plan: the rows the shape decisions (tile family, 192-row tiles, the small-grid fallback, non-temporal stores) are taken for when
 *   args is a row range of a larger GEMM whose other rows run beside it (0 or <= args->M: args->M). The forward's encoder runs each
 *   GEMM as two frame halves on two streams: each half gets the kernel the whole-clip GEMM would get - same family, same per-row
 *   arithmetic, same store policy - and is never row-split further.
 * ncu: the CUs to plan for (0 = the current device's, capped by vda_set_max_wgs).
 * sched_per_launch: != 0 when the caller gives every record its own args.sched counters (they belong to ONE launch, so a call that
 *   brings one block of them - vda_gemm_f16 - is not split).
 * Row split: a large dense GEMM on the 8-phase 256 x 256 tile runs rows [0, M1) as whole rounds of the chip and rows [M1, M) on
 *   192 x 256 tiles (a 192-row round costs ~0.8 of a 256-row one) when the cost model of vda_gemm_plan_split predicts a gain; never
 *   with tile_rows != 0 or lda == 0 (a broadcast row). A row's result is bit-identical either way. */
int vda_gemm_plan(const vda_gemm_args* args, int m_plan, int ncu, int sched_per_launch, vda_gemm_plan_t* out);
/* The kernel instantiation of a record exactly as a profiler prints it (without the namespace); returns the length, name cut to len. */
int vda_gemm_launch_name(const vda_gemm_launch* rec, char* name, int len);
/* 1 when the (family, tile, A mode, epilogue) instantiation exists in this build: the planner emits nothing else. */
int vda_gemm_built(int family, int bm, int bn, int per_cu, int a_mode, int epilogue);
/* Re-read the planner's environment switches (they are read once, at the first use): for tools and tests that compare settings. */
int vda_gemm_reload_tuning(void);
/* The two pieces of the row split on their own (tests and tools). vda_gemm_plan_split: M1 <= M of the cost model alone, for the
 * current device (M1 == M: no split pays, or the epilogue / shape has no 192-row kernel). vda_gemm_row_range: *out = the arguments of
 * rows [r0, r0 + rows) of *args, as the launch of a record builds them: A / out / res / res2 / out2 advanced by r0 rows, stats
 * (VDA_EPI_LN_*) and pos (VDA_EPI_SCALE_RES_SPLIT) by r0 rows of 2 floats, stats (VDA_EPI_SCALE_RES_SPLIT) by r0 rows of 2 floats
 * with stats_ld = M. lda / ldc of 0 are read as K / N HERE (a row range is of a real matrix); vda_gemm_f16 itself reads lda == 0 as
 * "every row is A's row 0". Any kernel family honours stats_ld (the 8-phase, one-barrier and 128-row kernels alike). */
int vda_gemm_plan_split(int M, int N, int K, int epilogue, int a_mode);
int vda_gemm_row_range(const vda_gemm_args* args, int r0, int rows, vda_gemm_args* out);
/* vda_gemm_launch_name of the last record vda_gemm_f16 launched on this thread ("" before the first). */
const char* vda_gemm_last_kernel(void);

/* ---------------------------------------------------------------- norms
 * LayerNorm over the last dim, fp32 statistics (dinov2.py:95,310; block.py:56,68;
 * motion_module.py:155,161,166). in: fp32 [rows, D]; out: fp16.
 *  group/skip: when group > 0, row r with r % group < skip is dropped and the
 *  output is compacted (cls token removal for the taps, dpt_temporal.py:61).
 *  pe/pe_rows_per_step: when pe != NULL, out += pe[(r / pe_rows_per_step) % pe_steps, :]
 *  (temporal sinusoidal PE added to the normed input, motion_module.py:235).
 */
int vda_layernorm_f32_f16(const float* in, void* out, const float* w, const float* b, float eps,
                          int rows, int D, int group, int skip,
                          const float* pe, int pe_rows_per_step, int pe_steps, vda_stream_t stream);

/* Residual add + LayerNorm in one pass (dinov2_layers/block.py:105-106 followed by :56/:68 of the next sub-block):
 *   x[r,:] += gamma[:] * y[r,:]   (x fp32 in place; y fp16 = the bias-added projection output; gamma = LayerScale, NULL = 1)
 *   out[r',:] = LayerNorm(x[r,:]) (fp16; group/skip as above)
 * The rounding of y to fp16 before the LayerScale multiply is the reference's own under autocast (the Linear returns fp16,
 * layer_scale.py:28 promotes to fp32). */
int vda_layernorm_residual_f32_f16(float* x, const void* y, const float* gamma, void* out, const float* w, const float* b,
                                   float eps, int rows, int D, int group, int skip, vda_stream_t stream);
/* fp32-operand path: same, fp32 out. */
int vda_layernorm_f32_f32(const float* in, float* out, const float* w, const float* b, float eps,
                          int rows, int D, int group, int skip,
                          const float* pe, int pe_rows_per_step, int pe_steps, vda_stream_t stream);

/* ---- LayerNorm folded into the neighbouring GEMMs (VDA_EPI_SCALE_RES_SPLIT / VDA_EPI_LN_*; block.py:56,68,105-106)
 * vda_split_stats_f32: fp32 rows x [rows, D] -> the two fp16 planes (hi = fp16(x), lo = fp16(x - hi)) and the row statistics
 *   stat[r] = (mean, rstd = 1/sqrt(var + eps)) (two-pass, fp32): the entry into the split stream after the patch embedding.
 * vda_split_center_stats_f32: the same with the row's mean taken out first: hi + lo = x - mean(x), stat[r] = (0, rstd) - the entry
 *   the model uses (the stream then stays relative to each token's mean: VDA_EPI_SCALE_RES_SPLIT's pos).
 * vda_ln_stats_finalize: partial[np, r, 2] (sum, centred sum of squares per 64 columns, as VDA_EPI_SCALE_RES_SPLIT writes them)
 *   -> stat[r] = (mean, rstd), combined in column order (Chan et al.), D = 64*np. overflow (device int32, may be NULL) is set to 1
 *   when a row's statistics are not finite: the fp16 planes hold a token only up to 65 504 from its own mean (the reference's
 *   stream is fp32, block.py:105-106, and has no such limit). A saturated element is hi = +-inf, lo = -+inf. The partials of the
 *   step that saturates are finite wherever the producer takes them from its fp32 values (the 256- and 192-row GEMM tiles,
 *   vda_mlp_fused_f16) and not finite where it re-reads the stored planes (the 128-row tiles); in either case the NEXT
 *   VDA_EPI_SCALE_RES_SPLIT GEMM over those planes reads hi + lo = NaN back and leaves NaN partials, which raise the flag here.
 *   Planes that no such GEMM reads again (after the last block) are checked by their reader, vda_layernorm_split_check_f16.
 * vda_layernorm_split_f16: LayerNorm of x = hi + lo (fp32 statistics), fp16 out, group/skip as vda_layernorm_f32_f16 (the taps).
 * vda_layernorm_split_check_f16: the same kernel, same bits out; overflow (device int32, may be NULL) is set to 1 when a row it
 *   normalises (not one that group/skip drops) holds a saturated element. Finite planes never raise it. Never cleared here.
 *   The handle's forward runs every tap through it: a forward whose depth depends on a saturated element returns status 4 and NaN.
 * vda_fold_ln_weight: pack-time fold of LayerNorm's affine into the Linear that follows it: Wf[n,k] = fp16(W[n,k]*ln_w[k]),
 *   c1[n] = sum_k Wf[n,k] (of the ROUNDED values, fp32), c2[n] = b[n] + sum_k W[n,k]*ln_b[k] (fp32; b may be NULL). */
int vda_split_stats_f32(const float* x, void* hi, void* lo, float* stat, float eps, int rows, int D, vda_stream_t stream);
int vda_split_center_stats_f32(const float* x, void* hi, void* lo, float* stat, float eps, int rows, int D, vda_stream_t stream);
int vda_ln_stats_finalize(const float* partial, float* stat, float eps, int rows, int np, int32_t* overflow, vda_stream_t stream);
int vda_layernorm_split_f16(const void* hi, const void* lo, void* out, const float* w, const float* b, float eps,
                            int rows, int D, int group, int skip, vda_stream_t stream);
int vda_layernorm_split_check_f16(const void* hi, const void* lo, void* out, const float* w, const float* b, float eps,
                                  int rows, int D, int group, int skip, int32_t* overflow, vda_stream_t stream);
int vda_fold_ln_weight(const float* W, const float* bias, const float* ln_w, const float* ln_b, void* Wf, float* c1, float* c2,
                       int N, int K, vda_stream_t stream);

/* ---- Pack-time fold of ConvTranspose2d(k == stride, weight Wt [Ci, Cm, k, k], bias bt [Cm]) into the bias-free 3x3 / pad 1 conv
 * behind it (Wr [Co, Cm, 3, 3]): the operands of VDA_EPI_CONVT_FOLD_F16. For output phase (py, px) and conv tap (ky, kx):
 * qy = py + ky - 1, dy = floor(qy / k) in {-1, 0, 1}, ConvTranspose row phase ry = qy - k*dy (the same in x), and
 *   Wf[(py*k + px)*Co + co][((dy+1)*3 + dx+1)*Cip + ci] = fp16( sum over (ky, kx) -> (dy, dx), cm of Wr[co,cm,ky,kx] * Wt[ci,cm,ry,rx] )
 *   Bc[py*k + px][3*cy + cx][co] = sum over the (ky, kx) whose (dy, dx) lies inside the image for border class (cy, cx), cm of
 *                                  Wr[co,cm,ky,kx] * bt[cm]        (class 0: d = -1 is outside; 2: d = +1 is outside; 1: neither)
 * composed in fp32 (fmaf, (ky, kx, cm) order) and rounded once. Cip >= Ci: the padded channel count of the GEMM's K (columns
 * ci >= Ci are zero). Wf fp16 [k*k*Co, 9*Cip], Bc fp32 [k*k, 9, Co]. */
int vda_fold_convt_weight(const float* Wt, const float* bt, const float* Wr, void* Wf, float* Bc, int k, int Ci, int Cm, int Co, int Cip,
                          vda_stream_t stream);

/* ---- One block's MLP branch on the split residual stream in ONE kernel (dinov2_layers/mlp.py:35-41, block.py:105-106,
 * layer_scale.py:27-28; fp16 path with the LayerNorm fold): hi + lo += gamma * (fc2(GELU(fc1(LayerNorm(hi + lo)))) + b2), hid never
 * leaves the registers. Built for the widths vda_mlp_fused_supported(D, hidden) reports (D = 384, hidden = 1536: ViT-S).
 *   hi_in  fp16 [M, D]   the A operand (the hi plane; may be `hi` itself: a workgroup reads and writes its own rows only)
 *   stats  fp32 [M, 2]   (mean, rstd) of the LayerNorm in front of fc1 (vda_ln_stats_finalize); mean also re-centres the stream
 *   w1, c1, c2           fc1 with the LayerNorm folded in: vda_fold_ln_weight's Wf [hidden, D], c1 [hidden], c2 [hidden]
 *   w2p    fp16 [D, hidden]  fc2's weight with its hidden columns in the order vda_mlp_permute_w2_f16 gives them
 *   b2, gamma fp32 [D]   fc2's bias, LayerScale
 *   hi, lo fp16 [M, D]   the planes, updated in place;   part fp32 [D/64, stats_ld, 2]: partial row statistics (as VDA_EPI_SCALE_RES_SPLIT)
 * Deterministic; a row's result does not depend on its position. */
int vda_mlp_fused_supported(int D, int hidden);
int vda_mlp_permute_w2_f16(const void* w2, void* w2p, int D, int hidden, vda_stream_t stream);
int vda_mlp_fused_f16(const void* hi_in, const float* stats, const void* w1, const float* c1, const float* c2, const void* w2p, const float* b2,
                      const float* gamma, void* hi, void* lo, float* part, int M, int D, int hidden, int stats_ld, vda_stream_t stream);

/* pe = 'rope' (motion_module.py:254-257, motion_module/attention.py:403-429): channel pairs (2i, 2i+1) of the q and k thirds of the
 * fused projection qkv [T*hw, 3*C] (frame-major rows) rotated in place by  frame * 10000^(-2i/C)  (fp32 arithmetic, over the FULL
 * width C, before the head split); v is untouched. */
int vda_rope_qk_f16(void* qkv, int T, int hw, int C, vda_stream_t stream);
int vda_rope_qk_f32(float* qkv, int T, int hw, int C, vda_stream_t stream);

/* GroupNorm(32 groups) per frame on NHWC fp16 [frames, hw, C] -> fp16 [frames*hw, C]
 * (motion_module.py:84,110). `partial` is workspace of frames*chunks*groups*2 floats. */
int vda_groupnorm_nhwc_f16(const void* in, void* out, const float* w, const float* b, float eps,
                           int frames, int hw, int C, int groups, float* partial, int chunks, vda_stream_t stream);
int vda_groupnorm_nhwc_f32(const float* in, float* out, const float* w, const float* b, float eps,
                           int frames, int hw, int C, int groups, float* partial, int chunks, vda_stream_t stream);

/* ---------------------------------------------------------------- attention
 * Spatial self-attention of the ViT (dinov2_layers/attention.py:51-59 or the xformers
 * call at :76): qkv fp16 [B, N, 3, heads, 64] -> out fp16 [B, N, heads*64],
 * softmax(q k^T / 8) v with fp32 softmax, never materialising the N x N scores. */
int vda_attention_f16(const void* qkv, void* out, int B, int N, int heads, vda_stream_t stream);
/* fp32-operand twin: qkv fp32 [B, N, 3, heads, 64] -> out fp32 [B, N, heads*64], every product on fp32 MFMA. */
int vda_attention_f32(const float* qkv, float* out, int B, int N, int heads, vda_stream_t stream);
/* A-B hook: -1 = the default kernel (10); 8 / 9 / 10 = the softmax reference point enters through the score MFMAs' C operand (Q
 * pre-scaled by log2(e)/8), 9 with the lazy rescale (reference point moved only when a score exceeds it by more than 2^6), 10 deciding
 * that from the row sums instead of a running maximum and staging K / V with scalar-offset buffer loads; 1 = the round-2
 * kernel (V^T fragments via ds_read_b64_tr_b16, scalar softmax math); 2 = packed fp32 softmax math; 0 = scalar LDS
 * reads of V (cross-check); 3 = row sums through the matrix pipe; 4 / 5 = running max through the matrix pipe (without / with 3);
 * 7 = software-pipelined form (next tile's score MFMAs inside the softmax; three waves per SIMD);
 * 11 = 10 with LDS counters in place of the per-tile workgroup barrier (A/B); 20 + k, k = 1..5 = timing ablations (WRONG results: no exp / max / row sums / PV MFMAs / 1 of 4 QK k-steps), tools/attn_one.py.
 * Any other code is refused: returns 1, vda_last_error() names it, the variant stays as it was. */
int vda_attention_set_variant(int v);

/* Temporal attention across T frames per pixel (motion_module.py:232-295,
 * motion_module/attention.py:182-211): qkv fp16 [T*hw, 3*C] frame-major rows,
 * 8 heads of d = C/8 -> out fp16 [T*hw, C]. Batch b>1 is expressed by calling per clip. */
int vda_temporal_attention_f16(const void* qkv, void* out, int T, int hw, int C, int heads, vda_stream_t stream);
int vda_temporal_attention_f32(const float* qkv, float* out, int T, int hw, int C, int heads, vda_stream_t stream);
/* 1 (default): MFMA kernel for head dims 32 / 64 / 128, VALU kernel otherwise; 0: VALU kernel everywhere (cross-check). */
int vda_temporal_attention_set_variant(int v);

/* ---------------------------------------------------------------- resampling / layout
 * Bilinear, align_corners=True (util/blocks.py:156-158, dpt_temporal.py:94-96,
 * video_depth.py:162,208). NHWC fp16 -> NHWC fp16, optional elementwise add of `add`
 * (same shape as out). */
int vda_bilinear_nhwc_f16(const void* in, void* out, const void* add, int B, int h, int w, int H, int W, int C,
                          vda_stream_t stream);
int vda_bilinear_nhwc_f32(const float* in, float* out, const float* add, int B, int h, int w, int H, int W, int C,
                          vda_stream_t stream);
/* fp32 planes [B,h,w] -> [B,H,W], optional relu (video_depth.py:162-163,208). */
int vda_bilinear_plane_f32(const float* in, float* out, int B, int h, int w, int H, int W, int relu, vda_stream_t stream);

/* Patch gather for the 14x14/s14 patch-embed conv (patch_embed.py:76): fp32 NCHW
 * [B,3,H,W] -> fp16 [B*(H/14)*(W/14), Kpad], column = c*196 + ky*14 + kx, zero padded to Kpad. */
int vda_patchify_f32_f16(const float* x, void* out, int B, int H, int W, int Kpad, vda_stream_t stream);
int vda_patchify_f32_f32(const float* x, float* out, int B, int H, int W, int Kpad, vda_stream_t stream);

/* Positional-embedding grid for a (ph x pw)-patch input (dinov2.py:185-210): pe fp32 [1 + g*g, D] -> out fp32 [1 + ph*pw, D];
 * row 0 (cls) is copied, the g x g grid is resampled bicubic (a = -0.75, half-pixel centres, clamped taps) with the
 * reference's explicit scale factors ((ph + 0.1)/g, (pw + 0.1)/g). Not needed when ph*pw == g*g and the input is square. */
int vda_pos_embed_resample_f32(const float* pe, float* out, int g, int ph, int pw, int D, vda_stream_t stream);

/* cls rows of the token matrix: tok[b*(P+1), :] = cls + pos[0] (dinov2.py:218-219). */
int vda_cls_rows_f32(float* tok, const float* cls, const float* pos, int B, int P, int D, vda_stream_t stream);

/* Input of the head's readout projection when use_clstoken=True (dpt_temporal.py:56-59, dpt.py:129-132): final-norm'd tokens
 * [frames*(P+1), D] (cls at row 0 of every frame) -> [frames*P, 2D] = cat(patch token, the frame's cls token). The projection itself
 * (Linear 2D -> D + GELU) is vda_gemm_* with VDA_EPI_BIAS_GELU_F16. */
int vda_readout_concat_f16(const void* tok, void* out, int frames, int P, int D, vda_stream_t stream);
int vda_readout_concat_f32(const float* tok, float* out, int frames, int P, int D, vda_stream_t stream);

/* Final 1x1 conv 32->1 + ReLU on NHWC fp16 [rows, Cpad] (first 32 channels used)
 * -> fp32 [rows] (dpt.py:121-122). */
int vda_head_out_f16_f32(const void* in, const float* w, float bias, float* out, int rows, int Cpad, vda_stream_t stream);
int vda_head_out_f32_f32(const float* in, const float* w, float bias, float* out, long long rows, int Cpad, vda_stream_t stream);

/* Fused depth tail (dpt.py:118-122, dpt_temporal.py:93-100, video_depth.py:162-163): NHWC fp16 [B,h,w,C] ->
 * [bilinear align_corners resize to H x W when (h,w) != (H,W)] -> 3x3 conv C->32 (+b2, ReLU) -> 1x1 conv 32->1 (+b3, ReLU)
 * -> fp32 [B,H,W]. w2: fp16 [32, 9*C] with K ordered (ky,kx,ci); C a multiple of 32; zero_page: >= 256 B of zeros. */
int vda_depth_tail_f16(const void* in, const void* w2, const float* b2, const float* w3, float b3, float* out,
                       const void* zero_page, int B, int h, int w, int H, int W, int C, vda_stream_t stream);
/* A/B switch of the resizing form: 0 (default) = the persistent kernel with the weights resident in LDS (C <= 128), 1 = the round-1
 * kernel (one 8 x 32 tile per workgroup). Same arithmetic, bit-identical results. 8 = the persistent kernel without its fill waves'
 * raised priority (timing A/B), 9 = 1 and 8 together. Any other value is refused: non-zero, vda_last_error names it, setting unchanged. */
int vda_depth_tail_set_variant(int v);
/* The kernel the last vda_depth_tail_f16 of this thread launched ("" before the first): "depth_tail_kernel<0>" (no resize),
 * "depth_tail_kernel<1>" (resize, one 8 x 32 tile per workgroup) or "depth_tail_up_kernel" (resize, persistent). */
const char* vda_depth_tail_last_kernel(void);

/* output_conv1 applied to the 2x-upsampled output of refinenet1 (dpt.py:117 over util/blocks.py:156-160's
 * F.interpolate(scale_factor=2, mode="bilinear", align_corners=True)) in one pass: NHWC fp16 in [B,h,w,C] ->
 * out [B,2h,2w,ldc] = conv3x3(bilinear2x(in)) + bias, channels 0..N-1 written. w: fp16 [N, 9*C] with K ordered (ky,kx,ci)
 * (the layout vda_gemm_f16's VDA_A_CONV3X3 takes); C a multiple of 16; N <= 128, N and ldc multiples of 4; bias fp32 [N] or NULL.
 * The interpolated pixels are rounded to fp16 once, exactly as vda_bilinear_nhwc_f16 would have stored them. */
int vda_conv3x3_up2_f16(const void* in, const void* w, const float* bias, void* out, int B, int h, int wd, int C, int N, int ldc,
                        vda_stream_t stream);
/* The fused kernel has one form: 0 is the only accepted value, any other is refused (non-zero, vda_last_error names it). */
int vda_conv3x3_up2_set_variant(int v);

/* ---- The same layer with the channel mixing at HALF resolution (option "oc1_mix"). refinenet1's out_conv (1x1: Wo [Fe, Fe], bo), the
 * 2x align_corners upsample and output_conv1 (W1 [Fh, Fe, 3, 3], b1) are linear with no nonlinearity between them, and channel mixing
 * commutes with spatial interpolation tap by tap. With r [B, h, w, Fe] the output of refinenet1's resConfUnit2:
 *   z[b, y, x, tap*Fhp + co] = sum_ci Wz[tap*Fhp + co][ci] * r[b, y, x, ci] + bz[tap*Fhp + co]      one dense GEMM, N = ldz >= 9*Fhp, K = Fe
 *   o1[b, Y, X, co] = b1[co] + sum over the taps (ky, kx) whose q = (Y + ky - 1, X + kx - 1) lies inside the 2h x 2w map (the others are
 *                     the conv's zero padding) of sum_j a_j(q) * z[b, s_j(q), (3*ky + kx)*Fhp + co]        (z [B, h, w, ldz]: channels 9*Fhp .. ldz - 1 are never read)
 * where s_j(q), a_j(q) are the four corners and weights of q on the h x w grid (align_corners: source = q * (h - 1) / (2h - 1), floor,
 * clamp, fraction - vda_conv3x3_up2_f16's arithmetic).
 * vda_fold_oc1_weight (pack time): Wz[tap*Fhp + co][ci] = fp16( sum_cm W1[co, cm, tap] * Wo[cm, ci] ), bz[tap*Fhp + co] =
 *   sum_cm W1[co, cm, tap] * bo[cm], composed in fp32 (fmaf, cm order) and rounded once; rows co >= Fh and rows >= 9*Fhp are zero. Wz fp16
 *   [ldz, Fe], bz fp32 [ldz]; Fhp >= Fh, Fhp and ldz multiples of 8.
 * vda_oc1_mix_combine_f16: z fp16 [B, h, w, ldz] -> out fp16 [B, 2h, 2w, Fhp] by the second formula (bias = b1 fp32 [Fhp] or NULL): fp32
 *   accumulation, one rounding at the store. No corner is read outside its own frame. Fhp and ldz multiples of 8.
 * vda_oc1_mix_ldz: the z row vda_forward uses for that Fhp: 9*Fhp, padded to a multiple of 256 where that adds at most an eighth (the
 *   GEMM planner's tile choice; csrc/oc1_mix.hip).
 * vda_oc1_mix_frames: the frames per z buffer vda_forward runs the pair with (GEMM -> combine per chunk).
 * vda_oc1_mix_default: the option's default for a head of that many `features` (or the environment's VDA_OC1_MIX). */
int vda_fold_oc1_weight(const float* W1, const float* Wo, const float* bo, void* Wz, float* bz, int Fh, int Fe, int Fhp, int ldz, vda_stream_t stream);
int vda_oc1_mix_combine_f16(const void* z, const float* bias, void* out, int B, int h, int w, int Fhp, int ldz, vda_stream_t stream);
int vda_oc1_mix_ldz(int Fhp);
int vda_oc1_mix_frames(void);
int vda_oc1_mix_default(int features);
/* The LDS-patch 3x3 convolution behind vda_gemm_f16 (N <= 64, stride 1): 0 (default) = the persistent C = 64 kernel where it applies,
 * 1 = the per-pass kernel for every shape. Bit-identical results; A/B only. Any other value is refused: non-zero, vda_last_error
 * names it, setting unchanged. */
int vda_conv_lds_set_variant(int v);

/* uint8 RGB frames [n,H,W,3] (already at network size) -> normalised fp32 NCHW
 * [n,3,H,W]: (x/255 - mean)/std  (video_depth.py:198, util/transform.py:134,147). */
int vda_normalize_u8_f32(const uint8_t* frames, float* out, int n, int H, int W, vda_stream_t stream);
/* Same, gathering frame idx[i] (device int32[n], each < n_video) of a uint8 video [n_video,H,W,3] resident in HBM:
 * the window gather + key-frame refill of video_depth.py:197-201 without a host round trip. */
int vda_gather_normalize_u8_f32(const uint8_t* video, const int32_t* idx, float* out, int n, int n_video, int H, int W,
                                vda_stream_t stream);

/* Window gather + resize to the network size + normalise, for source frames that are not already H x W (the usual case for
 * real video, util/transform.py:109-147): out[i] = normalise(bicubic(video[idx[i]] / 255)), uint8 [n_video,H0,W0,3] ->
 * fp32 NCHW [n,3,H,W]. Bicubic as cv2.INTER_CUBIC defines it: a = -0.75, half-pixel centres, taps clamped to the border,
 * no antialiasing. (cv2 is absent offline: parity of this leg against cv2 itself is unpinned; it is tested against the
 * same definition evaluated by torch on the CPU.) */
int vda_gather_resize_normalize_u8_f32(const uint8_t* video, const int32_t* idx, float* out, int n, int n_video, int H0, int W0,
                                       int H, int W, vda_stream_t stream);

/* ---- window stitcher on the device (video_depth.py:216-254) ------------------------------------------------
 * Least-squares scale / shift of `pred` against `target` over all n pixels (utils/util.py:40-62 with the all-ones
 * mask of video_depth.py:232): scale_shift[0..1] (device) = closed form on fp64 sums, (1, 0) when det == 0.
 * workspace: >= 4*nblk doubles (device); deterministic (fixed reduction order, no atomics). */
int vda_lsq_scale_shift_f32(const float* pred, const float* target, long long n, double* workspace, int nblk, float* scale_shift,
                            vda_stream_t stream);
/* One window k > 0, frames of px pixels, win = fp32 [32, px] (video_depth.py:235-250, utils/util.py:65-74), aff(d) = max(d*scale+shift, 0):
 *   chunk[0..7]  = tail[j]*wts[j] + aff(win[2+j])*wts[8+j]   (cross-fade, wts = (1-w_j | w_j), w = 0,1/7,..,1)
 *   chunk[8..21] = aff(win[10..23]);  tail[0..7] = aff(win[24..31]);  ref1 = aff(win[12]).
 * chunk: fp32 [22, px]; tail: fp32 [8, px] updated in place; scale_shift, wts: device fp32 [2], [16]. */
int vda_stitch_window_f32(const float* win, const float* scale_shift, float* chunk, float* tail, float* ref1, long long px,
                          const float* wts, vda_stream_t stream);
/* out[i] = aff(in[i]) for n elements, the same arithmetic as the stitch (video_depth.py:238,243,249): aligns key frames another rank
 * computed (the key-frame exchange of the multi-rank schedule). in == out is allowed. */
int vda_affine_clamp_f32(const float* in, const float* scale_shift, float* out, long long n, vda_stream_t stream);
/* Running range of a streamed video: minmax[0] = min(minmax[0], min x[0..n)), minmax[1] = max(minmax[1], max x[0..n)); minmax is
 * device fp32 [2] that the caller starts at (+inf, -inf). Exact (min / max do not round), deterministic, one workgroup, no atomics
 * and no workspace; x needs 4-byte alignment only. A NaN in x is never taken. Calls that share `minmax` must be stream-ordered. */
int vda_minmax_accum_f32(const float* x, long long n, float* minmax, vda_stream_t stream);

/* ---- benchmark scorer on the device (the reference's benchmark/eval/eval.py:67-122 and metric.py) -------------------------
 * Scores a depth video against ground truth in two streaming passes with one finisher each; all four calls queue on `stream`
 * and nothing returns to the host in between. Deterministic: fp64 partial rows, a fixed combination order, no atomics. The result
 * depends on the block counts and on how the video is cut into calls, never on timing.
 *   pred : fp32 model output, gt : fp32 (gt_is_f64 = 0) or fp64 (gt_is_f64 = 1) ground truth of the same shape, both dense.
 *   valid = (gt > 1e-3) & (gt < max_depth) in gt's own type; x = max(pred, 1e-3f).
 * A video that does not fit the device at once is fed in chunks of frames: pass 1 over every chunk (row_offset = rows written so
 * far), vda_eval_lsq_finish once, pass 2 over every chunk (frame_offset = frames scored so far), vda_eval_metric_finish once.
 *
 * Pass 1: nblk rows of 5 doubles {count, sum x, sum x^2, sum y, sum x*y}, y = 1 / (gt + 1e-8), over the valid pixels among n,
 * written to partial[(row_offset + b) * 5 ...]. nblk <= 4096. */
int vda_eval_lsq_partial(const float* pred, const void* gt, int gt_is_f64, long long n, double max_depth, double* partial, int row_offset,
                         int nblk, vda_stream_t stream);
/* Sums the nrows rows in index order and solves the 2x2 normal equations of  min || scale * x + shift - y ||^2  in fp64:
 * fit[0..2] = {scale, shift, n_valid} as DOUBLES on the device; scale = shift = NaN when n_valid < 2 or the determinant is 0. */
int vda_eval_lsq_finish(const double* partial, int nrows, double* fit, vda_stream_t stream);
/* Pass 2 over nframes frames of px pixels: p = clip(1 / max(scale * x + shift, 1e-3), 1e-3, max_depth) in fp64 (the product and
 * the sum round separately), and per frame and block 7 doubles {n, sum |p-g|/g, sum (p-g)^2/g, sum (p-g)^2, #r<1.25, #r<1.25^2,
 * #r<1.25^3}, r = max(p/g, g/p), at partial[((frame_offset + f) * blocks_per_frame + b) * 7 ...]. blocks_per_frame <= 4096 and
 * must be the same in every call of one video. */
int vda_eval_metric_partial(const float* pred, const void* gt, int gt_is_f64, int nframes, long long px, double max_depth, const double* fit,
                            double* partial, int frame_offset, int blocks_per_frame, vda_stream_t stream);
/* result[0..6] = {abs_relative_difference, squared_relative_difference, rmse_linear, delta1_acc, delta2_acc, delta3_acc, frames
 * used} as doubles on the device: per frame  sum / n  (rmse: sqrt of it; the deltas: float32 count / float32 n as metric.py has
 * them), then the mean over the frames that have a valid pixel. No such frame: the six metrics are NaN, frames used = 0. */
int vda_eval_metric_finish(const double* partial, int nframes, int blocks_per_frame, double* result, vda_stream_t stream);

/* ---- temporal alignment error on the device (the reference's benchmark/eval/eval_tae.py: eval_TAE and tae_torch) ------------
 * For every pair of neighbouring frames (i, i+1), in both directions: the aligned depth of one frame is unprojected with K[i],
 * moved with the relative pose, splatted into the other frame's pixel grid, and compared with that frame's own aligned depth.
 *   d    = clip(1 / max(scale * max(pred, 1e-3f) + shift, 1e-3), 1e-3, max_depth) in fp64 for EVERY pixel; `fit` = {scale, shift, ..}
 *          is what vda_eval_lsq_finish left on the device (the fit is the scorer's, run first over the whole video).
 *   cam  : fp64 device array, 28 doubles per pair: fx, fy, cx, cy, then rows 0..2 of the 4x4 T21 = inv(pose[i+1]) @ pose[i]
 *          (R|t, row-major, 12 doubles), then rows 0..2 of T12 = inv(T21). The host computes them.
 *   plane = 2 * pair + direction; direction 0 splats frame i into i+1 with T21, direction 1 frame i+1 into i with T12.
 * The splat is LAST WINS, as the reference's index assignment is on the CPU: of the source pixels that round to one target, the
 * one with the largest row-major index stays, whatever the sign of its depth. It is an integer atomic max of (source index + 1)
 * into `winner`, so it is deterministic; the sums are fp64 block rows combined in a fixed order. The result depends on
 * blocks_per_plane, never on timing or on how the pairs are cut into calls.
 * A video is fed `npairs` pairs at a time (pred, mask: the npairs + 1 frames the pairs touch; winner: 2 * npairs planes, reused
 * from call to call): vda_tae_splat then vda_tae_compare per chunk (pair_offset = pairs compared so far), vda_tae_finish once.
 * Refused: null or misaligned pointers, H * W >= 2^31 - 1 (a source index + 1 is a 32-bit word), npairs > 32767.
 *
 * Clears the 2 * npairs planes of `winner` ([2 * npairs, H, W] 32-bit words) on `stream`, then splats. pred: [npairs + 1, H, W]. */
int vda_tae_splat(const float* pred, int npairs, int H, int W, double max_depth, const double* fit, const double* cam, unsigned int* winner,
                  vda_stream_t stream);
/* Per plane and block 2 doubles {sum |dst - proj| / dst, count} over the target pixels with proj > 0, dst > 0 and mask != 0, at
 * partial[(((pair_offset + pair) * 2 + direction) * blocks_per_plane + b) * 2 ...]; proj is the winner's moved depth, recomputed.
 * mask: bytes [npairs + 1, H, W], 0 = excluded, or NULL for none. blocks_per_plane <= 4096, the same in every call of one video. */
int vda_tae_compare(const float* pred, const unsigned char* mask, int npairs, int H, int W, double max_depth, const double* fit, const double* cam,
                    const unsigned int* winner, double* partial, int pair_offset, int blocks_per_plane, vda_stream_t stream);
/* result[0] = TAE = 100 * (sum over planes of e) / (2 * npairs), e = sum / count of a plane's rows in index order (0 when the
 * count is 0), planes added in order; result[1 .. 2 npairs] = e per plane, result[1 + 2 npairs ..] = the counts. Doubles on the
 * device, 1 + 4 * npairs of them; npairs is the whole video's N - 1. */
int vda_tae_finish(const double* partial, int npairs, int blocks_per_plane, double* result, vda_stream_t stream);

/* ---- a prediction resized to the ground truth's grid (the reference's scorers: cv2.resize(infer, (W, H)) on a size mismatch) ----
 * n dense fp32 planes [h, w] -> n planes [H, W], cv2's INTER_LINEAR for CV_32F restated from its published algorithm. Per axis:
 *   scale = 1.0 / ((double)n_dst / (double)n_src);  f = (float)((d + 0.5) * scale - 0.5);  s = floor(f);  f -= (float)s
 * columns zero the weight at the border (s < 0: f = 0, s = 0;  s >= w - 1: f = 0, s = w - 1, and only tap s is read), rows keep f
 * and clamp the indices s, s + 1 into [0, h - 1];
 *   out = (S[y0][x0]*a0 + S[y0][x1]*a1) * b0 + (S[y1][x0]*a0 + S[y1][x1]*a1) * b1,  a0 = 1.f - fx, a1 = fx, b0 = 1.f - fy, b1 = fy
 * with every operation rounded to fp32 (no fused multiply-add), so the result is deterministic and a host restatement reproduces
 * it bit for bit. Non-finite inputs are outside the contract. Refused: null or misaligned (4-byte) pointers, a size < 1, in == out,
 * a row of more than 2^30 pixels, n * H or n * h beyond 31 bits. One launch on `stream`, no allocation, no synchronisation. */
int vda_resize_linear_f32(const float* in, float* out, int n, int h, int w, int H, int W, vda_stream_t stream);

/* ---- frames larger than max_res scaled down (the reference's cv2 branch of read_video_frames: cv2.resize(frame, (width, height))) ----
 * n dense interleaved uint8 images [h, w, c] -> n images [H, W, c], c = 1 or 3: cv2's INTER_LINEAR for 8-bit images restated from
 * its published algorithm. The coordinates, the column rule and the row rule are vda_resize_linear_f32's; the rest is integer:
 *   a0 = 1.f - fx, a1 = fx, b0 = 1.f - fy, b1 = fy, each the 16-bit integer rint(a * 2048.f) (half to even, saturated to short)
 *   T   = S[x0] * a0 + S[x1] * a1                                                   int32 (at most 255 * 2048), per source row
 *   out = (((b0 * (T0 >> 4)) >> 16) + ((b1 * (T1 >> 4)) >> 16) + 2) >> 2
 * so equal sizes reproduce the input and an exact halving of both axes gives (p00 + p01 + p10 + p11 + 2) >> 2. Deterministic; a
 * host restatement reproduces it byte for byte. Refused: null pointers, a size < 1 or c outside {1, 3}, in == out, a row of more
 * than 2^30 bytes, n * H or n * h beyond 31 bits. No pointer alignment is asked for; two fast paths take what is aligned and fall
 * back otherwise, with the same bytes either way: a 4-aligned `in` with source rows (w * c) of a multiple of 4 bytes is staged
 * through LDS with dword loads (when the part a workgroup needs fits 64 KB), anything else is read byte by byte; a 4-aligned `out`
 * with output rows (W * c) of a multiple of 4 bytes is stored a dword at a time, anything else byte by byte. One launch on `stream`
 * (up to 64 KB of dynamic LDS), no allocation, no synchronisation. */
int vda_resize_linear_u8(const uint8_t* in, uint8_t* out, int n, int h, int w, int c, int H, int W, vda_stream_t stream);

/* ---- metric depth unprojected to coloured points, as the bytes of a PLY vertex list (metric_depth/depth_to_pointcloud.py) ----
 * For frame i, pixel (row r, column c), z = depth[i, r, c], every operation in fp64 and rounded once (no fused multiply-add):
 *   X = (((double)c - cx) / fx) * (double)z      Y = (((double)r - cy) / fy) * (double)z      Z = (double)z
 * the IEEE division first, the product second (the reference's cx = W / 2.0, cy = H / 2.0 are the caller's to pass). A NaN X or Y
 * (z NaN, or 0 * Inf) is stored as the quiet NaN 0x7ff8000000000000: IEEE leaves the sign of a generated NaN to the machine.
 * One packed little-endian record per kept pixel, in row-major order:
 *   record_f32 = 0: 27 bytes, doubles X, Y, Z at 0 / 8 / 16, r, g, b at 24 / 25 / 26 (what Open3D writes)
 *   record_f32 = 1: 15 bytes, floats at 0 / 4 / 8 (X and Y the fp64 results rounded once, Z the depth's own bits), r, g, b at 12 / 13 / 14
 * max_depth = 0 keeps every pixel, values untouched (zeros, negatives, NaN, Inf included); max_depth = m > 0 keeps a pixel iff
 * 0 < z <= m (NaN is dropped). depth: fp32 [n,h,w]; rgb: uint8 [n,h,w,3]; records: n slots of vda_pointcloud_frame_stride bytes
 * (h * w records rounded up to 16 bytes), slot i holds counts[i] records from its first byte, the rest of it is not written;
 * counts: int32 [n]. All on the device. workspace: vda_pointcloud_workspace_bytes(n, h, w) device bytes, contents irrelevant.
 * Deterministic: a count pass, an integer scan and a write pass, no atomics. Refused: null pointers, a size < 1, fx or fy zero or
 * not finite, cx or cy not finite, max_depth negative or NaN, record_f32 outside {0, 1}, a workspace too small, depth, counts or
 * workspace not 4-byte aligned, records not 16-byte aligned, h * w > 2^30 or n * ceil(h * w / 256) > 2^31 - 1 (a pixel index and
 * a grid index are ints). Four launches on `stream` (two with max_depth = 0), no allocation, no synchronisation. */
size_t vda_pointcloud_frame_stride(int h, int w, int record_f32);       /* 0 for a size < 1 or record_f32 outside {0, 1} */
size_t vda_pointcloud_workspace_bytes(int n, int h, int w);             /* 0 for a size < 1 */
int vda_pointcloud_f32(const float* depth, const uint8_t* rgb, void* records, int* counts, void* workspace, size_t workspace_bytes,
                       int n, int h, int w, double fx, double fy, double cx, double cy, float max_depth, int record_f32,
                       vda_stream_t stream);

/* ---- depth mapped to the bytes of a visualisation video (utils/dc_utils.py save_video: global range to uint8, then a colour table) ----
 * For each of n dense fp32 pixels, every operation rounded to fp32 once (no fused multiply-add, no reciprocal):
 *   span = minmax[1] - minmax[0];  if (!(span > 0)) span = 1e-12f        (a constant video maps to 0)
 *   v    = ((depth[i] - minmax[0]) / span) * 255.f                       (the IEEE division, correctly rounded)
 *   k    = 0 if v is NaN or v < 0,  255 if v >= 255,  else v truncated
 * For finite depth inside [min, max] this is the reference's ((d - d_min) / (d_max - d_min) * 255).astype(np.uint8); the clamp
 * only defines what numpy leaves undefined. minmax: device fp32 [2] = {min, max}, exactly what vda_minmax_accum_f32 leaves, so
 * range and mapping chain on one stream without a host round trip. lut: device uint8 [256, 3], out[3 i .. 3 i + 2] = lut[k]
 * (3 n bytes, packed RGB), or NULL: out[i] = k (n bytes, grayscale). All pointers are device pointers. depth needs 4-byte
 * alignment only and out may sit at any byte address: a head of at most 3 pixels is peeled so that the body stores whole dwords
 * (four pixels are one dword of gray or three of RGB), and a tail of at most 3 pixels follows as single bytes. Nothing outside
 * out[0 .. n) / out[0 .. 3 n) is written. Deterministic. Refused: a null depth, minmax or out, n < 1, depth or minmax not
 * 4-byte aligned. Indices are long long (sizes past 2^31 pixels are untested). One launch on `stream`, no allocation, no
 * synchronisation, no atomics. */
int vda_depth_vis_u8(const float* depth, long long n, const float* minmax, const uint8_t* lut, uint8_t* out, vda_stream_t stream);

/* ---- frames as baseline JPEG scans, for a Motion-JPEG AVI (video_depth_anything_amd/mjpeg.py: encode_jpeg_numpy is the contract) ----
 * frames: device uint8 [n,h,w,channels], channels 3 (RGB, coded as Y Cb Cr 4:4:4) or 1 (gray); any h, w in 1..65535, the right and
 * bottom edges padded to a multiple of 8 by replicating the last column / row. All integer arithmetic (>> is the arithmetic shift):
 *   Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *   Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16       Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16
 *   s = sample - 128;  Ci[k][n] = rint(8192 c_k cos((2n+1) k pi / 16)), c_0 = sqrt(1/8), c_k = 1/2
 *   t[k][x] = (sum_n Ci[k][n] s[n][x] + 128) >> 8;   F[k][l] = (sum_m Ci[l][m] t[k][m] + 16384) >> 15     (F = 8 x the coefficient)
 *   q = sign(F) ((2 |F| + 8 Q) / (16 Q)), AC clamped to +-1023
 * qtables: HOST uint16, 64 luminance divisors then (channels = 3) 64 chrominance divisors, natural row-major order, each 1..255.
 * Entropy coding: baseline sequential with the four Huffman tables of ITU T.81 Annex K, zig-zag order, one MCU = the Y, Cb, Cr
 * blocks of one 8x8 tile, ONE RESTART INTERVAL PER MCU ROW (DRI = ceil(w / 8)): DC predictors reset, the interval's last byte
 * padded with 1-bits, FF -> FF 00, RSTm (m cycling 0..7) between intervals, EOI behind the last. out: the n scans back to back,
 * frame i at the sum of lengths[0 .. i), lengths[i] (device int64) bytes long, EOI included; a complete JPEG is the header
 * (SOI, APP0, DQT, SOF0, DHT, DRI, SOS: mjpeg.jpeg_header) followed by that slice. Deterministic: the bits of neighbouring
 * blocks meet in shared words through integer OR-atomics only, and the lengths are integer sums.
 * A block's bits are at most 64 * 26 before stuffing and twice that after, so with bh = ceil(h / 8), nb = ceil(w / 8) * channels
 *   vda_mjpeg_out_bytes       = n * (bh * (nb * 416 + 2) + 2)             the capacity `out` needs; the encoder never truncates
 *   vda_mjpeg_workspace_bytes = n * bh * nb * (128 + 208 + 416) + the two length tables      device bytes, contents irrelevant
 * (both 0 for a size < 1 or > 65535 or channels outside {1, 3}). Refused before any launch: a null frames, qtables, workspace,
 * out or lengths; n, h or w < 1; h or w > 65535; channels not 1 or 3; a table entry outside 1..255; more than 2^31 - 1
 * workgroups; a frame whose bound does not fit an int; workspace not 16-byte or lengths not 8-byte aligned; workspace_bytes or
 * out_capacity below the bound. Three launches on `stream` (transform, entropy, pack), no allocation, no synchronisation. */
size_t vda_mjpeg_workspace_bytes(int n, int h, int w, int channels);
size_t vda_mjpeg_out_bytes(int n, int h, int w, int channels);
int vda_mjpeg_encode_u8(const uint8_t* frames, int n, int h, int w, int channels, const uint16_t* qtables, void* workspace,
                        size_t workspace_bytes, uint8_t* out, size_t out_capacity, long long* lengths, vda_stream_t stream);

/* ---- baseline JPEG scans back to pixels (video_depth_anything_amd/mjpeg.py: decode_jpeg_numpy is the contract) -------------------
 * n frames of one geometry and one set of tables: h x w in 1..65535, components 1 (gray) or 3 (Y Cb Cr) with luma sampling
 * hs x vs = 1x1, 2x1 or 2x2 over 1x1 chroma (4:4:4, 4:2:2, 4:2:0). The caller has parsed the headers and cut the scans at their
 * restart markers (mjpeg.parse_jpeg, mjpeg.device_call_inputs):
 *   scan       device bytes, the frames' entropy-coded data back to back (scan_bytes of them, at most 2^31 - 16)
 *   intervals  HOST int [n_intervals][5]: frame, byte offset into scan, byte length, first MCU, MCU count - validated here, before
 *              any launch: the frame in [0, n), the bytes inside scan_bytes, the MCUs inside the frame; then copied to the device
 *   tables     HOST, one MjdTables record of csrc/mjpeg_decode_core.h (mjpeg.decode_tables): per component its DC and AC Huffman
 *              table, and the zig-zag order; the decoder masks every index it takes from them
 *   qtables    HOST uint16 [components][64], natural row-major order, each 1..255
 * out: device uint8 [n,h,w,3] RGB or [n,h,w]; status: device int [n], 0 = decoded, otherwise the largest error code of the frame's
 * intervals (MJD_* of mjpeg_decode_core.h, mjpeg.DECODE_STATUS) - such a frame's pixels are defined (the coefficients decoded
 * before the error, zeros behind it) but mean nothing. All integer arithmetic that wraps; libjpeg's islow IDCT, fancy upsampling
 * and 16-bit fixed-point colour conversion: bit for bit the twin, for corrupt scans too. No input, however
 * malformed, is read outside its interval's bytes or written outside its MCUs' blocks.
 *   vda_mjpeg_decode_workspace_bytes = the interval table + the tables + 192 bytes per 8x8 block (int16 coefficients, uint8 planes);
 *   0 for a size < 1 or > 65535, components outside {1, 3}, a sampling other than the above or intervals < 0.
 * Refused before any launch, each by its own message: a null pointer; n, h or w < 1; h or w > 65535; components; sampling;
 * scan_bytes > 2^31 - 16; n_intervals < 1; more than 2^31 - 1 workgroups; workspace not 16-byte or status not 4-byte aligned;
 * workspace_bytes or out_capacity below the bound; a table entry outside 1..255; a bad interval. Two small copies, two memsets
 * and three launches on `stream` (entropy: a lane per interval; IDCT; upsample + colour), no allocation. NOT free of host
 * synchronisation: the interval table and the tables are copied from the caller's pageable host memory, which hipMemcpyAsync does
 * synchronously through a staging buffer, so the call waits on the host until those two copies (and what `stream` holds before
 * them) are done, the host arrays may be freed when it returns, and the call cannot be captured into a graph. */
size_t vda_mjpeg_decode_workspace_bytes(int n, int h, int w, int components, int hs, int vs, int intervals);
int vda_mjpeg_decode_u8(const uint8_t* scan, size_t scan_bytes, const int* intervals, int n_intervals, const void* tables,
                        const uint16_t* qtables, int n, int h, int w, int components, int hs, int vs, void* workspace,
                        size_t workspace_bytes, uint8_t* out, size_t out_capacity, int* status, vda_stream_t stream);

/* ---- raw deflate (RFC 1951) of a device buffer, for .npz files (video_depth_anything_amd/deflate.py: deflate_numpy is the contract) ----
 * in: n device bytes at any byte address. The stream is cut into independent chunks of 16384 input bytes, a workgroup each:
 *   tokens   a run's first byte is a literal; its other bytes are distance-1 matches of 258 from the front and a rest, one more
 *            match when 3..257 long, literals when 1 or 2 (zlib's Z_RLE strategy); no match crosses a chunk boundary
 *   code     a dynamic Huffman block per chunk: lengths at most 15 bits from the counts by integer arithmetic with ties broken by
 *            (count, symbol) (csrc/deflate_core.h); one distance code; the lengths written one by one in a code-length code built
 *            the same way, at most 7 bits, without the repeat symbols
 *   end      end-of-block, then an empty stored block (a sync flush: the chunk ends on a byte with 00 00 FF FF) - except the last
 *            chunk when final = 1, whose block carries BFINAL instead. A chunk whose coded form would not be smaller than 5 + its
 *            bytes is one stored block. n = 0 gives 01 00 00 FF FF with final = 1 and no bytes with final = 0.
 * So a call with final = 0 leaves a byte-aligned open piece, and pieces followed by a final one are one valid stream. out: the
 * chunks back to back, *length (device int64) bytes of them; crcs: device uint32 per chunk, the CRC-32 (zlib's polynomial) of the
 * chunk's INPUT bytes, max(1, ceil(n / 16384)) entries (only ceil(n / 16384) are written when final = 0). Deterministic: bits of
 * neighbouring tokens meet in shared words through integer OR-atomics only.
 *   vda_deflate_out_bytes(n)       = n + 5 * max(1, ceil(n / 16384))         the capacity `out` needs; the encoder never truncates
 *   vda_deflate_workspace_bytes(n) = chunks * 16400 + up16(4 chunks) + up16(8 chunks), chunks = max(1, ceil(n / 16384)); device
 *                                    bytes, contents irrelevant      (both 0 for n > 2^44)
 * Refused before any launch: a null in (unless n = 0), workspace, out, length or crcs; n > 2^44; final outside {0, 1}; workspace not
 * 16-byte, length not 8-byte or crcs not 4-byte aligned; workspace_bytes or out_capacity below the bound. Four launches on `stream`
 * (encode, crc, offsets, pack), no allocation, no synchronisation. */
size_t vda_deflate_workspace_bytes(size_t n);
size_t vda_deflate_out_bytes(size_t n);
int vda_deflate_u8(const uint8_t* in, size_t n, int final, void* workspace, size_t workspace_bytes, uint8_t* out, size_t out_capacity,
                   long long* length, uint32_t* crcs, vda_stream_t stream);

/* ---- OpenEXR scanline files, ZIP compression, one FLOAT channel, from float32 depth (video_depth_anything_amd/exr.py:
 * encode_exr_numpy is the contract, byte for byte) ----
 * depth: device float32, frame f's h * w pixels dense at depth + f * frame_stride (frame_stride counts floats). A file is
 * header_bytes of header (the caller's: exr.exr_header; it depends on w and h only, 277 bytes for the channel Z) followed by the
 * frame's PAYLOAD, which is what this call makes:
 *   table    nb = ceil(h / 16) uint64: the position in the FILE of every block (so header_bytes is added)
 *   blocks   block b: int32 y = 16 b, int32 dataSize, dataSize bytes. Its raw bytes are its min(16, h - 16 b) rows back to back,
 *            L = 4 w rows bytes. OpenEXR's filter (even bytes, then odd bytes; then every byte but the first replaced by its
 *            difference to its predecessor plus 128) gives f. f is cut into k = ceil(L / 16384) balanced chunks of
 *            q = 64 ceil(L / (64 k)) bytes (the last shorter), each coded as vda_deflate_u8 codes a chunk (BFINAL on the block's
 *            last, a sync flush behind the others); the zlib stream is 78 01, the chunks, the Adler-32 of f big-endian. If that
 *            stream is strictly shorter than L it is the block's data, otherwise the raw rows are (dataSize = L).
 * payload: the frames' payloads back to back; offsets: device int64 [frames + 1], frame f's payload is bytes offsets[f] ..
 * offsets[f + 1] of `payload`. Deterministic. Only the gathered bytes of `depth` are read, any bit pattern is data.
 *   vda_exr_payload_bytes(frames, h, w)   = frames * (8 nb + 8 nb + 4 w h): every block raw; the capacity `payload` needs
 *   vda_exr_workspace_bytes(frames, h, w) = chunks * 16400 + 2 up16(4 chunks) + 16 chunks + 2 up16(4 blocks) + up16(8 blocks), with
 *                                           blocks = frames * nb and chunks = the k of all blocks; device bytes, contents irrelevant
 *   (both 0 for a size < 1, h or w > 65535 - a block is then below 2^22 bytes and 256 chunks, which the kernels' 32-bit chunk
 *   arithmetic holds - or more than 2^31 - 1 chunks in all)
 * Refused before any launch: a null depth, workspace, payload or offsets; frames, h or w < 1; sizes above the cap; frame_stride <
 * h * w; header_bytes < 0; depth not 4-byte, workspace not 16-byte or offsets not 8-byte aligned; workspace_bytes or
 * payload_capacity below the bound. Four launches on `stream` (encode, blocks, offsets, pack), no allocation, no synchronisation. */
size_t vda_exr_workspace_bytes(int frames, int h, int w);
size_t vda_exr_payload_bytes(int frames, int h, int w);
int vda_exr_zip_f32(const float* depth, int frames, int h, int w, long long frame_stride, long long header_bytes, void* workspace,
                    size_t workspace_bytes, uint8_t* payload, size_t payload_capacity, long long* offsets, vda_stream_t stream);

/* ---- validation losses on the device (the reference's utils/loss_MiDas.py and utils/loss.py: Loss_ssi, Loss_tgm) ---------------
 * What train.py's validation pass ranks checkpoints by, as inference-time arithmetic (no gradients). pred, y: dense fp32
 * [nframes, px] (nframes = B * N, px = H * W); mask: bytes of the same shape, 0 = excluded, or NULL for all valid. Every fp32
 * value is widened exactly and all arithmetic is fp64, each operation rounded once (no fused multiply-add). Finite inputs only.
 * Deterministic: fp64 partial rows per block, a fixed tree, rows combined in index order by one-workgroup finishers, no
 * floating-point atomics; a result depends on blocks_per_plane, never on timing. All calls queue on `stream`, nothing returns to
 * the host in between, no allocation. All pointers are device pointers; pred, y, med need 4-byte alignment only (a plane may start
 * at any dword, a mask plane at any byte), the fp64 buffers 8-byte. Refused before any launch: null or misaligned pointers, a size
 * < 1, blocks_per_plane outside 1..4096, more than 65535 planes, more than 2^22 partial rows (or image rows in the mad form).
 *   stats : 8 doubles per frame.  lsq: {n, mu_d, mu_y, s, t, loss, -, -}   mad: {med_d, sc_d, med_y, sc_y, n, -, -, -}
 *
 * Loss_ssi of loss_MiDas.py ("lsq"), three passes, vda_loss_lsq_partial then vda_loss_lsq_finish with the same `pass` each:
 *   pass 0  rows {n, sum d, sum y} over the valid pixels           -> stats n, mu_d = sum d / max(n, 1), mu_y likewise
 *   pass 1  rows {sum (d - mu_d)(y - mu_y), sum (d - mu_d)^2}      -> stats s = num / (den + eps), t = mu_y - s * mu_d
 *   pass 2  rows {sum ((s * d + t) - y)^2}                         -> stats loss = sum / max(n, 1);
 *           result[0] = the mean of loss over ALL nframes frames (a frame without a valid pixel counts as 0), result[1 + f] = loss
 * The row of (frame f, block b) is partial[(f * blocks_per_plane + b) * K ...], K = 3, 2, 1. result: 1 + nframes doubles (pass 2
 * only; may be NULL in passes 0 and 1). */
int vda_loss_lsq_partial(const float* pred, const float* y, const unsigned char* mask, int nframes, long long px, int pass, const double* stats,
                         double* partial, int blocks_per_plane, vda_stream_t stream);
int vda_loss_lsq_finish(const double* partial, int nframes, int blocks_per_plane, int pass, double eps, double* stats, double* result,
                        vda_stream_t stream);
/* Exact masked LOWER median per plane (torch.median's rule): med[f] = element (n - 1) / 2 of the sorted valid values of pred's
 * frame f, med[nframes + f] the same of y's (y may be NULL: only pred's are written); 0.0f for a plane without a valid pixel. The
 * value is an input element bit for bit, chosen by a radix select over order-preserving 32-bit keys (-0 sorts before +0): one
 * workgroup of 1024 threads per plane, four passes of 8 bits, integer LDS histograms, no global atomics. px < 2^31. */
int vda_loss_median(const float* pred, const float* y, const unsigned char* mask, int nframes, long long px, float* med, vda_stream_t stream);
/* Loss_ssi of loss.py ("mad"), after vda_loss_median: rows {n, sum |d - med_d|, sum |y - med_y|} at partial[(f * blocks_per_plane
 * + b) * 3 ...]; the finisher leaves stats {med_d, sc_d, med_y, sc_y, n} with sc = sum / n + eps (eps alone when n = 0). */
int vda_loss_mad_scale_partial(const float* pred, const float* y, const unsigned char* mask, int nframes, long long px, const float* med,
                               double* partial, int blocks_per_plane, vda_stream_t stream);
int vda_loss_mad_scale_finish(const double* partial, int nframes, int blocks_per_plane, double eps, const float* med, double* stats,
                              vda_stream_t stream);
/* rho = ((d - med_d) / sc_d - (y - med_y) / sc_y)^2 on valid pixels. loss.py normalises PER IMAGE ROW: rows[(f * H + r) * 2 ...] =
 * {sum rho, count of valid pixels} of row r of frame f (one wave per image row, so these do not depend on any launch parameter).
 * The finisher: result[1 + f] = the mean over frame f's H rows of sum / max(count, 1), result[0] = the mean over all nframes * H
 * rows; a row without a valid pixel counts as 0. rows: 2 * nframes * H doubles; result: 1 + nframes doubles. */
int vda_loss_mad_rows(const float* pred, const float* y, const unsigned char* mask, int nframes, int H, int W, const double* stats, double* rows,
                      vda_stream_t stream);
int vda_loss_mad_finish(const double* rows, int nframes, int H, double* result, vda_stream_t stream);
/* Loss_tgm (the same in both files) over B clips of N >= 2 frames, P = B * (N - 1) pairs of neighbouring frames: per pair
 *   valid = mask_i & mask_{i+1};  static = valid & (|y_{i+1} - y_i| < 0.05)   (fp64 difference, the double 0.05)
 * rows {n_valid, n_static, sum over static of | |d_{i+1} - d_i| - |y_{i+1} - y_i| |} at partial[(p * blocks_per_plane + b) * 3 ...].
 * The finisher: result[1 + p] = sum / n_static, or NaN for a skipped pair (n_valid = 0 or n_static = 0); result[1 + P + p] =
 * n_static; result[0] = the mean over clips of (sum of the clip's pairs in order) / (N - 1), skipped pairs staying in the divisor.
 * result: 1 + 2 P doubles. */
int vda_loss_tgm_partial(const float* pred, const float* y, const unsigned char* mask, int B, int N, long long px, double* partial,
                         int blocks_per_plane, vda_stream_t stream);
int vda_loss_tgm_finish(const double* partial, int B, int N, int blocks_per_plane, double* result, vda_stream_t stream);

/* ================================================================ handle API: the model behind one pointer
 * What a C / C++ host binds in place of the reference's Python class (the seam of SURVEY.md section 8b):
 *   VideoDepthAnything(**model_configs[enc])          run.py:45, video_depth.py:38-63      vda_create
 *   .load_state_dict(torch.load(ckpt), strict=True)   run.py:46                            vda_load_weight per tensor, then
 *                                                                                          vda_finalize_weights
 *   .to('cuda')                                       run.py:47                            (the handle lives on the device
 *                                                                                           that is current at vda_create)
 *   model.forward(x)                                  video_depth.py:89-93,161-164         vda_forward
 * Ownership: the caller owns `in`, `out` and (optionally) the workspace block; the handle owns its weights and frees them
 * in vda_destroy. Errors: non-zero return, text from vda_last_error() - for state-dict problems in torch's own wording
 * ("Missing key(s) in state_dict: ...", "Unexpected key(s) ...", "size mismatch for ..."). A handle is not thread-safe and
 * is bound to one device: every call must be made with that device current.
 * Allocation / synchronisation: vda_load_weight copies synchronously (host or device source); vda_finalize_weights packs
 * the fp16 layouts on the device and synchronises; the FIRST vda_forward of a new (shape, precision) - or vda_prepare -
 * may allocate (the fp32 weight pack, the positional embedding at that grid, the handle's own workspace when the caller
 * gave none). After that vda_forward only enqueues kernels on `stream` - and, with options "enc_split" and "head_lanes" (both default on;
 * fp16, not while `stream` is capturing), on one stream the handle owns per caller stream, forked from `stream` and joined back into it before
 * anything later on `stream` runs: completion of `stream`'s work still means the forward is done. */
typedef struct vda_model vda_model;

typedef struct vda_config {
    int32_t embed_dim;        /* 384 (vits) / 1024 (vitl); num_heads * 64                  dinov2.py:339-378 */
    int32_t depth;            /* 12 / 24 transformer blocks */
    int32_t num_heads;        /* 6 / 16 */
    int32_t taps[4];          /* blocks whose output feeds the head: 2,5,8,11 / 4,11,17,23   video_depth.py:53-56 */
    int32_t features;         /* 64 / 256                                                    run.py:41-42 */
    int32_t out_channels[4];  /* 48,96,192,384 / 256,512,1024,1024 */
    int32_t num_frames;       /* 32: temporal window (pos_encoder.pe rows) */
    int32_t use_clstoken;     /* 0 (every released config) / 1: head.readout_projects fold the cls token in, dpt.py:92-98 */
    int32_t use_bn;           /* 0 (every released config) / 1: BatchNorm2d after each conv of the fusion blocks' ResidualConvUnits
                                 (util/blocks.py:60-62,80-86; inference = an affine per channel, folded into the conv at pack time) */
    int32_t pe_rope;          /* 0 = pe 'ape' (every released config): sinusoidal pos_encoder.pe added before q/k/v; 1 = pe 'rope':
                                 no pe buffer in the checkpoint, q and k rotated per frame (motion_module.py:221-224,254-257) */
} vda_config;

enum vda_precision {
    VDA_PREC_F16 = 0,         /* fp16 MFMA operands, fp32 accumulate / residual streams / norm + softmax statistics */
    VDA_PREC_F32 = 1          /* fp32 operands everywhere (exact-fp32 MFMA): the reference's fp32=True */
};
enum vda_dtype { VDA_DTYPE_F32 = 0 };

int vda_create(const vda_config* cfg, vda_model** out);
int vda_destroy(vda_model* h);
/* Number of tensors the state dict must hold (351 for vits, 519 for vitl). */
int vda_num_weights(const vda_model* h);
/* One tensor of the flat fp32 state dict, under the reference's key (e.g. "pretrained.blocks.0.attn.qkv.weight"); `ptr` is
 * host or device memory and is copied. Unknown keys and shape mismatches are refused. */
int vda_load_weight(vda_model* h, const char* name, const void* ptr, const int64_t* dims, int ndim, int dtype);
/* strict=True check (every key present) + repack to the kernel layouts. */
int vda_finalize_weights(vda_model* h);
/* Bytes of workspace a forward of x[B,T,3,H,W] needs at this precision (-1 on error). */
int64_t vda_workspace_bytes(vda_model* h, int B, int T, int H, int W, int precision);
/* Optional: run in a caller-owned, 256-byte aligned block (e.g. a torch tensor) instead of one the handle allocates. */
int vda_set_workspace(vda_model* h, void* ptr, int64_t bytes);
/* Optional: do now whatever the first forward of this shape / precision would allocate. */
int vda_prepare(vda_model* h, int B, int T, int H, int W, int precision);
/* in: fp32 device [B,T,3,H,W] (normalised frames; H, W multiples of 14; T <= num_frames) -> out: fp32 device [B,T,H,W]. */
int vda_forward(vda_model* h, const float* in, float* out, int B, int T, int H, int W, int precision, vda_stream_t stream);
/* Deferred status of the forwards enqueued so far (vda_forward itself only enqueues). 0 = every forward whose stream work has
 * COMPLETED was valid; 4 = one of them left fp16's range in the split residual stream of the default fp16 path ("ln_fold": a token
 * further than 65 504 from its own mean; the reference's stream is fp32, block.py:105-106): its depth was overwritten with NaN and
 * vda_last_error() names the way out (vda_set_option "ln_fold" 0, or the fp32 path). Call it after synchronising the stream(s);
 * a report nobody collected fails the NEXT vda_forward instead. Reports are cleared once returned. */
int vda_forward_status(vda_model* h);
/* Parity hook: copy `bytes` of a named intermediate of the last forward ("tap0".."tap3", "l1", "l2", "l3t", "l4t", "p4t",
 * "p3t", "p2", "p1"; activation dtype of that forward's precision, channels padded to multiples of 64) to device `dst`.
 * "l1" / "l2" of a forward that ran that level folded (option "convt_fold") were never written: they are rebuilt first, on `stream`,
 * from the level's projection ("t0" / "t1") with the unfused ConvTranspose GEMM - what the unfused forward holds there, bit for bit.
 * "p1c" (refinenet1's out_conv output at half size, fp16 path) of a forward that ran option "oc1_mix" likewise: rebuilt from
 * resConfUnit2's output with the unfused out_conv GEMM. */
int vda_debug_copy(vda_model* h, const char* name, void* dst, int64_t bytes, vda_stream_t stream);
/* Test utility: occupy `wgs` workgroups (256 threads, lds_bytes of LDS each) for about `cycles` shader clocks on `stream` - a
 * stand-in for a communication kernel running beside the forward (tools/contention.py). Bounded: every wave leaves by itself. */
int vda_debug_occupy(int wgs, int lds_bytes, long long cycles, vda_stream_t stream);
/* Launch-sequence switches (A/B and cross-checks). "residual_in_ln" (default 0; fp16 path only): 1 = attn.proj / mlp.fc2 store
 * their output as fp16 and the residual add runs inside the following LayerNorm (vda_layernorm_residual_f32_f16); 0 = the add
 * is the GEMM's fp32 in-place epilogue (VDA_EPI_SCALE_RES_F32; measured 2 % faster end to end). Changes the workspace size.
 * "ln_fold" (default 1), "dyn_sched" (default 0): csrc/host.hip. "oc1_fused" (default 1; fp16 path): refinenet1's 2x upsample is
 * evaluated inside output_conv1 (vda_conv3x3_up2_f16) and path_1 never exists at full size; 0 = vda_bilinear_nhwc + the conv.
 * "mlp_fused" (default 0; fp16 path with ln_fold, widths vda_mlp_fused_supported reports): 1 = a block's fc1 + GELU + fc2 + residual
 * run as vda_mlp_fused_f16 instead of the two GEMM launches (measured slower on the MI355X: kept as a tested option).
 * "head_overlap" (default 0): 1 = the part of the head that needs taps 0..2 only (dpt_temporal.py:55-69 for i < 3, :75, :78-80) runs
 * on a side stream of the handle as soon as tap 2 exists, under the remaining encoder blocks; bit-identical results.
 * "head_lanes" (default 1, or the environment's VDA_HEAD_LANES; fp16 path; < 0 restores that default): after the encoder the head's
 * branches that do not depend on tap 3 (the tap 0..2 work above and the first conv of resConfUnit1 in refinenets 3, 2, 1) run on the
 * stream "enc_split" uses, beside proj3 .. motion module 2 on `stream`, joined back before refinenet 3 and refinenet 2
 * read what it made. Bit-identical results, the same workspace layout. Like "enc_split" it does not apply while `stream`
 * is capturing or another forward of the handle is in flight on a different stream, and not together with "head_overlap".
 * "convt_fold" (default 1, or the environment's VDA_CONVT_FOLD; fp16 path; < 0 restores that default): resize_layers[i] (ConvTranspose2d,
 * k == stride) and layer{i+1}_rn (3x3, no bias) for i = 0, 1 run as ONE implicit GEMM on the projection's grid (VDA_EPI_CONVT_FOLD_F16,
 * weights composed at pack time by vda_fold_convt_weight) wherever the unfused 3x3 conv would run on the 256 x 256 8-phase or the
 * 128-row GEMM kernel (ViT-L; not the 64-channel convs of ViT-S): "l1" / "l2" are then never written. Same workspace layout. Not
 * bit-identical to 0: one fp16 rounding of l1 / l2 less, one rounding of the composed weights more.
 * "oc1_mix" (default vda_oc1_mix_default(features); fp16 path, where "oc1_fused" applies; < 0 restores that default): refinenet1 stops
 * after resConfUnit2 and its out_conv + output_conv1 over the 2x upsample run as the z GEMM + vda_oc1_mix_combine_f16 (above), per
 * chunk of "oc1_mix_chunk" frames (default vda_oc1_mix_frames(); changes the workspace size). "p1c" is then never written and
 * vda_debug_copy rebuilds it from resConfUnit2's output with the unfused out_conv GEMM. Same workspace layout either way. Not
 * bit-identical to 0: one fp16 rounding of the composed weight and one of z more, the rounding of "p1c" less. */
int vda_set_option(vda_model* h, const char* name, int value);
/* Measurement hook (bench.py): from vda_profile_start until vda_profile_stop every `every`-th GEMM / conv launch of each
 * (shape, epilogue) inside vda_forward is bracketed by two events on the launch stream. vda_profile_stop waits for them and
 * writes a JSON object {kernel: {"launches", "flops", "timed", "timed_ms", "timed_flops"}} into json[cap]. */
int vda_profile_start(vda_model* h, int every);
int vda_profile_stop(vda_model* h, char* json, int cap);

#ifdef __cplusplus
}
#endif
#endif
