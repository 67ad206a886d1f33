// Benchmark scorer on the device: the arithmetic of the reference's benchmark/eval/eval.py:67-122 and metric.py as two streaming
// reductions, each with a one-workgroup finisher: fp64 partials, fixed combination order, no atomics - the pattern stated in reduce64.h.
//
//   pass 1 (eval_lsq_*)    over every valid pixel of the whole video: count, sum x, sum x^2, sum y, sum x*y with x = clip(pred, 1e-3)
//                          and y = 1 / (gt + 1e-8); the finisher solves the 2x2 normal equations and leaves {scale, shift, n_valid}
//                          as doubles on the device.
//   pass 2 (eval_metric_*) reads scale / shift from device memory (no host round trip), forms the aligned depth per pixel and
//                          accumulates per frame {n, sum |p-g|/g, sum (p-g)^2/g, sum (p-g)^2, #delta<1.25, <1.25^2, <1.25^3}; the
//                          finisher forms the per-frame ratios and their mean over the frames that have a valid pixel.
//
// A video larger than the caller's device budget is fed in chunks of frames: every chunk's partial rows land at an offset of the one
// workspace, each finisher runs once over all of them. The result depends on the chunking and on the block counts (they fix the order
// of the fp64 additions), never on timing.
//
// Both passes are HBM-bound streams (8 or 12 bytes per pixel); the fp64 divisions (one in pass 1, five in pass 2) are IEEE.
// THIS FILE IS BUILT WITH -ffp-contract=off (build.py PER_FILE): scale * x + shift rounds twice, as numpy evaluates it.
#include "reduce64.h"

namespace {

constexpr int EV_T = R64_T;
constexpr int LSQ_K = 5;      // count, sum x, sum x^2, sum y, sum x*y
constexpr int MET_K = 7;      // n, sum |p-g|/g, sum (p-g)^2/g, sum (p-g)^2, c1, c2, c3

// valid = (gt > 1e-3) & (gt < max_depth), compared in gt's OWN type as numpy compares an array with a python scalar: a float32
// ground truth meets float32(1e-3), which is not the double 1e-3.
template <typename GT>
__device__ __forceinline__ bool gt_valid(GT g, GT hi) {
    return g > (GT)1e-3 && g < hi;
}

template <typename GT>
__global__ void __launch_bounds__(EV_T) eval_lsq_partial_kernel(const float* __restrict__ pred, const GT* __restrict__ gt, long long n, double max_depth,
                                                                double* __restrict__ partial) {
    const GT hi = (GT)max_depth;
    plane_partial<LSQ_K>(n, partial + (size_t)blockIdx.x * LSQ_K, [&](long long i, double (&s)[LSQ_K]) {
        const GT g = gt[i];
        if (gt_valid(g, hi)) {
            const double x = (double)clip_pred(pred[i]);
            const double y = 1.0 / ((double)g + 1e-8);
            s[0] += 1.0;
            s[1] += x;
            s[2] += x * x;
            s[3] += y;
            s[4] += x * y;
        }
    });
}

// Rows summed in index order; fit = {scale, shift, n_valid}. Fewer than two points or a singular system: scale = shift = NaN.
__global__ void eval_lsq_finish_kernel(const double* __restrict__ partial, int nrows, double* __restrict__ fit) {
    const double* tot = column_sums<LSQ_K>(partial, nrows);
    if (threadIdx.x == 0) {
        const double a11 = tot[0], a01 = tot[1], a00 = tot[2], b1 = tot[3], b0 = tot[4];
        double sc = __builtin_nan(""), sh = __builtin_nan("");
        if (a11 >= 2.0) solve_2x2(a00, a01, a11, b0, b1, sc, sh);
        fit[0] = sc;
        fit[1] = sh;
        fit[2] = a11;
    }
}

// grid (blocks per frame, frames of this call); partial row of (frame f, block b) = partial[(f * gridDim.x + b) * 7 ...]
template <typename GT>
__global__ void __launch_bounds__(EV_T) eval_metric_partial_kernel(const float* __restrict__ pred, const GT* __restrict__ gt, long long px, double max_depth,
                                                                   const double* __restrict__ fit, double* __restrict__ partial) {
    const double scale = fit[0], shift = fit[1], dmax = max_depth;      // the depth clip is fp64 whatever gt's type
    const GT hi = (GT)max_depth;
    const float* __restrict__ pf = pred + (size_t)blockIdx.y * px;
    const GT* __restrict__ gf = gt + (size_t)blockIdx.y * px;
    double* row = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * MET_K;
    plane_partial<MET_K, 2>(px, row, [&](long long i, double (&s)[MET_K]) {
        const GT g32 = gf[i];
        if (gt_valid(g32, hi)) {
            const double g = (double)g32;
            const double p = aligned_depth(pf[i], scale, shift, dmax);
            const double d = p - g;
            const double r1 = p / g, r2 = g / p;
            const double r = r1 > r2 ? r1 : r2;
            s[0] += 1.0;
            s[1] += fabs(d) / g;
            s[2] += (d * d) / g;
            s[3] += d * d;
            s[4] += r < 1.25 ? 1.0 : 0.0;
            s[5] += r < 1.25 * 1.25 ? 1.0 : 0.0;
            s[6] += r < 1.25 * 1.25 * 1.25 ? 1.0 : 0.0;
        }
    });
}

// One workgroup. Thread t owns frames t, t + 256, ...: it sums a frame's block rows in index order, forms the frame's ratios and adds
// them to its own running sums (frames in increasing order); the threads' sums meet in the fixed tree. The delta ratios are float32
// count / n as metric.py's threshold_percentage has them (a float32 count tensor over an integer tensor); everything else is fp64.
// result = {abs_rel, sq_rel, rmse, delta1, delta2, delta3, frames used}; no frame with a valid pixel: the six metrics are NaN.
__global__ void __launch_bounds__(EV_T) eval_metric_finish_kernel(const double* __restrict__ partial, int nframes, int bpf, double* __restrict__ result) {
    double s[MET_K] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // frames used, then the six per-frame metrics
    for (int f = threadIdx.x; f < nframes; f += EV_T) {
        double a[MET_K];
        plane_rows_sum(partial, f, bpf, a);
        if (a[0] > 0.0) {
            const float nf = (float)a[0];
            s[0] += 1.0;
            s[1] += a[1] / a[0];
            s[2] += a[2] / a[0];
            s[3] += sqrt(a[3] / a[0]);
            s[4] += (double)((float)a[4] / nf);
            s[5] += (double)((float)a[5] / nf);
            s[6] += (double)((float)a[6] / nf);
        }
    }
    __shared__ double red[MET_K][EV_T];
#pragma unroll
    for (int k = 0; k < MET_K; ++k) red[k][threadIdx.x] = s[k];
    block_tree_sum(red);
    if (threadIdx.x < MET_K) {
        const double used = red[0][0];
        if (threadIdx.x == 0)
            result[MET_K - 1] = used;
        else
            result[threadIdx.x - 1] = used > 0.0 ? red[threadIdx.x][0] / used : __builtin_nan("");
    }
}

}  // namespace

extern "C" int vda_eval_lsq_partial(const float* pred, const void* gt, int gt_is_f64, long long n, double max_depth, double* partial, int row_offset,
                                    int nblk, vda_stream_t stream) {
    VDA_REQUIRE(pred && gt && partial, "vda_eval_lsq_partial: null pointer");
    VDA_REQUIRE(n > 0, "vda_eval_lsq_partial: bad size n=%lld", n);
    VDA_REQUIRE(nblk > 0 && nblk <= R64_MAX_BLOCKS, "vda_eval_lsq_partial: bad block count %d (1..%d)", nblk, R64_MAX_BLOCKS);
    VDA_REQUIRE(row_offset >= 0 && row_offset <= R64_MAX_ROWS - nblk, "vda_eval_lsq_partial: bad row offset %d", row_offset);
    VDA_REQUIRE(gt_is_f64 == 0 || gt_is_f64 == 1, "vda_eval_lsq_partial: gt_is_f64 must be 0 or 1");
    VDA_REQUIRE(aligned_to(partial, 8) && aligned_to(pred, 4) && aligned_to(gt, gt_is_f64 ? 8 : 4),
                "vda_eval_lsq_partial: misaligned pointer (the fp64 workspace needs 8-byte alignment)");
    double* rows = partial + (size_t)row_offset * LSQ_K;
    hipStream_t s = (hipStream_t)stream;
    if (gt_is_f64)
        hipLaunchKernelGGL(eval_lsq_partial_kernel<double>, dim3(nblk), dim3(EV_T), 0, s, pred, (const double*)gt, n, max_depth, rows);
    else
        hipLaunchKernelGGL(eval_lsq_partial_kernel<float>, dim3(nblk), dim3(EV_T), 0, s, pred, (const float*)gt, n, max_depth, rows);
    VDA_LAUNCH_CHECK();
    return 0;
}

extern "C" int vda_eval_lsq_finish(const double* partial, int nrows, double* fit, vda_stream_t stream) {
    VDA_REQUIRE(partial && fit, "vda_eval_lsq_finish: null pointer");
    VDA_REQUIRE(nrows > 0 && nrows <= R64_MAX_ROWS, "vda_eval_lsq_finish: bad row count n=%d (1..%d)", nrows, R64_MAX_ROWS);
    VDA_REQUIRE(aligned_to(partial, 8) && aligned_to(fit, 8), "vda_eval_lsq_finish: misaligned pointer (fp64 needs 8-byte alignment)");
    hipLaunchKernelGGL(eval_lsq_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, partial, nrows, fit);
    VDA_LAUNCH_CHECK();
    return 0;
}

extern "C" int vda_eval_metric_partial(const float* pred, const void* gt, int gt_is_f64, int nframes, long long px, double max_depth, const double* fit,
                                       double* partial, int frame_offset, int blocks_per_frame, vda_stream_t stream) {
    VDA_REQUIRE(pred && gt && fit && partial, "vda_eval_metric_partial: null pointer");
    if (check_plane_rows("vda_eval_metric_partial", "frame", nframes, R64_MAX_PLANES, px, blocks_per_frame, frame_offset)) return 1;
    VDA_REQUIRE(gt_is_f64 == 0 || gt_is_f64 == 1, "vda_eval_metric_partial: gt_is_f64 must be 0 or 1");
    VDA_REQUIRE(aligned_to(partial, 8) && aligned_to(fit, 8) && aligned_to(pred, 4) && aligned_to(gt, gt_is_f64 ? 8 : 4),
                "vda_eval_metric_partial: misaligned pointer (the fp64 workspace needs 8-byte alignment)");
    double* rows = partial + (size_t)frame_offset * blocks_per_frame * MET_K;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(blocks_per_frame, nframes);
    if (gt_is_f64)
        hipLaunchKernelGGL(eval_metric_partial_kernel<double>, grid, dim3(EV_T), 0, s, pred, (const double*)gt, px, max_depth, fit, rows);
    else
        hipLaunchKernelGGL(eval_metric_partial_kernel<float>, grid, dim3(EV_T), 0, s, pred, (const float*)gt, px, max_depth, fit, rows);
    VDA_LAUNCH_CHECK();
    return 0;
}

extern "C" int vda_eval_metric_finish(const double* partial, int nframes, int blocks_per_frame, double* result, vda_stream_t stream) {
    VDA_REQUIRE(partial && result, "vda_eval_metric_finish: null pointer");
    if (check_plane_rows("vda_eval_metric_finish", "frame", nframes, R64_MAX_ROWS, 1, blocks_per_frame)) return 1;
    VDA_REQUIRE(aligned_to(partial, 8) && aligned_to(result, 8), "vda_eval_metric_finish: misaligned pointer (fp64 needs 8-byte alignment)");
    hipLaunchKernelGGL(eval_metric_finish_kernel, dim3(1), dim3(EV_T), 0, (hipStream_t)stream, partial, nframes, blocks_per_frame, result);
    VDA_LAUNCH_CHECK();
    return 0;
}
