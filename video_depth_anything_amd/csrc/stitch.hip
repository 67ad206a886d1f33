// Window stitcher of infer_video_depth on the device (video_depth.py:216-254, utils/util.py:40-74).
//
// Per window k > 0 the reference (numpy, host) does: least-squares scale/shift of the window's first two frames
// against the two reference key frames, affine + clamp of frames 2..31, an 8-frame linear cross-fade into the
// previous window's tail, and appends the rest. Here that is one deterministic reduction (fp64 partials, fixed
// combination order, no atomics: the pattern stated in reduce64.h) and one fused element-wise kernel; scale/shift
// never leave the device, so the stitch of window k queues behind its forward on the same stream and costs ~20 us
// instead of ~15 ms of numpy.
//
// Both kernels are HBM-bound streaming passes (64 MB per 518x518 window).
#include "reduce64.h"

namespace {

constexpr int LSQ_T = R64_T;
constexpr int LSQ_K = 4;
constexpr int LSQ_UNROLL = 1;     // not unrolled: a hint of 4 doubles the kernel's registers (20 -> 42 VGPRs), HBM-bound either way

// partial[b] = { sum p*p, sum p, sum p*t, sum t } of block b's grid-stride slice, fp64
__global__ void __launch_bounds__(LSQ_T) lsq_partial_kernel(const float* __restrict__ pred, const float* __restrict__ target, long long n,
                                                            double* __restrict__ partial) {
    plane_partial<LSQ_K, LSQ_UNROLL>(n, partial + (size_t)blockIdx.x * LSQ_K, [&](long long i, double (&s)[LSQ_K]) {
        const double p = (double)pred[i], t = (double)target[i];
        s[0] += p * p;
        s[1] += p;
        s[2] += p * t;
        s[3] += t;
    });
}

// utils/util.py:40-62 with the all-ones mask: a_11 = n. The reference evaluates the closed form on fp32 sums, where
// det = a00*a11 - a01^2 cancels most of its digits; fp64 here, rounded to fp32 at the end. A singular system: scale 1, shift 0.
__global__ void lsq_finish_kernel(const double* __restrict__ partial, int nblk, double n, float* __restrict__ scale_shift) {
    const double* tot = column_sums<LSQ_K>(partial, nblk);
    if (threadIdx.x == 0) {
        double sc = 1.0, sh = 0.0;
        solve_2x2(tot[0], tot[1], n, tot[2], tot[3], sc, sh);
        scale_shift[0] = (float)sc;
        scale_shift[1] = (float)sh;
    }
}

// numpy evaluates a*b + c on float32 arrays with two roundings. THIS FILE IS BUILT WITH -ffp-contract=off (build.py
// PER_FILE): with -ffp-contract=fast the AMDGPU backend fuses mul+add whatever the source says (HIP's __fmul_rn is a
// plain multiply and `#pragma clang fp contract(off)` does not survive), which changes the last bit of the stitch.

// out = d * scale + shift; out[out < 0] = 0   (NaN stays NaN)
__device__ __forceinline__ float affine_clamp(float d, float sc, float sh) {
    const float m = d * sc;
    const float o = m + sh;
    return o < 0.f ? 0.f : o;
}

// One pixel per thread, every slot of the window:
//   chunk[j]     = tail[j] * (1 - w_j) + aff(win[2 + j]) * w_j      j = 0..7    cross-fade into the previous tail (util.py:65-74)
//   chunk[8 + j] = aff(win[10 + j])                                 j = 0..13   final frames
//   tail[j]      = aff(win[24 + j])                                 j = 0..7    may still be cross-faded by the next window
//   ref1         = aff(win[12])                                     second alignment key frame (video_depth.py:243-248)
__global__ void __launch_bounds__(256) stitch_window_kernel(const float* __restrict__ win, const float* __restrict__ scale_shift,
                                                            float* __restrict__ chunk, float* __restrict__ tail, float* __restrict__ ref1,
                                                            long long px, const float* __restrict__ wts) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= px) return;
    const float sc = scale_shift[0], sh = scale_shift[1];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float v = affine_clamp(win[(2 + j) * px + i], sc, sh);
        const float a = tail[j * px + i] * wts[j], b = v * wts[8 + j];
        chunk[j * px + i] = a + b;
    }
#pragma unroll
    for (int j = 0; j < 14; ++j) {
        const float v = affine_clamp(win[(10 + j) * px + i], sc, sh);
        chunk[(8 + j) * px + i] = v;
        if (j == 2) ref1[i] = v;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) tail[j * px + i] = affine_clamp(win[(24 + j) * px + i], sc, sh);
}

// out[i] = aff(in[i]): the aligned form of key frames other ranks computed (the key-frame exchange, scheduler.drive_windows_keys);
// the same affine_clamp as stitch_window_kernel, so a frame aligned here is bit-equal to the one its owner's stitch produces
__global__ void __launch_bounds__(256) affine_clamp_kernel(const float* __restrict__ in, const float* __restrict__ scale_shift, float* __restrict__ out,
                                                           long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = affine_clamp(in[i], scale_shift[0], scale_shift[1]);
}

}  // namespace

extern "C" int vda_affine_clamp_f32(const float* in, const float* scale_shift, float* out, long long n, vda_stream_t stream) {
    VDA_REQUIRE(in && scale_shift && out, "vda_affine_clamp_f32: null pointer");
    VDA_REQUIRE(n > 0 && n < (1ll << 31) * 256, "vda_affine_clamp_f32: bad size %lld", n);
    hipLaunchKernelGGL(affine_clamp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in, scale_shift, out, n);
    VDA_LAUNCH_CHECK();
    return 0;
}

extern "C" int vda_lsq_scale_shift_f32(const float* pred, const float* target, long long n, double* workspace, int nblk, float* scale_shift,
                                       vda_stream_t stream) {
    VDA_REQUIRE(pred && target && workspace && scale_shift, "vda_lsq_scale_shift_f32: null pointer");
    VDA_REQUIRE(n > 0 && nblk > 0 && nblk <= R64_MAX_BLOCKS, "vda_lsq_scale_shift_f32: bad sizes n=%lld nblk=%d", n, nblk);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(lsq_partial_kernel, dim3(nblk), dim3(LSQ_T), 0, s, pred, target, n, workspace);
    hipLaunchKernelGGL(lsq_finish_kernel, dim3(1), dim3(64), 0, s, (const double*)workspace, nblk, (double)n, scale_shift);
    VDA_LAUNCH_CHECK();
    return 0;
}

extern "C" int vda_stitch_window_f32(const float* win, const float* scale_shift, float* chunk, float* tail, float* ref1, long long px,
                                     const float* wts, vda_stream_t stream) {
    VDA_REQUIRE(win && scale_shift && chunk && tail && ref1 && wts, "vda_stitch_window_f32: null pointer");
    VDA_REQUIRE(px > 0 && px < (1ll << 31) * 256, "vda_stitch_window_f32: bad frame size %lld", px);
    hipLaunchKernelGGL(stitch_window_kernel, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, (hipStream_t)stream, win, scale_shift, chunk, tail,
                       ref1, px, wts);
    VDA_LAUNCH_CHECK();
    return 0;
}

// ---- running depth range of a streamed video (infer_video_depth_stream): minmax = (min(minmax[0], min x), max(minmax[1], max x)).
// ONE workgroup: the entry point takes no workspace and uses no atomics, so there is nowhere for several workgroups to meet. It runs
// on the consumer's stream beside two windows' forwards and reads one 22-frame chunk per window (26 MB at 518x518, well under a
// millisecond from one CU against ~50 ms of forward), so it is latency, not throughput, that it must not add to. Min and max are
// exact in any order: the result does not depend on the reduction tree. Comparisons, not fminf / fmaxf: a NaN is never taken (the
// stream raises on an overflowed window before its frames could reach this kernel).
namespace {

constexpr int MM_T = 1024;

__device__ __forceinline__ void mm_take(float v, float& lo, float& hi) {
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
}

__global__ void __launch_bounds__(MM_T) minmax_accum_kernel(const float* __restrict__ x, long long n, float* __restrict__ minmax) {
    float lo = __builtin_inff(), hi = -__builtin_inff();
    // elements before the first 16-byte boundary, then float4 loads, then the remainder: every index is < n
    long long head = (long long)(((16u - (unsigned)((uintptr_t)x & 15u)) & 15u) >> 2);
    if (head > n) head = n;
    if ((long long)threadIdx.x < head) mm_take(x[threadIdx.x], lo, hi);
    const f32x4* __restrict__ x4 = reinterpret_cast<const f32x4*>(x + head);
    const long long n4 = (n - head) >> 2;
#pragma unroll 4
    for (long long i = threadIdx.x; i < n4; i += MM_T) {
        const f32x4 v = x4[i];
        mm_take(v[0], lo, hi);
        mm_take(v[1], lo, hi);
        mm_take(v[2], lo, hi);
        mm_take(v[3], lo, hi);
    }
    const long long rest = head + (n4 << 2) + threadIdx.x;          // at most 3 elements
    if (rest < n) mm_take(x[rest], lo, hi);
    __shared__ float red[2][MM_T];
    red[0][threadIdx.x] = lo;
    red[1][threadIdx.x] = hi;
    __syncthreads();
    for (int w = MM_T / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            const float a = red[0][threadIdx.x + w], b = red[1][threadIdx.x + w];
            red[0][threadIdx.x] = a < red[0][threadIdx.x] ? a : red[0][threadIdx.x];
            red[1][threadIdx.x] = b > red[1][threadIdx.x] ? b : red[1][threadIdx.x];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float lo0 = minmax[0], hi0 = minmax[1];                // the running values (the caller starts them at +inf, -inf)
        minmax[0] = red[0][0] < lo0 ? red[0][0] : lo0;
        minmax[1] = red[1][0] > hi0 ? red[1][0] : hi0;
    }
}

}  // namespace

extern "C" int vda_minmax_accum_f32(const float* x, long long n, float* minmax, vda_stream_t stream) {
    VDA_REQUIRE(x && minmax, "vda_minmax_accum_f32: null pointer");
    VDA_REQUIRE(n > 0, "vda_minmax_accum_f32: bad size %lld", n);
    VDA_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)minmax & 3) == 0, "vda_minmax_accum_f32: pointers must be 4-byte aligned");
    hipLaunchKernelGGL(minmax_accum_kernel, dim3(1), dim3(MM_T), 0, (hipStream_t)stream, x, n, minmax);
    VDA_LAUNCH_CHECK();
    return 0;
}
