// Temporal alignment error on the device: the arithmetic of the reference's benchmark/eval/eval_tae.py (eval_TAE :150-217 after the
// fit, tae_torch :60-107) for every pair of neighbouring frames in both directions. The fit {scale, shift} is the one eval.hip's pass 1
// leaves on the device; nothing returns to the host between the passes.
//
//   splat   (tae_splat_kernel)    one thread per 4 source pixels of a plane = (pair, direction): aligned depth d from pred and the fit,
//                                 unproject with K, move with R|t, project, round half to even; a pixel that lands inside the image
//                                 does atomicMax(winner[v, u], source flat index + 1) on a zeroed 32-bit plane.
//   compare (tae_compare_kernel)  one thread per 4 target pixels: a non-zero winner names the source pixel whose Qz is the splat's
//                                 value there; Qz is recomputed by the same functions the splat pass called, so the passes cannot
//                                 disagree. use = (Qz > 0) & (dst > 0) & mask; {sum |dst - Qz| / dst, count} go to fp64 block rows.
//   finish  (tae_finish_kernel)   per plane sum / count over its rows in index order (0 when the count is 0), the planes' sum in plane
//                                 order, / (2 (N - 1)) * 100.
//
// LAST WINS. The reference splats with depth_proj[valid_Y, valid_X] = valid_Z, an index assignment with duplicate indices; on the CPU
// the source pixels are visited in row-major order and the last one stays, whatever its sign. "Last in row-major order" is "largest
// flat index", and an integer max does not depend on the order of arrival: the winner plane, and with it every count, is the same in
// every run. It is the only atomic in this file; all sums are fp64 rows combined in a fixed order (the pattern stated in reduce64.h).
//
// Both passes read pred through 16-byte loads when a plane's pixel count is a multiple of 4 (scalar, still coalesced, otherwise); the
// gather of the winner's source pixel in the compare pass is the one irregular access. pred is float32, everything derived from it
// is double. THIS FILE IS BUILT WITH -ffp-contract=off (build.py PER_FILE): every product and sum rounds on its own, as in eval.hip,
// and the two passes' Qz are the same IEEE operations in the same order.
#include "reduce64.h"

namespace {

constexpr int EV_T = R64_T;                  // threads per block
constexpr int TAE_V = 4;                     // pixels per thread and step
constexpr int TAE_K = 2;                     // sum |dst - proj| / dst, count
constexpr int TAE_CAM = 28;                  // doubles per pair: fx, fy, cx, cy, R|t of i -> i+1 (3x4 row-major), R|t of i+1 -> i
constexpr int TAE_MAX_PAIRS = R64_MAX_PLANES / 2;   // 2 planes per pair on gridDim.y

// aligned_depth (reduce64.h) is eval.hip's pass 2, here for EVERY pixel

struct Cam {
    double fx, fy, cx, cy;
    double m[12];                            // rows of R|t
};

// wave-uniform: the compiler keeps these in scalar registers
__device__ __forceinline__ Cam load_cam(const double* __restrict__ cam, int pair, int dir) {
    const double* c = cam + (size_t)pair * TAE_CAM;
    Cam k;
    k.fx = c[0], k.fy = c[1], k.cx = c[2], k.cy = c[3];
#pragma unroll
    for (int e = 0; e < 12; ++e) k.m[e] = c[4 + 12 * dir + e];
    return k;
}

// P = ((x - cx) * d / fx, (y - cy) * d / fy, d); row r of P @ R^T + t
__device__ __forceinline__ void unproject(const Cam& k, int x, int y, double d, double& X, double& Y) {
    X = ((double)x - k.cx) * d / k.fx;
    Y = ((double)y - k.cy) * d / k.fy;
}
__device__ __forceinline__ double moved(const Cam& k, int r, double X, double Y, double Z) {
    return X * k.m[4 * r] + Y * k.m[4 * r + 1] + Z * k.m[4 * r + 2] + k.m[4 * r + 3];
}
// Qz of source pixel (x, y): what the splat leaves at the pixel's target, and what the compare pass reads back
__device__ __forceinline__ double source_qz(const Cam& k, int x, int y, double d) {
    double X, Y;
    unproject(k, x, y, d, X, Y);
    return moved(k, 2, X, Y, d);
}

// TAE_V consecutive elements from i0; elements at or past n are `fill`. VEC: n is a multiple of TAE_V and the plane 16-byte aligned.
template <bool VEC>
__device__ __forceinline__ void load_v(const float* __restrict__ p, long long i0, long long n, float (&v)[TAE_V]) {
    if (VEC) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(p + i0);
#pragma unroll
        for (int e = 0; e < TAE_V; ++e) v[e] = a[e];
    } else {
#pragma unroll
        for (int e = 0; e < TAE_V; ++e) v[e] = i0 + e < n ? p[i0 + e] : 0.f;
    }
}
template <bool VEC>
__device__ __forceinline__ void load_v(const unsigned* __restrict__ p, long long i0, long long n, unsigned (&v)[TAE_V]) {
    if (VEC) {
        const uint4 a = *reinterpret_cast<const uint4*>(p + i0);
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
    } else {
#pragma unroll
        for (int e = 0; e < TAE_V; ++e) v[e] = i0 + e < n ? p[i0 + e] : 0u;
    }
}
template <bool VEC>
__device__ __forceinline__ void load_v(const unsigned char* __restrict__ p, long long i0, long long n, unsigned (&v)[TAE_V]) {
    if (VEC) {
        const unsigned a = *reinterpret_cast<const unsigned*>(p + i0);
#pragma unroll
        for (int e = 0; e < TAE_V; ++e) v[e] = (a >> (8 * e)) & 0xffu;
    } else {
#pragma unroll
        for (int e = 0; e < TAE_V; ++e) v[e] = i0 + e < n ? p[i0 + e] : 0u;
    }
}

// grid (ceil(px / (TAE_V * EV_T)), 2 * pairs); plane = 2 * pair + dir; dir 0 splats frame `pair` into pair + 1, dir 1 the other way
template <bool VEC>
__global__ void __launch_bounds__(EV_T) tae_splat_kernel(const float* __restrict__ pred, int H, int W, double max_depth, const double* __restrict__ fit,
                                                         const double* __restrict__ cam, unsigned* __restrict__ winner) {
    const long long px = (long long)H * W;
    const long long i0 = ((long long)blockIdx.x * EV_T + threadIdx.x) * TAE_V;
    if (i0 >= px) return;
    const int pair = blockIdx.y >> 1, dir = blockIdx.y & 1;
    const double scale = fit[0], shift = fit[1];
    const Cam k = load_cam(cam, pair, dir);
    unsigned* __restrict__ win = winner + (size_t)blockIdx.y * px;
    float p[TAE_V];
    load_v<VEC>(pred + (size_t)(pair + dir) * px, i0, px, p);
    int y = (int)(i0 / W), x = (int)(i0 - (long long)y * W);
#pragma unroll
    for (int e = 0; e < TAE_V; ++e) {
        if (i0 + e < px) {
            const double d = aligned_depth(p[e], scale, shift, max_depth);
            double X, Y;
            unproject(k, x, y, d, X, Y);
            const double qz = moved(k, 2, X, Y, d);
            const double u = rint(moved(k, 0, X, Y, d) * k.fx / qz + k.cx);
            const double v = rint(moved(k, 1, X, Y, d) * k.fy / qz + k.cy);
            // compared as doubles: NaN and anything beyond int's range fail here and are never converted
            if (u >= 0.0 && u < (double)W && v >= 0.0 && v < (double)H)
                atomicMax(win + ((long long)(int)v * W + (int)u), (unsigned)(i0 + e) + 1u);
        }
        if (++x == W) x = 0, ++y;
    }
}

// grid (blocks per plane, 2 * pairs), grid-stride over the plane; row of (plane, block) = partial[(plane * gridDim.x + block) * 2 ...]
template <bool VEC>
__global__ void __launch_bounds__(EV_T) tae_compare_kernel(const float* __restrict__ pred, const unsigned char* __restrict__ mask, int H, int W,
                                                           double max_depth, const double* __restrict__ fit, const double* __restrict__ cam,
                                                           const unsigned* __restrict__ winner, double* __restrict__ partial) {
    const long long px = (long long)H * W;
    const int pair = blockIdx.y >> 1, dir = blockIdx.y & 1;
    const double scale = fit[0], shift = fit[1];
    const Cam k = load_cam(cam, pair, dir);
    const float* __restrict__ src = pred + (size_t)(pair + dir) * px;
    const float* __restrict__ dst = pred + (size_t)(pair + 1 - dir) * px;
    const unsigned char* __restrict__ mk = mask ? mask + (size_t)(pair + 1 - dir) * px : nullptr;
    const unsigned* __restrict__ win = winner + (size_t)blockIdx.y * px;
    double s[TAE_K] = {0.0, 0.0};
    for (long long i0 =((long long)blockIdx.x * EV_T + threadIdx.x) * TAE_V; i0 < px; i0 += (long long)gridDim.x * EV_T * TAE_V) {
        unsigned w[TAE_V], m[TAE_V] = {1u, 1u, 1u, 1u};
        float t[TAE_V];
        load_v<VEC>(win, i0, px, w);
        load_v<VEC>(dst, i0, px, t);
        if (mk) load_v<VEC>(mk, i0, px, m);
#pragma unroll
        for (int e = 0; e < TAE_V; ++e) {
            if (w[e] != 0u && m[e] != 0u) {                               // w is 0 past the plane's end
                const int si = (int)(w[e] - 1u), sy = si / W, sx = si - sy * W;
                const double proj = source_qz(k, sx, sy, aligned_depth(src[si], scale, shift, max_depth));
                const double d = aligned_depth(t[e], scale, shift, max_depth);
                if (proj > 0.0 && d > 0.0) {
                    s[0] += fabs(d - proj) / d;
                    s[1] += 1.0;
                }
            }
        }
    }
    block_store_sums(s, partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * TAE_K);
}

// One workgroup. Thread t owns planes t, t + 256, ...: rows in index order, e = sum / count (0 without a count). Thread 0 then adds
// the planes' errors in plane order, which is the order the reference adds them in.
// result = {tae, error[nplanes], count[nplanes]}
__global__ void __launch_bounds__(EV_T) tae_finish_kernel(const double* __restrict__ partial, int nplanes, int bpp, double* __restrict__ result) {
    for (int p = threadIdx.x; p < nplanes; p += EV_T) {
        double a[TAE_K];
        plane_rows_sum(partial, p, bpp, a);
        result[1 + p] = a[1] > 0.0 ? a[0] / a[1] : 0.0;
        result[1 + nplanes + p] = a[1];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int p = 0; p < nplanes; ++p) tot += result[1 + p];
        result[0] = tot / (double)nplanes * 100.0;                        // nplanes = 2 (N - 1)
    }
}

// the shared refusals of the two passes; returns 0 when the arguments are fine
int check_planes(const char* who, const void* pred, const void* fit, const void* cam, const void* winner, int npairs, int H, int W) {
    VDA_REQUIRE(pred && fit && cam && winner, "%s: null pointer", who);
    VDA_REQUIRE(npairs > 0 && npairs <= TAE_MAX_PAIRS && H > 0 && W > 0, "%s: bad size n=%d pairs of %d x %d", who, npairs, H, W);
    VDA_REQUIRE((long long)H * W < 2147483647LL, "%s: plane too large (%d x %d: a source index + 1 must fit 31 bits)", who, H, W);
    VDA_REQUIRE(aligned_to(fit, 8) && aligned_to(cam, 8) && aligned_to(pred, 4) && aligned_to(winner, 4),
                "%s: misaligned pointer (the fp64 arrays need 8-byte alignment)", who);
    return 0;
}

}  // namespace

extern "C" int vda_tae_splat(const float* pred, int npairs, int H, int W, double max_depth, const double* fit, const double* cam, unsigned int* winner,
                             vda_stream_t stream) {
    if (check_planes("vda_tae_splat", pred, fit, cam, winner, npairs, H, W)) return 1;
    const long long px = (long long)H * W;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(winner, 0, (size_t)npairs * 2 * px * sizeof(unsigned), s) != hipSuccess) {
        vda_set_error("vda_tae_splat: clearing the winner planes failed");
        return 2;
    }
    const dim3 grid((unsigned)((px + TAE_V * EV_T - 1) / (TAE_V * EV_T)), 2 * npairs);
    if (px % TAE_V == 0 && ((uintptr_t)pred & 15) == 0)
        hipLaunchKernelGGL(tae_splat_kernel<true>, grid, dim3(EV_T), 0, s, pred, H, W, max_depth, fit, cam, winner);
    else
        hipLaunchKernelGGL(tae_splat_kernel<false>, grid, dim3(EV_T), 0, s, pred, H, W, max_depth, fit, cam, winner);
    VDA_LAUNCH_CHECK();
    return 0;
}

extern "C" int vda_tae_compare(const float* pred, const unsigned char* mask, int npairs, int H, int W, double max_depth, const double* fit,
                               const double* cam, const unsigned int* winner, double* partial, int pair_offset, int blocks_per_plane,
                               vda_stream_t stream) {
    if (check_planes("vda_tae_compare", pred, fit, cam, winner, npairs, H, W)) return 1;
    VDA_REQUIRE(partial, "vda_tae_compare: null pointer");
    VDA_REQUIRE(pair_offset >= 0, "vda_tae_compare: bad pair offset %d", pair_offset);
    const long long px = (long long)H * W;
    if (check_plane_rows("vda_tae_compare", "plane", 2LL * npairs, R64_MAX_PLANES, px, blocks_per_plane, 2LL * pair_offset)) return 1;
    VDA_REQUIRE(aligned_to(partial, 8), "vda_tae_compare: misaligned pointer (the fp64 workspace needs 8-byte alignment)");
    double* rows = partial + (size_t)pair_offset * 2 * blocks_per_plane * TAE_K;
    const dim3 grid(blocks_per_plane, 2 * npairs);
    hipStream_t s = (hipStream_t)stream;
    if (px % TAE_V == 0 && ((uintptr_t)pred & 15) == 0 && ((uintptr_t)winner & 15) == 0 && ((uintptr_t)mask & 3) == 0)
        hipLaunchKernelGGL(tae_compare_kernel<true>, grid, dim3(EV_T), 0, s, pred, mask, H, W, max_depth, fit, cam, winner, rows);
    else
        hipLaunchKernelGGL(tae_compare_kernel<false>, grid, dim3(EV_T), 0, s, pred, mask, H, W, max_depth, fit, cam, winner, rows);
    VDA_LAUNCH_CHECK();
    return 0;
}

extern "C" int vda_tae_finish(const double* partial, int npairs, int blocks_per_plane, double* result, vda_stream_t stream) {
    VDA_REQUIRE(partial && result, "vda_tae_finish: null pointer");
    if (check_plane_rows("vda_tae_finish", "plane", 2LL * npairs, R64_MAX_ROWS, 1, blocks_per_plane)) return 1;
    VDA_REQUIRE(aligned_to(partial, 8) && aligned_to(result, 8), "vda_tae_finish: misaligned pointer (fp64 needs 8-byte alignment)");
    hipLaunchKernelGGL(tae_finish_kernel, dim3(1), dim3(EV_T), 0, (hipStream_t)stream, partial, 2 * npairs, blocks_per_plane, result);
    VDA_LAUNCH_CHECK();
    return 0;
}
