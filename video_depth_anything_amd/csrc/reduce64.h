// The fixed-order fp64 reduction of the scorers, stated once: stitch.hip (window fit), eval.hip (benchmark scorer), tae.hip (temporal
// alignment error) and losses.hip (validation losses) compute every sum with the pieces below.
//
// THE DETERMINISM CONTRACT
//   1. Each thread keeps fp64 running sums over a grid-stride slice of a plane (plane_partial), elements in increasing index order.
//   2. The block's threads meet in a fixed LDS tree (block_tree_sum: thread t takes t + 128, then t + 64, ...) and the first K
//      threads write the block's K sums to its own row of a partial workspace with ordinary stores (block_store_sums).
//   3. A one-workgroup finisher adds a plane's rows in index order (plane_rows_sum; column_sums where there is one plane), then
//      combines the planes' values in a fixed order: thread t owns planes t, t + 256, ... and the threads meet in the same tree.
//   No floating-point atomics anywhere. A result therefore depends on the block counts and on the caller's chunking (they fix the
//   order of the additions), never on timing; tests/test_scorer_bits_gpu.py holds every kernel built from this header to recorded
//   bits. Changing the order of an addition here changes those bits and is a change of the contract.
//
// EVERY FILE THAT INCLUDES THIS HEADER IS BUILT WITH -ffp-contract=off (build.py PER_FILE; tests/test_abi.py checks it):
// aligned_depth's scale * x + shift rounds twice, as numpy evaluates it, solve_2x2's products round before they are subtracted, and
// the callers' centred sums (d - mu) * (y - mu) must not be fused either.
#pragma once
#include "vda_common.h"

constexpr int R64_T = 256;                   // threads per block of every kernel built from these pieces

// `red[k][t]` holds thread t's value of quantity k; afterwards red[k][0] is the block's. Fixed tree: the same order every run.
template <int K, int T>
__device__ __forceinline__ void block_tree_sum(double (&red)[K][T]) {
    __syncthreads();
    for (int w = T / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
#pragma unroll
            for (int k = 0; k < K; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + w];
        }
        __syncthreads();
    }
}

// The threads' sums s[K] -> LDS -> tree -> the first K threads store the block's sums to `row`.
template <int K>
__device__ __forceinline__ void block_store_sums(const double (&s)[K], double* __restrict__ row) {
    __shared__ double red[K][R64_T];
#pragma unroll
    for (int k = 0; k < K; ++k) red[k][threadIdx.x] = s[k];
    block_tree_sum(red);
    if ((int)threadIdx.x < K) row[threadIdx.x] = red[threadIdx.x][0];
}

// The block's sum of one value per thread, returned to every thread (a finisher's "the threads' sums meet in the fixed tree").
__device__ __forceinline__ double block_total(double v) {
    __shared__ double red[1][R64_T];
    red[0][threadIdx.x] = v;
    block_tree_sum(red);
    return red[0][0];
}

// vda_common.h's wave_sum in fp64, where a sum never leaves its wave: a fixed xor butterfly, every lane ends with the same bits.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One block's share of a plane of px pixels, blocks along gridDim.x: f(i, s) adds pixel i's terms to the thread's sums; the block's
// K sums go to `row`. UNROLL is the loop's unroll hint: each kernel keeps the one it was measured with.
template <int K, int UNROLL = 4, typename F>
__device__ __forceinline__ void plane_partial(long long px, double* __restrict__ row, F f) {
    double s[K];
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = 0.0;
#pragma unroll UNROLL
    for (long long i = (long long)blockIdx.x * R64_T + threadIdx.x; i < px; i += (long long)gridDim.x * R64_T) f(i, s);
    block_store_sums(s, row);
}

// a[K] = plane p's bpp block rows of K doubles, added in index order
template <int K>
__device__ __forceinline__ void plane_rows_sum(const double* __restrict__ partial, int p, int bpp, double (&a)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = 0.0;
    for (int b = 0; b < bpp; ++b) {
#pragma unroll
        for (int k = 0; k < K; ++k) a[k] += partial[((size_t)p * bpp + b) * K + k];
    }
}

// The column form, for a single plane: thread k < K adds column k of nrows rows in index order. Returns the K totals in LDS, readable
// by every thread of the block.
template <int K>
__device__ __forceinline__ const double* column_sums(const double* __restrict__ partial, int nrows) {
    __shared__ double tot[K];
    if ((int)threadIdx.x < K) {
        double a = 0.0;
        for (int b = 0; b < nrows; ++b) a += partial[(size_t)b * K + threadIdx.x];
        tot[threadIdx.x] = a;
    }
    __syncthreads();
    return tot;
}

// [a00 a01; a01 a11] [sc; sh] = [b0; b1] in closed form. A singular system leaves sc / sh as the caller set them (each caller has
// its own fallback) and returns false.
__device__ __forceinline__ bool solve_2x2(double a00, double a01, double a11, double b0, double b1, double& sc, double& sh) {
    const double det = a00 * a11 - a01 * a01;
    if (det == 0.0) return false;
    sc = (a11 * b0 - a01 * b1) / det;
    sh = (a00 * b1 - a01 * b0) / det;
    return true;
}

// np.clip(infs, 1e-3, None) on the float32 array (NaN stays NaN)
__device__ __forceinline__ float clip_pred(float p) { return p < 1e-3f ? 1e-3f : p; }

// clip(1 / clip(scale * clip(pred, 1e-3) + shift, 1e-3), 1e-3, max_depth): the scorers' aligned depth. eval.hip's pass 2 and both
// passes of tae.hip call this one function, so TAE scores the depth the fit was judged on, bit for bit.
__device__ __forceinline__ double aligned_depth(float p, double scale, double shift, double dmax) {
    const double m = scale * (double)clip_pred(p);
    double al = m + shift;                                  // two roundings (-ffp-contract=off)
    al = al < 1e-3 ? 1e-3 : al;
    double d = 1.0 / al;
    d = d < 1e-3 ? 1e-3 : d;
    return d > dmax ? dmax : d;
}

// ------------------------------------------------------------------------------------------------ host-side argument checks
constexpr int R64_MAX_BLOCKS = 4096;         // blocks per plane (per call where there is one plane)
constexpr int R64_MAX_ROWS = 1 << 22;        // partial rows one finisher walks
constexpr int R64_MAX_PLANES = 65535;        // planes of one launch: gridDim.y

inline bool aligned_to(const void* p, unsigned n) { return ((uintptr_t)p & (n - 1)) == 0; }

// The refusals of a launch over `planes` planes of px pixels with bpp blocks each, whose rows follow those of `first` earlier planes
// in the workspace, and of its finisher (px = 1; max_planes = R64_MAX_ROWS where the planes are not a grid dimension). `plane` names
// the caller's planes in the message. Returns 0 when the arguments are fine.
inline int check_plane_rows(const char* who, const char* plane, long long planes, long long max_planes, long long px, long long bpp,
                            long long first = 0) {
    VDA_REQUIRE(planes > 0 && planes <= max_planes && px > 0, "%s: bad sizes n=%lld %ss of %lld pixels", who, planes, plane, px);
    VDA_REQUIRE(bpp > 0 && bpp <= R64_MAX_BLOCKS, "%s: bad sizes: block count %lld per %s (1..%d)", who, bpp, plane, R64_MAX_BLOCKS);
    VDA_REQUIRE(first >= 0 && (first + planes) * bpp <= R64_MAX_ROWS, "%s: bad sizes: %s offset %lld or too many partial rows (%lld %ss x %lld blocks)",
                who, plane, first, planes, plane, bpp);
    return 0;
}
