// A prediction resized to the ground truth's grid, as the reference's scorers do it on a size mismatch (benchmark/eval/eval.py:
// get_infer -> cv2.resize(infer, (W, H)), and eval_tae.py after its optional hard crop): cv2's INTER_LINEAR on a CV_32F image,
// restated from its published algorithm (OpenCV modules/imgproc/src/resize.cpp). The arithmetic is the contract:
//
//   per axis   scale = 1.0 / ((double)n_dst / (double)n_src)            fp64, on the host, in this order
//              f     = (float)((d + 0.5) * scale - 0.5)                 fp64, rounded once to fp32
//              s     = floor(f);  f = f - (float)s                      fp32
//   columns    zero the weight at the border: s < 0 -> f = 0, s = 0;  s >= w - 1 -> f = 0, s = w - 1 (only tap s is read there)
//   rows       replicate the border: f stays, the indices s and s + 1 are each clamped into [0, h - 1]
//   out = (S[y0][x0]*a0 + S[y0][x1]*a1) * b0 + (S[y1][x0]*a0 + S[y1][x1]*a1) * b1,  a0 = 1.f - fx, a1 = fx, b0 = 1.f - fy, b1 = fy
//
// horizontal pass first, then vertical, EVERY operation rounded to fp32. Non-finite inputs are outside the contract.
// THIS FILE IS BUILT WITH -ffp-contract=off (build.py PER_FILE): the contract counts roundings and evaluate.resize_prediction_numpy
// reproduces them bit for bit.
//
// A plain HBM stream: 4 bytes written per output pixel and about 4 read (the four taps of neighbouring pixels share cache lines). One
// thread per output pixel of a row: a thread's column coordinate does not depend on the row, so it is computed once and kept while the
// block walks rows; the row coordinate is uniform over the block. No LDS, no atomics; every store is an ordinary coalesced vector store.
#include "vda_common.h"

namespace {

constexpr int RS_T = 256;
constexpr int RS_MAX_ROW_BLOCKS = 65535;     // gridDim.y
constexpr int RS_MAX_WIDTH = 1 << 30;        // blockIdx.x * 256 + threadIdx.x stays an int

// the coordinate of output index d on one axis: (source index before any border rule, weight of the next tap)
__device__ __forceinline__ void source_coord(int d, double scale, int& s, float& f) {
    const float c = (float)(((double)d + 0.5) * scale - 0.5);
    const float fl = floorf(c);
    s = (int)fl;
    f = c - fl;
}

// grid (ceil(W / 256), min(n * H, 65535)); block row r of n * H = (plane r / H, output row r % H)
__global__ void __launch_bounds__(RS_T) resize_linear_kernel(const float* __restrict__ in, float* __restrict__ out, int rows, int h, int w, int H, int W,
                                                             double scale_y, double scale_x) {
    const int x = blockIdx.x * RS_T + threadIdx.x;
    if (x >= W) return;
    int x0;
    float fx;
    source_coord(x, scale_x, x0, fx);
    if (x0 < 0) {
        fx = 0.f;
        x0 = 0;
    }
    if (x0 >= w - 1) {
        fx = 0.f;
        x0 = w - 1;
    }
    const int x1 = x0 + 1 < w ? x0 + 1 : w - 1;          // at the right border the second tap IS tap x0: nothing past the row is read
    const float a0 = 1.f - fx, a1 = fx;
    for (int r = blockIdx.y; r < rows; r += gridDim.y) {
        const int plane = r / H, y = r - plane * H;
        int sy;
        float fy;
        source_coord(y, scale_y, sy, fy);
        const int y0 = sy < 0 ? 0 : (sy > h - 1 ? h - 1 : sy);
        const int y1 = sy + 1 < 0 ? 0 : (sy + 1 > h - 1 ? h - 1 : sy + 1);
        const float b0 = 1.f - fy, b1 = fy;
        const float* __restrict__ src = in + (size_t)plane * h * w;
        const float* __restrict__ r0 = src + (size_t)y0 * w;
        const float* __restrict__ r1 = src + (size_t)y1 * w;
        const float t0 = r0[x0] * a0 + r0[x1] * a1;     // three roundings each (-ffp-contract=off)
        const float t1 = r1[x0] * a0 + r1[x1] * a1;
        out[(size_t)r * W + x] = t0 * b0 + t1 * b1;
    }
}

}  // namespace

extern "C" int vda_resize_linear_f32(const float* in, float* out, int n, int h, int w, int H, int W, vda_stream_t stream) {
    VDA_REQUIRE(in && out, "vda_resize_linear_f32: null pointer");
    VDA_REQUIRE(n > 0 && h > 0 && w > 0 && H > 0 && W > 0, "vda_resize_linear_f32: bad size n=%d planes of %d x %d to %d x %d", n, h, w, H, W);
    VDA_REQUIRE(w <= RS_MAX_WIDTH && W <= RS_MAX_WIDTH && (long long)n * H <= 0x7fffffffll && (long long)n * h <= 0x7fffffffll,
                "vda_resize_linear_f32: too large (a row of at most 2^30 pixels; n * H and n * h must fit 31 bits)");
    VDA_REQUIRE(((uintptr_t)in & 3) == 0 && ((uintptr_t)out & 3) == 0, "vda_resize_linear_f32: misaligned pointer (fp32 needs 4-byte alignment)");
    VDA_REQUIRE(in != out, "vda_resize_linear_f32: in == out (the resize is not in place)");
    const double scale_y = 1.0 / ((double)H / (double)h), scale_x = 1.0 / ((double)W / (double)w);
    const int rows = n * H;
    const dim3 grid((W + RS_T - 1) / RS_T, rows < RS_MAX_ROW_BLOCKS ? rows : RS_MAX_ROW_BLOCKS);
    hipLaunchKernelGGL(resize_linear_kernel, grid, dim3(RS_T), 0, (hipStream_t)stream, in, out, rows, h, w, H, W, scale_y, scale_x);
    VDA_LAUNCH_CHECK();
    return 0;
}
