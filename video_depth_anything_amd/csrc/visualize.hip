// Depth mapped to the bytes of a visualisation video (the reference's utils/dc_utils.py save_video: the global range to uint8, then
// matplotlib's 256-entry inferno table unless grayscale). The arithmetic is the contract, fp32 and every operation
// rounded once, no fused multiply-add and no reciprocal:
//
//   span = minmax[1] - minmax[0];  if (!(span > 0)) span = 1e-12f          (a constant video maps to 0)
//   v    = ((depth[i] - minmax[0]) / span) * 255.f                         (the IEEE division)
//   k    = 0 if v is NaN or v < 0,  255 if v >= 255,  else v truncated     (the clamp defines what numpy's astype leaves open)
//   out  = k (lut == NULL, one byte a pixel)  or  lut[k][0..2] (three bytes a pixel, packed RGB)
//
// THIS FILE IS BUILT WITH -ffp-contract=off (build.py PER_FILE) and visualize.colorize_numpy reproduces every byte.
//
// A pure stream: 4 bytes read and 1 or 3 written per pixel. `depth` is only 4-byte aligned and `out` may sit at any byte (a frame
// of 37 x 53 pixels inside [N, H, W]), so the launch peels `head` pixels (at most 3) after which the output address is a multiple
// of 4: gray advances one byte a pixel, RGB three, and 3 * head = -head (mod 4). From there a group of four pixels is one whole
// dword of gray or three of RGB, stored non-temporally (the bytes are never read again by this kernel or the next); the at most
// three pixels behind the last whole group are single bytes like the head. The table sits in LDS as 256 dwords r | g << 8 | b << 16,
// so a colour is one ds_read and a group's three dwords are shifts and ors of four of them. Grid-stride over the groups with a
// capped grid; one launch, no atomics, nothing depends on scheduling.
#include "vda_common.h"

namespace {

constexpr int VIS_T = 256;                 // threads of a workgroup
constexpr int VIS_MAX_WGS = 2048;          // 8 workgroups on each of 256 CUs: one pass of the grid covers 2^21 pixels, the rest is strided
typedef float vis_f32x4 __attribute__((ext_vector_type(4), aligned(4)));      // four pixels in one load, at the alignment of one

__device__ __forceinline__ uint32_t vis_level(float d, float lo, float span) {
    float v = ((d - lo) / span) * 255.f;
    v = v >= 0.f ? v : 0.f;                // NaN, or below the range
    v = v >= 255.f ? 255.f : v;
    return (uint32_t)(int)v;               // selects, not branches: the four pixels of a group stay one straight line
}

template <bool RGB>
__device__ __forceinline__ void vis_one(const float* __restrict__ depth, uint8_t* __restrict__ out, long long p, float lo, float span,
                                        const uint32_t* table) {
    const uint32_t k = vis_level(depth[p], lo, span);
    if constexpr (RGB) {
        const uint32_t c = table[k];
        out[3 * p] = (uint8_t)c, out[3 * p + 1] = (uint8_t)(c >> 8), out[3 * p + 2] = (uint8_t)(c >> 16);
    } else {
        out[p] = (uint8_t)k;
    }
}

// pixels [0, head) and [head + 4 * groups, n) as single bytes (workgroup 0), groups of four pixels from `head` on as whole dwords
template <bool RGB>
__global__ void __launch_bounds__(VIS_T) depth_vis_kernel(const float* __restrict__ depth, long long n, const float* __restrict__ minmax,
                                                          const uint8_t* __restrict__ lut, uint8_t* __restrict__ out, int head, long long groups) {
    __shared__ uint32_t table[VIS_T];
    const int t = threadIdx.x;
    if constexpr (RGB) {
        table[t] = (uint32_t)lut[3 * t] | ((uint32_t)lut[3 * t + 1] << 8) | ((uint32_t)lut[3 * t + 2] << 16);
        __syncthreads();
    }
    const float lo = minmax[0];
    float span = minmax[1] - lo;
    if (!(span > 0.f)) span = 1e-12f;
    if (blockIdx.x == 0) {
        const long long rest = head + 4 * groups + (t - 4);                   // threads 4 .. 6: the pixels behind the last group
        if (t < head) vis_one<RGB>(depth, out, t, lo, span, table);
        else if (t >= 4 && rest < n) vis_one<RGB>(depth, out, rest, lo, span, table);
    }
    const float* __restrict__ src = depth + head;
    uint32_t* __restrict__ dst = reinterpret_cast<uint32_t*>(out + (RGB ? 3 : 1) * head);     // 4-byte aligned: that is what head is for
    const long long stride = (long long)gridDim.x * VIS_T;
#pragma unroll 2
    for (long long g = (long long)blockIdx.x * VIS_T + t; g < groups; g += stride) {
        const vis_f32x4 d = *reinterpret_cast<const vis_f32x4*>(src + 4 * g);
        uint32_t k[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) k[j] = vis_level(d[j], lo, span);
        if constexpr (RGB) {
            const uint32_t c0 = table[k[0]], c1 = table[k[1]], c2 = table[k[2]], c3 = table[k[3]];
            __builtin_nontemporal_store(c0 | (c1 << 24), dst + 3 * g);
            __builtin_nontemporal_store((c1 >> 8) | (c2 << 16), dst + 3 * g + 1);
            __builtin_nontemporal_store((c2 >> 16) | (c3 << 8), dst + 3 * g + 2);
        } else {
            __builtin_nontemporal_store(k[0] | (k[1] << 8) | (k[2] << 16) | (k[3] << 24), dst + g);
        }
    }
}

}  // namespace

extern "C" int vda_depth_vis_u8(const float* depth, long long n, const float* minmax, const uint8_t* lut, uint8_t* out, vda_stream_t stream) {
    VDA_REQUIRE(depth, "vda_depth_vis_u8: depth is null");
    VDA_REQUIRE(minmax, "vda_depth_vis_u8: minmax is null");
    VDA_REQUIRE(out, "vda_depth_vis_u8: out is null");
    VDA_REQUIRE(n >= 1, "vda_depth_vis_u8: bad size n=%lld (at least one pixel)", n);
    VDA_REQUIRE(((uintptr_t)depth & 3) == 0, "vda_depth_vis_u8: depth is not 4-byte aligned");
    VDA_REQUIRE(((uintptr_t)minmax & 3) == 0, "vda_depth_vis_u8: minmax is not 4-byte aligned");
    const int a = (int)((uintptr_t)out & 3);
    const long long peel = lut ? a : (4 - a) & 3;                             // a + 3 * a and a + (4 - a) are multiples of 4
    const int head = (int)(peel < n ? peel : n);
    const long long groups = (n - head) / 4;
    const long long wgs = (groups + VIS_T - 1) / VIS_T;
    const dim3 grid((unsigned)(wgs < 1 ? 1 : wgs > VIS_MAX_WGS ? VIS_MAX_WGS : wgs)), block(VIS_T);
    if (lut)
        hipLaunchKernelGGL(depth_vis_kernel<true>, grid, block, 0, (hipStream_t)stream, depth, n, minmax, lut, out, head, groups);
    else
        hipLaunchKernelGGL(depth_vis_kernel<false>, grid, block, 0, (hipStream_t)stream, depth, n, minmax, lut, out, head, groups);
    VDA_LAUNCH_CHECK();
    return 0;
}
