// Baseline JPEG frames back to pixels (video_depth_anything_amd/mjpeg.py). The contract is mjpeg.decode_jpeg_numpy
// and every step is integer arithmetic that wraps (unsigned here, so that no overflow is undefined), so this file needs no
// special compile flag and reproduces the twin bit for bit - the statuses of corrupt streams included:
//
//   entropy   canonical Huffman codes, EXTEND, DC prediction per restart interval: mjpeg_decode_core.h (shared with the host
//             program that runs it under sanitizers)
//   pixels    d = coef * Q; libjpeg's islow IDCT: constants / 2^13, columns descaled by 11, rows by 18, + 128, clamped
//   chroma    cropped to ceil(W / 2) (x ceil(H / 2)), upsampled by libjpeg's "fancy" triangle filters with replicated edges:
//             h2v1  (3 a[i] + a[i-1] + 1) >> 2, (3 a[i] + a[i+1] + 2) >> 2
//             h2v2  r = 3 a[j] + a[j-1 | j+1], then (3 r[i] + r[i-1] + 8) >> 4, (3 r[i] + r[i+1] + 7) >> 4
//   colour    R = Y + ((91881 cr + 32768) >> 16), G = Y + ((-22554 cb - 46802 cr + 32768) >> 16), B = Y + ((116130 cb + 32768) >> 16)
//
// Three launches. (a) entropy: a lane per restart interval (64 per workgroup, the decode tables in LDS); the host found the
// intervals, the lane reads only inside its interval's bytes and writes only its MCUs' blocks of the zeroed coefficient
// workspace; an error becomes the frame's status through an atomic max and ends the lane. A stream without restart markers is one
// interval per frame: one lane decodes it, which is correct and slow by nature. (b) IDCT: a workgroup takes 32 blocks, a thread a
// column and then a row of one block (the workspace between the passes in LDS), and writes the row's 8 samples as one 8-byte
// store into the component's plane on the block grid. (c) upsample and colour: a workgroup takes 256 consecutive pixels of the
// output, reads the planes with clamped neighbours, stages the 768 bytes in LDS and stores them in address order.
#include "vda_common.h"

#include "mjpeg_decode_core.h"

namespace {

constexpr int MJD_T = 256;                 // threads of the pixel kernels
constexpr int MJD_LANES = 64;              // restart intervals per workgroup of the entropy kernel: one wave
constexpr int MJD_IV = 5;                  // ints per interval record: frame, byte offset, byte length, first MCU, MCU count

struct MjdQ {
    uint16_t q[3][64];                     // per component, natural order
};

struct MjdLayout {
    MjdGeom g;
    int plane_h[3], plane_w[3];            // each component's sample plane: its block grid x 8
    size_t plane_off[3], frame_samples;    // a frame's planes back to back
    size_t intervals, tables, coef, planes, total;
};

bool mjd_layout(int n, int h, int w, int components, int hs, int vs, int intervals, MjdLayout& L) {
    if (n < 1 || h < 1 || w < 1 || h > 65535 || w > 65535 || intervals < 0) return false;
    if (components != 1 && components != 3) return false;
    if (components == 1 ? !(hs == 1 && vs == 1) : !((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2))) return false;
    MjdGeom& g = L.g;
    g.components = components, g.hs = hs, g.vs = vs;
    g.mw = (w + 8 * hs - 1) / (8 * hs), g.mh = (h + 8 * vs - 1) / (8 * vs);
    size_t at = 0;
    for (int c = 0; c < 3; ++c) {
        const int hc = c == 0 ? hs : 1, vc = c == 0 ? vs : 1;
        g.comp_off[c] = (int)at, g.comp_bw[c] = g.mw * hc;
        L.plane_h[c] = g.mh * vc * 8, L.plane_w[c] = g.mw * hc * 8;
        L.plane_off[c] = at * 64;
        if (c < components) at += (size_t)g.mw * hc * g.mh * vc;          // at most 3 * 8192^2: fits an int
    }
    g.frame_blocks = (int)at;
    L.frame_samples = at * 64;
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    L.intervals = 0;
    L.tables = L.intervals + up16((size_t)intervals * MJD_IV * sizeof(int));
    L.coef = L.tables + up16(sizeof(MjdTables));
    L.planes = L.coef + (size_t)n * at * 128;
    L.total = L.planes + (size_t)n * at * 64;
    return true;
}

// -------------------------------------------------------------------------------------------------------------------- (a) entropy
// Lanes that decode different intervals diverge at every symbol: a wave takes as long as the longest chain of its lanes. (Measured
// together with a wider refill: 16 intervals to a wave instead of 64 was no faster - profiles/mjpeg/decode_entropy_variants.txt.)
__global__ void __launch_bounds__(MJD_LANES) mjpeg_decode_entropy_kernel(const uint8_t* __restrict__ scan, const int* __restrict__ intervals,
                                                                          int n_intervals, const MjdTables* __restrict__ tables, MjdGeom g,
                                                                          int16_t* __restrict__ coef, int* __restrict__ status) {
    __shared__ MjdTables t;
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(tables);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&t);
        for (int i = threadIdx.x; i < (int)(sizeof(MjdTables) / 4); i += MJD_LANES) dst[i] = src[i];
    }
    __syncthreads();
    const long long i = (long long)blockIdx.x * MJD_LANES + threadIdx.x;
    if (i >= n_intervals) return;
    const int* iv = intervals + i * MJD_IV;            // validated by the host side of the call: the frame, the bytes and the MCUs exist
    const int frame = iv[0];
    const int st = mjd_decode_interval(scan + iv[1], iv[2], iv[3], iv[4], g, t, coef + (long long)frame * g.frame_blocks * 64);
    if (st != MJD_OK) atomicMax(status + frame, st);
}

// ----------------------------------------------------------------------------------------------------------------------- (b) IDCT
// The 8-point islow butterfly on in[0..7], descaled by `shift`; unsigned arithmetic wraps as the twin's int32 does.
__device__ __forceinline__ void mjd_idct8(const int* in, int* out, int shift) {
    const uint32_t i0 = in[0], i1 = in[1], i2 = in[2], i3 = in[3], i4 = in[4], i5 = in[5], i6 = in[6], i7 = in[7];
    uint32_t z1 = (i2 + i6) * 4433u;
    const uint32_t t2 = z1 - i6 * 15137u, t3 = z1 + i2 * 6270u;
    const uint32_t t0 = (i0 + i4) << 13, t1 = (i0 - i4) << 13;
    const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    uint32_t a0 = i7, a1 = i5, a2 = i3, a3 = i1;
    z1 = a0 + a3;
    uint32_t z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const uint32_t z5 = (z3 + z4) * 9633u;
    a0 *= 2446u, a1 *= 16819u, a2 *= 25172u, a3 *= 12299u;
    z1 *= (uint32_t)-7373, z2 *= (uint32_t)-20995;
    z3 = z3 * (uint32_t)-16069 + z5, z4 = z4 * (uint32_t)-3196 + z5;
    a0 += z1 + z3, a1 += z2 + z4, a2 += z2 + z3, a3 += z1 + z4;
    const uint32_t r = 1u << (shift - 1);
    const uint32_t o[8] = {t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3};
#pragma unroll
    for (int k = 0; k < 8; ++k) out[k] = (int)(o[k] + r) >> shift;
}

// grid = ceil(n * frame_blocks / 32) workgroups; thread = (block of the workgroup, column | row)
__global__ void __launch_bounds__(MJD_T) mjpeg_decode_idct_kernel(const int16_t* __restrict__ coef, MjdQ q, MjdLayout L, long long blocks,
                                                                   uint8_t* __restrict__ planes) {
    __shared__ int ws[32][8][9];           // rows padded: the column pass writes 8 rows at one column
    const int t = threadIdx.x, lb = t >> 3, x = t & 7;
    const long long b = (long long)blockIdx.x * 32 + lb;
    const bool live = b < blocks;
    int frame = 0, fb = 0, c = 0;
    if (live) {
        frame = (int)(b / L.g.frame_blocks), fb = (int)(b - (long long)frame * L.g.frame_blocks);
        c = L.g.components == 3 ? (fb >= L.g.comp_off[2] ? 2 : fb >= L.g.comp_off[1] ? 1 : 0) : 0;
        int in[8], out[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) in[k] = (int)coef[b * 64 + k * 8 + x] * (int)q.q[c][k * 8 + x];       // |coef * Q| < 2^23
        mjd_idct8(in, out, 11);
#pragma unroll
        for (int k = 0; k < 8; ++k) ws[lb][k][x] = out[k];
    }
    __syncthreads();
    if (live) {
        int in[8], out[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) in[k] = ws[lb][x][k];                  // x is the row now
        mjd_idct8(in, out, 18);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lo |= (uint32_t)min(max(out[k] + 128, 0), 255) << (8 * k);
            hi |= (uint32_t)min(max(out[k + 4] + 128, 0), 255) << (8 * k);
        }
        const int cb = fb - L.g.comp_off[c], brow = cb / L.g.comp_bw[c], bcol = cb - brow * L.g.comp_bw[c];
        uint8_t* dst = planes + (size_t)frame * L.frame_samples + L.plane_off[c] + (size_t)(brow * 8 + x) * L.plane_w[c] + bcol * 8;
        *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);               // 8-byte aligned: plane widths and offsets are multiples of 8
    }
}

// -------------------------------------------------------------------------------------------------------- (c) upsample and colour
// grid = ceil(n * h * w / 256) workgroups over the output's pixels in address order
template <int components>
__global__ void __launch_bounds__(MJD_T) mjpeg_decode_colour_kernel(const uint8_t* __restrict__ planes, MjdLayout L, int h, int w, long long pixels,
                                                                     uint8_t* __restrict__ out) {
    __shared__ uint8_t rgb[MJD_T * components];
    const int t = threadIdx.x;
    const long long p0 = (long long)blockIdx.x * MJD_T, p = p0 + t;
    if (p < pixels) {
        const long long row = p / w;
        const int x = (int)(p - row * w), frame = (int)(row / h), y = (int)(row - (long long)frame * h);
        const uint8_t* fp = planes + (size_t)frame * L.frame_samples;
        const int Y = fp[L.plane_off[0] + (size_t)y * L.plane_w[0] + x];
        if constexpr (components == 1) {
            rgb[t] = (uint8_t)Y;
        } else {
            int cc[2];
            const int cw = (w + 1) >> 1, chh = (h + 1) >> 1;               // the chroma planes' cropped size when they are subsampled
#pragma unroll
            for (int c = 1; c < 3; ++c) {
                const uint8_t* a = fp + L.plane_off[c];
                const int pw = L.plane_w[c];
                int v;
                if (L.g.hs == 1) {
                    v = a[(size_t)y * pw + x];
                } else {
                    const int i = x >> 1, in = (x & 1) ? min(i + 1, cw - 1) : max(i - 1, 0);
                    if (L.g.vs == 1) {
                        v = (3 * a[(size_t)y * pw + i] + a[(size_t)y * pw + in] + ((x & 1) ? 2 : 1)) >> 2;
                    } else {
                        const int j = y >> 1, jn = (y & 1) ? min(j + 1, chh - 1) : max(j - 1, 0);
                        const int r0 = 3 * a[(size_t)j * pw + i] + a[(size_t)jn * pw + i];
                        const int r1 = 3 * a[(size_t)j * pw + in] + a[(size_t)jn * pw + in];
                        v = (3 * r0 + r1 + ((x & 1) ? 7 : 8)) >> 4;
                    }
                }
                cc[c - 1] = v - 128;
            }
            const int cb = cc[0], cr = cc[1];
            rgb[3 * t] = (uint8_t)min(max(Y + ((91881 * cr + 32768) >> 16), 0), 255);
            rgb[3 * t + 1] = (uint8_t)min(max(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0), 255);
            rgb[3 * t + 2] = (uint8_t)min(max(Y + ((116130 * cb + 32768) >> 16), 0), 255);
        }
    }
    __syncthreads();
    const long long live = min((long long)MJD_T, pixels - p0) * components;
    uint8_t* dst = out + p0 * components;
    for (int i = t; i < live; i += MJD_T) dst[i] = rgb[i];
}

}  // namespace

extern "C" size_t vda_mjpeg_decode_workspace_bytes(int n, int h, int w, int components, int hs, int vs, int intervals) {
    MjdLayout L;
    return mjd_layout(n, h, w, components, hs, vs, intervals, L) ? L.total : 0;
}

extern "C" int vda_mjpeg_decode_u8(const uint8_t* scan, size_t scan_bytes, const int* intervals, int n_intervals, const void* tables,
                                   const uint16_t* qtables, int n, int h, int w, int components, int hs, int vs, void* workspace,
                                   size_t workspace_bytes, uint8_t* out, size_t out_capacity, int* status, vda_stream_t stream) {
    VDA_REQUIRE(scan, "vda_mjpeg_decode_u8: scan is null");
    VDA_REQUIRE(intervals, "vda_mjpeg_decode_u8: intervals is null");
    VDA_REQUIRE(tables, "vda_mjpeg_decode_u8: tables is null");
    VDA_REQUIRE(qtables, "vda_mjpeg_decode_u8: qtables is null");
    VDA_REQUIRE(workspace, "vda_mjpeg_decode_u8: workspace is null");
    VDA_REQUIRE(out, "vda_mjpeg_decode_u8: out is null");
    VDA_REQUIRE(status, "vda_mjpeg_decode_u8: status is null");
    VDA_REQUIRE(n >= 1 && h >= 1 && w >= 1, "vda_mjpeg_decode_u8: bad size n=%d h=%d w=%d (each at least 1)", n, h, w);
    VDA_REQUIRE(h <= 65535 && w <= 65535, "vda_mjpeg_decode_u8: bad size h=%d w=%d (a JPEG frame is at most 65535 x 65535)", h, w);
    VDA_REQUIRE(components == 1 || components == 3, "vda_mjpeg_decode_u8: bad components=%d (1 gray or 3 YCbCr)", components);
    VDA_REQUIRE(components == 1 ? (hs == 1 && vs == 1) : ((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2)),
                "vda_mjpeg_decode_u8: bad sampling hs=%d vs=%d (1x1, 2x1 or 2x2 with 3 components, 1x1 with 1)", hs, vs);
    VDA_REQUIRE(scan_bytes <= 0x7ffffff0ULL, "vda_mjpeg_decode_u8: bad scan_bytes=%zu (at most 2^31 - 16: offsets are ints)", scan_bytes);
    VDA_REQUIRE(n_intervals >= 1, "vda_mjpeg_decode_u8: bad n_intervals=%d (at least 1)", n_intervals);
    MjdLayout L;
    mjd_layout(n, h, w, components, hs, vs, n_intervals, L);
    const long long blocks = (long long)n * L.g.frame_blocks, pixels = (long long)n * h * w;
    VDA_REQUIRE((blocks + 31) / 32 <= 0x7fffffffLL && (pixels + MJD_T - 1) / MJD_T <= 0x7fffffffLL,
                "vda_mjpeg_decode_u8: bad size n=%d h=%d w=%d (more than 2^31 - 1 workgroups)", n, h, w);
    VDA_REQUIRE(((uintptr_t)workspace & 15) == 0, "vda_mjpeg_decode_u8: workspace is not 16-byte aligned");
    VDA_REQUIRE(((uintptr_t)status & 3) == 0, "vda_mjpeg_decode_u8: status is not 4-byte aligned");
    VDA_REQUIRE(workspace_bytes >= L.total, "vda_mjpeg_decode_u8: workspace capacity %zu is below the %zu bytes of vda_mjpeg_decode_workspace_bytes",
                workspace_bytes, L.total);
    VDA_REQUIRE(out_capacity >= (size_t)pixels * components, "vda_mjpeg_decode_u8: out capacity %zu is below the %zu bytes of n * h * w * components",
                out_capacity, (size_t)pixels * components);
    MjdQ q = {};
    for (int i = 0; i < 64 * components; ++i) {
        VDA_REQUIRE(qtables[i] >= 1 && qtables[i] <= 255, "vda_mjpeg_decode_u8: bad qtables[%d]=%d (a baseline divisor is 1..255)", i, (int)qtables[i]);
        q.q[i >> 6][i & 63] = qtables[i];
    }
    const int total_mcus = L.g.mw * L.g.mh;
    for (int i = 0; i < n_intervals; ++i) {
        const int* iv = intervals + (size_t)i * MJD_IV;
        VDA_REQUIRE(iv[0] >= 0 && iv[0] < n, "vda_mjpeg_decode_u8: bad interval %d: frame %d of %d", i, iv[0], n);
        VDA_REQUIRE(iv[1] >= 0 && iv[2] >= 0 && (size_t)iv[1] + (size_t)iv[2] <= scan_bytes,
                    "vda_mjpeg_decode_u8: bad interval %d: bytes %d + %d outside the scan's %zu", i, iv[1], iv[2], scan_bytes);
        VDA_REQUIRE(iv[3] >= 0 && iv[4] >= 0 && (long long)iv[3] + iv[4] <= total_mcus,
                    "vda_mjpeg_decode_u8: bad interval %d: MCUs %d + %d outside the frame's %d", i, iv[3], iv[4], total_mcus);
    }
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    int* d_intervals = reinterpret_cast<int*>(ws + L.intervals);
    MjdTables* d_tables = reinterpret_cast<MjdTables*>(ws + L.tables);
    int16_t* coef = reinterpret_cast<int16_t*>(ws + L.coef);
    uint8_t* planes = ws + L.planes;
    hipStream_t s = (hipStream_t)stream;
    // From pageable host memory hipMemcpyAsync copies synchronously, through a staging buffer on the host (hip_runtime_api.h: "If
    // host or dst are not pinned, the memory copy will be performed synchronously"): the caller's arrays may go when this returns,
    // and the price is that the call waits on the host for these two copies and cannot be captured into a graph (vda.h says so).
    hipError_t e = hipMemcpyAsync(d_intervals, intervals, (size_t)n_intervals * MJD_IV * sizeof(int), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_tables, tables, sizeof(MjdTables), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(coef, 0, (size_t)blocks * 128, s);
    if (e == hipSuccess) e = hipMemsetAsync(status, 0, (size_t)n * sizeof(int), s);
    if (e != hipSuccess) {
        vda_set_error("vda_mjpeg_decode_u8: staging failed: %s", hipGetErrorString(e));
        return 2;
    }
    hipLaunchKernelGGL(mjpeg_decode_entropy_kernel, dim3((unsigned)((n_intervals + MJD_LANES - 1) / MJD_LANES)), dim3(MJD_LANES), 0, s, scan, d_intervals,
                       n_intervals, d_tables, L.g, coef, status);
    VDA_LAUNCH_CHECK();
    hipLaunchKernelGGL(mjpeg_decode_idct_kernel, dim3((unsigned)((blocks + 31) / 32)), dim3(MJD_T), 0, s, coef, q, L, blocks, planes);
    VDA_LAUNCH_CHECK();
    const dim3 grid((unsigned)((pixels + MJD_T - 1) / MJD_T));
    if (components == 3)
        hipLaunchKernelGGL(mjpeg_decode_colour_kernel<3>, grid, dim3(MJD_T), 0, s, planes, L, h, w, pixels, out);
    else
        hipLaunchKernelGGL(mjpeg_decode_colour_kernel<1>, grid, dim3(MJD_T), 0, s, planes, L, h, w, pixels, out);
    VDA_LAUNCH_CHECK();
    return 0;
}
