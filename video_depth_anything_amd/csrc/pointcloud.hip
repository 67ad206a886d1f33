// Metric depth unprojected to coloured points, written as the bytes of a PLY vertex list (the reference's
// metric_depth/depth_to_pointcloud.py, which builds each cloud on the host out of fp64 planes and hands it to Open3D's writer). The
// arithmetic is the contract, fp64 and every operation rounded once:
//
//   X = (((double)c - cx) / fx) * (double)z        Y = (((double)r - cy) / fy) * (double)z        Z = (double)z
//
// the IEEE division first, the product second: numpy's (x - width / 2) / fx followed by np.multiply(x, z). A NaN X or Y is stored
// as the quiet NaN 0x7ff8000000000000 (IEEE leaves the sign of a generated NaN open: 0 * Inf is negative on x86, positive here).
// THIS FILE IS BUILT WITH -ffp-contract=off (build.py PER_FILE) and pointcloud.unproject_numpy reproduces every byte.
//
// Records are packed, 27 bytes (three doubles, r, g, b) or 15 (three floats, r, g, b), in row-major order of the kept pixels.
// Keeping a subset (0 < z <= max_depth) is a count pass over tiles of 256 pixels, an integer scan of the tile counts per frame and
// a write pass: no atomics, nothing depends on scheduling.
//
// A pure HBM stream: 7 bytes read and 27 written per point (4 more read in the count pass). The divisions are done once per column
// and once per row, by a launch of their own into two tables in the workspace (W + H doubles, cache resident); a point costs two
// fp64 products. A record at a packed offset is aligned to nothing, so no thread stores its own record to memory: a workgroup lays
// its records out in LDS at the byte offset its output has in memory modulo 16, then stores the 16-byte aligned interior of its
// range as 16 bytes per lane, consecutive lanes consecutive addresses, and its ragged head and tail (fewer than 16 bytes each) as
// single bytes. The 16 bytes on the border of two workgroups' ranges are written by byte stores of each one's own bytes only: no
// workgroup reads or writes another's. Into LDS a record goes as whole dwords plus three single bytes: 27 = 6 * 4 + 3 and
// 15 = 3 * 4 + 3, so at every byte offset o a record covers exactly 6 (3) whole aligned dwords, the first at o + hd with
// hd = (4 - o % 4) % 4, with hd bytes in front of them and 3 - hd behind.
#include "vda_common.h"

#include <cmath>

namespace {

constexpr int PC_T = 256;                        // threads of a workgroup = pixels of a tile
constexpr long long PC_MAX_PIXELS = 1ll << 30;   // h * w: a pixel index, and tile * 256 + thread, are ints
constexpr long long PC_MAX_TILES = 0x7fffffffll; // n * tiles of a frame: the grid's x extent and the index into the tile counts

struct PcLayout {                                // the workspace: [xfac: w doubles][yfac: h doubles][tile counts: n * tiles ints]
    size_t tiles, table_bytes, bytes;
};
inline PcLayout pc_layout(int n, int h, int w) {
    PcLayout L;
    L.tiles = ((size_t)h * w + PC_T - 1) / PC_T;
    L.table_bytes = ((size_t)w + h) * sizeof(double);
    // 8 bytes of slack: the tables start at the first 8-byte aligned address of a workspace that need only be 4-byte aligned
    L.bytes = (8 + L.table_bytes + (size_t)n * L.tiles * sizeof(int) + 15) & ~(size_t)15;
    return L;
}
inline size_t pc_record_bytes(int record_f32) { return record_f32 ? 15 : 27; }

// xfac[c] = (c - cx) / fx, yfac[r] = (r - cy) / fy: the contract's first two operations, once per column and row
__global__ void __launch_bounds__(PC_T) pc_factors_kernel(double* __restrict__ xfac, double* __restrict__ yfac, int h, int w, double fx, double fy,
                                                          double cx, double cy) {
    const int i = blockIdx.x * PC_T + threadIdx.x;
    if (i < w)
        xfac[i] = ((double)i - cx) / fx;
    else if (i < w + h)
        yfac[i - w] = ((double)(i - w) - cy) / fy;
}

__device__ __forceinline__ bool pc_keep(float z, float max_depth) { return z > 0.f && z <= max_depth; }   // false for NaN

// How many kept threads come before this one in the workgroup, and how many there are in all. s_wave: 4 ints of LDS.
__device__ __forceinline__ int pc_rank(bool keep, int* s_wave, int& total) {
    const unsigned long long votes = __ballot(keep);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_wave[wave] = __popcll(votes);
    __syncthreads();
    int before = __popcll(votes & ((1ull << lane) - 1ull));
    total = 0;
#pragma unroll
    for (int k = 0; k < PC_T / 64; ++k) {
        const int c = s_wave[k];
        if (k < wave) before += c;
        total += c;
    }
    return before;
}

// grid n * tiles: tile_count[frame * tiles + tile] = kept pixels among the tile's 256
__global__ void __launch_bounds__(PC_T) pc_count_kernel(const float* __restrict__ depth, int* __restrict__ tile_count, int hw, int tiles, float max_depth) {
    __shared__ int s_wave[PC_T / 64];
    const int frame = blockIdx.x / tiles, tile = blockIdx.x - frame * tiles;
    const int p = tile * PC_T + threadIdx.x;
    const bool keep = p < hw && pc_keep(depth[(size_t)frame * hw + p], max_depth);
    int total;
    pc_rank(keep, s_wave, total);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

// grid n, one workgroup per frame: the frame's tile counts become the number of kept pixels before each tile; counts[frame] = all
__global__ void __launch_bounds__(PC_T) pc_scan_kernel(int* __restrict__ tile_count, int* __restrict__ counts, int tiles) {
    __shared__ int part[PC_T];
    int* __restrict__ row = tile_count + (size_t)blockIdx.x * tiles;
    const int t = threadIdx.x, chunk = (tiles + PC_T - 1) / PC_T;
    const long long b64 = (long long)t * chunk;
    const int b = b64 < tiles ? (int)b64 : tiles, e = b64 + chunk < tiles ? (int)(b64 + chunk) : tiles;
    int s = 0;
    for (int i = b; i < e; ++i) s += row[i];
    part[t] = s;
    __syncthreads();
    int off = 0;
    for (int k = 0; k < t; ++k) off += part[k];
    for (int i = b; i < e; ++i) {
        const int c = row[i];
        row[i] = off;
        off += c;
    }
    if (t == PC_T - 1) counts[blockIdx.x] = off;          // the last thread has every chunk behind it
}

// grid n * tiles. NDW: whole dwords of a record, 6 (three doubles) or 3 (three floats); the record is 4 * NDW + 3 bytes.
template <int NDW, bool FILTER>
__global__ void __launch_bounds__(PC_T) pc_write_kernel(const float* __restrict__ depth, const uint8_t* __restrict__ rgb, uint8_t* __restrict__ records,
                                                        int* __restrict__ counts, const int* __restrict__ tile_offset, const double* __restrict__ xfac,
                                                        const double* __restrict__ yfac, int hw, int w, int tiles, size_t stride, float max_depth) {
    constexpr int RS = 4 * NDW + 3;
    constexpr int STAGE = (16 + PC_T * RS + 15) & ~15;    // LDS byte j is byte (g0 - g0 % 16) + j of the frame's slot
    __shared__ __attribute__((aligned(16))) uint32_t stage32[STAGE / 4];
    __shared__ int s_wave[PC_T / 64];
    uint8_t* stage = reinterpret_cast<uint8_t*>(stage32);
    const int t = threadIdx.x;
    const int frame = blockIdx.x / tiles, tile = blockIdx.x - frame * tiles;
    const int p = tile * PC_T + t;
    float z = 0.f;
    bool keep = false;
    if (p < hw) {
        z = depth[(size_t)frame * hw + p];
        keep = FILTER ? pc_keep(z, max_depth) : true;
    }
    int rank, total, first;                               // this record's place in the tile, the tile's records, records before the tile
    if (FILTER) {
        rank = pc_rank(keep, s_wave, total);
        first = tile_offset[blockIdx.x];
    } else {
        rank = t;
        total = hw - tile * PC_T < PC_T ? hw - tile * PC_T : PC_T;
        first = tile * PC_T;
        if (tile == 0 && t == 0) counts[frame] = hw;
    }
    const size_t g0 = (size_t)first * RS, end = g0 + (size_t)total * RS;      // the tile's bytes of the slot
    const int mis = (int)(g0 & 15);
    if (keep) {
        const int r = p / w, c = p - r * w;
        const uint8_t* __restrict__ px = rgb + ((size_t)frame * hw + p) * 3;
        const double zd = (double)z;
        double X = xfac[c] * zd, Y = yfac[r] * zd;
        if (X != X) X = __longlong_as_double(0x7ff8000000000000ll);
        if (Y != Y) Y = __longlong_as_double(0x7ff8000000000000ll);
        uint32_t d[NDW + 1];
        if constexpr (NDW == 6) {
            const unsigned long long xb = (unsigned long long)__double_as_longlong(X), yb = (unsigned long long)__double_as_longlong(Y),
                                     zb = (unsigned long long)__double_as_longlong(zd);
            d[0] = (uint32_t)xb, d[1] = (uint32_t)(xb >> 32);
            d[2] = (uint32_t)yb, d[3] = (uint32_t)(yb >> 32);
            d[4] = (uint32_t)zb, d[5] = (uint32_t)(zb >> 32);
        } else {
            d[0] = __float_as_uint((float)X), d[1] = __float_as_uint((float)Y), d[2] = __float_as_uint(z);
        }
        d[NDW] = (uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16);
        const int o = mis + rank * RS;
        const int hd = (4 - (o & 3)) & 3;
        uint32_t* dst = reinterpret_cast<uint32_t*>(stage + o + hd);
#pragma unroll
        for (int k = 0; k < NDW; ++k) dst[k] = (uint32_t)(((((unsigned long long)d[k + 1]) << 32) | d[k]) >> (8 * hd));   // record bytes hd + 4k ..
#pragma unroll
        for (int j = 0; j < 3; ++j)                       // the bytes in front of the whole dwords, then those behind
            stage[o + (j < hd ? j : 4 * NDW + j)] = (uint8_t)((j < hd ? d[0] : d[NDW]) >> (8 * j));
    }
    __syncthreads();
    uint8_t* __restrict__ slot = records + (size_t)frame * stride;           // 16-byte aligned: records is, stride is a multiple of 16
    const size_t up = (g0 + 15) & ~(size_t)15, down = end & ~(size_t)15;
    const size_t a0 = up < end ? up : end, a1 = down > a0 ? down : a0;        // [g0, a0) head, [a0, a1) whole 16-byte lines, [a1, end) tail
    const size_t lds0 = g0 - mis;
    for (size_t q = a0 + 16 * (size_t)t; q < a1; q += 16 * PC_T)
        *reinterpret_cast<uint4*>(slot + q) = *reinterpret_cast<const uint4*>(stage + (q - lds0));
    if (t < 16) {
        const size_t q = g0 + t;
        if (q < a0) slot[q] = stage[q - lds0];
    } else if (t < 32) {
        const size_t q = a1 + (t - 16);
        if (q < end) slot[q] = stage[q - lds0];
    }
}

}  // namespace

extern "C" size_t vda_pointcloud_frame_stride(int h, int w, int record_f32) {
    if (h <= 0 || w <= 0 || (record_f32 != 0 && record_f32 != 1)) return 0;
    return ((size_t)h * w * pc_record_bytes(record_f32) + 15) & ~(size_t)15;
}

extern "C" size_t vda_pointcloud_workspace_bytes(int n, int h, int w) {
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    return pc_layout(n, h, w).bytes;
}

extern "C" int vda_pointcloud_f32(const float* depth, const uint8_t* rgb, void* records, int* counts, void* workspace, size_t workspace_bytes, int n,
                                  int h, int w, double fx, double fy, double cx, double cy, float max_depth, int record_f32, vda_stream_t stream) {
    VDA_REQUIRE(depth && rgb && records && counts && workspace, "vda_pointcloud_f32: null pointer");
    VDA_REQUIRE(n > 0 && h > 0 && w > 0, "vda_pointcloud_f32: bad size n=%d frames of %d x %d", n, h, w);
    VDA_REQUIRE(std::isfinite(fx) && std::isfinite(fy) && fx != 0.0 && fy != 0.0, "vda_pointcloud_f32: bad focal length fx=%g fy=%g (finite and not zero)", fx, fy);
    VDA_REQUIRE(std::isfinite(cx) && std::isfinite(cy), "vda_pointcloud_f32: bad principal point cx=%g cy=%g (finite)", cx, cy);
    VDA_REQUIRE(max_depth >= 0.f, "vda_pointcloud_f32: bad max_depth %g (0 keeps every pixel, m > 0 keeps 0 < z <= m)", (double)max_depth);
    VDA_REQUIRE(record_f32 == 0 || record_f32 == 1, "vda_pointcloud_f32: bad record type %d (0 = doubles, 27 bytes; 1 = floats, 15 bytes)", record_f32);
    const PcLayout L = pc_layout(n, h, w);
    VDA_REQUIRE((long long)h * w <= PC_MAX_PIXELS && (unsigned long long)n * L.tiles <= (unsigned long long)PC_MAX_TILES,
                "vda_pointcloud_f32: too large (h * w at most 2^30; n * ceil(h * w / 256) at most 2^31 - 1)");
    VDA_REQUIRE(workspace_bytes >= L.bytes, "vda_pointcloud_f32: workspace too small (%zu bytes, vda_pointcloud_workspace_bytes says %zu)", workspace_bytes,
                L.bytes);
    VDA_REQUIRE(((uintptr_t)depth & 3) == 0 && ((uintptr_t)counts & 3) == 0 && ((uintptr_t)workspace & 3) == 0 && ((uintptr_t)records & 15) == 0,
                "vda_pointcloud_f32: misaligned pointer (depth, counts and workspace need 4-byte alignment, records 16)");
    double* xfac = reinterpret_cast<double*>(((uintptr_t)workspace + 7) & ~(uintptr_t)7);
    double* yfac = xfac + w;
    int* tile_count = reinterpret_cast<int*>(yfac + h);
    const int hw = h * w, tiles = (int)L.tiles;
    const size_t stride = vda_pointcloud_frame_stride(h, w, record_f32);
    const dim3 grid((unsigned)(n * L.tiles)), block(PC_T);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pc_factors_kernel, dim3((w + h + PC_T - 1) / PC_T), block, 0, s, xfac, yfac, h, w, fx, fy, cx, cy);
    VDA_LAUNCH_CHECK();
    uint8_t* out = static_cast<uint8_t*>(records);
    if (max_depth > 0.f) {
        hipLaunchKernelGGL(pc_count_kernel, grid, block, 0, s, depth, tile_count, hw, tiles, max_depth);
        VDA_LAUNCH_CHECK();
        hipLaunchKernelGGL(pc_scan_kernel, dim3(n), block, 0, s, tile_count, counts, tiles);
        VDA_LAUNCH_CHECK();
        if (record_f32)
            hipLaunchKernelGGL((pc_write_kernel<3, true>), grid, block, 0, s, depth, rgb, out, counts, tile_count, xfac, yfac, hw, w, tiles, stride, max_depth);
        else
            hipLaunchKernelGGL((pc_write_kernel<6, true>), grid, block, 0, s, depth, rgb, out, counts, tile_count, xfac, yfac, hw, w, tiles, stride, max_depth);
    } else {
        if (record_f32)
            hipLaunchKernelGGL((pc_write_kernel<3, false>), grid, block, 0, s, depth, rgb, out, counts, tile_count, xfac, yfac, hw, w, tiles, stride, max_depth);
        else
            hipLaunchKernelGGL((pc_write_kernel<6, false>), grid, block, 0, s, depth, rgb, out, counts, tile_count, xfac, yfac, hw, w, tiles, stride, max_depth);
    }
    VDA_LAUNCH_CHECK();
    return 0;
}
