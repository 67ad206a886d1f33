// Frames larger than --max_res scaled down on the device, as the reference's cv2 branch scales them (utils/dc_utils.py:
// cv2.resize(frame, (width, height)) on uint8 frames): cv2's INTER_LINEAR for 8-bit images, restated from its published algorithm
// (OpenCV modules/imgproc/src/resize.cpp: resizeGeneric_ with HResizeLinear<uchar,int,short> and VResizeLinear<uchar,int,short>).
// The arithmetic is the contract; the coordinates are resize.hip's, the rest is integer:
//
//   per axis   scale = 1.0 / ((double)n_dst / (double)n_src)            fp64, on the host, in this order
//              f     = (float)((d + 0.5) * scale - 0.5)                 fp64, rounded once to fp32
//              s     = floor(f);  f = f - (float)s                      fp32
//   columns    zero the weight at the border: s < 0 -> f = 0, s = 0;  s >= w - 1 -> f = 0, s = w - 1 (only tap s is read there)
//   rows       replicate the border: f stays, the indices s and s + 1 are each clamped into [0, h - 1]
//   weights    a0 = 1.f - fx, a1 = fx, b0 = 1.f - fy, b1 = fy, each made a 16-bit integer rint(a * 2048.f) (half to even, saturated)
//   columns    T = S[x0] * a0 + S[x1] * a1                                                   int32, at most 255 * 2048
//   rows       out = (((b0 * (T0 >> 4)) >> 16) + ((b1 * (T1 >> 4)) >> 16) + 2) >> 2          int32, nothing negative
//
// THIS FILE IS BUILT WITH -ffp-contract=off (build.py PER_FILE): the coordinate is a product and a difference, each rounded.
// scale.resize_frames_numpy reproduces every step, so the bytes are the twin's.
//
// A plain HBM stream of interleaved pixels [h, w, c], c = 1 or 3. A thread owns FOUR consecutive bytes of an output row, whatever
// pixel and channel each belongs to, so a 3-byte pixel never splits a store: the four bytes leave as one dword. A byte's column taps
// and weights do not depend on the row: they are computed once and kept while the workgroup walks groups of up to RU8_ROWS
// consecutive output rows of one image; the row's own taps are uniform over the workgroup.
// The 16 source bytes behind a thread's dword are scattered single bytes: read as 16 byte loads from global memory they made the
// kernel run at a quarter of a copy's rate (measured, profiles/resize_u8; that the load count is the cause is inferred). So a
// workgroup first copies the part of the source its group of rows reads - the columns under its tile, the rows from the first
// row's upper tap to the last row's lower tap - into LDS with aligned dword loads, every source byte once, and takes the taps from
// there. That needs a 4-aligned source with rows of a multiple of 4 bytes and a part that fits the LDS the host asked for (it asks
// for fewer rows a group before it gives up); otherwise the taps are read from global memory, byte by byte. Likewise the dword
// store needs a 4-aligned `out` and output rows of a multiple of 4 bytes; otherwise (and nowhere else) the same thread stores its
// bytes one by one, the last thread of a row only those the row has. No atomics; every store is an ordinary vector store.
#include "vda_common.h"

namespace {

constexpr int RU8_T = 256;                     // threads of a workgroup
constexpr int RU8_TILE = 1024;                 // bytes of an output row one workgroup covers: a dword per thread
constexpr int RU8_ROWS = 8;                    // consecutive output rows of a group (4, 2, 1 when the source part would not fit)
constexpr int RU8_MAX_GROUP_BLOCKS = 65535;    // gridDim.y
constexpr int RU8_MAX_ROW_BYTES = 1 << 30;     // blockIdx.x * 1024 + threadIdx.x * 4 + 3 stays an int
constexpr int RU8_LDS_BYTES = 64 * 1024;       // the most a workgroup stages
static_assert(RU8_TILE == 4 * RU8_T, "a dword per thread");

// the coordinate of output index d on one axis: (source index before any border rule, weight of the next tap)
__device__ __forceinline__ void source_coord(int d, double scale, int& s, float& f) {
    const float c = (float)(((double)d + 0.5) * scale - 0.5);
    const float fl = floorf(c);
    s = (int)fl;
    f = c - fl;
}

// cv2's saturate_cast<short>(a * INTER_RESIZE_COEF_SCALE): rint (half to even), then saturated
__device__ __forceinline__ int coefficient(float a) {
    const int q = __float2int_rn(a * 2048.f);
    return q < -32768 ? -32768 : (q > 32767 ? 32767 : q);
}

// a column's two taps and the weight of the second, after the border rule
__device__ __forceinline__ void column_taps(int x, double scale_x, int w, int& x0, int& x1, float& fx) {
    source_coord(x, scale_x, x0, fx);
    if (x0 < 0) {
        fx = 0.f;
        x0 = 0;
    }
    if (x0 >= w - 1) {
        fx = 0.f;
        x0 = w - 1;
    }
    x1 = x0 + 1 < w ? x0 + 1 : w - 1;                            // at the right border the second tap IS tap x0: nothing past the row is read
}

// a row's two taps and the weight of the second, after the border rule
__device__ __forceinline__ void row_taps(int y, double scale_y, int h, int& y0, int& y1, float& fy) {
    int sy;
    source_coord(y, scale_y, sy, fy);
    y0 = sy < 0 ? 0 : (sy > h - 1 ? h - 1 : sy);
    y1 = sy + 1 < 0 ? 0 : (sy + 1 > h - 1 ? h - 1 : sy + 1);
}

// four output bytes of one row as a dword: r0 / r1 are the two source rows from column `lo` on (in global memory or in LDS: inlined
// once per space)
__device__ __forceinline__ uint32_t four_bytes(const uint8_t* r0, const uint8_t* r1, const unsigned (&o0)[4], const unsigned (&o1)[4], const int (&a0)[4],
                                               const int (&a1)[4], int b0, int b1) {
    uint32_t packed = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        unsigned p0 = o0[k], p1 = o1[k];
        asm volatile("" : "+v"(p0), "+v"(p1));                   // the offsets stay 32-bit registers here: a load is scalar row base + register
        // every factor is below 2^24 (a byte, a weight of at most 2^15, a sum of at most 255 * 2048 >> 4): 24-bit multiplies,
        // whose 32-bit results are the int32 products of the contract
        const int t0 = __mul24((int)r0[p0], a0[k]) + __mul24((int)r0[p1], a1[k]);
        const int t1 = __mul24((int)r1[p0], a0[k]) + __mul24((int)r1[p1], a1[k]);
        const int v = (int)((__umul24(b0, t0 >> 4) >> 16) + (__umul24(b1, t1 >> 4) >> 16) + 2) >> 2;
        packed |= (uint32_t)(v & 255) << (8 * k);
    }
    return packed;
}

// Only a thread that owns bytes of the row may call this (the kernel's `owner`: for the others nb is not positive and dst lies past
// the row). DWORD ignores nb: the host picks it only when the output rows are a multiple of 4 bytes, so that an owner owns all four.
template <bool DWORD>
__device__ __forceinline__ void store_bytes(uint8_t* dst, uint32_t packed, int nb) {
    if (DWORD) {
        *reinterpret_cast<uint32_t*>(dst) = packed;              // rows of a multiple of 4 bytes there: every thread owns four bytes
    } else {
        for (int k = 0; k < nb; ++k) dst[k] = (uint8_t)(packed >> (8 * k));
    }
}

// grid (ceil(W * C / 1024), min(n * groups_per_image, 65535)); group g = (image g / groups_per_image, output rows
// [(g % groups_per_image) * group_rows, + group_rows) of it). lds_dwords: the dynamic LDS of the launch, 0 = never stage.
template <int C, bool DWORD>
__global__ void __launch_bounds__(RU8_T) resize_linear_u8_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int n, int group_rows,
                                                                 int groups_per_image, int lds_dwords, int h, int w, int H, int W, double scale_y,
                                                                 double scale_x) {
    extern __shared__ uint32_t stage[];
    const int row_bytes = W * C;
    const int tile = blockIdx.x * RU8_TILE;                      // < row_bytes
    const int j0 = tile + threadIdx.x * 4;
    const bool owner = j0 < row_bytes;                           // a thread past the row's end only helps to stage
    const int nb = row_bytes - j0 < 4 ? row_bytes - j0 : 4;      // bytes of the row this thread owns (not positive when it is no owner)
    // the source columns under this tile, [lo, lo + 4 * nd): from the first pixel's left tap to the last pixel's right tap, widened
    // to dwords (the taps are monotonic in the column, so every tap of the tile lies inside; hi <= w * C when that is a multiple of 4)
    const int last = (tile + RU8_TILE < row_bytes ? tile + RU8_TILE : row_bytes) - 1;
    int xa0, xa1, xb0, xb1;
    float unused;
    column_taps(tile / C, scale_x, w, xa0, xa1, unused);
    column_taps(last / C, scale_x, w, xb0, xb1, unused);
    const int lo = (xa0 * C) & ~3, hi = (xb1 * C + C + 3) & ~3;
    const int nd = (hi - lo) >> 2;
    unsigned o0[4], o1[4];                                       // per byte: offsets of its two taps from column `lo` of a source row ...
    int a0[4], a1[4];                                            // ... and their weights
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = owner && k < nb ? j0 + k : row_bytes - 1;  // past the row: the last byte's taps, computed and never stored
        const int x = j / C, ch = j - x * C;
        int x0, x1;
        float fx;
        column_taps(x, scale_x, w, x0, x1, fx);
        o0[k] = x0 * C + ch - lo;
        o1[k] = x1 * C + ch - lo;
        a0[k] = coefficient(1.f - fx);
        a1[k] = coefficient(fx);
    }
    const size_t src_row_bytes = (size_t)w * C;
    const int groups = n * groups_per_image;                     // at most n * H: fits
    for (int g = blockIdx.y; g < groups; g += gridDim.y) {
        const int image = g / groups_per_image;
        const int ya = (g - image * groups_per_image) * group_rows;
        const int yb = H - ya < group_rows ? H : ya + group_rows;                        // output rows [ya, yb) of `image`
        const uint8_t* __restrict__ src = in + (size_t)image * h * src_row_bytes;
        uint8_t* __restrict__ dst = out + ((size_t)image * H + ya) * row_bytes + j0;
        int ys, ye, t;
        row_taps(ya, scale_y, h, ys, t, unused);
        row_taps(yb - 1, scale_y, h, t, ye, unused);                                     // source rows [ys, ye] (the taps are monotonic in the row)
        ys = __builtin_amdgcn_readfirstlane(ys);
        ye = __builtin_amdgcn_readfirstlane(ye);
        const bool staged = (long long)(ye - ys + 1) * nd <= (long long)lds_dwords;    // uniform over the workgroup
        if (staged) {
            for (int rr = 0; rr <= ye - ys; ++rr) {
                const uint32_t* __restrict__ from = reinterpret_cast<const uint32_t*>(src + (size_t)(ys + rr) * src_row_bytes + lo);
                for (int cc = threadIdx.x; cc < nd; cc += RU8_T) stage[rr * nd + cc] = from[cc];
            }
            __syncthreads();
        }
        if (owner) {
            for (int y = ya; y < yb; ++y) {
                int y0, y1;
                float fy;
                row_taps(y, scale_y, h, y0, y1, fy);
                // the row's taps and weights are the same in every lane: kept in scalar registers, so that a source row's address
                // is one scalar base and a load adds the thread's 32-bit offset to it
                y0 = __builtin_amdgcn_readfirstlane(y0);
                y1 = __builtin_amdgcn_readfirstlane(y1);
                const int b0 = __builtin_amdgcn_readfirstlane(coefficient(1.f - fy)), b1 = __builtin_amdgcn_readfirstlane(coefficient(fy));
                uint32_t packed;
                if (staged) {
                    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(stage);
                    packed = four_bytes(bytes + (y0 - ys) * nd * 4, bytes + (y1 - ys) * nd * 4, o0, o1, a0, a1, b0, b1);
                } else {
                    packed = four_bytes(src + (size_t)y0 * src_row_bytes + lo, src + (size_t)y1 * src_row_bytes + lo, o0, o1, a0, a1, b0, b1);
                }
                store_bytes<DWORD>(dst + (size_t)(y - ya) * row_bytes, packed, nb);
            }
        }
        if (staged) __syncthreads();                             // the next group's copy overwrites what this one read
    }
}

// the LDS to ask for with groups of `group_rows` rows: an upper bound of the part a workgroup copies (the kernel checks the part
// it really has against what it was given, so a bound that is too small costs speed, never correctness)
size_t stage_bytes(int c, int group_rows, double scale_y, double scale_x) {
    const double columns = ((RU8_TILE / c + 1) * scale_x + 4) * c + 8, rows = (group_rows - 1) * scale_y + 4;
    const double bytes = columns * rows;
    return bytes > (double)RU8_LDS_BYTES ? 0 : ((size_t)bytes + 3) & ~(size_t)3;
}

template <int C>
void launch(const uint8_t* in, uint8_t* out, int n, int h, int w, int H, int W, double scale_y, double scale_x, hipStream_t stream) {
    const int row_bytes = W * C;
    int group_rows = RU8_ROWS;
    size_t lds = 0;
    if (((uintptr_t)in & 3) == 0 && (((long long)w * C) & 3) == 0) {
        while ((lds = stage_bytes(C, group_rows, scale_y, scale_x)) == 0 && group_rows > 1) group_rows /= 2;
    }
    if (lds == 0) group_rows = RU8_ROWS;
    const int groups_per_image = (H + group_rows - 1) / group_rows;
    const long long groups = (long long)n * groups_per_image;
    const dim3 grid((row_bytes + RU8_TILE - 1) / RU8_TILE, (unsigned)(groups < RU8_MAX_GROUP_BLOCKS ? groups : RU8_MAX_GROUP_BLOCKS));
    const bool dword = ((uintptr_t)out & 3) == 0 && (row_bytes & 3) == 0;
    if (dword)
        hipLaunchKernelGGL((resize_linear_u8_kernel<C, true>), grid, dim3(RU8_T), lds, stream, in, out, n, group_rows, groups_per_image, (int)(lds / 4), h, w, H,
                           W, scale_y, scale_x);
    else
        hipLaunchKernelGGL((resize_linear_u8_kernel<C, false>), grid, dim3(RU8_T), lds, stream, in, out, n, group_rows, groups_per_image, (int)(lds / 4), h, w,
                           H, W, scale_y, scale_x);
}

}  // namespace

extern "C" int vda_resize_linear_u8(const uint8_t* in, uint8_t* out, int n, int h, int w, int c, int H, int W, vda_stream_t stream) {
    VDA_REQUIRE(in && out, "vda_resize_linear_u8: null pointer");
    VDA_REQUIRE(n > 0 && h > 0 && w > 0 && H > 0 && W > 0 && (c == 1 || c == 3),
                "vda_resize_linear_u8: bad size n=%d images of %d x %d x %d to %d x %d (c must be 1 or 3)", n, h, w, c, H, W);
    VDA_REQUIRE((long long)w * c <= RU8_MAX_ROW_BYTES && (long long)W * c <= RU8_MAX_ROW_BYTES && (long long)n * H <= 0x7fffffffll &&
                    (long long)n * h <= 0x7fffffffll,
                "vda_resize_linear_u8: too large (a row of at most 2^30 bytes; n * H and n * h must fit 31 bits)");
    VDA_REQUIRE(in != out, "vda_resize_linear_u8: in == out (the resize is not in place)");
    const double scale_y = 1.0 / ((double)H / (double)h), scale_x = 1.0 / ((double)W / (double)w);
    if (c == 3)
        launch<3>(in, out, n, h, w, H, W, scale_y, scale_x, (hipStream_t)stream);
    else
        launch<1>(in, out, n, h, w, H, W, scale_y, scale_x, (hipStream_t)stream);
    VDA_LAUNCH_CHECK();
    return 0;
}
