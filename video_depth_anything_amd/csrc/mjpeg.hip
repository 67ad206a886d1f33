// Frames as baseline JPEG scans, for a Motion-JPEG AVI (video_depth_anything_amd/mjpeg.py). The contract is
// mjpeg.encode_jpeg_numpy and every step is integer arithmetic, so this file needs no special compile flag and reproduces the
// twin's stream byte for byte:
//
//   colour    Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
//             Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16      Cr likewise; 4:4:4; gray input is Y alone
//   DCT       s = sample - 128, Ci = rint(8192 c_k cos((2n+1) k pi / 16)):
//             t[k][x] = (sum_n Ci[k][n] s[n][x] + 128) >> 8,  F[k][l] = (sum_m Ci[l][m] t[k][m] + 16384) >> 15   (F = 8 x coefficient)
//   quantise  q = sign(F) ((2 |F| + 8 Q) / (16 Q)), AC clamped to +-1023, stored in zig-zag order as int16
//   entropy   the four Annex K Huffman tables, one restart interval per MCU row, 1-bit padding, FF -> FF 00
//
// Three launches. (a) transform: a workgroup takes 8 neighbouring tiles of one MCU row, stages their 8 x 64 pixels in LDS with
// coalesced byte reads (edges replicated), converts, runs the two passes with one thread per column / row, and writes the
// quantised blocks as one contiguous run. (b) entropy: a workgroup per restart interval, a thread per block: bit length, a
// workgroup scan for the block's bit offset, then the bits go into the interval's zeroed staging words - plain stores for the
// words a block owns alone, integer OR-atomics for its first and last word, which neighbours share (OR is order-independent: the
// bytes never depend on scheduling); the staged bytes are then scanned for FF and written out stuffed. (c) pack: a workgroup
// per interval finds its place from the length tables and copies its bytes behind its RSTm marker; the last one appends EOI.
#include "vda_common.h"

namespace {

constexpr int MJ_T = 256;                  // threads of a workgroup
constexpr int MJ_TILES = 8;                // tiles (64 pixels of width) per workgroup of the transform kernel
constexpr int MJ_BLOCK_RAW_BYTES = 64 * 26 / 8;      // a block's bits before stuffing: DC at most 9 + 11, each AC at most 16 + 10
constexpr int MJ_BLOCK_OUT_BYTES = 2 * MJ_BLOCK_RAW_BYTES;

struct MjTables {
    uint16_t q[2][64];                     // luminance, chrominance; natural (row-major) order
};

__device__ const int MJ_DCT[8][8] = {{2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896},     {4017, 3406, 2276, 799, -799, -2276, -3406, -4017},
                                     {3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784}, {3406, -799, -4017, -2276, 2276, 4017, 799, -3406},
                                     {2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896}, {2276, -4017, 799, 3406, -3406, -799, 4017, -2276},
                                     {1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567}, {799, -2276, 3406, -4017, 4017, -3406, 2276, -799}};
// position in the scan of the coefficient at natural position row * 8 + column
__device__ const uint8_t MJ_ZIGZAG_OF[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                             41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                             46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
// code | length << 16 per symbol: [class][0..255] the AC table (symbol = run << 4 | size), [class][256 + size] the DC table
// (mjpeg.huffman_words() prints these from the Annex K bit counts and values)
constexpr int MJ_HUFF_N = 272;
__device__ const uint32_t MJ_HUFF[2][MJ_HUFF_N] = {
    {0x4000a,  0x20000,  0x20001,  0x30004,  0x4000b,  0x5001a,  0x70078,  0x800f8,  0xa03f6,  0x10ff82, 0x10ff83, 0, 0, 0, 0, 0,
     0,        0x4000c,  0x5001b,  0x70079,  0x901f6,  0xb07f6,  0x10ff84, 0x10ff85, 0x10ff86, 0x10ff87, 0x10ff88, 0, 0, 0, 0, 0,
     0,        0x5001c,  0x800f9,  0xa03f7,  0xc0ff4,  0x10ff89, 0x10ff8a, 0x10ff8b, 0x10ff8c, 0x10ff8d, 0x10ff8e, 0, 0, 0, 0, 0,
     0,        0x6003a,  0x901f7,  0xc0ff5,  0x10ff8f, 0x10ff90, 0x10ff91, 0x10ff92, 0x10ff93, 0x10ff94, 0x10ff95, 0, 0, 0, 0, 0,
     0,        0x6003b,  0xa03f8,  0x10ff96, 0x10ff97, 0x10ff98, 0x10ff99, 0x10ff9a, 0x10ff9b, 0x10ff9c, 0x10ff9d, 0, 0, 0, 0, 0,
     0,        0x7007a,  0xb07f7,  0x10ff9e, 0x10ff9f, 0x10ffa0, 0x10ffa1, 0x10ffa2, 0x10ffa3, 0x10ffa4, 0x10ffa5, 0, 0, 0, 0, 0,
     0,        0x7007b,  0xc0ff6,  0x10ffa6, 0x10ffa7, 0x10ffa8, 0x10ffa9, 0x10ffaa, 0x10ffab, 0x10ffac, 0x10ffad, 0, 0, 0, 0, 0,
     0,        0x800fa,  0xc0ff7,  0x10ffae, 0x10ffaf, 0x10ffb0, 0x10ffb1, 0x10ffb2, 0x10ffb3, 0x10ffb4, 0x10ffb5, 0, 0, 0, 0, 0,
     0,        0x901f8,  0xf7fc0,  0x10ffb6, 0x10ffb7, 0x10ffb8, 0x10ffb9, 0x10ffba, 0x10ffbb, 0x10ffbc, 0x10ffbd, 0, 0, 0, 0, 0,
     0,        0x901f9,  0x10ffbe, 0x10ffbf, 0x10ffc0, 0x10ffc1, 0x10ffc2, 0x10ffc3, 0x10ffc4, 0x10ffc5, 0x10ffc6, 0, 0, 0, 0, 0,
     0,        0x901fa,  0x10ffc7, 0x10ffc8, 0x10ffc9, 0x10ffca, 0x10ffcb, 0x10ffcc, 0x10ffcd, 0x10ffce, 0x10ffcf, 0, 0, 0, 0, 0,
     0,        0xa03f9,  0x10ffd0, 0x10ffd1, 0x10ffd2, 0x10ffd3, 0x10ffd4, 0x10ffd5, 0x10ffd6, 0x10ffd7, 0x10ffd8, 0, 0, 0, 0, 0,
     0,        0xa03fa,  0x10ffd9, 0x10ffda, 0x10ffdb, 0x10ffdc, 0x10ffdd, 0x10ffde, 0x10ffdf, 0x10ffe0, 0x10ffe1, 0, 0, 0, 0, 0,
     0,        0xb07f8,  0x10ffe2, 0x10ffe3, 0x10ffe4, 0x10ffe5, 0x10ffe6, 0x10ffe7, 0x10ffe8, 0x10ffe9, 0x10ffea, 0, 0, 0, 0, 0,
     0,        0x10ffeb, 0x10ffec, 0x10ffed, 0x10ffee, 0x10ffef, 0x10fff0, 0x10fff1, 0x10fff2, 0x10fff3, 0x10fff4, 0, 0, 0, 0, 0,
     0xb07f9,  0x10fff5, 0x10fff6, 0x10fff7, 0x10fff8, 0x10fff9, 0x10fffa, 0x10fffb, 0x10fffc, 0x10fffd, 0x10fffe, 0, 0, 0, 0, 0,
     0x20000,  0x30002,  0x30003,  0x30004,  0x30005,  0x30006,  0x4000e,  0x5001e,  0x6003e,  0x7007e,  0x800fe,  0x901fe, 0, 0, 0, 0},
    {0x20000,  0x20001,  0x30004,  0x4000a,  0x50018,  0x50019,  0x60038,  0x70078,  0x901f4,  0xa03f6,  0xc0ff4,  0, 0, 0, 0, 0,
     0,        0x4000b,  0x60039,  0x800f6,  0x901f5,  0xb07f6,  0xc0ff5,  0x10ff88, 0x10ff89, 0x10ff8a, 0x10ff8b, 0, 0, 0, 0, 0,
     0,        0x5001a,  0x800f7,  0xa03f7,  0xc0ff6,  0xf7fc2,  0x10ff8c, 0x10ff8d, 0x10ff8e, 0x10ff8f, 0x10ff90, 0, 0, 0, 0, 0,
     0,        0x5001b,  0x800f8,  0xa03f8,  0xc0ff7,  0x10ff91, 0x10ff92, 0x10ff93, 0x10ff94, 0x10ff95, 0x10ff96, 0, 0, 0, 0, 0,
     0,        0x6003a,  0x901f6,  0x10ff97, 0x10ff98, 0x10ff99, 0x10ff9a, 0x10ff9b, 0x10ff9c, 0x10ff9d, 0x10ff9e, 0, 0, 0, 0, 0,
     0,        0x6003b,  0xa03f9,  0x10ff9f, 0x10ffa0, 0x10ffa1, 0x10ffa2, 0x10ffa3, 0x10ffa4, 0x10ffa5, 0x10ffa6, 0, 0, 0, 0, 0,
     0,        0x70079,  0xb07f7,  0x10ffa7, 0x10ffa8, 0x10ffa9, 0x10ffaa, 0x10ffab, 0x10ffac, 0x10ffad, 0x10ffae, 0, 0, 0, 0, 0,
     0,        0x7007a,  0xb07f8,  0x10ffaf, 0x10ffb0, 0x10ffb1, 0x10ffb2, 0x10ffb3, 0x10ffb4, 0x10ffb5, 0x10ffb6, 0, 0, 0, 0, 0,
     0,        0x800f9,  0x10ffb7, 0x10ffb8, 0x10ffb9, 0x10ffba, 0x10ffbb, 0x10ffbc, 0x10ffbd, 0x10ffbe, 0x10ffbf, 0, 0, 0, 0, 0,
     0,        0x901f7,  0x10ffc0, 0x10ffc1, 0x10ffc2, 0x10ffc3, 0x10ffc4, 0x10ffc5, 0x10ffc6, 0x10ffc7, 0x10ffc8, 0, 0, 0, 0, 0,
     0,        0x901f8,  0x10ffc9, 0x10ffca, 0x10ffcb, 0x10ffcc, 0x10ffcd, 0x10ffce, 0x10ffcf, 0x10ffd0, 0x10ffd1, 0, 0, 0, 0, 0,
     0,        0x901f9,  0x10ffd2, 0x10ffd3, 0x10ffd4, 0x10ffd5, 0x10ffd6, 0x10ffd7, 0x10ffd8, 0x10ffd9, 0x10ffda, 0, 0, 0, 0, 0,
     0,        0x901fa,  0x10ffdb, 0x10ffdc, 0x10ffdd, 0x10ffde, 0x10ffdf, 0x10ffe0, 0x10ffe1, 0x10ffe2, 0x10ffe3, 0, 0, 0, 0, 0,
     0,        0xb07f9,  0x10ffe4, 0x10ffe5, 0x10ffe6, 0x10ffe7, 0x10ffe8, 0x10ffe9, 0x10ffea, 0x10ffeb, 0x10ffec, 0, 0, 0, 0, 0,
     0,        0xe3fe0,  0x10ffed, 0x10ffee, 0x10ffef, 0x10fff0, 0x10fff1, 0x10fff2, 0x10fff3, 0x10fff4, 0x10fff5, 0, 0, 0, 0, 0,
     0xa03fa,  0xf7fc3,  0x10fff6, 0x10fff7, 0x10fff8, 0x10fff9, 0x10fffa, 0x10fffb, 0x10fffc, 0x10fffd, 0x10fffe, 0, 0, 0, 0, 0,
     0x20000,  0x20001,  0x20002,  0x30006,  0x4000e,  0x5001e,  0x6003e,  0x7007e,  0x800fe,  0x901fe,  0xa03fe,  0xb07fe, 0, 0, 0, 0}};

// exclusive scan of v over the workgroup's threads in thread order; `total` = the sum. `sh`: MJ_T / 64 words of LDS.
__device__ __forceinline__ uint32_t mj_scan(uint32_t v, uint32_t& total, uint32_t* sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    if (lane == 63) sh[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < MJ_T / 64; ++i) {
        const uint32_t s = sh[i];
        before += i < wave ? s : 0u;
        all += s;
    }
    total = all;
    __syncthreads();                       // sh may be written again
    return before + incl - v;
}

// ------------------------------------------------------------------------------------------------------------------ (a) transform
// grid = n * bh * chunks workgroups: frame f, MCU row `brow`, tiles [8 chunk, 8 chunk + 8) of that row. `ch` is a template
// parameter so that the gather's index arithmetic divides by constants.
template <int ch>
__global__ void __launch_bounds__(MJ_T) mjpeg_transform_kernel(const uint8_t* __restrict__ frames, int h, int w, MjTables tables,
                                                               int16_t* __restrict__ coef, int* __restrict__ frame_len, int bh, int bw, int chunks) {
    __shared__ uint8_t raw[8 * 64 * 3];
    __shared__ int s[3][8][65];            // rows padded: the row pass reads 8 rows at one column offset
    __shared__ __attribute__((aligned(16))) int16_t zz[MJ_TILES * 3 * 64];
    __shared__ uint32_t qt[2][64], qmagic[2][64];
    const int t = threadIdx.x;
    int b = blockIdx.x;
    const int chunk = b % chunks;
    b /= chunks;
    const int brow = b % bh, f = b / bh;
    if (chunk == 0 && brow == 0 && t == 0) frame_len[f] = 0;              // the entropy kernel adds the intervals' sizes up
    if (t < 64 * (ch == 3 ? 2 : 1)) {
        // x / (16 Q) = (x * magic) >> 32 exactly for x * 16 Q < 2^32 (x = 2 |F| + 8 Q < 2^15, 16 Q < 2^12): no division per coefficient
        const uint32_t Q = tables.q[t >> 6][t & 63];
        qt[t >> 6][t & 63] = Q;
        qmagic[t >> 6][t & 63] = 0xffffffffu / (16 * Q) + 1;
    }
    const int x0 = chunk * 64, y0 = brow * 8, rowbytes = 64 * ch;
    for (int i = t; i < 8 * rowbytes; i += MJ_T) {
        const int row = i / rowbytes, rem = i - row * rowbytes, px = rem / ch, c = rem - px * ch;
        const int x = min(x0 + px, w - 1), y = min(y0 + row, h - 1);      // the last column / row again beyond the edge
        raw[i] = frames[(((long long)f * h + y) * w + x) * ch + c];
    }
    __syncthreads();
    for (int p = t; p < 8 * 64; p += MJ_T) {
        const int row = p >> 6, px = p & 63;
        if constexpr (ch == 3) {
            const int r = raw[3 * p], g = raw[3 * p + 1], bl = raw[3 * p + 2];
            s[0][row][px] = ((19595 * r + 38470 * g + 7471 * bl + 32768) >> 16) - 128;
            s[1][row][px] = ((-11059 * r - 21709 * g + 32768 * bl + (128 << 16) + 32767) >> 16) - 128;
            s[2][row][px] = ((32768 * r - 27439 * g - 5329 * bl + (128 << 16) + 32767) >> 16) - 128;
        } else {
            s[0][row][px] = (int)raw[p] - 128;
        }
    }
    __syncthreads();
    const int c = t >> 6, col = t & 63;
    if (c < ch) {                          // columns: thread = (component, pixel column), in place
        int in[8];
#pragma unroll
        for (int n = 0; n < 8; ++n) in[n] = s[c][n][col];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            int acc = 0;
#pragma unroll
            for (int n = 0; n < 8; ++n) acc += MJ_DCT[k][n] * in[n];
            s[c][k][col] = (acc + 128) >> 8;
        }
    }
    __syncthreads();
    if (c < ch) {                          // rows: thread = (component, tile, row k of the tile)
        const int tile = col >> 3, k = col & 7;
        int in[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) in[m] = s[c][k][tile * 8 + m];
        const uint32_t *q = qt[c ? 1 : 0], *magic = qmagic[c ? 1 : 0];
#pragma unroll
        for (int l = 0; l < 8; ++l) {
            int acc = 0;
#pragma unroll
            for (int m = 0; m < 8; ++m) acc += MJ_DCT[l][m] * in[m];
            const int F = (acc + 16384) >> 15;                             // 8 x the coefficient
            const uint32_t Q = q[k * 8 + l], a = (uint32_t)(F < 0 ? -F : F);
            uint32_t v = __umulhi(2 * a + 8 * Q, magic[k * 8 + l]);
            if (k | l) v = min(v, 1023u);
            zz[(tile * ch + c) * 64 + MJ_ZIGZAG_OF[k * 8 + l]] = (int16_t)(F < 0 ? -(int)v : (int)v);
        }
    }
    __syncthreads();
    const int tiles = min(MJ_TILES, bw - chunk * MJ_TILES);
    uint32_t* dst = reinterpret_cast<uint32_t*>(coef + (((long long)f * bh + brow) * bw + (long long)chunk * MJ_TILES) * ch * 64);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(zz);
    for (int i = t; i < tiles * ch * 32; i += MJ_T) dst[i] = src[i];
}

// -------------------------------------------------------------------------------------------------------------------- (b) entropy
// One block's symbols. WRITE = false: only the bit count. WRITE = true: the bits go to `words` from bit `pos` on (bit 0 = the most
// significant bit of word 0): the first and the last word this block touches may be shared with its neighbours and are OR-ed in
// atomically, the words between them are this block's alone and are stored.
template <bool WRITE>
__device__ __forceinline__ uint32_t mj_block(const int16_t* __restrict__ blk, int dc_prev, const uint32_t* huff, uint32_t* words, uint32_t pos) {
    uint32_t cw[32];
    const uint4* p = reinterpret_cast<const uint4*>(blk);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint4 v = p[i];
        cw[4 * i] = v.x, cw[4 * i + 1] = v.y, cw[4 * i + 2] = v.z, cw[4 * i + 3] = v.w;
    }
    uint32_t total = 0, widx = pos >> 5;
    unsigned long long acc = 0;
    int nacc = pos & 31;                   // the word starts with bits that are not this block's: zeros here, OR leaves them alone
    bool first = true;
    auto put = [&](uint32_t bits, int n) {                                 // n <= 27 and nacc < 32: acc never loses a bit
        total += n;
        if constexpr (WRITE) {
            acc = (acc << n) | bits;
            nacc += n;
            if (nacc >= 32) {
                nacc -= 32;
                const uint32_t word = (uint32_t)(acc >> nacc);
                if (first) atomicOr(words + widx, word);
                else words[widx] = word;
                first = false;
                ++widx;
            }
        }
    };
    auto coded = [&](uint32_t entry, int v, int size) {                    // a Huffman code and the `size` amplitude bits of v
        const uint32_t amp = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1u);
        put(((entry & 0xffffu) << size) | amp, (int)(entry >> 16) + size);
    };
    const int dc = (int)(int16_t)(cw[0] & 0xffffu) - dc_prev;
    const int dsize = 32 - __clz(dc < 0 ? -dc : dc);
    coded(huff[256 + dsize], dc, dsize);
    int run = 0;
#pragma unroll
    for (int k = 1; k < 64; ++k) {
        const int v = (int)(int16_t)((cw[k >> 1] >> (16 * (k & 1))) & 0xffffu);
        if (v == 0) {
            ++run;
        } else {
            for (; run >= 16; run -= 16) put(huff[0xF0] & 0xffffu, (int)(huff[0xF0] >> 16));
            const int size = 32 - __clz(v < 0 ? -v : v);
            coded(huff[(run << 4) | size], v, size);
            run = 0;
        }
    }
    if (run > 0) put(huff[0] & 0xffffu, (int)(huff[0] >> 16));            // EOB, unless coefficient 63 is not zero
    if constexpr (WRITE) {
        if (nacc > 0) atomicOr(words + widx, (uint32_t)(acc << (32 - nacc)));
    }
    return total;
}

// grid = n * bh workgroups, one per restart interval = MCU row: nb = bw * ch blocks in stream order (tile, then component)
__global__ void __launch_bounds__(MJ_T) mjpeg_entropy_kernel(const int16_t* __restrict__ coef, int nb, int ch, int bh, uint32_t* __restrict__ raw,
                                                             uint8_t* __restrict__ stuffed, int* __restrict__ interval_len,
                                                             int* __restrict__ frame_len) {
    __shared__ uint32_t huff[2][MJ_HUFF_N];
    __shared__ uint32_t sh[MJ_T / 64];
    const int t = threadIdx.x;
    const long long interval = blockIdx.x;
    for (int i = t; i < 2 * MJ_HUFF_N; i += MJ_T) huff[i / MJ_HUFF_N][i % MJ_HUFF_N] = MJ_HUFF[i / MJ_HUFF_N][i % MJ_HUFF_N];
    __syncthreads();
    const int16_t* blocks = coef + interval * nb * 64;
    uint32_t* words = raw + interval * nb * (MJ_BLOCK_RAW_BYTES / 4);
    uint32_t carry = 0;                    // bits of the interval so far
    for (int base = 0; base < nb; base += MJ_T) {
        const int j = base + t;
        const bool live = j < nb;
        const uint32_t* table = huff[live && (j % ch) ? 1 : 0];
        const int dc_prev = live && j >= ch ? (int)blocks[(long long)(j - ch) * 64] : 0;      // the left neighbour of the same component
        uint32_t total;
        const uint32_t bits = live ? mj_block<false>(blocks + (long long)j * 64, dc_prev, table, nullptr, 0) : 0u;
        const uint32_t at = carry + mj_scan(bits, total, sh);
        // the words that begin inside [carry, carry + total): the one `carry` cuts through was cleared by the pass before
        for (uint32_t wd = ((carry + 31) >> 5) + t; wd < ((carry + total + 31) >> 5); wd += MJ_T) words[wd] = 0;
        __syncthreads();
        if (live) mj_block<true>(blocks + (long long)j * 64, dc_prev, table, words, at);
        carry += total;
    }
    const uint32_t nbytes = (carry + 7) >> 3;
    if (t == 0 && (carry & 7)) {           // the last byte's free bits are ones
        const uint32_t byte = carry >> 3;
        atomicOr(words + (byte >> 2), ((1u << (8 - (carry & 7))) - 1u) << (24 - 8 * (byte & 3)));
    }
    __syncthreads();
    uint8_t* dst = stuffed + interval * nb * MJ_BLOCK_OUT_BYTES;
    const uint32_t nwords = (nbytes + 3) >> 2;
    uint32_t done = 0;                     // stuffed bytes so far
    for (uint32_t base = 0; base < nwords; base += MJ_T) {
        const uint32_t wi = base + t;
        uint32_t word = 0, cnt = 0;
        int valid = 0;
        if (wi < nwords) {
            // written by other threads' atomics and stores before the barrier: read where the atomics landed
            word = __hip_atomic_load(words + wi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            valid = (int)min(4u, nbytes - 4 * wi);
            for (int i = 0; i < valid; ++i) cnt += 1 + (((word >> (24 - 8 * i)) & 0xffu) == 0xffu);
        }
        uint32_t total;
        uint32_t o = done + mj_scan(cnt, total, sh);
        for (int i = 0; i < valid; ++i) {
            const uint32_t byte = (word >> (24 - 8 * i)) & 0xffu;
            dst[o++] = (uint8_t)byte;
            if (byte == 0xffu) dst[o++] = 0;
        }
        done += total;
    }
    if (t == 0) {
        interval_len[interval] = (int)done;
        atomicAdd(frame_len + interval / bh, (int)done + (interval % bh ? 2 : 0));            // RSTm in front of every interval but the first
    }
}

// ----------------------------------------------------------------------------------------------------------------------- (c) pack
// grid = n * bh workgroups: interval r of frame f goes behind the frames before f (each frame_len + 2 for EOI) and the intervals
// before r (each with its two marker bytes)
__global__ void __launch_bounds__(MJ_T) mjpeg_pack_kernel(const uint8_t* __restrict__ stuffed, int nb, int bh, const int* __restrict__ interval_len,
                                                          const int* __restrict__ frame_len, uint8_t* __restrict__ out, long long* __restrict__ lengths) {
    __shared__ unsigned long long sum;
    const int t = threadIdx.x;
    const long long interval = blockIdx.x;
    const int f = (int)(interval / bh), r = (int)(interval % bh);
    if (t == 0) sum = 0;
    __syncthreads();
    unsigned long long part = 0;
    for (int j = t; j < f; j += MJ_T) part += (unsigned long long)frame_len[j] + 2;
    for (int k = t; k < r; k += MJ_T) part += (unsigned long long)interval_len[(long long)f * bh + k] + 2;
    if (part) atomicAdd(&sum, part);       // integers: the order does not matter
    __syncthreads();
    // the sum counted 2 for each of the r intervals before this one: the r - 1 markers between them and this interval's own
    uint8_t* dst = out + sum;
    const int len = interval_len[interval];
    if (r > 0 && t == 0) dst[-2] = 0xff, dst[-1] = (uint8_t)(0xd0 + ((r - 1) & 7));
    const uint8_t* src = stuffed + interval * nb * MJ_BLOCK_OUT_BYTES;
    for (int i = t; i < len; i += MJ_T) dst[i] = src[i];
    if (r == bh - 1 && t == 0) {
        dst[len] = 0xff, dst[len + 1] = 0xd9;
        lengths[f] = (long long)frame_len[f] + 2;
    }
}

struct MjLayout {
    size_t coef, raw, stuffed, interval_len, frame_len, total, out;
    int bh, bw, nb;
};

bool mj_layout(int n, int h, int w, int channels, MjLayout& L) {
    if (n < 1 || h < 1 || w < 1 || h > 65535 || w > 65535 || (channels != 1 && channels != 3)) return false;
    L.bh = (h + 7) / 8, L.bw = (w + 7) / 8, L.nb = L.bw * channels;
    const size_t intervals = (size_t)n * L.bh, blocks = intervals * L.nb;
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    L.coef = 0;
    L.raw = L.coef + blocks * 128;
    L.stuffed = L.raw + blocks * MJ_BLOCK_RAW_BYTES;
    L.interval_len = L.stuffed + blocks * MJ_BLOCK_OUT_BYTES;
    L.frame_len = L.interval_len + up16(intervals * 4);
    L.total = L.frame_len + up16((size_t)n * 4);
    L.out = (size_t)n * ((size_t)L.bh * ((size_t)L.nb * MJ_BLOCK_OUT_BYTES + 2) + 2);
    return true;
}

}  // namespace

extern "C" size_t vda_mjpeg_workspace_bytes(int n, int h, int w, int channels) {
    MjLayout L;
    return mj_layout(n, h, w, channels, L) ? L.total : 0;
}

extern "C" size_t vda_mjpeg_out_bytes(int n, int h, int w, int channels) {
    MjLayout L;
    return mj_layout(n, h, w, channels, L) ? L.out : 0;
}

extern "C" int vda_mjpeg_encode_u8(const uint8_t* frames, int n, int h, int w, int channels, const uint16_t* qtables, void* workspace,
                                   size_t workspace_bytes, uint8_t* out, size_t out_capacity, long long* lengths, vda_stream_t stream) {
    VDA_REQUIRE(frames, "vda_mjpeg_encode_u8: frames is null");
    VDA_REQUIRE(qtables, "vda_mjpeg_encode_u8: qtables is null");
    VDA_REQUIRE(workspace, "vda_mjpeg_encode_u8: workspace is null");
    VDA_REQUIRE(out, "vda_mjpeg_encode_u8: out is null");
    VDA_REQUIRE(lengths, "vda_mjpeg_encode_u8: lengths is null");
    VDA_REQUIRE(n >= 1 && h >= 1 && w >= 1, "vda_mjpeg_encode_u8: bad size n=%d h=%d w=%d (each at least 1)", n, h, w);
    VDA_REQUIRE(h <= 65535 && w <= 65535, "vda_mjpeg_encode_u8: bad size h=%d w=%d (a JPEG frame is at most 65535 x 65535)", h, w);
    VDA_REQUIRE(channels == 1 || channels == 3, "vda_mjpeg_encode_u8: bad channels=%d (1 gray or 3 RGB)", channels);
    MjTables tables = {};
    for (int i = 0; i < 64 * (channels == 3 ? 2 : 1); ++i) {
        VDA_REQUIRE(qtables[i] >= 1 && qtables[i] <= 255, "vda_mjpeg_encode_u8: bad qtables[%d]=%d (a baseline divisor is 1..255)", i, (int)qtables[i]);
        tables.q[i >> 6][i & 63] = qtables[i];
    }
    MjLayout L;
    mj_layout(n, h, w, channels, L);
    const int chunks = (L.bw + MJ_TILES - 1) / MJ_TILES;
    VDA_REQUIRE((long long)n * L.bh * chunks <= 0x7fffffffLL, "vda_mjpeg_encode_u8: bad size n=%d h=%d w=%d (more than 2^31 - 1 workgroups)", n, h, w);
    VDA_REQUIRE(L.out / n <= 0x7fffffffULL, "vda_mjpeg_encode_u8: bad size h=%d w=%d (a frame's bound of %zu bytes does not fit an int)", h, w, L.out / n);
    VDA_REQUIRE(((uintptr_t)workspace & 15) == 0, "vda_mjpeg_encode_u8: workspace is not 16-byte aligned");
    VDA_REQUIRE(((uintptr_t)lengths & 7) == 0, "vda_mjpeg_encode_u8: lengths is not 8-byte aligned");
    VDA_REQUIRE(workspace_bytes >= L.total, "vda_mjpeg_encode_u8: workspace capacity %zu is below the %zu bytes of vda_mjpeg_workspace_bytes", workspace_bytes,
                L.total);
    VDA_REQUIRE(out_capacity >= L.out, "vda_mjpeg_encode_u8: out capacity %zu is below the %zu bytes of vda_mjpeg_out_bytes", out_capacity, L.out);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    int16_t* coef = reinterpret_cast<int16_t*>(ws + L.coef);
    uint32_t* raw = reinterpret_cast<uint32_t*>(ws + L.raw);
    uint8_t* stuffed = ws + L.stuffed;
    int* interval_len = reinterpret_cast<int*>(ws + L.interval_len);
    int* frame_len = reinterpret_cast<int*>(ws + L.frame_len);
    const dim3 block(MJ_T);
    const unsigned intervals = (unsigned)(n * L.bh);
    if (channels == 3)
        hipLaunchKernelGGL(mjpeg_transform_kernel<3>, dim3(intervals * chunks), block, 0, (hipStream_t)stream, frames, h, w, tables, coef, frame_len, L.bh,
                           L.bw, chunks);
    else
        hipLaunchKernelGGL(mjpeg_transform_kernel<1>, dim3(intervals * chunks), block, 0, (hipStream_t)stream, frames, h, w, tables, coef, frame_len, L.bh,
                           L.bw, chunks);
    VDA_LAUNCH_CHECK();
    hipLaunchKernelGGL(mjpeg_entropy_kernel, dim3(intervals), block, 0, (hipStream_t)stream, coef, L.nb, channels, L.bh, raw, stuffed, interval_len,
                       frame_len);
    VDA_LAUNCH_CHECK();
    hipLaunchKernelGGL(mjpeg_pack_kernel, dim3(intervals), block, 0, (hipStream_t)stream, stuffed, L.nb, L.bh, interval_len, frame_len, out, lengths);
    VDA_LAUNCH_CHECK();
    return 0;
}
