// The patch-in-LDS direct 3x3 convolutions (conv_lds.hip, tail.hip, conv_up.hip): the steps they share, written once.
//
// All of them keep the pixel patch a tile of outputs needs (tile + 1-pixel halo) in LDS beside the weights and form the nine taps from
// it with v_mfma_f32_32x32x16_f16: A = weights [32 cout][16 k], B = patch [16 k][32 pixels], D[cout][pixel]. A wave owns 2 output
// rows; patch row R serves (output row R, ky = 0), (R - 1, ky = 1), (R - 2, ky = 2), so per (kx, k-step) a wave reads 4 patch-row
// fragments P and 3 weight fragments per 32-cout block for 6 MFMAs: tap_group(). Every kernel of the family accumulates through that
// one function, k-steps ascending, kx inside a 32-channel pass, ky inside tap_group: "the same accumulation order" - what makes
// c64 == per-pass and tail v2 == v1 bit for bit - is a property of this file.
//
// LDS rows and banks, once: a ds_read_b128 is served 16 lanes at a time against one 256-byte bank row = sixteen 16-byte slots. The 16
// lanes read the same chunk index of 16 consecutive rows (pixels or couts), so with rows of 64 / 128 / 32 bytes rows 4 / 2 / 8 apart
// would hit the same slot; XOR-ing the chunk with (i >> 2) & 3 / (i >> 1) & 7 / (i >> 3) & 1 spreads them over all sixteen. i is the
// row index (swz below, conv_up's lds_off) or, in the persistent kernels, the pixel's COLUMN in the patch (tail's swzc, c64's swz64,
// conv_up's patch_off): equally conflict-free, and a reading lane's swizzle then depends on pixel + kx only, so fragment addresses
// are a few lane constants + immediates.
#pragma once
#include "vda_common.h"

namespace vda_patch {

// ---- geometry
namespace tile8 {                              // 8 x 32 outputs, 32-channel passes in 64-byte rows (conv_lds.hip, tail.hip v1)
constexpr int TH = 8, TW = 32;                 // output tile
constexpr int PH = TH + 2, PW = TW + 2;        // patch with halo
constexpr int NPIX = PH * PW;                  // 340
constexpr int NP_PATCH = (NPIX + 15) / 16;     // 1-KiB DMA pieces (16 rows x 64 B)
constexpr int PATCH_BYTES = NP_PATCH * 1024;
}  // namespace tile8
namespace tile16 {                             // 16 x 32 outputs under an upsample (tail.hip v2, conv_up.hip)
constexpr int TH = 16, TW = 32;
constexpr int PW = TW + 2;                     // patch with halo: 18 x 34
constexpr int NPIX = (TH + 2) * PW;            // 612
}  // namespace tile16
constexpr int CC = 32;                         // channels per pass
constexpr int ROWB = CC * 2;                   // 64-byte LDS rows
__device__ __forceinline__ int swz(int r) { return (r >> 2) & 3; }

// ---- tile walk
// workgroups are dealt to the 8 XCDs round-robin: give XCD x the contiguous tile range [x * per_xcd, (x+1) * per_xcd), so that the
// workgroups of one XCD take neighbouring tiles (shared halo / source pixels in that XCD's L2)
__device__ __forceinline__ int xcd_tile() {
    const int per_xcd = gridDim.x >> 3;
    return (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
}
// persistent form: XCD x owns tiles [tb, te), dealt to its workgroups tile by tile; this one takes tb + slot, + per_xcd, ...: nmy tiles
// (none if tb + slot >= te)
struct TileShare {
    int tb, te, nmy, per_xcd, slot;
};
__device__ __forceinline__ TileShare xcd_share(int ntiles) {
    TileShare s;
    const int xcd = blockIdx.x & 7;
    s.per_xcd = gridDim.x >> 3;
    s.slot = blockIdx.x >> 3;
    s.tb = (int)((long long)ntiles * xcd / 8);
    s.te = (int)((long long)ntiles * (xcd + 1) / 8);
    s.nmy = (s.te - s.tb - s.slot + s.per_xcd - 1) / s.per_xcd;
    return s;
}
struct TilePos {
    int b, ty, tx, y0, x0;
};
template <int TH_, int TW_>
__device__ __forceinline__ TilePos tile_pos(int tile, int tiles_x, int tiles_y) {
    TilePos p;
    const int tyb = tile / tiles_x;
    p.tx = tile % tiles_x;
    p.ty = tyb % tiles_y;
    p.b = tyb / tiles_y;
    p.y0 = p.ty * TH_;
    p.x0 = p.tx * TW_;
    return p;
}
// workgroup barrier of the persistent kernels: this wave's LDS traffic done, and nothing scheduled across it
__device__ __forceinline__ void wg_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::: "memory");
}

// ---- the tap group: the 6 * CB MFMAs of one (kx, k-step)
template <int CB>
__device__ __forceinline__ void tap_group(const h16x8 (&P)[4], const h16x8 (&Wf)[CB][3], f32x16 (&acc)[2][CB]) {
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int r = 0; r < 2; ++r) acc[r][cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Wf[cb][ky], P[r + ky], acc[r][cb], 0, 0, 0);
}
template <int CB>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[2][CB]) {
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[r][cb][e] = 0.f;
}

// ---- per-pass steps of the 8 x 32 kernels (4 waves; one pass = 32 input channels)
// weights: rows R = tap * (32 * CB) + cout, 32 channels each (rows of couts >= N read row N - 1: never stored)
template <int CB>
__device__ __forceinline__ void stage_weights(const h16* __restrict__ wt, char* wl, int wave, int lane, int C, int N, int c0) {
    constexpr int NP_W = 9 * 32 * CB / 16;     // 1-KiB pieces
    const int lr = lane >> 2, lp = lane & 3;
    for (int piece = wave; piece < NP_W; piece += 4) {
        const int R = piece * 16 + lr;
        const int tap = R / (32 * CB), co = min(R - tap * (32 * CB), N - 1);
        glds16(wt + co * (9 * C) + tap * C + c0 + ((lp ^ swz(R)) << 3), wl + piece * 1024);
    }
}
// patch (zero page outside the image = the conv's padding)
__device__ __forceinline__ void stage_patch(const h16* __restrict__ in, const h16* __restrict__ zero_page, char* patch, int wave, int lane, int b,
                                            int y0, int x0, int H, int W, int C, int c0) {
    using namespace tile8;
    const int lr = lane >> 2, lp = lane & 3;
    for (int piece = wave; piece < NP_PATCH; piece += 4) {
        const int q = piece * 16 + lr;
        const int py = q / PW, pxx = q - py * PW;
        const int iy = y0 - 1 + py, ix = x0 - 1 + pxx;
        const bool ok = q < NPIX && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
        const int sc = (lp ^ swz(q)) << 3;
        const h16* src = ok ? in + ((b * H + iy) * W + ix) * C + c0 + sc : zero_page + sc;
        glds16(src, patch + piece * 1024);
    }
}
// 3 kx x 2 k-steps: D[cout][pixel] += W[cout][(ky, kx), c0 + 16 ks ..] . patch[row + ky][pixel + kx][..]; RELU: max(patch, relu_thr) first
template <int CB, bool RELU>
__device__ __forceinline__ void mfma_pass(const char* patch, const char* wl, int wave, int px, int hh, h16x8 relu_thr, f32x16 (&acc)[2][CB]) {
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            h16x8 P[4], Wf[CB][3];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int q = (wave * 2 + j) * tile8::PW + px + kx;
                P[j] = *reinterpret_cast<const h16x8*>(patch + q * ROWB + (((2 * ks + hh) ^ swz(q)) << 4));
                if constexpr (RELU) P[j] = __builtin_elementwise_max(P[j], relu_thr);
            }
#pragma unroll
            for (int cb = 0; cb < CB; ++cb)
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
                    const int R = (ky * 3 + kx) * (32 * CB) + cb * 32 + px;      // A operand: row = cout (lane & 31)
                    Wf[cb][ky] = *reinterpret_cast<const h16x8*>(wl + R * ROWB + (((2 * ks + hh) ^ swz(R)) << 4));
                }
            tap_group<CB>(P, Wf, acc);
        }
    }
}

// ---- epilogues. Accumulator layout: lane = pixel (lane & 31) of row r, hh = lane >> 5; registers 4g..4g+3 of block cb = channels
// n = cb*32 + 8g + 4hh .. +3
__device__ __forceinline__ f32x4 acc4(const f32x16& a, int g) { return f32x4{a[4 * g], a[4 * g + 1], a[4 * g + 2], a[4 * g + 3]}; }
__device__ __forceinline__ void add4(f32x4& v, h16x4 a) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] += (float)a[e];
}
__device__ __forceinline__ h16x4 round4(f32x4 v, int relu_out) {
    if (relu_out) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
    }
    return h16x4{(h16)v[0], (h16)v[1], (h16)v[2], (h16)v[3]};
}
// fp16 narrow: + bias, + up to two residuals, ReLU, one 8-byte store of channels n .. n+3 of the pixel at element offset row
__device__ __forceinline__ void store_narrow(f32x4 v, const float* bias, const h16* res, const h16* res2, int relu_out, h16* out, size_t row, int n) {
    if (bias) v += *reinterpret_cast<const f32x4*>(bias + n);
    if (res) add4(v, *reinterpret_cast<const h16x4*>(res + row + n));
    if (res2) add4(v, *reinterpret_cast<const h16x4*>(res2 + row + n));
    *reinterpret_cast<h16x4*>(out + row + n) = round4(v, relu_out);
}
// fp16 wide (N, ldc multiples of 8, 16-byte aligned tensors): the two lanes of a pixel hold the interleaved 4-channel groups 8g + 4hh of
// a 32-channel block as packed pairs pk[g]; one v_permlane32_swap per register (upper lanes' groups 0, 1 <-> lower lanes' groups 2, 3:
// its own inverse) hands the lower lane channels 0..15 of the block and the upper lane 16..31, so each lane moves 2 x 16 bytes, not 4 x 8
__device__ __forceinline__ void pack4(unsigned (&pk)[2], h16x4 o) {
    pk[0] = reinterpret_cast<const unsigned*>(&o)[0];
    pk[1] = reinterpret_cast<const unsigned*>(&o)[1];
}
__device__ __forceinline__ void swap_halves(unsigned (&pk)[4][2]) {
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const auto sw = __builtin_amdgcn_permlane32_swap(pk[g][e], pk[g + 2][e], false, false);
            pk[g][e] = sw[0];
            pk[g + 2][e] = sw[1];
        }
}
__device__ __forceinline__ void store_wide(unsigned (&pk)[4][2], h16* out, size_t row, int cb, int hh, bool inb, int N) {
    swap_halves(pk);
#pragma unroll
    for (int j = 0; j < 2; ++j) {                   // lower lane: channels 8j..8j+7 of the block, upper lane: 16 + 8j ..
        const int n = cb * 32 + 16 * hh + 8 * j;
        if (inb && n < N) {
            const uint4 o = {pk[j][0], pk[j][1], pk[j + 2][0], pk[j + 2][1]};
            *reinterpret_cast<uint4*>(out + row + n) = o;
        }
    }
}
// ---- upsampled patches (align_corners=True): the source region under the patch of the tile at (y0, x0) is staged in LDS, SH x SW pixels
// from (sy0, sx0); a patch pixel's four corners are LDS offsets into it, two 16-bit halves per word: ia = (ya, xa) | (ya, xb) << 16,
// ib = the same in row yb. For pixels outside the image each caller substitutes its zero chunk (four reads of it = the conv's padding) in
// its own words, and those words are part of its arithmetic: whether hipcc branches or selects there decides whether the source
// coordinate's multiply and the subtraction that forms the fractional offset share a block and fuse (-ffp-contract=fast: the backend
// fuses whatever the pragmas say) - the offset's last bit. tail.hip chooses with a conditional expression around the call (a branch: not
// fused, as in its v1), conv_up.hip overrides afterwards (a select: fused).
__device__ __forceinline__ void src_origin(float ys, float xs, int y0, int x0, int h, int w, int& sy0, int& sx0) {
    sy0 = min((int)(ys * (float)max(y0 - 1, 0)), h - 1);
    sx0 = min((int)(xs * (float)max(x0 - 1, 0)), w - 1);
}
struct Corners {
    unsigned ia, ib;
};
template <class Off>                           // off(row of the region) = LDS byte offset of this lane's chunk in that row
__device__ __forceinline__ Corners corner_offsets(int ya, int yb, int xa, int xb, int sy0, int sx0, int SH, int SW, Off off) {
    const int fa = min(max(ya - sy0, 0), SH - 1), fb = min(max(yb - sy0, 0), SH - 1);
    const int ga = min(max(xa - sx0, 0), SW - 1), gb = min(max(xb - sx0, 0), SW - 1);
    return Corners{off(fa * SW + ga) | (off(fa * SW + gb) << 16), off(fb * SW + ga) | (off(fb * SW + gb) << 16)};
}

// ---- host side
inline long long tile_count(int B, int H, int W, int th, int tw, int& tiles_x, int& tiles_y) {
    tiles_x = (W + tw - 1) / tw;
    tiles_y = (H + th - 1) / th;
    return (long long)tiles_x * tiles_y * B;
}
inline unsigned grid8(long long ntiles) { return (unsigned)((ntiles + 7) / 8 * 8); }      // xcd_tile / xcd_share need a multiple of 8
inline int persistent_grid(long long ntiles, int ncu) { return ntiles < ncu ? (int)grid8(ntiles) : ncu; }      // one workgroup per CU

}  // namespace vda_patch
