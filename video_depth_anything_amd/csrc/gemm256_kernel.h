// Large-tile fp16 MFMA GEMM / implicit-GEMM conv for gfx950 on v_mfma_f32_32x32x16_f16: 256 x BN x 64 tiles, 8 waves, one
// workgroup per CU, one barrier per K tile. An A/B family: the planner never picks it by default (gemm256s_kernel.h is the same
// tile on 16x16x32 MFMA, gemm8p_kernel.h its 8-phase schedule). Tile walk, staging pieces and grid rule: gemm_tile.h.
//
// Why this shape: with a 128x128 tile every 32 MFMAs per wave need 32 KB staged from L2 into LDS; at MFMA
// peak that is more than the L2 can deliver, so the small tile is staging-bound. 256x256 halves the staged
// bytes per FLOP (64 KB per 64 MFMAs per wave) and the 128x64 wave tile cuts LDS fragment reads to
// 0.75 ds_read_b128 per v_mfma_f32_32x32x16_f16.
//
// Pipeline (one __syncthreads per 64-deep K tile):
//   LDS holds two K tiles (2 x 64 KB at BN=256). Fragments are register double-buffered at 16-deep k-step
//   granularity: while the 8 MFMAs of step t issue, the 6 ds_read_b128 of step t+1 are in flight. The last
//   step of tile k waits for tile k+1 (issued one whole tile earlier), barriers once, issues the 8
//   global_load_lds of tile k+2 into the buffer tile k just vacated, and prefetches tile k+1's first
//   fragments while its own MFMAs run, so the barrier never exposes an LDS or HBM round trip.
//
// LDS image: [rows][8 x 16 B], chunk ^= (row >> 1) & 7 (conflict-free for the 32-row ds_read_b128 fragment),
// applied on the DMA SOURCE address and on the read address. MFMA operands are swapped (W rows as "A",
// activation rows as "B") so a lane's accumulator registers are runs of 4 consecutive output columns.
#pragma once
#include "gemm_tile.h"

namespace vda_gemm256 {

using namespace vda_gemm;
constexpr int BM = 256;
constexpr int NW = 8;                 // waves
constexpr int NT = NW * 64;

template <int BN, int AMODE, int EPI>
__global__ void __launch_bounds__(NT) gemm256_kernel(const vda_gemm_args p) {
    constexpr int WN = BN == 256 ? 4 : 2;          // waves along N
    constexpr int WM = NW / WN;                    // waves along M
    constexpr int WTM = BM / WM, WTN = BN / WN;    // wave tile: 128x64 (BN=256) or 64x64 (BN=128)
    constexpr int MI = WTM / 32, NJ = WTN / 32;    // 32x32 subtiles per wave
    constexpr int AJ = BM / 8 / NW, WJ = BN / 8 / NW;   // 1-KiB DMA pieces per wave
    constexpr int A_BYTES = BM * ROW_BYTES, W_BYTES = BN * ROW_BYTES, STAGE = A_BYTES + W_BYTES;

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;

    // Persistent workgroups, one per CU (gemm_tile.h): the plain XCD mapping in every round
    const TileWalk walk = tile_walk<BM, BN>(p);
    auto tile_of = [&](int round) { return walk.plain(round); };
    const int ntiles = walk.ntiles;

    // ---- per-lane DMA sources (the pieces: gemm_tile.h). Only the conv row decomposition (two divisions per piece) is cached per tile.
    const int lrow = lane >> 3;
    const int src_chk = ((lane & 7) ^ ((((wave & 1) << 2) + (lrow >> 1)) & 7)) * 8;     // halves
    int a_pix[AJ], a_yx[AJ];          // conv: b*H*W, and (oy*stride-1) | (ox*stride-1) << 16
    int tm0 = 0, tn0 = 0;             // origin of the tile being staged
    auto set_sources = [&](int t) {
        walk.origin<BM, BN>(t, tm0, tn0);
        if constexpr (AMODE == VDA_A_CONV3X3) {
#pragma unroll
            for (int j = 0; j < AJ; ++j) {
                int m = tm0 + (wave + NW * j) * 8 + lrow;
                const bool ok = m < p.M;
                m = min(m, p.M - 1);
                const int hw = p.cHo * p.cWo;
                const int b = m / hw, rem = m - b * hw;
                const int oy = rem / p.cWo, ox = rem - oy * p.cWo;
                a_pix[j] = b * p.cH * p.cW;
                const int iy0 = ok ? oy * p.cStride - 1 : -20000, ix0 = ox * p.cStride - 1;
                a_yx[j] = (iy0 & 0xffff) | (ix0 << 16);
            }
        }
    };

    auto stage = [&](int kt, char* buf) {
        const int k0 = kt * BK;
        if constexpr (AMODE == VDA_A_DENSE) {
#pragma unroll
            for (int j = 0; j < AJ; ++j) stage_a_piece(p, tm0, wave + NW * j, lrow, src_chk, k0, buf);
        } else {
            const int tap = k0 / p.cCin, ci0 = k0 - tap * p.cCin;
            const int ky = tap / 3, kx = tap - ky * 3;
#pragma unroll
            for (int j = 0; j < AJ; ++j) {
                const int iy = (int)(short)(a_yx[j] & 0xffff) + ky, ix = (a_yx[j] >> 16) + kx;
                const bool ok = (unsigned)iy < (unsigned)p.cH && (unsigned)ix < (unsigned)p.cW;
                const h16* src = ok ? (const h16*)p.A + ((size_t)(a_pix[j] + iy * p.cW + ix) * p.cCin + ci0 + src_chk)
                                    : (const h16*)p.zero_page + src_chk;
                glds16(src, buf + (wave + NW * j) * 1024);
            }
        }
#pragma unroll
        for (int j = 0; j < WJ; ++j) stage_w_piece(p, tn0, wave + NW * j, lrow, src_chk, k0, buf + A_BYTES);
    };

    // fragment addressing: row = lane & 31 inside a 32-row subtile, k-chunk = 2*step + (lane >> 5)
    const int frow = lane & 31, fh = lane >> 5, fsw = (lane >> 1) & 7;     // ((row >> 1) & 7) with row = subtile*32 + frow
    const int a_off = (wm * WTM + frow) * ROW_BYTES, w_off = A_BYTES + (wn * WTN + frow) * ROW_BYTES;
    const h16x8 relu_thr = relu_threshold(p);

    struct Frags {
        h16x8 a[MI];
        h16x8 w[NJ];
    };
    auto read_frags = [&](const char* buf, int step, Frags& f) {
        const int coff = ((2 * step + fh) ^ fsw) << 4;
#pragma unroll
        for (int i = 0; i < MI; ++i) f.a[i] = *reinterpret_cast<const h16x8*>(buf + a_off + i * 32 * ROW_BYTES + coff);
#pragma unroll
        for (int j = 0; j < NJ; ++j) f.w[j] = *reinterpret_cast<const h16x8*>(buf + w_off + j * 32 * ROW_BYTES + coff);
    };

    const int nt = p.K / BK;
    static_assert(WTN == 64, "epilogue staging assumes a 64-column wave tile");
    // epilogue staging (8 waves x 8 KiB): inside pipeline buffer 1 when that is 64 KiB (BN=256), else after the buffers
    constexpr int STG_OFF = (STAGE >= 8 * 8192) ? STAGE : 2 * STAGE;
    char* stg = smem + STG_OFF + wave * 8192;
    const int wr_row = lane & 31, wr_h = lane >> 5;

    int tile = tile_of(0);
    if (tile >= ntiles) return;                        // uniform per workgroup
    set_sources(tile);
    stage(0, smem);
    for (int round = 0; tile < ntiles; ++round) {
        int m0, n0;
        walk.origin<BM, BN>(tile, m0, n0);

        f32x16 acc[MI][NJ];
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
        auto mma = [&](Frags& f) {
            if constexpr (AMODE == VDA_A_CONV3X3) {
#pragma unroll
                for (int i = 0; i < MI; ++i) f.a[i] = __builtin_elementwise_max(f.a[i], relu_thr);
            }
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.w[j], f.a[i], acc[i][j], 0, 0, 0);
        };

        // K tile 0 of this tile was issued before the previous tile's epilogue (or above, for the first tile).
        Frags f0, f1;
        if (round > 0) set_sources(tile);       // recomputed rather than kept live across the epilogue
        // Full barrier (with its fences, so no LDS read can be scheduled above it): K tile 0 has landed everywhere.
        // K tile 1 is issued after it and has the whole of K tile 0's MFMA work to land, as in the steady state.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (nt > 1) stage(1, smem + STAGE);
        read_frags(smem, 0, f0);
        for (int kt = 0; kt < nt; ++kt) {
            char* cb = smem + (kt & 1) * STAGE;
            char* nb = smem + ((kt + 1) & 1) * STAGE;
            read_frags(cb, 1, f1);
            mma(f0);
            read_frags(cb, 2, f0);
            mma(f1);
            read_frags(cb, 3, f1);
            mma(f0);
            // Tile kt+1 must have landed everywhere and every wave must be done READING tile kt (its last
            // fragments, step 3, are already in f1 once lgkmcnt drains): one full barrier per K tile.
            // The vmcnt wait is explicit: hipcc does NOT reliably drain LDS-DMA before __syncthreads() (one
            // instantiation of this very loop was emitted with lgkmcnt(0) only, and raced).
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (kt + 2 < nt) stage(kt + 2, cb);
            if (kt + 1 < nt) read_frags(nb, 0, f0);
            mma(f1);
        }
        // After the loop's last barrier nobody reads the pipeline buffers any more: start the NEXT tile's first
        // K tile now, so its HBM/L2 latency is covered by this tile's epilogue.
        const int next = tile_of(round + 1);
        if (next < ntiles) {
            set_sources(next);
            stage(0, smem);
        }

        // ---- epilogue. Accumulator register e of subtile (i,j) is row m = lane & 31, column 8*(e>>2) + 4*(lane>>5) + (e&3):
        // stored straight from this layout a wave instruction would touch 32 rows x 16 B (32 partial lines). Instead each
        // wave transposes one 32-row x 64-column fp32 block at a time through its own 8 KiB of (idle) pipeline buffer 1
        // (16-byte chunks XOR-swizzled by row: conflict-free both ways) and then owns whole row segments: bias / LayerScale /
        // residual reads and the output stores become contiguous 16-byte accesses covering full 128-byte lines.
        const int bm0 = m0 + wm * WTM, bn0 = n0 + wn * WTN;
        const bool interior = bm0 + WTM <= p.M && bn0 + WTN <= p.N;       // wave-uniform
        {
            using RT = vda_gemm::RowTraits<EPI>;
            constexpr int NC = RT::NC, RR = RT::f32_out ? 8 : 4;            // columns per lane, row groups per 32-row block
            // lane -> (row inside a group, column block): fp32 out: 4 rows x 16 lanes x 4 cols; fp16 out: 8 rows x 8 lanes x 8 cols
            const int lrow_e = RT::f32_out ? (lane >> 4) : (lane >> 3);
            const int c0 = RT::f32_out ? (lane & 15) : 2 * (lane & 7);      // first 16-byte (4-column) chunk of the lane
            const int en = bn0 + c0 * 4;
            const bool geglu_idle = (EPI == VDA_EPI_GEGLU_F16) && (c0 & 7) >= 4;   // gate lanes only feed their value lanes
            vda_gemm::ColConst<NC> cc;
            vda_gemm::load_col_const<EPI, NC>(p, en, cc);
            constexpr int RG = RT::f32_out ? 4 : 2;                          // rows per row group
            vda_gemm::RowAux carry[RG];                                      // the next block's first group, loaded a group early
#pragma unroll
            for (int i = 0; i < MI; ++i) {
#pragma unroll
                for (int j = 0; j < NJ; ++j)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int c = j * 8 + 2 * g + wr_h;                       // 16-byte chunk = 4 columns
                        const f32x4 v = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
                        *reinterpret_cast<f32x4*>(stg + wr_row * 256 + ((c ^ (wr_row & 15)) << 4)) = v;
                    }
                // The transposition is a cross-LANE exchange inside one wave: the hardware runs a wave's LDS ops in order,
                // but the compiler must not reorder the reads below across the writes above (it only reasons per thread).
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                // Row groups are processed RG at a time: phase 1 issues every row-dependent global load of the group,
                // phase 2 reads the transposed accumulators back, finishes and stores.
                // Row-dependent loads (residuals, pos-embed) run ONE ROW GROUP AHEAD of the stores: vmcnt retires in order and
                // counts stores, so a load issued after a group's stores cannot complete before them - issued before, it can.
                auto row_groups = [&](auto guard) {
                    constexpr bool GUARD = decltype(guard)::value;
                    constexpr int NG = RR / RG;                                  // row groups per 32-row block
                    auto load_group = [&](int blk, int r0, vda_gemm::RowAux (&ax)[RG]) {
                        if (!geglu_idle) {
#pragma unroll
                            for (int q = 0; q < RG; ++q)
                                vda_gemm::load_row_aux<EPI, GUARD>(p, bm0 + blk * 32 + (r0 + q) * (32 / RR) + lrow_e, en, ax[q]);
                        }
                    };
                    vda_gemm::RowAux aux[2][RG];
                    if (i == 0) load_group(0, 0, aux[0]);
                    else {
#pragma unroll
                        for (int q = 0; q < RG; ++q) aux[0][q] = carry[q];
                    }
#pragma unroll
                    for (int g = 0; g < NG; ++g) {
                        const int r0 = g * RG;
                        if (g + 1 < NG) load_group(i, r0 + RG, aux[(g + 1) & 1]);
                        else if (i + 1 < MI) load_group(i + 1, 0, carry);        // first group of the next block
#pragma unroll
                        for (int q = 0; q < RG; ++q) {
                            const int row = (r0 + q) * (32 / RR) + lrow_e;
                            const char* rp = stg + row * 256;
                            const f32x4 a = *reinterpret_cast<const f32x4*>(rp + ((c0 ^ (row & 15)) << 4));
                            if constexpr (RT::f32_out) {
                                vda_gemm::finish_row4<EPI, GUARD>(p, bm0 + i * 32 + row, en, a, cc, aux[g & 1][q]);
                            } else {
                                const f32x4 b = *reinterpret_cast<const f32x4*>(rp + (((c0 + 1) ^ (row & 15)) << 4));
                                float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
                                float gt[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                                if constexpr (EPI == VDA_EPI_GEGLU_F16) {
                                    const f32x4 ga = *reinterpret_cast<const f32x4*>(rp + (((c0 + 4) & 15) ^ (row & 15)) * 16);
                                    const f32x4 gb = *reinterpret_cast<const f32x4*>(rp + (((c0 + 5) & 15) ^ (row & 15)) * 16);
#pragma unroll
                                    for (int e = 0; e < 4; ++e) {
                                        gt[e] = ga[e];
                                        gt[4 + e] = gb[e];
                                    }
                                }
                                if (!geglu_idle) vda_gemm::finish_row8<EPI, GUARD>(p, bm0 + i * 32 + row, en, v, gt, cc, aux[g & 1][q]);
                                if constexpr (EPI == VDA_EPI_SCALE_RES_SPLIT) {      // all 8 lanes of the row store the same pair: no divergence
                                    if (!GUARD || (bm0 + i * 32 + row < p.M && en < p.N)) vda_gemm::store_split_stats(p, bm0 + i * 32 + row, en, aux[g & 1][q]);
                                }
                            }
                        }
                    }
                };
                // interior wave tiles (all but the matrix's last row / column of tiles) take the branch-free form
                if (interior) row_groups(std::false_type{});
                else row_groups(std::true_type{});
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // reads of this block done before the next block's writes
            }
        }
        // Every wave is done with its staging slice before the next tile's stage(1) overwrites buffer 1.
        __syncthreads();
        tile = next;
    }
}

template <int BN, int AMODE, int EPI>
int launch256(const vda_gemm_args& a, hipStream_t s) {
    constexpr int stage_bytes = (BM + BN) * ROW_BYTES;
    constexpr int smem = stage_bytes >= 8 * 8192 ? 2 * stage_bytes : 2 * stage_bytes + 8 * 8192;
    static_assert(smem <= 160 * 1024, "LDS budget");
    static VdaKernelDeviceState dev_state;
    const int num_cu = vda_prepare_kernel(reinterpret_cast<const void*>(&gemm256_kernel<BN, AMODE, EPI>), smem, dev_state);
    if (num_cu < 0) return 2;
    const int grid = persistent_grid(tile_count<BM, BN>(a), num_cu);     // one persistent workgroup per CU
    hipLaunchKernelGGL((gemm256_kernel<BN, AMODE, EPI>), dim3(grid), dim3(NT), smem, s, a);
    VDA_LAUNCH_CHECK();
    return 0;
}

// One case per epilogue of the family's list (gemm_epilogue.h: the lists the planner plans with); -1 = not built, which the planner
// never asks for. Dense A: every epilogue but the LayerNorm-fold ones. Conv A: the three the head uses.
#define VDA_256_CASE(E, AMODE) case E: return launch256<BN, AMODE, E>(a, s);
template <int BN>
int launch_dense(const vda_gemm_args& a, hipStream_t s) {
    switch (a.epilogue) { VDA_EPIS_DENSE_MFMA32(VDA_256_CASE, VDA_A_DENSE) default: return -1; }
}
template <int BN>
int launch_conv(const vda_gemm_args& a, hipStream_t s) {
    switch (a.epilogue) { VDA_EPIS_CONV(VDA_256_CASE, VDA_A_CONV3X3) default: return -1; }
}
#undef VDA_256_CASE

}  // namespace vda_gemm256
