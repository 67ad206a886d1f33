// Steps the large-tile fp16 GEMM / implicit-conv kernels share (gemm256_kernel.h, gemm256s_kernel.h, gemm8p_kernel.h), each written
// once: the persistent tile walk, the last-round stagger, the dense-A and W staging pieces, the conv (tap, channel slice) cursor,
// the ReLU threshold and the launchers' grid rule. What makes those three files three kernels - the K loop: when DMA, LDS reads,
// barriers and MFMAs are issued - is not here. Neither are the steps whose shared form moved a kernel's registers, scratch or
// waits (profiles/r14/gemm_refactor_ab.txt): the swizzled source chunk, the conv row decomposition and pointer gather, the
// 16x16x32 fragment reads and the row-layout epilogue stay written out in each kernel.
#pragma once
#include "gemm_epilogue.h"

namespace vda_gemm {

constexpr int BK = 64;                // K tile depth
constexpr int ROW_BYTES = BK * 2;     // one LDS row: 8 chunks of 16 B, chunk ^= (row >> 1) & 7

// ---- Tile walk. Persistent workgroups, each walks tiles round by round. In round r the workgroups of an XCD (equal bid % 8) take
// per_xcd CONSECUTIVE tiles (N fastest), so concurrently running tiles share A / W panels in that XCD's L2.
struct TileWalk {
    int nbn, nbm, ntiles, nwg, bid, per_xcd;
    int full_rounds, rem;             // whole rounds, and the tiles of the last, partial one
    bool deal_last;
    template <int BM, int BN>
    __device__ __forceinline__ void origin(int t, int& m0, int& n0) const {       // first row / column of tile t
        const int bm = t / nbn, bn = t - bm * nbn;
        m0 = bm * BM;
        n0 = bn * BN;
    }
    __device__ __forceinline__ int plain(int round) const { return round * nwg + (bid & 7) * per_xcd + (bid >> 3); }
    // The LAST, partial round is dealt to the XCDs in groups of nbn consecutive tiles (one row panel), round robin, so that every
    // XCD keeps the same share of busy CUs instead of whole XCDs going idle (needs nbn | per_xcd; otherwise the plain mapping
    // stays). A workgroup without a tile in that round has one tile time of slack: see stagger_last_round.
    __device__ __forceinline__ int dealt(int round) const {
        if (deal_last && round == full_rounds) {
            const int slot = bid >> 3, j = ((slot / nbn) * 8 + (bid & 7)) * nbn + slot % nbn;
            return j < rem ? round * nwg + j : ntiles;
        }
        return plain(round);
    }
};
template <int BM, int BN>
__device__ __forceinline__ TileWalk tile_walk(const vda_gemm_args& p) {
    TileWalk w;
    w.nbn = (p.N + BN - 1) / BN, w.nbm = (p.M + BM - 1) / BM;
    w.ntiles = w.nbm * w.nbn;
    w.nwg = gridDim.x, w.bid = blockIdx.x;
    w.per_xcd = w.nwg >> 3;                                          // launch guarantees nwg % 8 == 0
    w.full_rounds = w.ntiles / w.nwg, w.rem = w.ntiles - w.full_rounds * w.nwg;
    w.deal_last = w.rem > 0 && w.full_rounds > 0 && w.per_xcd % w.nbn == 0;
    return w;
}

// ---- Last-round stagger. Workgroups that sit out the last round (tile_of(full_rounds) past the end) can start up to 3/4 of a tile
// time late, in four phases, for free - the launch ends with the others' last tile - and take their epilogues out of phase.
// UNITS = 64-cycle sleep units per K tile of the calling kernel; VDA_FLAG_NO_STAGGER switches it off.
template <int UNITS, class TileOf>
__device__ __forceinline__ void stagger_last_round(const vda_gemm_args& p, const TileWalk& w, int nt, TileOf tile_of) {
    if (!VDA_OPT_FLAG(p.relu_in, VDA_FLAG_NO_STAGGER) && w.rem > 0 && w.full_rounds > 0 && tile_of(w.full_rounds) >= w.ntiles) {
        // phase by slot: the nbn workgroups of an XCD that share an A row panel land in DIFFERENT phases (keeping them in phase -
        // VDA_GEMM_STAGGER=2 - is slower than no stagger at all: it is those neighbours' epilogues that collide)
        const int q = VDA_OPT_FLAG(p.relu_in, VDA_FLAG_STAGGER_PANEL) ? ((w.bid >> 3) / (w.nbn <= 8 ? w.nbn : 8)) & 3 : (w.bid >> 3) & 3;
        const int units = (nt * UNITS + 260) * q / 4;
        for (int i = 0; i < units; i += 120) __builtin_amdgcn_s_sleep(120);
    }
}

// ---- Staging sources. A DMA piece is 8 rows x 128 B = 1 KiB; lane -> (row lrow = lane >> 3 of the piece, LDS chunk lane & 7); wave
// w stages pieces w, w + NW, ...; src_chk is the lane's swizzled source chunk, in halves (a lane constant, computed by the kernel).
// Dense / W offsets are recomputed per K tile from the tile origin (3 VALU ops per piece) instead of being kept in registers.
// Rows past the matrix re-read its last row (their results are never stored).
__device__ __forceinline__ void stage_a_piece(const vda_gemm_args& p, int tm0, int piece, int lrow, int src_chk, int k0, char* buf) {
    const int m = min(tm0 + piece * 8 + lrow, p.M - 1);
    glds16((const h16*)p.A + (size_t)(unsigned)(m * p.lda + src_chk + k0), buf + piece * 1024);
}
__device__ __forceinline__ void stage_w_piece(const vda_gemm_args& p, int tn0, int piece, int lrow, int src_chk, int k0, char* buf) {
    const int n = min(tn0 + piece * 8 + lrow, p.N - 1);
    glds16((const h16*)p.W + (size_t)(unsigned)(n * p.K + src_chk + k0), buf + piece * 1024);
}

// conv: (3x3 tap, 64-channel slice) of the K tile being staged. seek() at the tile seams (one integer division by the runtime
// channel count), next() inside the K loop: the division is a ~40-instruction dependent chain that would sit between the barrier
// and the DMA burst of every K tile.
struct TapCursor {
    int tap = 0, ci0 = 0;
    __device__ __forceinline__ void seek(const vda_gemm_args& p, int kt) {
        const int k0 = kt * BK;
        tap = k0 / p.cCin;
        ci0 = k0 - tap * p.cCin;
    }
    __device__ __forceinline__ bool next_slice(const vda_gemm_args& p) {     // true: the tap's last slice is behind, move the tap
        ci0 += BK;
        if (ci0 < p.cCin) return false;
        ci0 = 0;
        return true;
    }
    __device__ __forceinline__ void next(const vda_gemm_args& p) {
        if (next_slice(p)) ++tap;
    }
    __device__ __forceinline__ int ky() const { return (tap * 11) >> 5; }    // tap / 3 for tap = 0..8
};

// relu on the activation operand (conv only), branch-free: max(x, 0) or max(x, -inf)
__device__ __forceinline__ h16x8 relu_threshold(const vda_gemm_args& p) {
    const h16 relu_floor = (p.relu_in & VDA_OPT_RELU_IN) ? (h16)0.f : (h16)(-65504.f);
    h16x8 thr;
#pragma unroll
    for (int e = 0; e < 8; ++e) thr[e] = relu_floor;
    return thr;
}

// ---- Launch: one persistent workgroup per slot (CUs x workgroups per CU), or one per tile rounded up to the eight XCDs
template <int BM, int BN>
inline int tile_count(const vda_gemm_args& a) {
    return ((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN);
}
inline int persistent_grid(int ntiles, int slots) { return ntiles < slots ? (ntiles + 7) / 8 * 8 : slots; }

}  // namespace vda_gemm
