// fp16 MFMA GEMM / implicit-GEMM conv for gfx950 (MI355X).
//
//   out = epilogue( A[M,K] * W[N,K]^T )          fp16 operands, fp32 accumulate
//
// Both operands are K-contiguous, which is exactly the v_mfma_f32_16x16x32_f16 fragment
// shape (8 consecutive k per lane), so tiles go HBM -> LDS with 16-byte
// global_load_lds (no VGPR round trip) and LDS -> VGPR with ds_read_b128.
//
// Tile: BM x BN x 64, 4 waves (2 x 2), each wave (BM/2) x (BN/2) as 16x16 MFMA subtiles.
// LDS image per operand tile: [rows][8 chunks of 16 B] with chunk ^= (row & 7). The DMA
// writes LDS linearly (wave-uniform base + lane*16), so the swizzle is applied to the
// per-lane SOURCE address and again on the ds_read address (same involution both sides).
// The MFMA is issued with W as the "A" operand and the activation tile as "B", so a lane's
// 4 accumulator registers are 4 CONSECUTIVE output columns of one row: bias / LayerScale /
// residual are read and the result stored as one 8- or 16-byte access per subtile.
//
// A-operand generators: dense rows, or the 3x3/pad-1 window of an NHWC tensor
// (K ordered (ky,kx,ci); a 64-wide K step never straddles a tap because Cin % 64 == 0).
// Rows past M / N are clamped on load and dropped on store.
#include "gemm_epilogue.h"

namespace {
using vda_gemm::store_one;

constexpr int BK = 64;                 // halves per K step
constexpr int ROW_BYTES = BK * 2;      // 128 B per tile row
constexpr int NWAVES = 4;
constexpr int NTHREADS = NWAVES * 64;

// FOLD (VDA_EPI_CONVT_FOLD_F16, vda.h; conv A): the K loop visits only the taps the tile's output phases reach, and the epilogue is
// that one. A kernel of its own (gemm_fold_kernel), so that the other kernels' code and names do not change.
// RELU (conv A): the input ReLU is compiled in, a packed max per A fragment whose threshold p.relu_in sets (0, or -65504 = identity).
// Without it (gemm_plain_kernel: what a conv without an input ReLU runs) the K loop has no max.
template <int BM, int BN, int AMODE, bool FOLD, bool RELU>
__device__ __forceinline__ void gemm_tile(const vda_gemm_args& p) {
    static_assert(!FOLD || AMODE == VDA_A_CONV3X3, "the folded mode is a conv A mode");
    static_assert(RELU || AMODE == VDA_A_CONV3X3, "the form without the max is a conv A form");
    constexpr int WTM = BM / 2, WTN = BN / 2;     // wave tile
    constexpr int MI = WTM / 16, NI = WTN / 16;   // 16x16 subtiles per wave
    constexpr int AJ = BM / 8 / NWAVES;           // 1-KiB DMA pieces per wave, A tile
    constexpr int WJ = BN / 8 / NWAVES;
    constexpr int A_BYTES = BM * ROW_BYTES, W_BYTES = BN * ROW_BYTES, STAGE = A_BYTES + W_BYTES;

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;

    // ---- block -> tile, XCD-aware: blocks that share an XCD (bid % 8) get a contiguous run of
    // tiles with the N index fastest, so an A row panel stays in that XCD's L2 across its N tiles.
    const int nbn = (p.N + BN - 1) / BN;
    const int nwg = gridDim.x;
    const int bid = blockIdx.x;
    const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    const int t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    const int bm = t / nbn, bn = t - bm * nbn;
    const int m0 = bm * BM, n0 = bn * BN;

    // ---- per-lane DMA sources
    const int lrow = lane >> 3;                   // row inside an 8-row piece
    const int lchk = ((lane & 7) ^ lrow) * 8;     // swizzled source chunk, in halves
    const h16* a_src[AJ];
    int a_pix[AJ], a_iy0[AJ], a_ix0[AJ];
    const h16* w_src[WJ];
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
        int m = m0 + (wave + NWAVES * j) * 8 + lrow;
        if constexpr (AMODE == VDA_A_DENSE) {
            m = min(m, p.M - 1);
            a_src[j] = (const h16*)p.A + (size_t)m * p.lda + lchk;
        } else {
            const bool ok = m < p.M;
            m = min(m, p.M - 1);
            const int hw = p.cHo * p.cWo;
            const int b = m / hw, rem = m - b * hw;
            const int oy = rem / p.cWo, ox = rem - oy * p.cWo;
            a_pix[j] = b * p.cH * p.cW;
            a_iy0[j] = ok ? oy * p.cStride - 1 : -100000;
            a_ix0[j] = ox * p.cStride - 1;
            a_src[j] = (const h16*)p.A + lchk;
        }
    }
#pragma unroll
    for (int j = 0; j < WJ; ++j) {
        const int n = min(n0 + (wave + NWAVES * j) * 8 + lrow, p.N - 1);
        w_src[j] = (const h16*)p.W + (size_t)n * p.K + lchk;
    }

    [[maybe_unused]] const int tap_mask = FOLD ? vda_gemm::fold_tap_mask(n0, min(n0 + BN, p.N), p.tK, p.tCout) : 0x1FF;
    auto stage = [&](int kt, char* buf) {
        const int k0 = kt * BK;
        [[maybe_unused]] int kw = k0;             // W's K offset (FOLD: it follows the tap)
        if constexpr (AMODE == VDA_A_DENSE) {
#pragma unroll
            for (int j = 0; j < AJ; ++j) glds16(a_src[j] + k0, buf + (wave + NWAVES * j) * 1024);
        } else {
            const int tap0 = k0 / p.cCin, ci0 = k0 - tap0 * p.cCin;
            const int tap = FOLD ? vda_gemm::fold_nth_tap(tap_mask, tap0) : tap0;      // FOLD: the tap0-th SET tap of the mask
            if constexpr (FOLD) kw = tap * p.cCin + ci0;
            const int ky = tap / 3, kx = tap - ky * 3;
#pragma unroll
            for (int j = 0; j < AJ; ++j) {
                const int iy = a_iy0[j] + ky, ix = a_ix0[j] + kx;
                const bool ok = (unsigned)iy < (unsigned)p.cH && (unsigned)ix < (unsigned)p.cW;
                const h16* src = ok ? a_src[j] + ((size_t)(a_pix[j] + iy * p.cW + ix) * p.cCin + ci0)
                                    : (const h16*)p.zero_page + lchk;
                glds16(src, buf + (wave + NWAVES * j) * 1024);
            }
        }
#pragma unroll
        for (int j = 0; j < WJ; ++j) glds16(w_src[j] + (FOLD ? kw : k0), buf + A_BYTES + (wave + NWAVES * j) * 1024);
    };

    f32x4 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // fragment read offsets: row = lane&15 (so row&7 == lane&7), k-chunk = ks*4 + (lane>>4)
    const int frow = lane & 15, fchk = lane >> 4, fsw = lane & 7;
    const h16 relu_floor = p.relu_in ? (h16)0.f : (h16)(-65504.f);
    [[maybe_unused]] h16x8 relu_thr;
#pragma unroll
    for (int e = 0; e < 8; ++e) relu_thr[e] = relu_floor;

    auto compute = [&](const char* buf) {
        const char* At = buf + (wm * WTM + frow) * ROW_BYTES;
        const char* Wt = buf + A_BYTES + (wn * WTN + frow) * ROW_BYTES;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int coff = ((ks * 4 + fchk) ^ fsw) << 4;
            h16x8 af[MI], wf[NI];
#pragma unroll
            for (int i = 0; i < MI; ++i) af[i] = *reinterpret_cast<const h16x8*>(At + i * 16 * ROW_BYTES + coff);
#pragma unroll
            for (int j = 0; j < NI; ++j) wf[j] = *reinterpret_cast<const h16x8*>(Wt + j * 16 * ROW_BYTES + coff);
            if constexpr (AMODE == VDA_A_CONV3X3 && RELU) {
#pragma unroll
                for (int i = 0; i < MI; ++i) af[i] = __builtin_elementwise_max(af[i], relu_thr);
            }
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[j], af[i], acc[i][j], 0, 0, 0);
        }
    };

    const int nt = FOLD ? __builtin_popcount(tap_mask) * (p.cCin / BK) : p.K / BK;
    stage(0, smem);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int cur = 0;
    for (int kt = 0; kt < nt; ++kt) {
        if (kt + 1 < nt) stage(kt + 1, smem + (cur ^ 1) * STAGE);
        compute(smem + cur * STAGE);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        cur ^= 1;
    }

    // ---- epilogue: lane holds, per subtile, 4 consecutive columns of one row
    const int em = m0 + wm * WTM + (lane & 15);
    const int en = n0 + wn * WTN + (lane >> 4) * 4;
    auto run = [&](auto epi_tag) {
        constexpr int EPI = decltype(epi_tag)::value;
        if constexpr (EPI == VDA_EPI_GEGLU_F16) {
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; j += 2) store_one<EPI>(p, em + i * 16, en + j * 16, acc[i][j], acc[i][j + 1]);
        } else {
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j) store_one<EPI>(p, em + i * 16, en + j * 16, acc[i][j], acc[i][j]);
        }
    };
    if constexpr (FOLD) run(std::integral_constant<int, VDA_EPI_CONVT_FOLD_F16>{});
    else vda_gemm::dispatch_epilogue(p.epilogue, run);
}

template <int BM, int BN, int AMODE>
__global__ void __launch_bounds__(NTHREADS) gemm_kernel(const vda_gemm_args p) {
    gemm_tile<BM, BN, AMODE, false, true>(p);
}
template <int BM, int BN>
__global__ void __launch_bounds__(NTHREADS) gemm_fold_kernel(const vda_gemm_args p) {
    gemm_tile<BM, BN, VDA_A_CONV3X3, true, true>(p);
}
// conv A without an input ReLU, plain or folded (vda_gemm_launch_name reports gemm_kernel / gemm_fold_kernel for either)
template <int BM, int BN, bool FOLD>
__global__ void __launch_bounds__(NTHREADS) gemm_plain_kernel(const vda_gemm_args p) {
    gemm_tile<BM, BN, VDA_A_CONV3X3, FOLD, false>(p);
}

template <int BM, int BN, int AMODE, bool FOLD = false, bool RELU = true>
int launch(const vda_gemm_args& a, hipStream_t s) {
    constexpr int smem = 2 * (BM + BN) * ROW_BYTES;
    static VdaKernelDeviceState dev_state;
    void (*const kern)(const vda_gemm_args) = [] {
        if constexpr (!RELU) return &gemm_plain_kernel<BM, BN, FOLD>;
        else if constexpr (FOLD) return &gemm_fold_kernel<BM, BN>;
        else return &gemm_kernel<BM, BN, AMODE>;
    }();
    if (vda_prepare_kernel(reinterpret_cast<const void*>(kern), smem, dev_state) < 0) return 2;
    const int nbm = (a.M + BM - 1) / BM, nbn = (a.N + BN - 1) / BN;
    hipLaunchKernelGGL(kern, dim3(nbm * nbn), dim3(NTHREADS), smem, s, a);
    VDA_LAUNCH_CHECK();
    return 0;
}

// Partial row statistics of the split stream for the kernels whose epilogue is not row-layout (small problems only):
// part[j, m, :] = (sum, centred sum of squares) of hi + lo over columns 64j..64j+63, one lane per (row, 64-column block).
__global__ void __launch_bounds__(256) split_partials_kernel(const h16* __restrict__ hi, const h16* __restrict__ lo, float* __restrict__ part,
                                                             int M, int N, int ldc, int ld) {
    const int np = N >> 6;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)M * np) return;
    const int m = (int)(i / np), j = (int)(i - (long long)m * np);
    const h16* a = hi + (size_t)m * ldc + j * 64;
    const h16* b = lo + (size_t)m * ldc + j * 64;
    float sum = 0.f;
    for (int e = 0; e < 64; ++e) sum += (float)a[e] + (float)b[e];
    const float mean = sum * (1.f / 64.f);
    float sq = 0.f;
    for (int e = 0; e < 64; ++e) {
        const float d = ((float)a[e] + (float)b[e]) - mean;
        sq = fmaf(d, d, sq);
    }
    part[2 * ((size_t)j * ld + m)] = sum;             // ld = rows per column block of the array (stats_ld: M of the WHOLE GEMM for a row range)
    part[2 * ((size_t)j * ld + m) + 1] = sq;
}

}  // namespace

// The family launchers. Each returns -1 for an (A mode, epilogue) pair its family is not built for (gemm_epilogue.h); the planner
// asks vda_gemm_built first, so -1 from a planned launch is an internal error.
int vda_gemm256_dense_bn256(const vda_gemm_args& a, hipStream_t s);          // gemm256_*.hip: 32x32x16 MFMA
int vda_gemm256_dense_bn128(const vda_gemm_args& a, hipStream_t s);
int vda_gemm256_conv_bn256(const vda_gemm_args& a, hipStream_t s);
int vda_gemm256_conv_bn128(const vda_gemm_args& a, hipStream_t s);
int vda_gemm256s_dense_bn256(const vda_gemm_args& a, hipStream_t s);         // gemm256s_*.hip: the same tiles on 16x16x32 MFMA
int vda_gemm256s_dense_bn128(const vda_gemm_args& a, hipStream_t s);
int vda_gemm256s_conv_bn256(const vda_gemm_args& a, hipStream_t s);
int vda_gemm256s_conv_bn128(const vda_gemm_args& a, hipStream_t s);
int vda_gemm256s_dense_bn128_bm192(const vda_gemm_args& a, hipStream_t s);      // 192 x 128 tiles, six waves
int vda_gemm256s_dense_bn128_bm192_x2(const vda_gemm_args& a, hipStream_t s);   // the same tile, TWO workgroups per CU (variant 11)
int vda_gemm256s_dense_bn384_bm192(const vda_gemm_args& a, hipStream_t s);      // 192 x 384 tiles, twelve waves
int vda_gemm8p_dense_bn256(const vda_gemm_args& a, hipStream_t s);           // gemm8p_*.hip: 8-phase two-group schedule
int vda_gemm8p_conv_bn256(const vda_gemm_args& a, hipStream_t s);
int vda_gemm8p_dense_bn256_sched(const vda_gemm_args& a, hipStream_t s, int sched);
int vda_gemm8p_dense_bn128(const vda_gemm_args& a, hipStream_t s);
int vda_gemm8p_dense_bn256_bm192(const vda_gemm_args& a, hipStream_t s);     // 192 x 256 tiles
int vda_gemm8p_conv_bn128(const vda_gemm_args& a, hipStream_t s);
int vda_gemm8p_conv_fold_bn256(const vda_gemm_args& a, hipStream_t s);       // VDA_EPI_CONVT_FOLD_F16
int vda_conv3x3_lds(const vda_gemm_args& a, hipStream_t s);                  // conv_lds.hip: patch-in-LDS direct 3x3 convolution for
bool vda_conv3x3_lds_covers(const vda_gemm_args& a);                         // narrow outputs, and the problems it covers

// the 128-row kernel (any size, any epilogue)
static int launch_small(const vda_gemm_args& a, hipStream_t s) {
    const bool narrow = a.N <= 64;
    if (a.a_mode == VDA_A_DENSE) {
        const int rc = narrow ? launch<128, 64, VDA_A_DENSE>(a, s) : launch<128, 128, VDA_A_DENSE>(a, s);
        if (rc == 0 && a.epilogue == VDA_EPI_SCALE_RES_SPLIT) {
            // this kernel's epilogue does not own whole row segments: the partial statistics come from a pass over the planes
            const long long items = (long long)a.M * (a.N >> 6);
            hipLaunchKernelGGL(split_partials_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, (const h16*)a.out, (const h16*)a.out2, a.stats, a.M,
                               a.N, a.ldc, a.stats_ld ? a.stats_ld : a.M);
            VDA_LAUNCH_CHECK();
        }
        return rc;
    }
    // conv A: the instantiation with the max only where the kernel would have applied the ReLU (p.relu_in != 0; VDA_GEMM_PLAIN_CONV=0: always)
    const bool relu = a.relu_in || !vda_gemm_plain_conv();
    if (a.epilogue == VDA_EPI_CONVT_FOLD_F16)                                                          // (N = k * k * Cout: never narrow)
        return relu ? launch<128, 128, VDA_A_CONV3X3, true>(a, s) : launch<128, 128, VDA_A_CONV3X3, true, false>(a, s);
    if (relu) return narrow ? launch<128, 64, VDA_A_CONV3X3>(a, s) : launch<128, 128, VDA_A_CONV3X3>(a, s);
    return narrow ? launch<128, 64, VDA_A_CONV3X3, false, false>(a, s) : launch<128, 128, VDA_A_CONV3X3, false, false>(a, s);
}

extern "C" int vda_gemm_built(int family, int bm, int bn, int per_cu, int a_mode, int epilogue) {
    const bool dense = a_mode == VDA_A_DENSE, conv = a_mode == VDA_A_CONV3X3, wide = bn == 256 || bn == 128;
    if (epilogue < 0 || epilogue > VDA_EPI_CONVT_FOLD_F16 || !(dense || conv)) return 0;
    // the folded ConvTranspose + conv: conv A on the 128-row kernel's 128 x 128 tile and the 8-phase 256 x 256 tile, nowhere else
    if (epilogue == VDA_EPI_CONVT_FOLD_F16)
        return conv && per_cu == 1 && ((family == VDA_GEMM_FAM_128 && bm == 128 && bn == 128) || (family == VDA_GEMM_FAM_8P && bm == 256 && bn == 256));
    switch (family) {
        case VDA_GEMM_FAM_128: return bm == 128 && (bn == 64 || bn == 128) && per_cu == 1;
        case VDA_GEMM_FAM_256: return bm == 256 && wide && per_cu == 1 && (dense ? VDA_EPI_BUILT(VDA_EPIS_DENSE_MFMA32, epilogue) : VDA_EPI_BUILT(VDA_EPIS_CONV, epilogue));
        case VDA_GEMM_FAM_256S:
            if (bm == 256) return wide && per_cu == 1 && (dense ? VDA_EPI_BUILT(VDA_EPIS_DENSE, epilogue) : VDA_EPI_BUILT(VDA_EPIS_CONV, epilogue));
            if (bm != 192 || !dense) return 0;
            if (bn == 384) return per_cu == 1 && VDA_EPI_BUILT(VDA_EPIS_256S_BN384, epilogue);
            return bn == 128 && (per_cu == 2 ? VDA_EPI_BUILT(VDA_EPIS_256S_BM192_X2, epilogue) : per_cu == 1 && VDA_EPI_BUILT(VDA_EPIS_256S_BM192, epilogue));
        case VDA_GEMM_FAM_8P:
            if (per_cu != 1) return 0;
            if (bm == 192) return bn == 256 && dense && VDA_EPI_BUILT(VDA_EPIS_8P_BM192, epilogue);
            return bm == 256 && wide && (dense ? VDA_EPI_BUILT(VDA_EPIS_DENSE, epilogue) : VDA_EPI_BUILT(VDA_EPIS_CONV, epilogue));
        case VDA_GEMM_FAM_CONV_LDS: return bm == 0 && (bn == 32 || bn == 64) && per_cu == 1 && conv && VDA_EPI_BUILT(VDA_EPIS_CONV, epilogue);
        default: return 0;
    }
}

// Everything the planner reads besides the call's own arguments, in one place: the A/B integers of vda_gemm_set_variant /
// vda_gemm_set_debug and the environment switches (read once, at the first use; vda_gemm_reload_tuning reads them again).
struct GemmTuning {
    int variant = -1;      // vda_gemm_set_variant: -1 auto; 0 = 128-row tiles; 1 / 2 = 256x256 / 256x128 on 32x32x16 MFMA; 3 / 4 = the same on
                           // 16x16x32 MFMA; 5 (+ 16 * flags + 32 * sched) = 256x256 8-phase; 7 = patch-in-LDS conv; 8 = 192x128; 9 = 256x128
                           // 8-phase; 10 = 192x384; 11 = 192x128 twice per CU
    int debug = 0;         // vda_gemm_set_debug: diagnostic switches of the 8-phase kernel (VDA_DEBUG_*)
    int split, r192;       // VDA_GEMM_SPLIT (1; 0 = never, 2 = whenever the round count says so, any K), VDA_GEMM_R192 (84: cost of a 192-row round, %)
    int big_min_n;         // VDA_GEMM_BIG_MIN_N (192): narrower outputs stay on the 128-row kernel
    int eight128;          // VDA_GEMM_8P128 (0): 256 x 128 on the 8-phase schedule too (ViT-S's N = 384 / 1152 / 1536 GEMMs, output_conv1: -4..+2 %)
    int stagger;           // VDA_GEMM_STAGGER (0; 1 / 2 = start stagger, see gemm8p_kernel.h)
    long long nt_mb;       // VDA_GEMM_NT_MB (192; 0 = never): outputs of that many megabytes and up get non-temporal stores
    int bm192;             // VDA_GEMM_BM192 (1): 192 x 128 tiles when they quantise better
    int small_grid;        // VDA_GEMM_SMALL_GRID (1): the 128-row kernel when 256-row tiles fill at most half of the CUs
    int bn384;             // VDA_GEMM_BN384 (2): where 192 x 384 tiles apply, see plan_one
    int conv_lds;          // VDA_CONV_LDS (1): narrow-output 3x3 convs as a patch-in-LDS direct convolution
    int plain_conv;        // VDA_GEMM_PLAIN_CONV (1; 0 = A/B): 3x3 convs without relu_in run the instantiation without the max (vda_common.h)
    void read_env() {
        auto env = [](const char* k, long long d) { const char* v = getenv(k); return v ? atoll(v) : d; };
        split = (int)env("VDA_GEMM_SPLIT", 1), r192 = (int)env("VDA_GEMM_R192", 84), big_min_n = (int)env("VDA_GEMM_BIG_MIN_N", 192);
        eight128 = (int)env("VDA_GEMM_8P128", 0), stagger = (int)env("VDA_GEMM_STAGGER", 0), nt_mb = env("VDA_GEMM_NT_MB", 192);
        bm192 = (int)env("VDA_GEMM_BM192", 1), small_grid = (int)env("VDA_GEMM_SMALL_GRID", 1), bn384 = (int)env("VDA_GEMM_BN384", 2);
        conv_lds = (int)env("VDA_CONV_LDS", 1), plain_conv = (int)env("VDA_GEMM_PLAIN_CONV", 1);
    }
};
static GemmTuning& tuning() {
    static GemmTuning t = [] { GemmTuning x; x.read_env(); return x; }();
    return t;
}
bool vda_gemm_plain_conv() { return tuning().plain_conv != 0; }
extern "C" int vda_gemm_set_variant(int v) { return tuning().variant = v, 0; }
extern "C" int vda_gemm_set_debug(int flags) { return tuning().debug = flags & VDA_OPT_BYTE, 0; }
extern "C" int vda_gemm_reload_tuning(void) { return tuning().read_env(), 0; }

static int device_cus() {
    static thread_local int ncu = 0;
    if (ncu == 0) {
        int dev = 0, cu = 0;
        (void)hipGetDevice(&dev);
        (void)hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev);
        ncu = cu < 8 ? 8 : (cu & ~7);
    }
    const int cap = g_vda_max_wgs;             // vda_set_max_wgs: the planner's rounds are rounds of the CAPPED grid
    return (cap >= 8 && cap < ncu) ? (cap & ~7) : ncu;
}

// Rows [0, M1) on 256 x 256 tiles in whole rounds of the chip, rows [M1, M) on 192 x 256 tiles. Cost model, calibrated on the MI355X
// (tools/gemm_ab.py -1,5,1029, round 3): a round of 256-row tiles takes t = 1.6 us per K tile + 5 us; a round of 192-row tiles 0.84 t
// (not 0.75: the load sections of the two-group schedule shrink less than its MFMA sections); the second launch costs ~10 us
// (boundary, pipeline refill, no cross-launch prefetch). What that leaves: K = 4096 (fc2: 3 rounds -> 2 + 0.84: 315 -> 301 us with the
// plain epilogue, 357 -> 348 with the split-residual one) pays; K = 1024 (qkv 9 -> 6 + 3 x 0.84: 260 -> 272 us; proj) does not - a
// partial last round already runs faster than a full one, which a round count cannot see: K < 2048 never splits. M1 == M unless
// the model predicts at least 1.5 % (VDA_GEMM_SPLIT=0: never; 2: whenever the round count says so, any K - the A/B switch).
static int plan_split(const GemmTuning& t, long long ncu, int M, int N, int K, int epilogue, int a_mode) {
    const int allow = t.split;
    if (!allow || a_mode != VDA_A_DENSE || !VDA_EPI_BUILT(VDA_EPIS_8P_BM192, epilogue) || M < 4096 || N < 256 || K < (allow == 2 ? 256 : 2048)) return M;
    const long long nbn = (N + 255) / 256, rt = (M + 255) / 256;
    auto rounds = [&](long long tiles) { return (tiles + ncu - 1) / ncu; };
    const double tk = 1.6 * (K / 64) + 5.0, launch = allow == 2 ? 0.0 : 10.0;         // us (VDA_GEMM_SPLIT=2: A/B, split whenever rounds say so)
    const double single = (double)rounds(rt * nbn) * tk;
    double best = single * 0.985;
    int best_m1 = M;
    for (long long r = 8; r * 256 < M; ++r) {               // (both parts stay on the 8-phase kernels: >= 2048 rows each, so a row's
        const long long m2 = M - r * 256;                   // arithmetic - K order, bias in the accumulators' start - is the same in either)
        if (m2 < 2048) break;
        const double cost = (double)rounds(r * nbn) * tk + 0.01 * t.r192 * (double)rounds(((m2 + 191) / 192) * nbn) * tk + launch;
        if (cost < best) {
            best = cost;
            best_m1 = (int)(r * 256);
        }
    }
    return best_m1;
}
extern "C" int vda_gemm_plan_split(int M, int N, int K, int epilogue, int a_mode) { return plan_split(tuning(), device_cus(), M, N, K, epilogue, a_mode); }

// args of the row range [r0, r0 + rows) of a dense GEMM (the layout rules of vda_gemm_row_range's comment in vda.h)
static vda_gemm_args row_range(const vda_gemm_args& a0, int r0, int rows) {
    vda_gemm_args a = a0;
    if (a.lda == 0) a.lda = a.K;       // vda.h: a row range reads 0 as "dense, K" (vda_gemm_f16 itself reads lda == 0 as a broadcast
    if (a.ldc == 0) a.ldc = a.N;       // row, and the planner never row-splits such a GEMM)
    vda_gemm_args p = a;
    auto adv = [&](const void* q, size_t bytes_per_row) -> const void* { return q ? (const char*)q + (size_t)r0 * bytes_per_row : nullptr; };
    const bool f32_out = a.epilogue == VDA_EPI_SCALE_RES_F32;
    const size_t ob = f32_out ? 4 : 2;
    p.A = adv(a.A, (size_t)a.lda * 2);
    p.out = const_cast<void*>(adv(a.out, (size_t)a.ldc * ob));
    if (a.epilogue == VDA_EPI_SCALE_RES_F32) p.res = adv(a.res, (size_t)a.ldc * 4);
    if (a.epilogue == VDA_EPI_SCALE_RES_SPLIT) {
        p.res = adv(a.res, (size_t)a.ldc * 2);
        p.res2 = adv(a.res2, (size_t)a.ldc * 2);
        p.out2 = const_cast<void*>(adv(a.out2, (size_t)a.ldc * 2));
        p.stats = (float*)const_cast<void*>(adv(a.stats, 8));
        p.stats_ld = a.stats_ld ? a.stats_ld : a.M;
        if (a.pos != nullptr && (const void*)a.pos != a.zero_page) p.pos = (const float*)adv(a.pos, 8);
    }
    if (a.epilogue == VDA_EPI_LN_BIAS_F16) p.stats = (float*)const_cast<void*>(adv(a.stats, 8));
    p.M = rows;
    return p;
}

extern "C" int vda_gemm_row_range(const vda_gemm_args* args, int r0, int rows, vda_gemm_args* out) {
    VDA_REQUIRE(args && out && r0 >= 0 && rows > 0 && r0 + rows <= args->M, "vda_gemm_row_range: bad range");
    VDA_REQUIRE(args->a_mode == VDA_A_DENSE && VDA_EPI_BUILT(VDA_EPIS_8P_BM192, args->epilogue), "vda_gemm_row_range: dense A and a row-splittable epilogue only");
    *out = row_range(*args, r0, rows);
    return 0;
}

// ---- 1. validate. operands = false (the planner): the shape and mode rules alone, no pointer is looked at.
static int validate(vda_gemm_args& a, bool operands) {
#define VDA_PTR(cond) (!operands || (cond))
    VDA_REQUIRE(VDA_PTR(a.A && a.W && a.out), "vda_gemm_f16: null operand");
    VDA_REQUIRE(a.M > 0 && a.N > 0 && a.K > 0, "vda_gemm_f16: empty problem M=%d N=%d K=%d", a.M, a.N, a.K);
    VDA_REQUIRE(a.K % BK == 0, "vda_gemm_f16: K=%d must be a multiple of %d (pad at pack time)", a.K, BK);
    VDA_REQUIRE(a.N % 4 == 0 && a.ldc % 4 == 0, "vda_gemm_f16: N=%d and ldc=%d must be multiples of 4", a.N, a.ldc);
    VDA_REQUIRE(VDA_PTR(((uintptr_t)a.A & 15) == 0 && ((uintptr_t)a.W & 15) == 0 && ((uintptr_t)a.out & 15) == 0),
                "vda_gemm_f16: operands must be 16-byte aligned");
    VDA_REQUIRE(a.epilogue >= 0 && a.epilogue <= VDA_EPI_CONVT_FOLD_F16, "vda_gemm_f16: bad epilogue %d", a.epilogue);
    if (a.a_mode == VDA_A_DENSE) {
        VDA_REQUIRE(a.relu_in == 0, "vda_gemm_f16: relu_in is only built for the conv A operand");
        VDA_REQUIRE((a.lda >= a.K || a.lda == 0) && a.lda % 8 == 0, "vda_gemm_f16: lda=%d must be >= K (or 0 = broadcast row) and a multiple of 8", a.lda);
    } else if (a.a_mode == VDA_A_CONV3X3) {
        VDA_REQUIRE(VDA_PTR(a.zero_page != nullptr), "vda_gemm_f16: conv needs zero_page");
        VDA_REQUIRE(a.cCin % BK == 0 && a.K == 9 * a.cCin, "vda_gemm_f16: conv needs Cin%%64==0 and K==9*Cin (Cin=%d K=%d)", a.cCin, a.K);
        VDA_REQUIRE(a.cStride == 1 || a.cStride == 2, "vda_gemm_f16: conv stride %d", a.cStride);
        VDA_REQUIRE(a.cHo == (a.cH + 2 - 3) / a.cStride + 1 && a.cWo == (a.cW + 2 - 3) / a.cStride + 1,
                    "vda_gemm_f16: conv output size mismatch");
        VDA_REQUIRE(a.M == a.cB * a.cHo * a.cWo, "vda_gemm_f16: conv M=%d != B*Ho*Wo", a.M);
        VDA_REQUIRE((long long)a.cB * a.cH * a.cW * a.cCin < (1ll << 31), "vda_gemm_f16: conv input too large for 32-bit pixel index");
    } else {
        VDA_REQUIRE(false, "vda_gemm_f16: bad a_mode %d", a.a_mode);
    }
    switch (a.epilogue) {
        case VDA_EPI_SCALE_RES_F32:
        case VDA_EPI_SCALE_RES_F32_H:
        case VDA_EPI_RES_F16:
            VDA_REQUIRE(VDA_PTR(a.res != nullptr), "vda_gemm_f16: residual epilogue needs res");
            break;
        case VDA_EPI_GEGLU_F16:
            VDA_REQUIRE(a.N % 32 == 0, "vda_gemm_f16: GEGLU needs N%%32==0");
            break;
        case VDA_EPI_SCALE_RES_SPLIT:
            VDA_REQUIRE(VDA_PTR(a.res != nullptr && a.res2 != nullptr && a.out2 != nullptr && a.stats != nullptr),
                        "vda_gemm_f16: the split-residual epilogue needs res, res2 (hi / lo planes), out2 and stats");
            VDA_REQUIRE(a.N % 64 == 0 && a.ldc % 8 == 0 && a.a_mode == VDA_A_DENSE, "vda_gemm_f16: the split-residual epilogue needs a dense A operand, N%%64==0 and ldc%%8==0");
            VDA_REQUIRE(((uintptr_t)a.res & 15) == 0 && ((uintptr_t)a.res2 & 15) == 0 && ((uintptr_t)a.out2 & 15) == 0 && ((uintptr_t)a.stats & 7) == 0,
                        "vda_gemm_f16: split-residual planes must be 16-byte aligned");
            if (!operands) break;
            // re-centring rows (pos = [M, 2] (mean, rstd), optional): the kernels load pos[m * P] unconditionally
            // (pos == zero_page is this function's own "no re-centring" form coming back with a record of a split: stride 0 stays)
            if (a.pos != nullptr && (const void*)a.pos != a.zero_page) {
                VDA_REQUIRE(((uintptr_t)a.pos & 7) == 0, "vda_gemm_f16: pos (re-centring statistics) must be 8-byte aligned");
                a.P = 2;
            } else {
                VDA_REQUIRE(a.zero_page != nullptr, "vda_gemm_f16: the split-residual epilogue without pos needs zero_page");
                a.pos = (const float*)a.zero_page;
                a.P = 0;
            }
            break;
        case VDA_EPI_LN_BIAS_F16:
        case VDA_EPI_LN_GELU_F16:
            VDA_REQUIRE(VDA_PTR(a.stats != nullptr && a.gamma != nullptr && a.bias != nullptr) && a.a_mode == VDA_A_DENSE,
                        "vda_gemm_f16: a LayerNorm-folded epilogue needs a dense A operand, stats (mean, rstd rows), gamma (= c1) and bias (= c2)");
            VDA_REQUIRE(((uintptr_t)a.stats & 7) == 0, "vda_gemm_f16: stats must be 8-byte aligned");
            break;
        case VDA_EPI_PATCH_F32:
            VDA_REQUIRE(VDA_PTR(a.pos != nullptr) && a.P > 0 && a.M % a.P == 0, "vda_gemm_f16: patch epilogue needs pos and M%%P==0");
            break;
        case VDA_EPI_CONVT_F16:
            VDA_REQUIRE(a.tK > 0 && a.tCout > 0 && a.tCout % 4 == 0 && a.N == a.tK * a.tK * a.tCout && a.M % (a.tH * a.tW) == 0,
                        "vda_gemm_f16: bad ConvTranspose geometry");
            break;
        case VDA_EPI_CONVT_FOLD_F16:
            VDA_REQUIRE(a.a_mode == VDA_A_CONV3X3 && a.cStride == 1, "vda_gemm_f16: the folded ConvTranspose epilogue needs the conv A operand at stride 1");
            VDA_REQUIRE(a.tK >= 2 && a.tCout > 0 && a.tCout % 8 == 0 && a.N == a.tK * a.tK * a.tCout && a.tH == a.cH && a.tW == a.cW && a.ldc % 8 == 0,
                        "vda_gemm_f16: bad folded ConvTranspose geometry (k=%d Cout=%d N=%d, %d x %d on a %d x %d grid)", a.tK, a.tCout, a.N, a.tH, a.tW, a.cH, a.cW);
            VDA_REQUIRE(VDA_PTR(a.bias != nullptr), "vda_gemm_f16: the folded ConvTranspose epilogue needs bias (the class-bias table of vda_fold_convt_weight)");
            VDA_REQUIRE((long long)a.M * a.tK * a.tK * a.ldc < (1ll << 31), "vda_gemm_f16: folded ConvTranspose output too large for 32-bit offsets");
            break;
        default:
            break;
    }
#undef VDA_PTR
    return 0;
}

// ---- 2. plan. ONE launch of `a`, its shape decisions taken for Mp >= a.M rows (vda_gemm_plan's m_plan). Reads the shape and mode
// fields, tile_rows and whether sched is set. *splittable: the automatic path reached the 8-phase 256 x 256 tile with dense A, where a
// row split may apply; what the record then holds is the launch of the whole GEMM.
static int plan_one(const GemmTuning& t, const vda_gemm_args& a, int Mp, int ncu, vda_gemm_launch* r, bool* splittable) {
    const int v = t.variant;
    const bool dense = a.a_mode == VDA_A_DENSE;
    *splittable = false;
    *r = vda_gemm_launch{0, a.M, VDA_GEMM_FAM_128, 128, a.N <= 64 ? 64 : 128, 1, 1, 0, a.relu_in, a.tile_rows, a.a_mode, a.epilogue};
    auto pick = [&](int family, int bm, int bn, int per_cu, int options) {
        if (!vda_gemm_built(family, bm, bn, per_cu, a.a_mode, a.epilogue)) return false;
        r->family = family, r->bm = bm, r->bn = bn, r->per_cu = per_cu, r->options = options;
        return true;
    };
    // Narrow-output 3x3 convs (Cout <= 64: the ViT-S head) run as a patch-in-LDS direct convolution instead of an implicit GEMM
    // (variant 7 forces it, any other explicit variant or VDA_CONV_LDS=0 keeps the GEMM: A/B and cross-checks).
    if (!dense && ((v < 0 && t.conv_lds) || v == 7) && vda_conv3x3_lds_covers(a) && pick(VDA_GEMM_FAM_CONV_LDS, 0, a.N <= 32 ? 32 : 64, 1, a.relu_in)) return 0;
    const bool fold = a.epilogue == VDA_EPI_CONVT_FOLD_F16;
    if (fold) r->bn = 128;
    const bool fits32 = (dense ? (long long)a.M * a.lda : 0ll) + a.K < (1ll << 31) && (long long)a.N * a.K < (1ll << 31);
    VDA_REQUIRE(fits32 || v <= 0, "vda_gemm_f16: operand too large for the 256-row kernel's 32-bit offsets");
    if (!fits32) return 0;
    // ---- the A/B integer: tile width, MFMA shape, 8-phase schedule and its switches
    int big = (v == 1 || v == 3) ? 256 : (v == 2 || v == 4 || v == 8 || v == 9 || v == 10 || v == 11) ? 128 : 0;
    const bool mfma32 = v == 1 || v == 2;
    bool eight = v == 9 || (v >= 5 && (v & 15) == 5);                         // 5 + 16 * flags + 32 * sched (the two overlap, as they always did)
    if (eight && v != 9) big = 256;
    const int sched8 = eight ? ((v >> 5) & 3) : 0;
    if (v < 0 && a.N >= t.big_min_n && Mp >= 2048) {
        // large-tile kernel, BN picked for the smaller padded width. 256 x 256: the 8-phase two-group schedule (tools/gemm_ab.py,
        // in-process A/B: -4..-15 % on every encoder shape and epilogue; the conv A operand too, gathered by bounds-checked buffer
        // loads: +7..10 % over the one-barrier kernel on the head's 256-channel convs). 256 x 128 on that schedule is not the default.
        const int pad256 = (a.N + 255) / 256 * 256, pad128 = (a.N + 127) / 128 * 128;
        big = pad128 < pad256 ? 128 : 256;
        eight = big == 256 || t.eight128;
    }
    if (big && (a.N % 8 != 0 || a.ldc % 8 != 0)) {
        VDA_REQUIRE(v < 0, "vda_gemm_f16: the 256-row kernel needs N and ldc to be multiples of 8");
        big = 0;                            // its epilogue owns 8-column (16-byte) row segments
    }
    if (!big) return 0;
    if (fold && !(eight && big == 256)) return 0;          // built for the 8-phase 256 x 256 tile only: anything else is the 128-row kernel's
    // ---- the option word
    int opt = a.relu_in;
    if (!t.stagger) opt |= VDA_FLAG_NO_STAGGER << VDA_OPT_FLAGS_SHIFT;
    if (t.stagger == 2) opt |= VDA_FLAG_STAGGER_PANEL << VDA_OPT_FLAGS_SHIFT;
    if (eight && v > 0) opt = (a.relu_in & VDA_OPT_BYTE) | (((v >> 4) & VDA_OPT_BYTE) << VDA_OPT_FLAGS_SHIFT);      // A/B switches
    opt |= t.debug << VDA_OPT_DEBUG_SHIFT;
    // Non-temporal output stores (8-phase kernel, fp16 row stores) for outputs that no cache will hand to the next kernel.
    // ViT-L: qkv, hid, the GEGLU hidden, the 148^2 conv maps; ViT-S: none.
    if (t.nt_mb > 0 && (long long)Mp * a.N * 2 >= t.nt_mb * 1000000ll) opt |= VDA_OPT_NT_STORES;
    // 192-row tiles when they quantise better on this device: rounds of 256-row tiles against 3/4-size rounds of 192-row tiles
    // (ViT-S proj / fc2: 3 against 2.25; variant 8 forces them). Only the one-barrier 256 x 128 family has the shape.
    bool tall192 = v == 8 && dense;
    if (v < 0 && !eight && big == 128 && dense) {
        const long long nbn = (a.N + 127) / 128;
        const long long r256 = (((Mp + 255) / 256) * nbn + ncu - 1) / ncu, r192 = (((Mp + 191) / 192) * nbn + ncu - 1) / ncu;
        tall192 = t.bm192 && r192 * 3 * 100 < r256 * 4 * 85;                 // at least 15 % fewer tile-time units (a 192-row tile costs ~0.8, not 0.75, of a 256-row one)
    }
    // Few large tiles leave most of the chip idle for a whole K loop: when the 256-row tiling fills at most half of the CUs the
    // 128-row kernel (four times the tiles, two workgroups per CU) is faster - the head's 19x19 maps: rn4 (46 tiles, K = 9216)
    // 223 -> 133 us, the refinenet4 convs 62 -> 39 us (tools/gemm_ab.py, AB_SHAPES=small).
    if (v < 0 && t.small_grid && ((long long)(Mp + 255) / 256) * ((a.N + big - 1) / big) * 2 <= ncu) return 0;
    // N a multiple of 384 (ViT-S's embedding width): 192 x 384 tiles on twelve waves, one tile per row panel and column third - A and
    // the residual rows are read once, 229 row panels are one round of the chip. Since the epilogue's lane-derived addresses stay out of
    // the K loop's live set (gemm256s_kernel.h, round 4) it wins on fc2's shape with any built epilogue (split residual 86.9 -> 69.5 us)
    // and with the LayerNorm-folded epilogues on qkv (60.4 -> 55.5 us) and fc1 (against the 8-phase 256 x 256 tile: 107.0 -> 91.1 us);
    // proj's shape is a tie (profiles/r04/vits_bn384_ab.txt). VDA_GEMM_BN384 = 2 (default): N = 384 with K >= 1024 and N <= 1536 with a
    // LayerNorm-folded epilogue; 1 = every N % 384 == 0 up to 1152 off the 8-phase tile; 3 / 4 = A/B subsets; 0 = never. Variant 10 forces it.
    const bool ln_epi = a.epilogue == VDA_EPI_LN_BIAS_F16 || a.epilogue == VDA_EPI_LN_GELU_F16, fc2_384 = a.N == 384 && a.K >= 1024;
    const bool auto384 = v < 0 && a.tile_rows == 0 &&
                         (t.bn384 == 1 ? (!eight && a.N <= 1152) : t.bn384 == 2 ? (fc2_384 || (ln_epi && a.N <= 1536))
                          : t.bn384 == 3 ? fc2_384 : t.bn384 == 4 ? (fc2_384 || (ln_epi && a.N == 1536)) : false);
    if (dense && a.N % 384 == 0 && (auto384 || v == 10) && pick(VDA_GEMM_FAM_256S, 192, 384, 1, opt)) return 0;
    *splittable = eight && big == 256 && dense && v < 0;
    if (eight && big == 256 && dense && (a.tile_rows == 192 || v == 5 + 16 * VDA_FLAG_BM192) && pick(VDA_GEMM_FAM_8P, 192, 256, 1, opt))
        return r->dyn = a.sched != nullptr, 0;
    if (v == 11 && dense && pick(VDA_GEMM_FAM_256S, 192, 128, 2, opt)) return 0;      // (A/B only, see gemm256s_kernel.h)
    if (tall192 && pick(VDA_GEMM_FAM_256S, 192, 128, 1, opt)) return 0;
    // (the 32x32x16 kernel reads no option bits: it gets the caller's word)
    if (!pick(eight ? VDA_GEMM_FAM_8P : mfma32 ? VDA_GEMM_FAM_256 : VDA_GEMM_FAM_256S, 256, big, 1, mfma32 && !eight ? a.relu_in : opt)) return 0;   // not built: 128-row tiles
    if (eight) {
        // the name reports the schedule ASKED for (vda_gemm8p_dense_bn256_sched falls back to the default one for other epilogues)
        r->ksched = sched8 == 1 ? 0 : sched8 == 2 ? 2 : 1;
        r->dyn = a.sched != nullptr && r->ksched == 1 && !fold;        // (the folded mode has no dynamic-draw instantiation)
    }
    return 0;
}

// the plan of a validated call
static int plan_call(const vda_gemm_args& a, int m_plan, int ncu, int sched_per_launch, vda_gemm_plan_t* out) {
    const GemmTuning& t = tuning();
    if (ncu <= 0) ncu = device_cus();
    bool splittable = false;
    out->n = 1;
    if (int rc = plan_one(t, a, m_plan > a.M ? m_plan : a.M, ncu, &out->rec[0], &splittable)) return rc;
    // Row split: whole rounds of 256-row tiles + one launch of 192-row tiles for the remainder, each part planned as a GEMM of its own.
    // Not for a row range of a larger GEMM (its other rows run beside it), a part of a split made by hand, or a broadcast row.
    if (!splittable || m_plan > a.M || a.tile_rows != 0 || (a.sched != nullptr && !sched_per_launch) || a.lda == 0) return 0;
    const int m1 = plan_split(t, ncu, a.M, a.N, a.K, a.epilogue, a.a_mode);
    if (m1 >= a.M) return 0;
    vda_gemm_args part = a;
    for (int i = 0; i < 2; ++i) {
        part.M = i == 0 ? m1 : a.M - m1;
        part.tile_rows = i == 0 ? 0 : 192;
        if (int rc = plan_one(t, part, m_plan > part.M ? m_plan : part.M, ncu, &out->rec[i], &splittable)) return rc;
        out->rec[i].r0 = i == 0 ? 0 : m1;
    }
    out->n = 2;
    return 0;
}

extern "C" int vda_gemm_plan(const vda_gemm_args* args, int m_plan, int ncu, int sched_per_launch, vda_gemm_plan_t* out) {
    VDA_REQUIRE(args != nullptr && out != nullptr, "vda_gemm_plan: null args");
    vda_gemm_args a = *args;
    if (int rc = validate(a, false)) return rc;
    return plan_call(a, m_plan, ncu, sched_per_launch, out);
}

extern "C" int vda_gemm_launch_name(const vda_gemm_launch* r, char* name, int len) {
    switch (r->family) {
        case VDA_GEMM_FAM_128:
            if (r->epilogue == VDA_EPI_CONVT_FOLD_F16) return snprintf(name, len, "gemm_fold_kernel<%d, %d>", r->bm, r->bn);
            return snprintf(name, len, "gemm_kernel<%d, %d, %d>", r->bm, r->bn, r->a_mode);
        case VDA_GEMM_FAM_256: return snprintf(name, len, "gemm256_kernel<%d, %d, %d>", r->bn, r->a_mode, r->epilogue);
        case VDA_GEMM_FAM_256S: return snprintf(name, len, "gemm256s_kernel<%d, %d, %d, %d, %d>", r->bn, r->a_mode, r->epilogue, r->bm, r->per_cu);
        case VDA_GEMM_FAM_8P:   // (every template argument, defaults included, as the profiler prints them)
            return snprintf(name, len, "gemm8p_kernel<%d, %d, %d, %d, %d, %s>", r->bn, r->a_mode, r->epilogue, r->ksched, r->bm, r->dyn ? "true" : "false");
        case VDA_GEMM_FAM_CONV_LDS: return snprintf(name, len, "conv3x3_lds_kernel<%d>", r->bn / 32);      // (also what the C = 64 persistent kernel reports as)
        default: return snprintf(name, len, "%s", "");
    }
}

static thread_local vda_gemm_launch g_last_launch = {0, 0, -1};

extern "C" const char* vda_gemm_last_kernel(void) {
    static thread_local char name[64];
    vda_gemm_launch_name(&g_last_launch, name, sizeof(name));
    return name;
}

// ---- 3. launch one record of a plan of a0 (validated): its row range, its option word, the one launcher of its family
static int launch_record(const vda_gemm_launch& r, const vda_gemm_args& a0, hipStream_t s) {
    vda_gemm_args a = (r.r0 == 0 && r.rows == a0.M) ? a0 : row_range(a0, r.r0, r.rows);
    a.relu_in = r.options;
    a.tile_rows = r.tile_rows;
    const bool dense = a.a_mode == VDA_A_DENSE, wide = r.bn == 256;
    int rc = -1;
    switch (r.family) {
        case VDA_GEMM_FAM_128: rc = launch_small(a, s); break;
        case VDA_GEMM_FAM_CONV_LDS: rc = vda_conv3x3_lds(a, s); break;
        case VDA_GEMM_FAM_256:
            rc = dense ? (wide ? vda_gemm256_dense_bn256(a, s) : vda_gemm256_dense_bn128(a, s)) : (wide ? vda_gemm256_conv_bn256(a, s) : vda_gemm256_conv_bn128(a, s));
            break;
        case VDA_GEMM_FAM_256S:
            if (r.bm == 192) rc = r.bn == 384 ? vda_gemm256s_dense_bn384_bm192(a, s) : r.per_cu == 2 ? vda_gemm256s_dense_bn128_bm192_x2(a, s) : vda_gemm256s_dense_bn128_bm192(a, s);
            else rc = dense ? (wide ? vda_gemm256s_dense_bn256(a, s) : vda_gemm256s_dense_bn128(a, s)) : (wide ? vda_gemm256s_conv_bn256(a, s) : vda_gemm256s_conv_bn128(a, s));
            break;
        case VDA_GEMM_FAM_8P:
            if (r.bm == 192) rc = vda_gemm8p_dense_bn256_bm192(a, s);
            else if (!wide) rc = dense ? vda_gemm8p_dense_bn128(a, s) : vda_gemm8p_conv_bn128(a, s);
            else if (!dense) rc = a.epilogue == VDA_EPI_CONVT_FOLD_F16 ? vda_gemm8p_conv_fold_bn256(a, s) : vda_gemm8p_conv_bn256(a, s);
            else rc = r.ksched != 1 ? vda_gemm8p_dense_bn256_sched(a, s, r.ksched == 0 ? 1 : 2) : vda_gemm8p_dense_bn256(a, s);
            break;
        default: break;
    }
    VDA_REQUIRE(rc >= 0, "vda_gemm_f16: internal error, the plan chose a kernel that is not built (family %d, %d x %d tiles, A mode %d, epilogue %d)", r.family,
                r.bm, r.bn, a.a_mode, a.epilogue);
    g_last_launch = r;
    return rc;
}

int vda_gemm_f16_record(const vda_gemm_args* args, const vda_gemm_launch* rec, vda_stream_t stream) {
    VDA_REQUIRE(args != nullptr && rec != nullptr, "vda_gemm_f16: null args");
    vda_gemm_args a = *args;
    if (int rc = validate(a, true)) return rc;
    return launch_record(*rec, a, (hipStream_t)stream);
}

extern "C" int vda_gemm_f16(const vda_gemm_args* args, vda_stream_t stream) {
    VDA_REQUIRE(args != nullptr, "vda_gemm_f16: null args");
    vda_gemm_args a = *args;
    if (int rc = validate(a, true)) return rc;
    vda_gemm_plan_t plan;
    if (int rc = plan_call(a, 0, 0, 0, &plan)) return rc;
    for (int i = 0; i < plan.n; ++i)
        if (int rc = launch_record(plan.rec[i], a, (hipStream_t)stream)) return rc;
    return 0;
}
