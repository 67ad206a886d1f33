// Row normalisation for gfx950: LayerNorm of fp32 rows (fp16 or fp32 out, optionally with the residual add in front), the split
// residual stream's entry and tap LayerNorm (fp32 rows <-> two fp16 planes + row statistics), the pieces of LayerNorm folded into
// the neighbouring GEMMs, and per-frame GroupNorm (NHWC -> token-major). All are HBM-bound streaming kernels: 16-byte accesses,
// statistics in fp32, one pass over the data for LayerNorm (row kept in registers), two launches with a fixed-order
// (deterministic) partial-sum tree for GroupNorm.
#include "vda_common.h"
#include <initializer_list>
#include <type_traits>

namespace {

// ---------------------------------------------------------------- LayerNorm
// A row is split over LPR lanes, 8 consecutive elements per lane per chunk (two 16-byte loads in, one 16-byte
// store out); a wave holds 64/LPR rows, so small D (temporal modules: 64..256) still fills the wave. The row
// stays in registers; statistics are fp32, two-pass (mean, then centred sum of squares). Cross-lane sums use
// DPP (quad_perm / row_half_mirror / row_mirror) and v_readlane, not ds_bpermute: no LDS round trips.
template <int CTRL>
__device__ __forceinline__ float dpp_xchg(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}

template <int LPR>
__device__ __forceinline__ float segment_sum(float v, int lane) {
    v += dpp_xchg<0xB1>(v);                 // quad_perm [1,0,3,2]
    v += dpp_xchg<0x4E>(v);                 // quad_perm [2,3,0,1]
    v += dpp_xchg<0x141>(v);                // row_half_mirror: 8 lanes
    if constexpr (LPR >= 16) v += dpp_xchg<0x140>(v);    // row_mirror: 16 lanes
    if constexpr (LPR == 32) {
        const float lo = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0)) +
                         __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
        const float hi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32)) +
                         __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
        v = lane < 32 ? lo : hi;
    }
    if constexpr (LPR == 64) {
        v = (__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0)) +
             __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16))) +
            (__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32)) +
             __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48)));
    }
    return v;
}

// Where a lane stands: lane `sub` of the LPR that share row `row`; a wave holds 64 / LPR rows, a workgroup four waves.
struct RowLanes {
    int sub, row;
    bool row_ok;
};
template <int LPR>
__device__ __forceinline__ RowLanes row_lanes(int lane, int rows) {
    const int row = (blockIdx.x * 4 + (threadIdx.x >> 6)) * (64 / LPR) + lane / LPR;
    return {lane % LPR, row, row < rows};
}

// 8 consecutive elements of a row. The per-chunk steps take it BY VALUE: a step that takes the register image by reference
// is optimised before it is inlined, with the image in memory, and comes out scheduled with more live registers
// (profiles/r10: the D > 1024 kernels lost occupancy that way).
struct Chunk {
    float e[8];
};
__device__ __forceinline__ float chunk_sum(Chunk x) {                    // pairwise
    return ((x.e[0] + x.e[1]) + (x.e[2] + x.e[3])) + ((x.e[4] + x.e[5]) + (x.e[6] + x.e[7]));
}
__device__ __forceinline__ float chunk_sq(float sq, Chunk x, float mean, bool ok) {    // sq + centred squares, element order
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float d = ok ? x.e[e] - mean : 0.f;
        sq += d * d;
    }
    return sq;
}

// The row's register image and its (mean, rstd). v[c] is chunk sub + c * LPR, zeros where the row has no such chunk (they
// add nothing to the sums); load(ch) fetches chunk ch - the one step in which the kernels differ on the way in. Two-pass fp32
// statistics: chunk sums in chunk order, then the centred squares in (chunk, element) order, each across the row's lanes by
// segment_sum. Every kernel of this file that normalises a row takes its statistics here, so paths through different kernels
// agree to the bit (tests/test_forward_gpu.py relies on it).
template <int LPR, int NCH, typename LOAD>
__device__ __forceinline__ float2 load_row_stats(Chunk (&v)[NCH], const RowLanes p, int nchunk, int D, float eps, int lane, LOAD load) {
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int ch = p.sub + c * LPR;
        v[c] = Chunk{};
        if (p.row_ok && ch < nchunk) v[c] = load(ch);
        sum += chunk_sum(v[c]);
    }
    const float mean = segment_sum<LPR>(sum, lane) / (float)D;
    float sq = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) sq = chunk_sq(sq, v[c], mean, p.sub + c * LPR < nchunk);
    return float2{mean, rsqrtf(segment_sum<LPR>(sq, lane) / (float)D + eps)};
}

// Output row of input row `row` when the first `skip` rows of every `group` are dropped (the cls token); -1 for a dropped row.
__device__ __forceinline__ int out_row(int row, int group, int skip) {
    if (group <= 0) return row;
    const int g = row / group, i = row - g * group;
    return i < skip ? -1 : g * (group - skip) + (i - skip);
}

// dst[0..8) = (x - mean) * rstd * w + b, then + per (NULL = nothing) - in that order.
template <typename OT>
__device__ __forceinline__ void affine_store(Chunk x, float mean, float rstd, const float* __restrict__ w, const float* __restrict__ b,
                                             const float* __restrict__ per, OT* __restrict__ dst) {
    float o[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const f32x4 ww = *reinterpret_cast<const f32x4*>(w + h * 4);
        const f32x4 bb = *reinterpret_cast<const f32x4*>(b + h * 4);
        f32x4 y = {x.e[h * 4], x.e[h * 4 + 1], x.e[h * 4 + 2], x.e[h * 4 + 3]};
        y = (y - mean) * rstd * ww + bb;
        if (per) y += *reinterpret_cast<const f32x4*>(per + h * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[h * 4 + e] = y[e];
    }
    store8(dst, o);
}

// fp32 rows -> LayerNorm -> OT (h16 or float), optionally dropping the cls rows (group / skip) and adding pe after the affine.
// RES: the row is first updated in place, in[r,:] += gamma * y[r,:] (y fp16: the bias-added output of the preceding projection,
// gamma = LayerScale or NULL = 1) - the encoder's residual add (block.py:105-106) rides on the LayerNorm that follows it, so the
// projection GEMM stores 2 bytes per element instead of reading and writing the fp32 stream in its (fabric-bound) epilogue.
template <int LPR, int NCH, typename OT, bool RES>
__global__ void __launch_bounds__(256) layernorm_kernel(float* __restrict__ in, OT* __restrict__ out,
                                                        const float* __restrict__ w, const float* __restrict__ b,
                                                        float eps, int rows, int D, int group, int skip,
                                                        const float* __restrict__ pe, int pe_rows_per_step, int pe_steps,
                                                        const h16* __restrict__ y, const float* __restrict__ gamma) {
    const int lane = threadIdx.x & 63, nchunk = D >> 3;             // 8-element chunks per row
    const RowLanes p = row_lanes<LPR>(lane, rows);
    float* src = in + (size_t)(p.row_ok ? p.row : 0) * D;
    Chunk v[NCH];
    const float2 st = load_row_stats<LPR>(v, p, nchunk, D, eps, lane, [=](int ch) {
        Chunk x;
        load8(src + ch * 8, x.e);
        if constexpr (RES) {
            const h16x8 yy = *reinterpret_cast<const h16x8*>(y + (size_t)p.row * D + ch * 8);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                f32x4 g = {1.f, 1.f, 1.f, 1.f};
                if (gamma) g = *reinterpret_cast<const f32x4*>(gamma + ch * 8 + h * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) x.e[h * 4 + e] = fmaf(g[e], (float)yy[h * 4 + e], x.e[h * 4 + e]);
            }
            store8(src + ch * 8, x.e);
        }
        return x;
    });
    if (!p.row_ok) return;
    const int orow = out_row(p.row, group, skip);
    if (orow < 0) return;
    const float* per = pe ? pe + (size_t)((p.row / pe_rows_per_step) % pe_steps) * D : nullptr;
    OT* dst = out + (size_t)orow * D;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int ch = p.sub + c * LPR;
        if (ch < nchunk) affine_store(v[c], st.x, st.y, w + ch * 8, b + ch * 8, per ? per + ch * 8 : nullptr, dst + ch * 8);
    }
}

// ---------------------------------------------------------------- GroupNorm
// Stage 1: grid (chunks, frames). A block sums x and x^2 per channel over its rows of one frame,
// folds channels into groups in a fixed order, writes partial[frame][chunk][group][2].
template <typename T>
__global__ void __launch_bounds__(256) groupnorm_partial_kernel(const T* __restrict__ in, float* __restrict__ partial,
                                                                int hw, int C, int groups, int chunks) {
    extern __shared__ __attribute__((aligned(16))) float red[];   // [rows_par][C][2] then [C][2]
    const int frame = blockIdx.y, chunk = blockIdx.x;
    const int nv = C >> 3;                       // 16-byte vectors per row
    const int rows_par = 256 / nv;               // rows processed concurrently (>= 2 for C <= 1024)
    const int tid = threadIdx.x;
    const int rl = tid / nv, vi = tid - rl * nv;
    const int rows_per_chunk = (hw + chunks - 1) / chunks;
    const int r0 = chunk * rows_per_chunk, r1 = min(hw, r0 + rows_per_chunk);
    float s[8], q[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = q[e] = 0.f;
    if (rl < rows_par) {
        const T* base = in + (size_t)frame * hw * C + vi * 8;
        for (int r = r0 + rl; r < r1; r += rows_par) {
            float x[8];
            load8(base + (size_t)r * C, x);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                s[e] += x[e];
                q[e] += x[e] * x[e];
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            red[((size_t)rl * C + vi * 8 + e) * 2 + 0] = s[e];
            red[((size_t)rl * C + vi * 8 + e) * 2 + 1] = q[e];
        }
    }
    __syncthreads();
    float* chs = red + (size_t)rows_par * C * 2;                 // per-channel totals
    for (int c = tid; c < C; c += 256) {
        float a = 0.f, bq = 0.f;
        for (int k = 0; k < rows_par; ++k) {
            a += red[((size_t)k * C + c) * 2 + 0];
            bq += red[((size_t)k * C + c) * 2 + 1];
        }
        chs[c * 2 + 0] = a;
        chs[c * 2 + 1] = bq;
    }
    __syncthreads();
    if (tid < groups) {
        const int cpg = C / groups;
        float a = 0.f, bq = 0.f;
        for (int k = 0; k < cpg; ++k) {
            a += chs[(tid * cpg + k) * 2 + 0];
            bq += chs[(tid * cpg + k) * 2 + 1];
        }
        float* p = partial + (((size_t)frame * chunks + chunk) * groups + tid) * 2;
        p[0] = a;
        p[1] = bq;
    }
}

// Stage 2: grid (row blocks, frames). Combine the frame's partials (double, fixed order), normalise.
template <typename T>
__global__ void __launch_bounds__(256) groupnorm_apply_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                              const float* __restrict__ w, const float* __restrict__ b,
                                                              const float* __restrict__ partial, float eps, int hw, int C,
                                                              int groups, int chunks, int rows_per_block) {
    __shared__ float mean_s[64], rstd_s[64];
    const int frame = blockIdx.y, tid = threadIdx.x;
    const int cpg = C / groups;
    if (tid < groups) {
        double a = 0.0, q = 0.0;
        for (int k = 0; k < chunks; ++k) {
            const float* p = partial + (((size_t)frame * chunks + k) * groups + tid) * 2;
            a += (double)p[0];
            q += (double)p[1];
        }
        const double n = (double)hw * cpg;
        const double mean = a / n;
        double var = q / n - mean * mean;
        if (var < 0.0) var = 0.0;
        mean_s[tid] = (float)mean;
        rstd_s[tid] = (float)(1.0 / sqrt(var + (double)eps));
    }
    __syncthreads();
    const int nv = C >> 3;
    const int r0 = blockIdx.x * rows_per_block, r1 = min(hw, r0 + rows_per_block);
    const size_t fbase = (size_t)frame * hw * C;
    for (int idx = tid; idx < (r1 - r0) * nv; idx += 256) {
        const int r = r0 + idx / nv, vi = idx % nv;
        const size_t off = fbase + (size_t)r * C + vi * 8;
        float x[8], y[8];
        load8(in + off, x);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = vi * 8 + e;
            const int g = c / cpg;
            y[e] = (x[e] - mean_s[g]) * rstd_s[g] * w[c] + b[c];
        }
        store8(out + off, y);
    }
}

// ---------------------------------------------------------------- LayerNorm folded into the neighbouring GEMMs
// The fp32 residual stream of the encoder is kept as two fp16 planes, x = hi + lo (vda.h, VDA_EPI_SCALE_RES_SPLIT).
//   MODE 0 (vda_split_stats_f32): fp32 rows -> hi, lo planes + stat[row] = (mean, rstd): the entry into the split stream.
//   MODE 1 (vda_layernorm_split_f16, vda_layernorm_split_check_f16): LayerNorm(hi + lo) * w + b -> fp16, group / skip as
//           layernorm_kernel (the taps). overflow (optional): set to 1 when a row that is normalised - not a skipped one - holds a
//           saturated element (hi = +-inf, lo = -+inf: hi + lo = NaN, and so is the row's mean). A finite row cannot raise it: D <=
//           2048 elements of at most 2 * 65 504 sum to less than 2^29, their centred squares to less than 2^46.
//   MODE 2 (vda_split_center_stats_f32): as MODE 0 with the row's mean taken out: hi + lo = x - mean(x), stat[row] = (0, rstd).
// The steps of layernorm_kernel around its own loader (fp32 or hi + lo) and, for MODE 0 / 2, its own writer (planes + stat).
template <int LPR, int NCH, int MODE>
__global__ void __launch_bounds__(256) ln_split_kernel(const float* __restrict__ xin, const h16* __restrict__ hin, const h16* __restrict__ lin,
                                                       h16* __restrict__ o0, h16* __restrict__ o1, float* __restrict__ stat,
                                                       const float* __restrict__ w, const float* __restrict__ b, float eps, int rows, int D,
                                                       int group, int skip, int* __restrict__ overflow) {
    const int lane = threadIdx.x & 63, nchunk = D >> 3;
    const RowLanes p = row_lanes<LPR>(lane, rows);
    const size_t base = (size_t)(p.row_ok ? p.row : 0) * D;
    Chunk v[NCH];
    const float2 st = load_row_stats<LPR>(v, p, nchunk, D, eps, lane, [=](int ch) {
        Chunk x;
        if constexpr (MODE != 1) {
            load8(xin + base + ch * 8, x.e);
        } else {
            const h16x8 a = *reinterpret_cast<const h16x8*>(hin + base + ch * 8), l = *reinterpret_cast<const h16x8*>(lin + base + ch * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) x.e[e] = (float)a[e] + (float)l[e];
        }
        return x;
    });
    const float mean = st.x, rstd = st.y;
    if (!p.row_ok) return;
    const int orow = MODE == 1 ? out_row(p.row, group, skip) : p.row;
    if (orow < 0) return;
    if (MODE == 1 && overflow != nullptr && p.sub == 0 && !(__builtin_isfinite(mean) && __builtin_isfinite(rstd))) *overflow = 1;   // (same value from every writer)
    // MODE 2: the planes hold x - mean (the mean of what they hold is 0 up to fp32 rounding: 1e-7 of the row's spread)
    const float ctr = MODE == 2 ? mean : 0.f;
    if (MODE != 1 && p.sub == 0) *reinterpret_cast<float2*>(stat + 2 * (size_t)p.row) = float2{mean - ctr, rstd};
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int ch = p.sub + c * LPR;
        if (ch >= nchunk) continue;
        if constexpr (MODE == 1) {
            affine_store(v[c], mean, rstd, w + ch * 8, b + ch * 8, nullptr, o0 + (size_t)orow * D + ch * 8);
        } else {
            h16x8 a, l;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = v[c].e[e] - ctr;
                a[e] = (h16)d;
                l[e] = (h16)(d - (float)a[e]);
            }
            *reinterpret_cast<h16x8*>(o0 + base + ch * 8) = a;
            *reinterpret_cast<h16x8*>(o1 + base + ch * 8) = l;
        }
    }
}

// partial[np, r, 2] = (sum, centred sum of squares) per 64 columns -> stat[r] = (mean, rstd); pairwise update in column order
// (Chan, Golub, LeVeque): no E[x^2] - mean^2 cancellation, fixed order.
// overflow (optional): set to 1 when a row's mean or m2 is not finite. The row-layout GEMM families and the fused MLP kernel take
// the partials from their fp32 values, not from the fp16 planes they store, so the step in which a plane first saturates (an element
// beyond 65 504 of the token's mean: hi = +-inf, lo = -+inf) still has FINITE statistics there; only the 128-row kernel, whose
// partials are re-read from the stored planes, shows it at once. Otherwise the flag rises one step later, when a residual GEMM has
// read hi + lo = NaN back into its partials. After the last block's fc2 there is no such GEMM: the tap LayerNorm, the one
// remaining reader of the planes, reports that step (ln_split_kernel's overflow).
__global__ void __launch_bounds__(64) ln_stats_finalize_kernel(const float* __restrict__ partial, float* __restrict__ stat, float eps, int rows, int np,
                                                               int* __restrict__ overflow) {
    const int r = blockIdx.x * 64 + threadIdx.x;          // one wave per workgroup: 685 workgroups for a ViT-L clip, every CU gets some
    if (r >= rows) return;
    const float2* p = reinterpret_cast<const float2*>(partial) + r;
    float n = 0.f, mean = 0.f, m2 = 0.f;
    // the loads of a batch are issued together (a row's np partials are np independent 8-byte loads, a column block apart): the
    // plain loop waited for each before the next (8 us per launch for 5.6 MB, 47 launches per ViT-L clip)
    constexpr int BATCH = 8;
    for (int j0 = 0; j0 < np; j0 += BATCH) {
        float2 q[BATCH];
#pragma unroll
        for (int u = 0; u < BATCH; ++u) q[u] = p[(size_t)min(j0 + u, np - 1) * rows];
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            if (j0 + u < np) {                   // same arithmetic, same order as before: the combination is a fixed sequence
                const float mb = q[u].x * (1.f / 64.f), delta = mb - mean, nn = n + 64.f;
                mean += delta * (64.f / nn);
                m2 += q[u].y + delta * delta * (n * 64.f / nn);
                n = nn;
            }
        }
    }
    *reinterpret_cast<float2*>(stat + 2 * (size_t)r) = float2{mean, rsqrtf(m2 / n + eps)};
    if (overflow != nullptr && !(__builtin_isfinite(mean) && __builtin_isfinite(m2))) *overflow = 1;      // (same value from every writer)
}

// Pack-time fold of LayerNorm's affine into the following Linear: one wave per output row.
__global__ void __launch_bounds__(64) fold_ln_weight_kernel(const float* __restrict__ W, const float* __restrict__ bias, const float* __restrict__ ln_w,
                                                            const float* __restrict__ ln_b, h16* __restrict__ Wf, float* __restrict__ c1,
                                                            float* __restrict__ c2, int N, int K) {
    const int n = blockIdx.x, lane = threadIdx.x;
    float s1 = 0.f, s2 = 0.f;
    for (int k = lane; k < K; k += 64) {
        const float wv = W[(size_t)n * K + k];
        float t = wv * ln_w[k];
        asm volatile("" : "+v"(t));             // round to fp32, then to fp16 (no fused multiply-convert): the documented definition
        const h16 f = (h16)t;
        Wf[(size_t)n * K + k] = f;
        s1 += (float)f;
        s2 = fmaf(wv, ln_b[k], s2);
    }
    s1 = segment_sum<64>(s1, lane);
    s2 = segment_sum<64>(s2, lane);
    if (lane == 0) {
        c1[n] = s1;
        c2[n] = s2 + (bias ? bias[n] : 0.f);
    }
}

}  // namespace

// The checks every row-normalisation entry shares, under the entry's own name: `must` may not be NULL, `must` and `may` (NULL
// allowed) take 16-byte accesses.
static int ln_check(const char* name, int rows, int D, int group, int skip, std::initializer_list<const void*> must,
                    std::initializer_list<const void*> may = {}) {
    for (const void* q : must) VDA_REQUIRE(q != nullptr, "%s: null pointer", name);
    VDA_REQUIRE(rows > 0 && D > 0 && D % 8 == 0 && D <= 2048, "%s: D=%d must be a multiple of 8 and <= 2048", name, D);
    VDA_REQUIRE(group == 0 || (group > 0 && skip >= 0 && skip < group && rows % group == 0), "%s: bad group/skip", name);
    for (const auto& list : {must, may})
        for (const void* q : list) VDA_REQUIRE(((uintptr_t)q & 15) == 0, "%s: 16-byte alignment required", name);
    return 0;
}

// The ladder: D / 8 chunks per row -> <LPR lanes per row, NCH chunks per lane>, and the grid (4 waves of 64 / LPR rows per
// workgroup). launch(LPR, NCH, grid) receives the pair as std::integral_constants.
template <typename LAUNCH>
static void ln_ladder(int rows, int D, LAUNCH launch) {
    const int nchunk = D / 8;
    auto rung = [&](auto lpr, auto nch) { launch(lpr, nch, dim3((rows + 4 * (64 / lpr()) - 1) / (4 * (64 / lpr())))); };
    using std::integral_constant;
    if (nchunk <= 8) rung(integral_constant<int, 8>{}, integral_constant<int, 1>{});
    else if (nchunk <= 16) rung(integral_constant<int, 16>{}, integral_constant<int, 1>{});
    else if (nchunk <= 32) rung(integral_constant<int, 32>{}, integral_constant<int, 1>{});
    else if (nchunk <= 64) rung(integral_constant<int, 64>{}, integral_constant<int, 1>{});
    else if (nchunk <= 128) rung(integral_constant<int, 64>{}, integral_constant<int, 2>{});
    else rung(integral_constant<int, 64>{}, integral_constant<int, 4>{});
}

template <typename OT, bool RES = false>
static int layernorm_launch(float* in, OT* out, const float* w, const float* b, float eps, int rows, int D, int group, int skip,
                            const float* pe, int pe_rows_per_step, int pe_steps, vda_stream_t stream, const h16* y = nullptr,
                            const float* gamma = nullptr) {
    if (RES && ln_check("vda_layernorm_residual", rows, D, group, skip, {y}, {gamma})) return 1;
    if (ln_check("vda_layernorm", rows, D, group, skip, {in, out, w, b}, {pe})) return 1;
    VDA_REQUIRE(pe == nullptr || (pe_rows_per_step > 0 && pe_steps > 0), "vda_layernorm: bad pe geometry");
    ln_ladder(rows, D, [&](auto lpr, auto nch, dim3 grid) {
        hipLaunchKernelGGL((layernorm_kernel<lpr(), nch(), OT, RES>), grid, dim3(256), 0, (hipStream_t)stream, in, out, w, b, eps, rows, D,
                           group, skip, pe, pe_rows_per_step, pe_steps, y, gamma);
    });
    VDA_LAUNCH_CHECK();
    return 0;
}

extern "C" int vda_layernorm_f32_f16(const float* in, void* out, const float* w, const float* b, float eps, int rows, int D,
                                     int group, int skip, const float* pe, int pe_rows_per_step, int pe_steps,
                                     vda_stream_t stream) {
    return layernorm_launch<h16>(const_cast<float*>(in), (h16*)out, w, b, eps, rows, D, group, skip, pe, pe_rows_per_step, pe_steps, stream);
}

extern "C" int vda_layernorm_residual_f32_f16(float* x, const void* y, const float* gamma, void* out, const float* w, const float* b,
                                              float eps, int rows, int D, int group, int skip, vda_stream_t stream) {
    return layernorm_launch<h16, true>(x, (h16*)out, w, b, eps, rows, D, group, skip, nullptr, 0, 0, stream, (const h16*)y, gamma);
}

extern "C" int vda_layernorm_f32_f32(const float* in, float* out, const float* w, const float* b, float eps, int rows, int D,
                                     int group, int skip, const float* pe, int pe_rows_per_step, int pe_steps,
                                     vda_stream_t stream) {
    return layernorm_launch<float>(const_cast<float*>(in), out, w, b, eps, rows, D, group, skip, pe, pe_rows_per_step, pe_steps, stream);
}

// The three entries of ln_split_kernel; each passes the operands its MODE reads and NULL for the rest.
template <int MODE>
static int ln_split_launch(const char* name, const float* xin, const h16* hin, const h16* lin, h16* o0, h16* o1, float* stat, const float* w,
                           const float* b, float eps, int rows, int D, int group, int skip, vda_stream_t stream, int32_t* overflow = nullptr) {
    if (MODE == 1 ? ln_check(name, rows, D, group, skip, {hin, lin, o0, w, b}) : ln_check(name, rows, D, group, skip, {xin, o0, o1})) return 1;
    VDA_REQUIRE(MODE == 1 || (stat != nullptr && ((uintptr_t)stat & 7) == 0), "%s: stat must be an 8-byte aligned pointer", name);
    ln_ladder(rows, D, [&](auto lpr, auto nch, dim3 grid) {
        hipLaunchKernelGGL((ln_split_kernel<lpr(), nch(), MODE>), grid, dim3(256), 0, (hipStream_t)stream, xin, hin, lin, o0, o1, stat, w, b,
                           eps, rows, D, group, skip, (int*)overflow);
    });
    VDA_LAUNCH_CHECK();
    return 0;
}

extern "C" int vda_split_stats_f32(const float* x, void* hi, void* lo, float* stat, float eps, int rows, int D, vda_stream_t stream) {
    return ln_split_launch<0>("vda_split_stats_f32", x, nullptr, nullptr, (h16*)hi, (h16*)lo, stat, nullptr, nullptr, eps, rows, D, 0, 0, stream);
}

extern "C" int vda_split_center_stats_f32(const float* x, void* hi, void* lo, float* stat, float eps, int rows, int D, vda_stream_t stream) {
    return ln_split_launch<2>("vda_split_center_stats_f32", x, nullptr, nullptr, (h16*)hi, (h16*)lo, stat, nullptr, nullptr, eps, rows, D, 0, 0, stream);
}

extern "C" int vda_layernorm_split_f16(const void* hi, const void* lo, void* out, const float* w, const float* b, float eps, int rows, int D,
                                       int group, int skip, vda_stream_t stream) {
    return ln_split_launch<1>("vda_layernorm_split_f16", nullptr, (const h16*)hi, (const h16*)lo, (h16*)out, nullptr, nullptr, w, b, eps, rows, D,
                              group, skip, stream);
}

extern "C" int vda_layernorm_split_check_f16(const void* hi, const void* lo, void* out, const float* w, const float* b, float eps, int rows,
                                             int D, int group, int skip, int32_t* overflow, vda_stream_t stream) {
    VDA_REQUIRE(((uintptr_t)overflow & 3) == 0, "vda_layernorm_split_check_f16: overflow must be a 4-byte aligned pointer");
    return ln_split_launch<1>("vda_layernorm_split_check_f16", nullptr, (const h16*)hi, (const h16*)lo, (h16*)out, nullptr, nullptr, w, b, eps, rows,
                              D, group, skip, stream, overflow);
}

extern "C" int vda_ln_stats_finalize(const float* partial, float* stat, float eps, int rows, int np, int32_t* overflow, vda_stream_t stream) {
    VDA_REQUIRE(partial && stat && rows > 0 && np > 0, "vda_ln_stats_finalize: bad arguments");
    VDA_REQUIRE(((uintptr_t)partial & 7) == 0 && ((uintptr_t)stat & 7) == 0, "vda_ln_stats_finalize: 8-byte alignment required");
    hipLaunchKernelGGL(ln_stats_finalize_kernel, dim3((rows + 63) / 64), dim3(64), 0, (hipStream_t)stream, partial, stat, eps, rows, np, (int*)overflow);
    VDA_LAUNCH_CHECK();
    return 0;
}

extern "C" int vda_fold_ln_weight(const float* W, const float* bias, const float* ln_w, const float* ln_b, void* Wf, float* c1, float* c2, int N,
                                  int K, vda_stream_t stream) {
    VDA_REQUIRE(W && ln_w && ln_b && Wf && c1 && c2 && N > 0 && K > 0, "vda_fold_ln_weight: bad arguments");
    hipLaunchKernelGGL(fold_ln_weight_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, W, bias, ln_w, ln_b, (h16*)Wf, c1, c2, N, K);
    VDA_LAUNCH_CHECK();
    return 0;
}

template <typename T>
static int groupnorm_launch(const T* in, T* out, const float* w, const float* b, float eps, int frames, int hw, int C, int groups,
                            float* partial, int chunks, vda_stream_t stream) {
    VDA_REQUIRE(in && out && w && b && partial, "vda_groupnorm: null pointer");
    VDA_REQUIRE(frames > 0 && hw > 0 && C > 0 && groups > 0 && groups <= 64 && C % groups == 0 && C % 8 == 0 && C <= 1024,
                "vda_groupnorm: bad geometry C=%d groups=%d", C, groups);
    VDA_REQUIRE(chunks > 0 && chunks <= hw, "vda_groupnorm: chunks=%d out of range", chunks);
    VDA_REQUIRE(((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 15) == 0, "vda_groupnorm: 16-byte alignment required");
    const int nv = C / 8, rows_par = 256 / nv;
    const size_t smem = ((size_t)rows_par * C * 2 + (size_t)C * 2) * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL((groupnorm_partial_kernel<T>), dim3(chunks, frames), dim3(256), smem, s, in, partial, hw, C, groups, chunks);
    VDA_LAUNCH_CHECK();
    const int rows_per_block = 32;
    hipLaunchKernelGGL((groupnorm_apply_kernel<T>), dim3((hw + rows_per_block - 1) / rows_per_block, frames), dim3(256), 0, s, in, out, w,
                       b, partial, eps, hw, C, groups, chunks, rows_per_block);
    VDA_LAUNCH_CHECK();
    return 0;
}

extern "C" int vda_groupnorm_nhwc_f16(const void* in, void* out, const float* w, const float* b, float eps, int frames, int hw,
                                      int C, int groups, float* partial, int chunks, vda_stream_t stream) {
    return groupnorm_launch<h16>((const h16*)in, (h16*)out, w, b, eps, frames, hw, C, groups, partial, chunks, stream);
}

extern "C" int vda_groupnorm_nhwc_f32(const float* in, float* out, const float* w, const float* b, float eps, int frames, int hw,
                                      int C, int groups, float* partial, int chunks, vda_stream_t stream) {
    return groupnorm_launch<float>(in, out, w, b, eps, frames, hw, C, groups, partial, chunks, stream);
}
