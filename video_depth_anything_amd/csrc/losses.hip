// Validation losses on the device: the arithmetic of the reference's utils/loss_MiDas.py (Loss_ssi, Loss_tgm: what train.py's
// validation pass ranks checkpoints by) and utils/loss.py (the Depth-Anything form of Loss_ssi) restated as streaming fp64 reductions
// in the pattern stated in reduce64.h: fp64 partial rows per block, a fixed LDS tree, rows combined in index order by a one-block
// finisher, ordinary vector stores, no floating-point atomics. Every float32 input is widened exactly to fp64 and all arithmetic is fp64.
// Nothing returns to the host between the passes; the result depends on the block counts, never on timing.
//
//   ssi "lsq" (loss_MiDas.py)   pass 0 {n, sum d, sum y} -> means; pass 1 {sum (d-mu_d)(y-mu_y), sum (d-mu_d)^2} -> s, t;
//                               pass 2 {sum (s*d + t - y)^2} -> per-frame loss and the mean over frames. The centred two-pass form
//                               is the contract: raw moments cancel.
//   ssi "mad" (loss.py)         an exact masked lower median per (frame, tensor) by radix select (below), then {n, sum |d - med_d|,
//                               sum |y - med_y|} -> scales; then one {sum rho, count} PER IMAGE ROW: that file normalises per row.
//   tgm                         per pair of neighbouring frames {n_valid, n_static, sum | |d'-d| - |y'-y| |} over the static pixels.
//
// Planes are H*W*4 bytes apart and H*W may be odd, so a plane's base is only 4-byte aligned (its mask's only 1-byte aligned):
// 16-byte loads would need a scalar head and tail per plane. They are given up: every kernel here reads one dword (and one mask
// byte) per lane, consecutive lanes consecutive pixels, which coalesces whatever the base.
//
// The median is the one kernel of another kind: a radix select over order-preserving uint32 keys of the float32 bits (the sign bit
// flipped for non-negative values, all bits for negative ones), one workgroup of 1024 threads per (frame, tensor) plane, four passes
// of 8 bits. Each pass counts the digits of the keys that still match the prefix into a 256-bin histogram in LDS (one copy per
// wave; integer LDS atomics, so the counts do not depend on the order), scans it, and narrows the prefix and the remaining rank.
// No inter-workgroup synchronisation, no global atomics; after four passes the prefix IS the key of an input element, bit for bit,
// whatever the launch geometry. -0 sorts before +0.
// THIS FILE IS BUILT WITH -ffp-contract=off (build.py PER_FILE): s * d + t rounds twice, as numpy evaluates it.
#include "reduce64.h"

namespace {

constexpr int LS_T = R64_T;
constexpr int LS_STATS = 8;          // doubles per frame in `stats`
// lsq: n, mu_d, mu_y, s, t, loss
enum { ST_N = 0, ST_MU_D = 1, ST_MU_Y = 2, ST_S = 3, ST_T = 4, ST_LOSS = 5 };
// mad: med_d, sc_d, med_y, sc_y, n
enum { SM_MED_D = 0, SM_SC_D = 1, SM_MED_Y = 2, SM_SC_Y = 3, SM_N = 4 };

// ------------------------------------------------------------------------------------------------ ssi, least-squares form
// grid (blocks per plane, frames); row of (frame f, block b) = partial[(f * gridDim.x + b) * K ...], K = 3, 2, 1 for pass 0, 1, 2
template <int PASS>
__global__ void __launch_bounds__(LS_T) loss_lsq_partial_kernel(const float* __restrict__ pred, const float* __restrict__ y,
                                                                const unsigned char* __restrict__ mask, long long px,
                                                                const double* __restrict__ stats, double* __restrict__ partial) {
    constexpr int K = PASS == 0 ? 3 : (PASS == 1 ? 2 : 1);
    const size_t f = blockIdx.y;
    const float* __restrict__ pf = pred + f * px;
    const float* __restrict__ yf = y + f * px;
    const unsigned char* __restrict__ mf = mask ? mask + f * px : nullptr;
    double* row = partial + (f * gridDim.x + blockIdx.x) * K;
    if constexpr (PASS == 0) {
        plane_partial<K>(px, row, [&](long long i, double (&s)[K]) {
            if (!mf || mf[i]) {
                s[0] += 1.0;
                s[1] += (double)pf[i];
                s[2] += (double)yf[i];
            }
        });
    } else if constexpr (PASS == 1) {
        const double mu_d = stats[f * LS_STATS + ST_MU_D], mu_y = stats[f * LS_STATS + ST_MU_Y];
        plane_partial<K>(px, row, [&](long long i, double (&s)[K]) {
            if (!mf || mf[i]) {
                const double dd = (double)pf[i] - mu_d, dy = (double)yf[i] - mu_y;
                s[0] += dd * dy;
                s[1] += dd * dd;
            }
        });
    } else {
        const double sc = stats[f * LS_STATS + ST_S], sh = stats[f * LS_STATS + ST_T];
        plane_partial<K>(px, row, [&](long long i, double (&s)[K]) {
            if (!mf || mf[i]) {
                const double m = sc * (double)pf[i];
                const double r = (m + sh) - (double)yf[i];          // two roundings, then the difference (-ffp-contract=off)
                s[0] += r * r;
            }
        });
    }
}

// One workgroup; thread t owns frames t, t + 256, ...: a frame's block rows are summed in index order.
//   pass 0: stats {n, mu_d, mu_y}, the means over max(n, 1)      pass 1: stats {s, t}, s = num / (den + eps), t = mu_y - s * mu_d
//   pass 2: stats {loss} = sum / max(n, 1); result[0] = the mean over ALL frames (one without a valid pixel counts as 0),
//           result[1 + f] = the frame's loss. The per-thread sums (frames in increasing order) meet in the fixed tree.
template <int PASS>
__global__ void __launch_bounds__(LS_T) loss_lsq_finish_kernel(const double* __restrict__ partial, int nframes, int bpp, double eps,
                                                               double* __restrict__ stats, double* __restrict__ result) {
    constexpr int K = PASS == 0 ? 3 : (PASS == 1 ? 2 : 1);
    double total = 0.0;
    for (int f = threadIdx.x; f < nframes; f += LS_T) {
        double a[K];
        plane_rows_sum(partial, f, bpp, a);
        double* st = stats + (size_t)f * LS_STATS;
        if constexpr (PASS == 0) {
            const double n = a[0] > 1.0 ? a[0] : 1.0;
            st[ST_N] = a[0];
            st[ST_MU_D] = a[1] / n;
            st[ST_MU_Y] = a[2] / n;
        } else if constexpr (PASS == 1) {
            const double s = a[0] / (a[1] + eps);
            const double m = s * st[ST_MU_D];
            st[ST_S] = s;
            st[ST_T] = st[ST_MU_Y] - m;
        } else {
            const double n = st[ST_N] > 1.0 ? st[ST_N] : 1.0;
            const double loss = a[0] / n;
            st[ST_LOSS] = loss;
            result[1 + f] = loss;
            total += loss;
        }
    }
    if constexpr (PASS == 2) {
        total = block_total(total);
        if (threadIdx.x == 0) result[0] = total / (double)nframes;
    }
}

// ------------------------------------------------------------------------------------------------ exact masked lower median
constexpr int SEL_T = 1024;
constexpr int SEL_WAVES = SEL_T / 64;
constexpr int SEL_U = 8;             // values in flight per thread

__device__ __forceinline__ unsigned key_of(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// grid (frames, tensors): tensor 0 = pred, 1 = y; med[tensor * nframes + frame] = element (n - 1) / 2 of the sorted valid values of
// the plane (torch.median's lower median), 0.0f when the plane has no valid pixel. px < 2^31: the counts are 32-bit.
__global__ void __launch_bounds__(SEL_T) loss_median_kernel(const float* __restrict__ pred, const float* __restrict__ y,
                                                            const unsigned char* __restrict__ mask, long long px, int nframes,
                                                            float* __restrict__ med) {
    __shared__ unsigned hist[SEL_WAVES][256];
    __shared__ unsigned scan[2][256];
    __shared__ unsigned sel[2];
    const size_t f = blockIdx.x;
    const float* __restrict__ x = (blockIdx.y ? y : pred) + f * px;
    const unsigned char* __restrict__ m = mask ? mask + f * px : nullptr;
    const int tid = threadIdx.x, wave = tid >> 6;
    unsigned prefix = 0, rank = 0;
#pragma unroll 1
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        for (int e = tid; e < SEL_WAVES * 256; e += SEL_T) (&hist[0][0])[e] = 0u;
        __syncthreads();
        // One workgroup per CU has only its own 16 waves to hide memory latency with, and a value load that waits for its mask byte
        // makes two dependent round trips per pixel (measured: 190 us per pass over 518^2 values). So SEL_U values and mask bytes
        // are loaded unconditionally (every index is inside the plane) before any of them is used. Every thread makes the same
        // number of trips.
        for (long long base = 0; base < px; base += SEL_T * SEL_U) {
            float v[SEL_U];
            unsigned char ok[SEL_U];
#pragma unroll
            for (int u = 0; u < SEL_U; ++u) {
                const long long i = base + (long long)u * SEL_T + tid;
                const bool in = i < px;
                v[u] = in ? x[i] : 0.0f;
                ok[u] = in ? (m ? m[i] : (unsigned char)1) : (unsigned char)0;
            }
#pragma unroll
            for (int u = 0; u < SEL_U; ++u) {
                const unsigned k = key_of(v[u]);
                const bool take = ok[u] && (unsigned)((unsigned long long)k >> (shift + 8)) == prefix;
                // One LDS atomic per lane. A wave-aggregated add (ballot the lanes that share the first lane's digit, one add of
                // their count, two rounds, then the rest singly) was measured and is slower: profiles/losses/README.txt.
                if (take) atomicAdd(&hist[wave][(k >> shift) & 255u], 1u);
            }
        }
        __syncthreads();
        unsigned tot = 0;
        if (tid < 256) {
#pragma unroll
            for (int w = 0; w < SEL_WAVES; ++w) tot += hist[w][tid];
            scan[0][tid] = tot;
        }
        __syncthreads();
        int src = 0;
        for (int off = 1; off < 256; off <<= 1) {              // inclusive scan of the 256 bins (Hillis-Steele, ping-pong)
            if (tid < 256) scan[src ^ 1][tid] = scan[src][tid] + (tid >= off ? scan[src][tid - off] : 0u);
            __syncthreads();
            src ^= 1;
        }
        if (pass == 0) {
            const unsigned n = scan[src][255];
            if (n == 0) {                                      // uniform: every thread reads the same word
                if (tid == 0) med[(size_t)blockIdx.y * nframes + f] = 0.0f;
                return;
            }
            rank = (n - 1) / 2;
        }
        if (tid < 256) {
            const unsigned incl = scan[src][tid], excl = incl - tot;
            if (tot > 0 && rank >= excl && rank < incl) {      // exactly one bin holds the rank
                sel[0] = (unsigned)tid;
                sel[1] = rank - excl;
            }
        }
        __syncthreads();
        prefix = (prefix << 8) | sel[0];
        rank = sel[1];
        __syncthreads();                                       // sel and hist are rewritten by the next pass
    }
    if (tid == 0) med[(size_t)blockIdx.y * nframes + f] = value_of(prefix);
}

// ------------------------------------------------------------------------------------------------ ssi, median / mean-deviation form
// grid (blocks per plane, frames); row = {n, sum |d - med_d|, sum |y - med_y|} at partial[(f * gridDim.x + b) * 3 ...]
__global__ void __launch_bounds__(LS_T) loss_mad_scale_partial_kernel(const float* __restrict__ pred, const float* __restrict__ y,
                                                                      const unsigned char* __restrict__ mask, long long px,
                                                                      const float* __restrict__ med, double* __restrict__ partial) {
    const size_t f = blockIdx.y;
    const float* __restrict__ pf = pred + f * px;
    const float* __restrict__ yf = y + f * px;
    const unsigned char* __restrict__ mf = mask ? mask + f * px : nullptr;
    const double md = (double)med[f], my = (double)med[(size_t)gridDim.y + f];
    plane_partial<3>(px, partial + (f * gridDim.x + blockIdx.x) * 3, [&](long long i, double (&s)[3]) {
        if (!mf || mf[i]) {
            s[0] += 1.0;
            s[1] += fabs((double)pf[i] - md);
            s[2] += fabs((double)yf[i] - my);
        }
    });
}

// stats {med_d, sc_d, med_y, sc_y, n}: sc = sum / n + eps, or eps when the frame has no valid pixel (its medians are 0 already)
__global__ void __launch_bounds__(LS_T) loss_mad_scale_finish_kernel(const double* __restrict__ partial, int nframes, int bpp, double eps,
                                                                     const float* __restrict__ med, double* __restrict__ stats) {
    for (int f = threadIdx.x; f < nframes; f += LS_T) {
        double a[3];
        plane_rows_sum(partial, f, bpp, a);
        double* st = stats + (size_t)f * LS_STATS;
        st[SM_MED_D] = (double)med[f];
        st[SM_MED_Y] = (double)med[(size_t)nframes + f];
        st[SM_SC_D] = a[0] > 0.0 ? a[1] / a[0] + eps : eps;
        st[SM_SC_Y] = a[0] > 0.0 ? a[2] / a[0] + eps : eps;
        st[SM_N] = a[0];
    }
}

// One WAVE per image row (4 rows per block): lane l reads columns l, l + 64, ... of its row, so a wave's loads are 64 consecutive
// dwords of one row - coalesced, whatever W and the row's alignment - and the row's sum never leaves the wave: the lanes' sums meet
// in a fixed xor butterfly. rows[(f * H + r) * 2 ...] = {sum rho, count of valid pixels} of row r of frame f.
__global__ void __launch_bounds__(LS_T) loss_mad_rows_kernel(const float* __restrict__ pred, const float* __restrict__ y,
                                                             const unsigned char* __restrict__ mask, long long nrows, int H, int W,
                                                             const double* __restrict__ stats, double* __restrict__ rows) {
    const long long r = (long long)blockIdx.x * (LS_T / 64) + (threadIdx.x >> 6);
    if (r >= nrows) return;                                    // whole waves leave together; no barrier follows
    const int lane = threadIdx.x & 63;
    const double* st = stats + (size_t)(r / H) * LS_STATS;
    const double md = st[SM_MED_D], sd = st[SM_SC_D], my = st[SM_MED_Y], sy = st[SM_SC_Y];
    const float* __restrict__ pr = pred + (size_t)r * W;
    const float* __restrict__ yr = y + (size_t)r * W;
    const unsigned char* __restrict__ mr = mask ? mask + (size_t)r * W : nullptr;
    double sum = 0.0, cnt = 0.0;
    for (int c = lane; c < W; c += 64) {
        if (!mr || mr[c]) {
            const double a = ((double)pr[c] - md) / sd, b = ((double)yr[c] - my) / sy;
            const double d = a - b;
            sum += d * d;
            cnt += 1.0;
        }
    }
    sum = wave_sum(sum);
    cnt = wave_sum(cnt);
    if (lane == 0) {
        rows[(size_t)r * 2] = sum;
        rows[(size_t)r * 2 + 1] = cnt;
    }
}

// One workgroup. Wave w takes frames w, w + 4, ...: lane l adds rows l, l + 64, ... of the frame (sum / max(count, 1) each) and the
// lanes meet in the fixed xor butterfly; then the frames' sums meet (thread t adds frames t, t + 256, ..., then the fixed tree).
// result[1 + f] = the frame's mean over its H rows, result[0] = the mean over all nframes * H rows. Nothing depends on a launch parameter.
__global__ void __launch_bounds__(LS_T) loss_mad_finish_kernel(const double* __restrict__ rows, int nframes, int H, double* __restrict__ result) {
    const int lane = threadIdx.x & 63;
    for (int f = threadIdx.x >> 6; f < nframes; f += LS_T / 64) {
        double s = 0.0;
        for (int r = lane; r < H; r += 64) {
            const double* row = rows + ((size_t)f * H + r) * 2;
            s += row[0] / (row[1] > 1.0 ? row[1] : 1.0);
        }
        s = wave_sum(s);
        if (lane == 0) result[1 + f] = s;                     // the frame's sum; divided by H below
    }
    __syncthreads();                                           // the frames' sums are read by other threads of this block
    double total = 0.0;
    for (int f = threadIdx.x; f < nframes; f += LS_T) total += result[1 + f];
    total = block_total(total);                                // its barriers also order the reads above before the writes below
    if (threadIdx.x == 0) result[0] = total / ((double)nframes * (double)H);
    for (int f = threadIdx.x; f < nframes; f += LS_T) result[1 + f] = result[1 + f] / (double)H;
}

// ------------------------------------------------------------------------------------------------ temporal gradient matching
// grid (blocks per plane, pairs); pair p = clip p / (N - 1), frames i = p % (N - 1) and i + 1 of it;
// row = {n_valid, n_static, sum} at partial[(p * gridDim.x + b) * 3 ...]
__global__ void __launch_bounds__(LS_T) loss_tgm_partial_kernel(const float* __restrict__ pred, const float* __restrict__ y,
                                                                const unsigned char* __restrict__ mask, int N, long long px,
                                                                double* __restrict__ partial) {
    const size_t p = blockIdx.y;
    const size_t f0 = (p / (N - 1)) * N + p % (N - 1);
    const float* __restrict__ d0 = pred + f0 * px;
    const float* __restrict__ d1 = d0 + px;
    const float* __restrict__ y0 = y + f0 * px;
    const float* __restrict__ y1 = y0 + px;
    const unsigned char* __restrict__ m0 = mask ? mask + f0 * px : nullptr;
    const unsigned char* __restrict__ m1 = mask ? m0 + px : nullptr;
    plane_partial<3>(px, partial + (p * gridDim.x + blockIdx.x) * 3, [&](long long i, double (&s)[3]) {
        if (!m0 || (m0[i] && m1[i])) {
            const double gy = fabs((double)y1[i] - (double)y0[i]);
            s[0] += 1.0;
            if (gy < 0.05) {
                const double gd = fabs((double)d1[i] - (double)d0[i]);
                s[1] += 1.0;
                s[2] += fabs(gd - gy);
            }
        }
    });
}

// One workgroup. result[1 + p] = sum / n_static of pair p (NaN for a skipped pair: no commonly valid or no static pixel),
// result[1 + P + p] = n_static, P = B * (N - 1); then thread t owns clips t, t + 256, ...: a clip's pairs are added in order
// (skipped ones add nothing) and divided by N - 1; result[0] = the mean over the clips.
__global__ void __launch_bounds__(LS_T) loss_tgm_finish_kernel(const double* __restrict__ partial, int B, int N, int bpp, double* __restrict__ result) {
    const int P = B * (N - 1);
    for (int p = threadIdx.x; p < P; p += LS_T) {
        double a[3];
        plane_rows_sum(partial, p, bpp, a);
        result[1 + p] = (a[0] > 0.0 && a[1] > 0.0) ? a[2] / a[1] : __builtin_nan("");
        result[1 + P + p] = a[1];
    }
    __syncthreads();                                           // the pair values are read back by other threads of this block
    double total = 0.0;
    for (int c = threadIdx.x; c < B; c += LS_T) {
        double s = 0.0;
        for (int i = 0; i < N - 1; ++i) {
            const double v = result[1 + (size_t)c * (N - 1) + i];
            if (v == v) s += v;
        }
        total += s / (double)(N - 1);
    }
    total = block_total(total);
    if (threadIdx.x == 0) result[0] = total / (double)B;
}

}  // namespace

// every finisher here is refused what its partial launch is: at most gridDim.y planes
#define LOSS_REQUIRE_PLANES(name, planes, px, bpp) \
    if (check_plane_rows(name, "plane", planes, R64_MAX_PLANES, px, bpp)) return 1

extern "C" int vda_loss_lsq_partial(const float* pred, const float* y, const unsigned char* mask, int nframes, long long px, int pass,
                                    const double* stats, double* partial, int blocks_per_plane, vda_stream_t stream) {
    VDA_REQUIRE(pred && y && stats && partial, "vda_loss_lsq_partial: null pointer");
    LOSS_REQUIRE_PLANES("vda_loss_lsq_partial", nframes, px, blocks_per_plane);
    VDA_REQUIRE(pass >= 0 && pass <= 2, "vda_loss_lsq_partial: pass must be 0, 1 or 2, got %d", pass);
    VDA_REQUIRE(aligned_to(pred, 4) && aligned_to(y, 4) && aligned_to(stats, 8) && aligned_to(partial, 8),
                "vda_loss_lsq_partial: misaligned pointer (the fp64 buffers need 8-byte alignment)");
    const dim3 grid(blocks_per_plane, nframes);
    hipStream_t s = (hipStream_t)stream;
    if (pass == 0)
        hipLaunchKernelGGL(loss_lsq_partial_kernel<0>, grid, dim3(LS_T), 0, s, pred, y, mask, px, stats, partial);
    else if (pass == 1)
        hipLaunchKernelGGL(loss_lsq_partial_kernel<1>, grid, dim3(LS_T), 0, s, pred, y, mask, px, stats, partial);
    else
        hipLaunchKernelGGL(loss_lsq_partial_kernel<2>, grid, dim3(LS_T), 0, s, pred, y, mask, px, stats, partial);
    VDA_LAUNCH_CHECK();
    return 0;
}

extern "C" int vda_loss_lsq_finish(const double* partial, int nframes, int blocks_per_plane, int pass, double eps, double* stats, double* result,
                                   vda_stream_t stream) {
    VDA_REQUIRE(partial && stats && (result || pass != 2), "vda_loss_lsq_finish: null pointer");
    LOSS_REQUIRE_PLANES("vda_loss_lsq_finish", nframes, 1, blocks_per_plane);
    VDA_REQUIRE(pass >= 0 && pass <= 2, "vda_loss_lsq_finish: pass must be 0, 1 or 2, got %d", pass);
    VDA_REQUIRE(aligned_to(partial, 8) && aligned_to(stats, 8) && aligned_to(result, 8),
                "vda_loss_lsq_finish: misaligned pointer (fp64 needs 8-byte alignment)");
    hipStream_t s = (hipStream_t)stream;
    if (pass == 0)
        hipLaunchKernelGGL(loss_lsq_finish_kernel<0>, dim3(1), dim3(LS_T), 0, s, partial, nframes, blocks_per_plane, eps, stats, result);
    else if (pass == 1)
        hipLaunchKernelGGL(loss_lsq_finish_kernel<1>, dim3(1), dim3(LS_T), 0, s, partial, nframes, blocks_per_plane, eps, stats, result);
    else
        hipLaunchKernelGGL(loss_lsq_finish_kernel<2>, dim3(1), dim3(LS_T), 0, s, partial, nframes, blocks_per_plane, eps, stats, result);
    VDA_LAUNCH_CHECK();
    return 0;
}

extern "C" int vda_loss_median(const float* pred, const float* y, const unsigned char* mask, int nframes, long long px, float* med,
                               vda_stream_t stream) {
    VDA_REQUIRE(pred && med, "vda_loss_median: null pointer");
    VDA_REQUIRE(nframes > 0 && nframes <= R64_MAX_PLANES && px > 0, "vda_loss_median: bad size n=%d planes of %lld pixels", nframes, px);
    VDA_REQUIRE(px < (1ll << 31), "vda_loss_median: a plane of %lld pixels is too large (the counts are 32-bit)", px);
    VDA_REQUIRE(aligned_to(pred, 4) && aligned_to(y, 4) && aligned_to(med, 4), "vda_loss_median: misaligned pointer");
    hipLaunchKernelGGL(loss_median_kernel, dim3(nframes, y ? 2 : 1), dim3(SEL_T), 0, (hipStream_t)stream, pred, y, mask, px, nframes, med);
    VDA_LAUNCH_CHECK();
    return 0;
}

extern "C" int vda_loss_mad_scale_partial(const float* pred, const float* y, const unsigned char* mask, int nframes, long long px, const float* med,
                                          double* partial, int blocks_per_plane, vda_stream_t stream) {
    VDA_REQUIRE(pred && y && med && partial, "vda_loss_mad_scale_partial: null pointer");
    LOSS_REQUIRE_PLANES("vda_loss_mad_scale_partial", nframes, px, blocks_per_plane);
    VDA_REQUIRE(aligned_to(pred, 4) && aligned_to(y, 4) && aligned_to(med, 4) && aligned_to(partial, 8),
                "vda_loss_mad_scale_partial: misaligned pointer (the fp64 workspace needs 8-byte alignment)");
    hipLaunchKernelGGL(loss_mad_scale_partial_kernel, dim3(blocks_per_plane, nframes), dim3(LS_T), 0, (hipStream_t)stream, pred, y, mask, px, med,
                       partial);
    VDA_LAUNCH_CHECK();
    return 0;
}

extern "C" int vda_loss_mad_scale_finish(const double* partial, int nframes, int blocks_per_plane, double eps, const float* med, double* stats,
                                         vda_stream_t stream) {
    VDA_REQUIRE(partial && med && stats, "vda_loss_mad_scale_finish: null pointer");
    LOSS_REQUIRE_PLANES("vda_loss_mad_scale_finish", nframes, 1, blocks_per_plane);
    VDA_REQUIRE(aligned_to(partial, 8) && aligned_to(med, 4) && aligned_to(stats, 8),
                "vda_loss_mad_scale_finish: misaligned pointer (fp64 needs 8-byte alignment)");
    hipLaunchKernelGGL(loss_mad_scale_finish_kernel, dim3(1), dim3(LS_T), 0, (hipStream_t)stream, partial, nframes, blocks_per_plane, eps, med, stats);
    VDA_LAUNCH_CHECK();
    return 0;
}

extern "C" int vda_loss_mad_rows(const float* pred, const float* y, const unsigned char* mask, int nframes, int H, int W, const double* stats,
                                 double* rows, vda_stream_t stream) {
    VDA_REQUIRE(pred && y && stats && rows, "vda_loss_mad_rows: null pointer");
    VDA_REQUIRE(nframes > 0 && H > 0 && W > 0, "vda_loss_mad_rows: bad size n=%d frames of %d x %d", nframes, H, W);
    VDA_REQUIRE((long long)nframes * H <= R64_MAX_ROWS, "vda_loss_mad_rows: too many image rows (%d frames x %d)", nframes, H);
    VDA_REQUIRE(aligned_to(pred, 4) && aligned_to(y, 4) && aligned_to(stats, 8) && aligned_to(rows, 8),
                "vda_loss_mad_rows: misaligned pointer (the fp64 buffers need 8-byte alignment)");
    const long long nrows = (long long)nframes * H;
    const int per_block = LS_T / 64;
    hipLaunchKernelGGL(loss_mad_rows_kernel, dim3((unsigned)((nrows + per_block - 1) / per_block)), dim3(LS_T), 0, (hipStream_t)stream, pred, y, mask,
                       nrows, H, W, stats, rows);
    VDA_LAUNCH_CHECK();
    return 0;
}

extern "C" int vda_loss_mad_finish(const double* rows, int nframes, int H, double* result, vda_stream_t stream) {
    VDA_REQUIRE(rows && result, "vda_loss_mad_finish: null pointer");
    VDA_REQUIRE(nframes > 0 && H > 0, "vda_loss_mad_finish: bad size n=%d frames of %d rows", nframes, H);
    VDA_REQUIRE((long long)nframes * H <= R64_MAX_ROWS, "vda_loss_mad_finish: too many image rows (%d frames x %d)", nframes, H);
    VDA_REQUIRE(aligned_to(rows, 8) && aligned_to(result, 8), "vda_loss_mad_finish: misaligned pointer (fp64 needs 8-byte alignment)");
    hipLaunchKernelGGL(loss_mad_finish_kernel, dim3(1), dim3(LS_T), 0, (hipStream_t)stream, rows, nframes, H, result);
    VDA_LAUNCH_CHECK();
    return 0;
}

extern "C" int vda_loss_tgm_partial(const float* pred, const float* y, const unsigned char* mask, int B, int N, long long px, double* partial,
                                    int blocks_per_plane, vda_stream_t stream) {
    VDA_REQUIRE(pred && y && partial, "vda_loss_tgm_partial: null pointer");
    VDA_REQUIRE(B > 0 && N >= 2 && (long long)B * (N - 1) <= R64_MAX_PLANES, "vda_loss_tgm_partial: bad size n=%d clips of %d frames (N >= 2)", B, N);
    LOSS_REQUIRE_PLANES("vda_loss_tgm_partial", B * (N - 1), px, blocks_per_plane);
    VDA_REQUIRE(aligned_to(pred, 4) && aligned_to(y, 4) && aligned_to(partial, 8),
                "vda_loss_tgm_partial: misaligned pointer (the fp64 workspace needs 8-byte alignment)");
    hipLaunchKernelGGL(loss_tgm_partial_kernel, dim3(blocks_per_plane, B * (N - 1)), dim3(LS_T), 0, (hipStream_t)stream, pred, y, mask, N, px, partial);
    VDA_LAUNCH_CHECK();
    return 0;
}

extern "C" int vda_loss_tgm_finish(const double* partial, int B, int N, int blocks_per_plane, double* result, vda_stream_t stream) {
    VDA_REQUIRE(partial && result, "vda_loss_tgm_finish: null pointer");
    VDA_REQUIRE(B > 0 && N >= 2 && (long long)B * (N - 1) <= R64_MAX_PLANES, "vda_loss_tgm_finish: bad size n=%d clips of %d frames (N >= 2)", B, N);
    LOSS_REQUIRE_PLANES("vda_loss_tgm_finish", B * (N - 1), 1, blocks_per_plane);
    VDA_REQUIRE(aligned_to(partial, 8) && aligned_to(result, 8), "vda_loss_tgm_finish: misaligned pointer (fp64 needs 8-byte alignment)");
    hipLaunchKernelGGL(loss_tgm_finish_kernel, dim3(1), dim3(LS_T), 0, (hipStream_t)stream, partial, B, N, blocks_per_plane, result);
    VDA_LAUNCH_CHECK();
    return 0;
}
