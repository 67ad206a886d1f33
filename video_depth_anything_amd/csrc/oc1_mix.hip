// output_conv1 over refinenet1's 2x upsample with the CHANNEL MIXING done at half resolution (option "oc1_mix", vda.h has the algebra):
//     o1[b, Y, X, :] = b1 + sum over the taps (ky, kx) whose q = (Y + ky - 1, X + kx - 1) lies inside the 2h x 2w map of
//                      bilinear(z[b, :, :, tap, :])(q),            z = r . Wz^T + bz  at h x w, 9 * Fhp channels ordered (tap, cout)
// out_conv (1x1), the align_corners upsample and the 3x3 conv are all linear with no nonlinearity between them, so the 3x3 conv's
// per-tap channel mixing commutes with the interpolation: one dense GEMM at h x w (the planner's kernels, unchanged) and the
// gather-and-add pass below, which has no matrix work.
//
// Pack (vda_fold_oc1_weight): Wz[tap*Fhp + co][ci] = fp16( sum_cm W1[co, cm, tap] * Wo[cm, ci] ), bz[tap*Fhp + co] = sum_cm W1[co, cm, tap] * bo[cm],
// fp32 fmaf in cm order, one thread per element (a fixed order: the handle and the Python engine compare bits). Rows 9 * Fhp .. ldz - 1
// are zero: vda_oc1_mix_ldz pads z's row to a multiple of 256 channels where that costs at most an eighth (ViT-L: 1152 -> 1280), because
// the GEMM planner then takes the 8-phase 256 x 256 tile instead of the one-barrier 256 x 128 one: measured on the 1 x 32 x 148^2 z GEMM
// (K = 256) 0.87 -> 0.70 ms per clip although it stores 11 % more (profiles/r12/oc1_mix). The combine pass never reads the padding.
//
// Combine (vda_oc1_mix_combine_f16): the bilinear weights are separable, so a thread that owns one output column X and 8 channels walks
// down the rows Y of its strip and keeps, per ky, the HORIZONTALLY interpolated and kx-summed rows of the two source rows under
// q.y = Y + ky - 1:
//     S[ky][sy] = sum_kx (1 - fx) z[sy, xa, (ky, kx)] + fx z[sy, xb, (ky, kx)]        (xa, xb, fx of q.x = X + kx - 1; 0 if q.x is outside)
//     o1[Y, X]  = b1 + sum_ky (1 - fy) S[ky][ya] + fy S[ky][yb]                        (ya, yb, fy of q.y; the term is skipped if q.y is outside)
// The source row advances by 0 or 1 per output row (scale (h-1)/(2h-1) < 1/2): a new row costs 6 16-byte loads and 48 FMAs per
// ky, an output row 48 FMAs - 9 loads per 16-byte store instead of the 36 of the tap-by-tap sum, with every corner shared by the
// output rows above and below it in registers and by the neighbouring columns in the vector L1 (the lanes of a pixel read one
// contiguous Fhp * 2-byte run of z, the pixels of a wave are neighbours). Corners are clamped inside their own frame: nothing is
// read from another frame or from behind the buffer. The coordinate arithmetic (scale, floor, clamp, fraction) is conv_up.hip's.
// fp32 throughout, one rounding at the store.
#include "vda_common.h"

namespace {

constexpr int NT = 256;
constexpr int TY = 16;                         // output rows per strip: ~10 source rows per ky instead of 8 (the strip's halo)
// Frames per z buffer (GEMM -> combine per chunk). Measured at ViT-L, 1 x 32 x 518 x 518, in one process (vda_set_option
// "oc1_mix_chunk", profiles/r12/oc1_mix): 1: 49.44, 2: 48.89, 16: 48.58, 32: 48.51 ms per clip; another box 4: 47.98, 8: 47.83, 32: 47.74.
// Nothing is gained from a z that would fit the 256 MB Infinity Cache (4 frames = 224 MB): each halving costs launches and tile rounds.
// 32 = a whole clip of the largest T in one pass, at 1.79 GB of workspace for ViT-L.
#ifndef VDA_OC1_MIX_FRAMES
#define VDA_OC1_MIX_FRAMES 32
#endif
// The option's default: on from this head width up. ViT-S (features 64, z of 288 channels) is slower with it, 7.60 -> 7.79 and
// 7.67 -> 7.90 ms per clip (A/A spread 0.25 ms): its output_conv1 is cheap in conv3x3_up2_kernel and z is 4.5 x the output.
#ifndef VDA_OC1_MIX_MIN_FEATURES
#define VDA_OC1_MIX_MIN_FEATURES 256
#endif

__global__ void __launch_bounds__(256) fold_oc1_weight_kernel(const float* __restrict__ W1, const float* __restrict__ Wo, h16* __restrict__ Wz, int Fh, int Fe,
                                                              int Fhp, int ldz) {
    const long long total = (long long)ldz * Fe;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int ci = (int)(i % Fe);
        const int co = (int)((i / Fe) % Fhp);
        const int tap = (int)(i / ((long long)Fe * Fhp));
        float acc = 0.f;
        if (co < Fh && tap < 9) {
            const float* w1 = W1 + (size_t)co * Fe * 9 + tap;                                // [co][cm][tap]: stride 9 in cm
            for (int cm = 0; cm < Fe; ++cm) acc = fmaf(w1[(size_t)cm * 9], Wo[(size_t)cm * Fe + ci], acc);
        }
        Wz[i] = (h16)acc;
    }
}

__global__ void __launch_bounds__(256) fold_oc1_bias_kernel(const float* __restrict__ W1, const float* __restrict__ bo, float* __restrict__ bz, int Fh, int Fe,
                                                            int Fhp, int ldz) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ldz) return;
    const int co = i % Fhp, tap = i / Fhp;
    float acc = 0.f;
    if (co < Fh && tap < 9) {
        const float* w1 = W1 + (size_t)co * Fe * 9 + tap;
        for (int cm = 0; cm < Fe; ++cm) acc = fmaf(w1[(size_t)cm * 9], bo[cm], acc);
    }
    bz[i] = acc;
}

// grid = (column tiles, row strips, frames); thread -> (column x0 + tid / CL, channels 8 * (tid % CL) ..), CL = Fhp / 8
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(4, 8)))
oc1_mix_combine_kernel(const h16* __restrict__ z, const float* __restrict__ bias, h16* __restrict__ out, int h, int w, int Fhp, int N9, int CL, int TX) {
    const int tid = threadIdx.x;
    const int xi = tid / CL, c8 = (tid - xi * CL) * 8;
    const int H = 2 * h, W = 2 * w;
    const int X = blockIdx.x * TX + xi, y0 = blockIdx.y * TY, b = blockIdx.z;
    if (xi >= TX || X >= W) return;                     // (no barrier below)
    const float ys = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f, xs = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
    // (N9: z's row, ldz >= 9 * Fhp channels)
    // the column's three kx: corners and weights are the same on every row. A q.x outside the map keeps in-frame addresses, weights 0
    int offa[3], offb[3];
    float wa[3], wb[3];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
        const int qx = X + kx - 1;
        const bool ok = (unsigned)qx < (unsigned)W;
        const float sx = xs * (float)min(max(qx, 0), W - 1);
        const int xa = min((int)sx, w - 1), xb = min(xa + 1, w - 1);
        const float fx = sx - (float)xa;
        wa[kx] = ok ? 1.f - fx : 0.f;
        wb[kx] = ok ? fx : 0.f;
        offa[kx] = xa * N9 + kx * Fhp + c8;
        offb[kx] = xb * N9 + kx * Fhp + c8;
    }
    const h16* const zf = z + (size_t)b * h * w * N9;
    // source row sy of tap row ky: the six corners as loaded, then S[ky][sy]
    auto fetch = [&](int ky, int sy, h16x8 (&L)[6]) {
        const h16* const row = zf + (size_t)sy * w * N9 + ky * 3 * Fhp;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            L[2 * kx] = *reinterpret_cast<const h16x8*>(row + offa[kx]);
            L[2 * kx + 1] = *reinterpret_cast<const h16x8*>(row + offb[kx]);
        }
    };
    auto hsum = [&](const h16x8 (&L)[6], float (&S)[8]) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float a = wa[0] * (float)L[0][e];
            a = fmaf(wb[0], (float)L[1][e], a);
            a = fmaf(wa[1], (float)L[2][e], a);
            a = fmaf(wb[1], (float)L[3][e], a);
            a = fmaf(wa[2], (float)L[4][e], a);
            S[e] = fmaf(wb[2], (float)L[5][e], a);
        }
    };
    auto coord = [&](int qy, int& ya, float& fy) {       // uniform over the workgroup
        const float sy = ys * (float)qy;
        ya = __builtin_amdgcn_readfirstlane(min((int)sy, h - 1));      // (a scalar: the row's base address stays in SGPRs)
        fy = sy - (float)ya;
    };
    float SA[3][8], SB[3][8];
    int cur[3];
    // prologue: the two rows under the strip's first q.y per ky (q.y = -1 starts on row 0, where q.y = 0 finds it)
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        h16x8 L[2][6];
        float fy;
        coord(min(max(y0 + ky - 1, 0), H - 1), cur[ky], fy);
        fetch(ky, cur[ky], L[0]);
        fetch(ky, min(cur[ky] + 1, h - 1), L[1]);
        hsum(L[0], SA[ky]);
        hsum(L[1], SB[ky]);
        // one ky's twelve loads in flight at a time, summed before the next ky's are issued: left alone, hipcc sinks the sums into
        // the loop below and carries all 36 loaded vectors there (144 registers, spilled at four waves per SIMD)
#pragma unroll
        for (int e = 0; e < 8; ++e) asm volatile("" : "+v"(SA[ky][e]), "+v"(SB[ky][e]));
        __builtin_amdgcn_sched_barrier(0);
    }
    float bv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) bv[e] = bias ? bias[c8 + e] : 0.f;
    const int y1 = min(y0 + TY, H);
    h16* op = out + (((size_t)b * H + y0) * W + X) * Fhp + c8;
    for (int Y = y0; Y < y1; ++Y, op += (size_t)W * Fhp) {
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = bv[e];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int qy = Y + ky - 1;
            if ((unsigned)qy >= (unsigned)H) continue;       // the conv's zero padding (uniform over the workgroup, as every branch here)
            int ya;
            float fy;
            coord(qy, ya, fy);
            if (ya != cur[ky]) {                             // then ya == cur + 1, and SB holds that row
                h16x8 L[6];
                fetch(ky, min(ya + 1, h - 1), L);
#pragma unroll
                for (int e = 0; e < 8; ++e) SA[ky][e] = SB[ky][e];
                hsum(L, SB[ky]);
                cur[ky] = ya;
            }
            const float uy = 1.f - fy;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = fmaf(fy, SB[ky][e], fmaf(uy, SA[ky][e], acc[e]));
        }
        h16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (h16)acc[e];
        *reinterpret_cast<h16x8*>(op) = o;
    }
}

}  // namespace

extern "C" int vda_oc1_mix_frames(void) { return VDA_OC1_MIX_FRAMES; }

extern "C" int vda_oc1_mix_default(int features) {
    static const int env = getenv("VDA_OC1_MIX") ? atoi(getenv("VDA_OC1_MIX")) : -1;      // (A/B through an unmodified caller)
    return env >= 0 ? env != 0 : features >= VDA_OC1_MIX_MIN_FEATURES;
}

extern "C" int vda_oc1_mix_ldz(int Fhp) {
    const int n = 9 * Fhp, p = (n + 255) / 256 * 256;
    return (p - n) * 8 <= n ? p : n;
}

extern "C" int vda_fold_oc1_weight(const float* W1, const float* Wo, const float* bo, void* Wz, float* bz, int Fh, int Fe, int Fhp, int ldz, vda_stream_t stream) {
    VDA_REQUIRE(W1 && Wo && bo && Wz && bz, "vda_fold_oc1_weight: null argument");
    VDA_REQUIRE(Fh > 0 && Fe > 0 && Fhp >= Fh && Fhp % 8 == 0 && ldz >= 9 * Fhp && ldz % 8 == 0, "vda_fold_oc1_weight: bad geometry Fh=%d Fe=%d Fhp=%d ldz=%d", Fh, Fe, Fhp, ldz);
    VDA_REQUIRE((long long)ldz * Fe < (1ll << 31), "vda_fold_oc1_weight: composed weight too large");
    const long long blocks = ((long long)ldz * Fe + 255) / 256;
    hipLaunchKernelGGL(fold_oc1_weight_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, W1, Wo, (h16*)Wz, Fh, Fe, Fhp, ldz);
    VDA_LAUNCH_CHECK();
    hipLaunchKernelGGL(fold_oc1_bias_kernel, dim3((ldz + 255) / 256), dim3(256), 0, (hipStream_t)stream, W1, bo, bz, Fh, Fe, Fhp, ldz);
    VDA_LAUNCH_CHECK();
    return 0;
}

extern "C" int vda_oc1_mix_combine_f16(const void* z, const float* bias, void* out, int B, int h, int w, int Fhp, int ldz, vda_stream_t stream) {
    VDA_REQUIRE(z && out, "vda_oc1_mix_combine: null pointer");
    VDA_REQUIRE(B > 0 && B <= 65535 && h > 0 && w > 0 && Fhp > 0 && Fhp % 8 == 0 && Fhp <= 8 * NT && ldz >= 9 * Fhp && ldz % 8 == 0,
                "vda_oc1_mix_combine: bad geometry B=%d h=%d w=%d Fhp=%d ldz=%d (multiples of 8, ldz >= 9 Fhp)", B, h, w, Fhp, ldz);
    VDA_REQUIRE(((uintptr_t)z & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)bias & 3) == 0, "vda_oc1_mix_combine: alignment (16 bytes)");
    VDA_REQUIRE((double)h * w * ldz < 2147483647.0 && (double)B * 4 * h * w < 2147483647.0, "vda_oc1_mix_combine: frame exceeds 32-bit element offsets");
    const int CL = Fhp / 8, TX = NT / CL;
    const int gx = (2 * w + TX - 1) / TX, gy = (2 * h + TY - 1) / TY;
    VDA_REQUIRE(gy <= 65535, "vda_oc1_mix_combine: too many row strips");
    hipLaunchKernelGGL(oc1_mix_combine_kernel, dim3(gx, gy, B), dim3(NT), 0, (hipStream_t)stream, (const h16*)z, bias, (h16*)out, h, w, Fhp, ldz, CL, TX);
    VDA_LAUNCH_CHECK();
    return 0;
}
