// Pack-time fold of ConvTranspose2d(k == stride) into the bias-free 3x3 / pad 1 conv behind it (resize_layers[i] -> layer{i+1}_rn,
// dpt.py:71-82, dpt_temporal.py:78-79): the operands of VDA_EPI_CONVT_FOLD_F16 (vda.h has the algebra).
//
// Output pixel (k*y + py, k*x + px) of the pair reads conv taps (ky, kx) at rows k*y + qy, qy = py + ky - 1 in [-1, k]: input pixel
// y + dy with dy = floor(qy / k), ConvTranspose row phase qy - k*dy. The sums run in fp32 with explicit fmaf in (ky, kx, cm) order -
// one thread per output element, so the order is fixed - and are rounded once.
#include "vda_common.h"

namespace {

// d = floor(q / k) for q in [-1, k], and the row phase q - k*d
__device__ __forceinline__ int fold_split(int q, int k, int& r) {
    const int d = q < 0 ? -1 : (q >= k ? 1 : 0);
    r = q - d * k;
    return d;
}

__global__ void __launch_bounds__(256) fold_convt_weight_kernel(const float* __restrict__ Wt, const float* __restrict__ Wr, h16* __restrict__ Wf, int k,
                                                                int Ci, int Cm, int Co, int Cip) {
    const long long total = (long long)k * k * Co * 9 * Cip;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int ci = (int)(i % Cip);
        const int tap = (int)((i / Cip) % 9);
        const int co = (int)((i / (9ll * Cip)) % Co);
        const int ph = (int)(i / (9ll * Cip * Co));
        const int py = ph / k, px = ph - py * k, dy = tap / 3 - 1, dx = tap % 3 - 1;
        float acc = 0.f;
        if (ci < Ci) {
            for (int ky = 0; ky < 3; ++ky) {
                int ry;
                if (fold_split(py + ky - 1, k, ry) != dy) continue;
                for (int kx = 0; kx < 3; ++kx) {
                    int rx;
                    if (fold_split(px + kx - 1, k, rx) != dx) continue;
                    const float* wr = Wr + ((size_t)co * Cm * 3 + ky) * 3 + kx;              // [co][cm][ky][kx]: stride 9 in cm
                    const float* wt = Wt + ((size_t)ci * Cm * k + ry) * k + rx;              // [ci][cm][ry][rx]: stride k*k in cm
                    for (int cm = 0; cm < Cm; ++cm) acc = fmaf(wr[(size_t)cm * 9], wt[(size_t)cm * k * k], acc);
                }
            }
        }
        Wf[i] = (h16)acc;
    }
}

__global__ void __launch_bounds__(256) fold_convt_bias_kernel(const float* __restrict__ bt, const float* __restrict__ Wr, float* __restrict__ Bc, int k, int Cm,
                                                              int Co) {
    const int total = k * k * 9 * Co;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int co = i % Co, cls = (i / Co) % 9, ph = i / (9 * Co);
    const int py = ph / k, px = ph - py * k, cy = cls / 3, cx = cls - cy * 3;
    float acc = 0.f;
    for (int ky = 0; ky < 3; ++ky) {
        int r;
        const int dy = fold_split(py + ky - 1, k, r);
        if ((dy < 0 && cy == 0) || (dy > 0 && cy == 2)) continue;                            // that tap row is the conv's zero padding
        for (int kx = 0; kx < 3; ++kx) {
            const int dx = fold_split(px + kx - 1, k, r);
            if ((dx < 0 && cx == 0) || (dx > 0 && cx == 2)) continue;
            const float* wr = Wr + ((size_t)co * Cm * 3 + ky) * 3 + kx;
            for (int cm = 0; cm < Cm; ++cm) acc = fmaf(wr[(size_t)cm * 9], bt[cm], acc);
        }
    }
    Bc[i] = acc;
}

}  // namespace

extern "C" int vda_fold_convt_weight(const float* Wt, const float* bt, const float* Wr, void* Wf, float* Bc, int k, int Ci, int Cm, int Co, int Cip,
                                     vda_stream_t stream) {
    VDA_REQUIRE(Wt && bt && Wr && Wf && Bc, "vda_fold_convt_weight: null argument");
    VDA_REQUIRE(k >= 2 && k <= 8 && Ci > 0 && Cm > 0 && Co > 0 && Cip >= Ci, "vda_fold_convt_weight: bad geometry k=%d Ci=%d Cm=%d Co=%d Cip=%d", k, Ci, Cm, Co, Cip);
    VDA_REQUIRE((long long)k * k * Co * 9 * Cip < (1ll << 31), "vda_fold_convt_weight: folded weight too large");
    const long long total = (long long)k * k * Co * 9 * Cip;
    const long long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(fold_convt_weight_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, Wt, Wr, (h16*)Wf, k, Ci, Cm, Co, Cip);
    VDA_LAUNCH_CHECK();
    hipLaunchKernelGGL(fold_convt_bias_kernel, dim3((k * k * 9 * Co + 255) / 256), dim3(256), 0, (hipStream_t)stream, bt, Wr, Bc, k, Cm, Co);
    VDA_LAUNCH_CHECK();
    return 0;
}
