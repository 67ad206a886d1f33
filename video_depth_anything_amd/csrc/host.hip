// Model handle of the C ABI (include/vda.h, "handle API"): the seam a C / C++ host uses in place of the reference's
//   VideoDepthAnything(**cfg)                      video_depth.py:38-63      -> vda_create
//   .load_state_dict(sd, strict=True)              run.py:46                 -> vda_load_weight x N + vda_finalize_weights
//   .forward(x)                                    video_depth.py:89-93,161-164 -> vda_forward
// The handle owns the weights (raw fp32 as loaded + the kernel layouts packed on the device) and the launch sequence of one
// forward pass over the per-kernel entry points; nothing here computes on the host. The Python facade
// (video_depth_anything_amd/video_depth.py) calls exactly these functions through ctypes.
//
// Workspace: every intermediate lives in ONE caller-visible block. The launch sequence is written once (Run::forward) and
// executed in two modes: a dry pass that only records each named buffer's largest request (this is vda_workspace_bytes and
// the layout), and the real pass that resolves names to offsets in the block. No allocation happens in a steady-state
// vda_forward (layouts, the resampled pos-embed and the fp32 weight pack are created the first time a shape / precision is
// seen), so a steady-state forward is graph-capturable.
#include "vda_common.h"
#include "weight_table.h"
#include <string.h>
#include <algorithm>
#include <exception>
#include <type_traits>
#include <array>
#include <map>
#include <string>
#include <vector>

namespace {

constexpr int GN_GROUPS = 32, TEMPORAL_HEADS = 8;      // (PATCH, POS_GRID, KPATCH, pad64: weight_table.h)
constexpr float ENC_LN_EPS = 1e-6f, GN_EPS = 1e-6f, TMP_LN_EPS = 1e-5f;

#define VDA_TRY(expr)            \
    do {                         \
        const int rc_ = (expr);  \
        if (rc_ != 0) return rc_; \
    } while (0)

#define VDA_HIP(expr)                                                      \
    do {                                                                   \
        const hipError_t e_ = (expr);                                      \
        if (e_ != hipSuccess) {                                            \
            vda_set_error("%s: %s", #expr, hipGetErrorString(e_));         \
            return 2;                                                      \
        }                                                                  \
    } while (0)

// ------------------------------------------------------------------ weight packing (device)
template <typename T>
__global__ void pack_matrix_kernel(const float* __restrict__ src, T* __restrict__ dst, int N, int K, int Npad, int Kpad) {
    const size_t total = (size_t)Npad * Kpad;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int n = (int)(i / Kpad), k = (int)(i - (size_t)n * Kpad);
        dst[i] = (n < N && k < K) ? (T)src[(size_t)n * K + k] : (T)0.f;
    }
}
// Conv2d weight [Co,Ci,3,3] -> [Copad, (ky,kx,ci) = 9*Cipad]
template <typename T>
__global__ void pack_conv3x3_kernel(const float* __restrict__ src, T* __restrict__ dst, int Co, int Ci, int Copad, int Cipad) {
    const size_t total = (size_t)Copad * 9 * Cipad;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int ci = (int)(i % Cipad);
        const size_t t = i / Cipad;
        const int tap = (int)(t % 9), co = (int)(t / 9);
        dst[i] = (co < Co && ci < Ci) ? (T)src[((size_t)co * Ci + ci) * 9 + tap] : (T)0.f;
    }
}
// ConvTranspose2d (k == stride) weight [Ci,Co,k,k] -> [(ky,kx,co) = k*k*cpad, ci = cpad]
template <typename T>
__global__ void pack_convt_kernel(const float* __restrict__ src, T* __restrict__ dst, int Ci, int Co, int k, int cpad) {
    const size_t total = (size_t)k * k * cpad * cpad;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int ci = (int)(i % cpad);
        const size_t t = i / cpad;
        const int co = (int)(t % cpad), tap = (int)(t / cpad);
        dst[i] = (co < Co && ci < Ci) ? (T)src[((size_t)ci * Co + co) * k * k + tap] : (T)0.f;
    }
}
__global__ void expand_convt_bias_kernel(const float* __restrict__ b, float* __restrict__ dst, int Co, int kk, int cpad) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= kk * cpad) return;
    const int co = i % cpad;
    dst[i] = co < Co ? b[co] : 0.f;
}
// GEGLU proj [2n, K], rows [value(n) | gate(n)] -> interleaved [16 value | 16 gate] per 32 rows (K = 1: the bias)
template <typename T>
__global__ void pack_geglu_kernel(const float* __restrict__ src, T* __restrict__ dst, int n, int K) {
    const size_t total = (size_t)2 * n * K;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int R = (int)(i / K), k = (int)(i - (size_t)R * K);
        const int blk = R >> 5, within = R & 31;
        const int srow = within < 16 ? blk * 16 + within : n + blk * 16 + (within - 16);
        dst[i] = (T)src[(size_t)srow * K + k];
    }
}

inline unsigned grid_for(size_t items) {
    const size_t b = (items + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 65535 ? 65535 : b));
}

#ifndef VDA_LN_FOLD_DEFAULT
#define VDA_LN_FOLD_DEFAULT 1
#endif

// A forward whose split residual stream left fp16's range has no valid result: its depth is overwritten with NaN so that the
// failure is visible in the data as well as in the status (a clamped ReLU would otherwise turn NaN activations into zeros).
// ... and the report goes to a STICKY word in pinned host memory (written only when set: a later, clean forward cannot erase it however
// far the host runs ahead of the device).
__global__ void __launch_bounds__(256) poison_on_overflow_kernel(const int* __restrict__ flag, float* __restrict__ depth, long long n,
                                                                 volatile int* __restrict__ host_report) {
    if (*flag == 0) return;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) depth[i] = __builtin_nanf("");
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *host_report = 1;
        __threadfence_system();
    }
}

struct Raw {
    float* d = nullptr;       // the tensor as loaded (its shape: vda_model::spec)
};

// Optional per-launch timing of the GEMM / conv launches of vda_forward (bench.py's roofline): every `every`-th launch of each
// (shape, epilogue) is bracketed by two events on the launch stream; all launches are counted. Bracketing every launch costs
// ~1 ms per ViT-L clip in event packets (measured), 1 in 4 keeps the timed region honest.
struct ProfSample {
    std::string name;
    double flops;
    hipEvent_t e0, e1;
};
struct Profile {
    int every = 0;
    double min_flops = 0.0;                  // launches below it are counted, never bracketed (vda_set_option "profile_min_gflop")
    std::map<std::array<int, 5>, int> seen;
    std::map<std::string, std::pair<long long, double>> launches;      // kernel name -> (launches, algorithmic flops)
    std::vector<ProfSample> samples;
};

struct Layout {
    int gemm_launches = 0;                                      // GEMM / conv launches of one forward (dynamic-schedule counters)
    std::map<std::string, std::pair<size_t, size_t>> bufs;      // name -> (offset, bytes)
    std::vector<std::string> order;
    size_t total = 0;
};

}  // namespace

struct vda_model {
    vda_config cfg;
    int device = 0;
    std::vector<WEntry> table;                // csrc/weight_table.h: every checkpoint tensor and how it is packed
    std::map<std::string, std::vector<int64_t>> spec;      // its name -> shape
    std::map<std::string, Raw> raw;
    std::map<std::string, void*> mat[2];      // packed matrices per precision
    std::map<std::string, float*> vec;        // fp32 vectors (biases, affine, LayerScale, PE), shared by both precisions
    bool finalized = false, packed[2] = {false, false};
    float oc3_bias = 0.f;
    void* zero_page = nullptr;
    std::map<std::pair<int, int>, float*> pos_cache;
    void* ws = nullptr;
    int64_t ws_bytes = 0;
    bool ws_owned = false;
    std::map<std::array<int, 5>, Layout> layouts;
    std::vector<void*> owned;                 // every hipMalloc of the handle
    int ocp[4] = {0, 0, 0, 0}, Fhp = 0;
    std::array<int, 5> last_key = {0, 0, 0, 0, -1};
    Profile prof;
    int residual_in_ln = 0;                   // vda_set_option("residual_in_ln"): see Run::block_deferred (off: measured slower end to end)
    int dyn_sched = 0;                        // vda_set_option("dyn_sched"): dynamic tile draw in the 8-phase GEMM (vda_gemm_args.sched); for
                                              // processes that share the GPU with communication kernels (multi-rank runs turn it on)
    int ln_fold = VDA_LN_FOLD_DEFAULT;        // vda_set_option("ln_fold"): LayerNorm folded into the encoder GEMMs either side of it (fp16 path)
    int oc1_fused = 1;                        // vda_set_option("oc1_fused"): refinenet1's 2x upsample folded into output_conv1 (fp16 path)
    int head_overlap = 0;                     // vda_set_option("head_overlap"): the head's tap-0..2 work on a side stream under the last encoder blocks.
                                              // OFF: in-process A/B the sign depends on the box (+0.8 % ViT-L / +1.5 % ViT-S on a 52.1 ms box,
                                              // -0.3 .. -0.5 % on a 50.0 ms box; two clips in flight -0.4 %), profiles/r04/head_overlap_ab.txt
    struct Side {
        hipStream_t stream = nullptr;
        hipEvent_t fork = nullptr, join = nullptr, join2 = nullptr;      // (join2: the lane's second join under head_lanes)
    };
    std::map<hipStream_t, Side> sides;        // one side stream + event pair per caller stream (two forwards may be in flight on two)
    // vda_set_option("enc_split") (environment default VDA_ENC_SPLIT): the fp16 ln_fold encoder runs as two frame halves, half B on a
    // LANE stream (one per caller stream) forked after the token rows exist and joined back before the head - see Run::encoder
    // Not while a forward of this handle on ANOTHER caller stream is still in flight (two windows / clips in flight already fill each
    // other's idle time; splitting them too measured -4 %): `tails` holds the end of the last forward enqueued on each caller stream.
    int enc_split = 1;
    std::map<hipStream_t, Side> lanes;
    std::map<hipStream_t, hipEvent_t> tails;
    // vda_set_option("head_lanes") (environment default VDA_HEAD_LANES): after the encoder's join the head's branches that do not
    // depend on tap 3 (head_early and conv1 of resConfUnit1 in refinenets 3, 2, 1) run on the LANE stream beside the chain
    // proj3 .. motion module 2 on the caller's stream - see Run::head. Same exclusions as enc_split, and not together with
    // head_overlap. ON: in-process A/B, both orders, ViT-L 51.32 -> 50.36 and 51.41 -> 50.47 ms per clip (A/A spread 0.16 ms), ViT-S
    // 8.23 -> 7.83 and 8.20 -> 7.89 ms (A/A spread 0.14 ms); profiles/r10/head_lanes/.
    int head_lanes = 1;
    // vda_set_option("convt_fold") (environment default VDA_CONVT_FOLD): resize_layers[i] + layer{i+1}_rn (i = 0, 1) as one folded
    // GEMM on the projection's grid (VDA_EPI_CONVT_FOLD_F16) where Run::fold_level says so. folded[i]: what the LAST forward did at
    // level i - its "l1" / "l2" were then never written and vda_debug_copy rebuilds them. DESIGN section 4 [r11].
    int convt_fold = 1;
    bool folded[2] = {false, false};
    // vda_set_option("oc1_mix") (environment default VDA_OC1_MIX): refinenet1's out_conv + output_conv1 over the 2x upsample as one GEMM
    // at half resolution (z, 9 * Fhp channels) + vda_oc1_mix_combine_f16, per chunk of oc1_mix_chunk frames out of one z buffer.
    // mixed: what the LAST forward did - its "p1c" was then never written and vda_debug_copy rebuilds it. DESIGN section 4 [r12].
    int oc1_mix = 0;
    int oc1_mix_chunk = 0;
    bool mixed = false;
    int mlp_fused = 0;                        // vda_set_option("mlp_fused"): fc1 + GELU + fc2 + residual in one kernel where built (D = 384; needs ln_fold).
                                              // OFF: measured slower than the two GEMM launches (ViT-S clip 8.69 -> 9.00 ms, mlp_fused.hip's header)
    // Split-stream overflow report (ln_fold): one sticky word in pinned host memory, set by the device at the end of a forward whose
    // flag was raised; vda_forward_status / the next vda_forward read (and clear) it.
    volatile int32_t* ovf_host = nullptr;     // hipHostMalloc'ed, device-visible
};

namespace {

int dev_alloc(vda_model* h, size_t bytes, void** out) {
    void* p = nullptr;
    VDA_HIP(hipMalloc(&p, bytes < 256 ? 256 : bytes));
    h->owned.push_back(p);
    *out = p;
    return 0;
}

int require_device(const vda_model* h, const char* what) {
    int dev = -1;
    VDA_HIP(hipGetDevice(&dev));
    if (dev != h->device) {
        vda_set_error("%s: the handle lives on device %d but device %d is current (one handle per device; make it current)", what, h->device, dev);
        return 1;
    }
    return 0;
}

// use_bn: BatchNorm2d in inference is y = (x - running_mean) / sqrt(running_var + 1e-5) * weight + bias per channel, directly behind a
// conv (util/blocks.py:80-81,85-86): folded into it, W'[co] = W[co] * s, b' = (b - running_mean) * s + bias, s = weight / sqrt(var + eps)
__global__ void __launch_bounds__(256) fold_bn_kernel(const float* __restrict__ W, const float* __restrict__ b, const float* __restrict__ g,
                                                      const float* __restrict__ beta, const float* __restrict__ rm, const float* __restrict__ rv,
                                                      float* __restrict__ Wo, float* __restrict__ bo, int Co, int per_co) {
    const long long n = (long long)Co * per_co;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int co = (int)(i / per_co);
        const float sc = g[co] / sqrtf(rv[co] + 1e-5f);
        Wo[i] = W[i] * sc;
        if (i - (long long)co * per_co == 0) bo[co] = (b[co] - rm[co]) * sc + beta[co];
    }
}

// ---- packing of one precision (T = h16 / float); vectors are packed once with the first precision (`vecs`)
// One row of the table (csrc/weight_table.h) from its fp32 source; the first W_ROWS tensor of a key allocates the key's whole block.
template <typename T>
int pack_entry(vda_model* h, int prec, bool vecs, const WEntry& e, const float* src) {
    if (e.kind == W_NONE || (e.is_vec() && !vecs)) return 0;
    hipStream_t s = nullptr;
    const size_t elems = e.packed_elems();
    void* d = nullptr;
    const auto shared = h->mat[prec].find(e.key);
    if (e.kind == W_ROWS && shared != h->mat[prec].end()) d = shared->second;
    else VDA_TRY(dev_alloc(h, elems * (e.is_vec() ? sizeof(float) : sizeof(T)), &d));
    if (e.is_vec()) h->vec[e.key] = (float*)d;
    else h->mat[prec][e.key] = d;
    const int N = e.N(), K = e.K();
    const dim3 grid(grid_for(e.kind == W_ROWS ? (size_t)N * e.kpad : elems)), block(256);
    switch (e.kind) {
    case W_NONE: break;
    case W_VEC: hipLaunchKernelGGL((pack_matrix_kernel<float>), grid, block, 0, s, src, (float*)d, 1, K, 1, e.kpad); break;
    case W_MAT: hipLaunchKernelGGL((pack_matrix_kernel<T>), grid, block, 0, s, src, (T*)d, N, K, e.npad, e.kpad); break;
    case W_ROWS: hipLaunchKernelGGL((pack_matrix_kernel<T>), grid, block, 0, s, src, (T*)d + (size_t)e.row * e.kpad, N, K, N, e.kpad); break;
    case W_CONV3: hipLaunchKernelGGL((pack_conv3x3_kernel<T>), grid, block, 0, s, src, (T*)d, N, (int)e.shape[1], e.npad, e.kpad); break;
    case W_CONVT: hipLaunchKernelGGL((pack_convt_kernel<T>), grid, block, 0, s, src, (T*)d, N, (int)e.shape[1], (int)e.shape[2], e.npad); break;
    case W_CONVT_BIAS: hipLaunchKernelGGL(expand_convt_bias_kernel, grid, block, 0, s, src, (float*)d, K, e.npad / e.kpad, e.kpad); break;
    case W_GEGLU: hipLaunchKernelGGL((pack_geglu_kernel<T>), grid, block, 0, s, src, (T*)d, N / 2, K); break;
    case W_GEGLU_BIAS: hipLaunchKernelGGL((pack_geglu_kernel<float>), grid, block, 0, s, src, (float*)d, K / 2, 1); break;
    }
    return 0;
}

// The weights made of SEVERAL tensors, behind the table's rows: the fp16 path's folds (LayerNorm into the Linear behind it, fc2 permuted
// for the fused MLP, options oc1_mix and convt_fold) and, in both precisions, use_bn's BatchNorm folded into the resConfUnit convs.
template <typename T>
int pack_derived(vda_model* h, int prec, bool vecs) {
    const vda_config& c = h->cfg;
    hipStream_t s = nullptr;
    auto raw = [&](const std::string& k) -> const float* { return h->raw.at(k).d; };
    auto n = [](int i) { return std::to_string(i); };
    const int D = c.embed_dim, Fe = c.features, Fh = Fe / 2, Fhp = h->Fhp;
    const int *oc = c.out_channels, *ocp = h->ocp;
    const std::string hd = "head.", sc = hd + "scratch.";
    if constexpr (std::is_same<T, h16>::value) {
        auto mat = [&](const std::string& key, size_t elems, T** out) -> int {
            void* p = nullptr;
            VDA_TRY(dev_alloc(h, elems * sizeof(T), &p));
            h->mat[prec][key] = p;
            *out = (T*)p;
            return 0;
        };
        auto vec = [&](const std::string& key, size_t elems, float** out) -> int {
            void* p = nullptr;
            VDA_TRY(dev_alloc(h, elems * sizeof(float), &p));
            h->vec[key] = *out = (float*)p;
            return 0;
        };
        // (the head's composed weights first: their kernels are the long ones, and run while the host allocates for the blocks)
        // option oc1_mix: output_conv1 composed with refinenet1's out_conv (vda_fold_oc1_weight), fp16 path only. oc1.w / .b and
        // ref1.out.* stay: the fp32 path, the option's off setting and vda_debug_copy's rebuild of "p1c" run them.
        {
            T* d = nullptr;
            float* bp = nullptr;
            const int ldz = vda_oc1_mix_ldz(Fhp);
            VDA_TRY(mat("oc1.mix.w", (size_t)ldz * Fe, &d));
            VDA_TRY(vec("oc1.mix.b", ldz, &bp));
            VDA_TRY(vda_fold_oc1_weight(raw(sc + "output_conv1.weight"), raw(sc + "refinenet1.out_conv.weight"), raw(sc + "refinenet1.out_conv.bias"), d, bp, Fh, Fe, Fhp, ldz, s));
        }
        // option convt_fold: resize_layers[i] composed with layer{i+1}_rn (vda_fold_convt_weight), fp16 path only. resize{i}.w / .b
        // stay: the fp32 path, the option's off setting and vda_debug_copy's rebuild of "l1" / "l2" run the unfused pair.
        for (int i = 0; i < 2; ++i) {
            const int kk = i == 0 ? 4 : 2;
            const std::string k = "rn" + n(i + 1) + ".fold", rs = hd + "resize_layers." + n(i);
            T* d = nullptr;
            float* bp = nullptr;
            VDA_TRY(mat(k + ".w", (size_t)kk * kk * Fe * 9 * ocp[i], &d));
            VDA_TRY(vec(k + ".b", (size_t)kk * kk * 9 * Fe, &bp));
            VDA_TRY(vda_fold_convt_weight(raw(rs + ".weight"), raw(rs + ".bias"), raw(sc + "layer" + n(i + 1) + "_rn.weight"), d, bp, kk, oc[i], oc[i], Fe, ocp[i], s));
        }
        for (int i = 0; i < c.depth; ++i) {
            const std::string b = "pretrained.blocks." + n(i) + ".", k = "b" + n(i) + ".";
            // LayerNorm folded into the Linear behind it (vda.h, VDA_EPI_LN_*): W * diag(ln_w) in fp16, c1 = its row sums, c2 = b + W.ln_b
            const char* pairs[2][2] = {{"attn.qkv", "norm1"}, {"mlp.fc1", "norm2"}};
            for (int j = 0; j < 2; ++j) {
                const std::string lk = pairs[j][0], nk = pairs[j][1];
                const int out = (int)h->spec.at(b + lk + ".weight")[0];
                T* d = nullptr;
                float *c1 = nullptr, *c2 = nullptr;
                VDA_TRY(mat(k + lk + ".weight.ln", (size_t)out * D, &d));
                VDA_TRY(vec(k + lk + ".c1", out, &c1));
                VDA_TRY(vec(k + lk + ".c2", out, &c2));
                VDA_TRY(vda_fold_ln_weight(raw(b + lk + ".weight"), raw(b + lk + ".bias"), raw(b + nk + ".weight"), raw(b + nk + ".bias"), d, c1, c2, out, D, s));
            }
            // the fused MLP kernel (vda_mlp_fused_f16; widths it is built for) takes fc2's weight with its hidden columns permuted
            if (vda_mlp_fused_supported(D, 4 * D)) {
                T* d = nullptr;
                VDA_TRY(mat(k + "mlp.fc2.weight.perm", (size_t)D * 4 * D, &d));
                VDA_TRY(vda_mlp_permute_w2_f16(h->mat[prec].at(k + "mlp.fc2.weight"), d, D, 4 * D, s));
            }
        }
    }
    if (!c.use_bn) return 0;
    for (int i = 1; i <= 4; ++i)
        for (int u = 1; u <= 2; ++u)
            for (int cc = 1; cc <= 2; ++cc) {
                // the folded fp32 conv replaces the raw one for packing (kept under its own key: a re-pack in the other
                // precision finds it again; a re-load of the state dict overwrites it)
                const std::string r = sc + "refinenet" + n(i) + ".resConfUnit" + n(u), rn = r + ".conv" + n(cc), bn = r + ".bn" + n(cc) + ".";
                const std::string kn = "ref" + n(i) + ".rcu" + n(u) + ".c" + n(cc);
                const WEntry w{rn + ".weight.bn", h->spec.at(rn + ".weight"), W_CONV3, kn + ".w", Fe, Fe, 0};
                const WEntry b{rn + ".bias.bn", h->spec.at(rn + ".bias"), W_VEC, kn + ".b", 1, Fe, 0};
                Raw& fw = h->raw[w.name];
                Raw& fb = h->raw[b.name];
                if (fw.d == nullptr) {
                    void *pw = nullptr, *pb = nullptr;
                    VDA_TRY(dev_alloc(h, (size_t)w.numel() * sizeof(float), &pw));
                    VDA_TRY(dev_alloc(h, (size_t)b.numel() * sizeof(float), &pb));
                    fw.d = (float*)pw, fb.d = (float*)pb;
                }
                hipLaunchKernelGGL(fold_bn_kernel, dim3(grid_for((size_t)w.numel())), dim3(256), 0, s, raw(rn + ".weight"), raw(rn + ".bias"), raw(bn + "weight"),
                                   raw(bn + "bias"), raw(bn + "running_mean"), raw(bn + "running_var"), fw.d, fb.d, w.N(), w.K());
                VDA_TRY(pack_entry<T>(h, prec, vecs, w, fw.d));
                VDA_TRY(pack_entry<T>(h, prec, vecs, b, fb.d));
            }
    return 0;
}

template <typename T>
int pack_all(vda_model* h, int prec) {
    const bool vecs = h->vec.empty();
    for (const WEntry& e : h->table) VDA_TRY(pack_entry<T>(h, prec, vecs, e, h->raw.at(e.name).d));
    VDA_TRY(pack_derived<T>(h, prec, vecs));
    VDA_HIP(hipGetLastError());
    VDA_HIP(hipStreamSynchronize(nullptr));
    h->packed[prec] = true;
    return 0;
}

// a side / lane stream and its events, created at first use
int open_side(vda_model::Side& sd) {
    if (sd.stream != nullptr) return 0;
    VDA_HIP(hipStreamCreateWithFlags(&sd.stream, hipStreamNonBlocking));
    VDA_HIP(hipEventCreateWithFlags(&sd.fork, hipEventDisableTiming));
    VDA_HIP(hipEventCreateWithFlags(&sd.join, hipEventDisableTiming));
    VDA_HIP(hipEventCreateWithFlags(&sd.join2, hipEventDisableTiming));
    return 0;
}

// ------------------------------------------------------------------ one forward pass
// the derived sizes of one clip: token grid, token rows, the head's four map sizes and widths
struct Geom {
    int B, T, H, W, BT, ph, pw, P, D, NH, Nt, rows, h1, w1, h2, w2, h4, w4, Fe, Fhp;
    Geom(const vda_model* h, int B_, int T_, int H_, int W_) : B(B_), T(T_), H(H_), W(W_) {
        BT = B * T, ph = H / PATCH, pw = W / PATCH, P = ph * pw, D = h->cfg.embed_dim, NH = h->cfg.num_heads, Nt = P + 1, rows = BT * Nt;
        h1 = 4 * ph, w1 = 4 * pw, h2 = 2 * ph, w2 = 2 * pw, h4 = (ph - 1) / 2 + 1, w4 = (pw - 1) / 2 + 1, Fe = h->cfg.features, Fhp = h->Fhp;
    }
};

struct Run {
    vda_model* h;
    int prec;                 // VDA_PREC_F16 / VDA_PREC_F32
    // Sizing pass: record buffer requests, launch nothing. The layout must not depend on an option that can change between two
    // forwards (head_overlap, head_lanes, convt_fold, oc1_mix): wherever such an option picks between two forms, the dry pass
    // requests the buffers of BOTH and counts the launches of the larger one - the members below say `dry` where they do so.
    bool dry;
    Layout* lay;
    hipStream_t s;            // the launch stream and ...
    std::string sp;           // ... the prefix of the helpers' scratch names below, switched together and only by `On`. head_early
                              // takes "e." in every configuration (one layout, whichever stream it runs on) and so does everything
                              // option head_lanes issues to the lane stream: work there never shares a block with the caller's stream's
    const Geom g;
    const size_t ab;          // bytes per activation element
    int32_t* sched = nullptr; // dynamic-schedule counters: 8 per GEMM launch of the forward, zeroed at its start
    int nsched = 0;           // launches so far (dry pass: the count that sizes the block)

    Run(vda_model* h_, int prec_, bool dry_, Layout* lay_, hipStream_t s_, int B, int T, int H, int W)
        : h(h_), prec(prec_), dry(dry_), lay(lay_), s(s_), g(h_, B, T, H, W), ab(prec_ == VDA_PREC_F32 ? 4 : 2) {}
    // launches go to `stream`, scratch names take `prefix`, until the scope ends (however it ends)
    struct On {
        Run& r;
        const hipStream_t s;
        const std::string sp;
        On(Run& r_, hipStream_t stream, const std::string& prefix) : r(r_), s(r_.s), sp(r_.sp) { r.s = stream, r.sp = prefix; }
        ~On() { r.s = s, r.sp = sp; }
    };

    void* buf(const std::string& name, size_t elems, size_t esize) {
        const size_t bytes = (elems * esize + 255) & ~(size_t)255;
        if (dry) {
            auto it = lay->bufs.find(name);
            if (it == lay->bufs.end()) {
                lay->bufs[name] = {0, bytes};
                lay->order.push_back(name);
            } else if (it->second.second < bytes) {
                it->second.second = bytes;
            }
            return (void*)(uintptr_t)256;          // never dereferenced: every launch helper returns early in a dry pass
        }
        return (char*)h->ws + lay->bufs.at(name).first;
    }
    void* act(const std::string& name, size_t elems) { return buf(name, elems, ab); }
    float* f32(const std::string& name, size_t elems) { return (float*)buf(name, elems, 4); }
    // packed weights by key; a dry pass may run before this precision's pack exists and never dereferences them
    const void* W(const std::string& k) const { return dry ? nullptr : h->mat[prec].at(k); }
    const float* V(const std::string& k) const { return dry ? nullptr : h->vec.at(k); }

    // One GEMM = the records of its plan (vda_gemm_plan: a large dense GEMM runs as two launches when that quantises better on this
    // device). Planned HERE rather than inside vda_gemm_f16 so that each launch has its own dynamic-schedule counters and its own
    // profile bracket (kernel name, FLOPs of its rows). m_plan != 0: `a` is a frame half of enc_split, planned as the m_plan-row GEMM of
    // the whole clip would be and run as ONE launch: the remainder launch pays only when the GEMM has the chip to itself, and beside
    // the other half it lost (ViT-L fc2, in-process A/B: 50.52 -> 50.13 ms per clip without it, profiles/r05).
    int gemm(vda_gemm_args a, int m_plan = 0) {
        if (a.lda == 0) a.lda = a.K;
        if (a.ldc == 0) a.ldc = a.N;
        a.zero_page = h->zero_page;
        if (prec == VDA_PREC_F32) return dry ? 0 : bracket(a, nullptr);
        vda_gemm_plan_t plan;
        const bool dyn = h->dyn_sched && sched != nullptr;      // (inside a forward that laid the counters out: not vda_debug_copy's rebuilds)
        if (dyn) a.sched = sched;                   // (planned as a dynamic-draw launch; each record gets its own counters below)
        VDA_TRY(vda_gemm_plan(&a, m_plan, 0, 1, &plan));
        for (int i = 0; i < plan.n; ++i) {
            if (dyn) a.sched = sched + 8 * nsched++;
            if (!dry) VDA_TRY(bracket(a, &plan.rec[i]));
        }
        return 0;
    }
    // one launch (rec == nullptr: the fp32 kernel) inside its profile bracket
    int bracket(const vda_gemm_args& a, const vda_gemm_launch* rec) {
        auto run = [&] { return rec == nullptr ? vda_gemm_f32(&a, s) : vda_gemm_f16_record(&a, rec, s); };
        Profile& pf = h->prof;
        if (pf.every <= 0) return run();
        const int rows = rec ? rec->rows : a.M;
        const std::array<int, 5> key = {rows, a.N, a.K, a.epilogue, a.a_mode};
        const int n = pf.seen[key]++;
        const double flops = 2.0 * rows * a.N * a.K;
        const bool timed = n % pf.every == 0 && flops >= pf.min_flops;
        ProfSample smp;
        if (timed) {
            VDA_HIP(hipEventCreate(&smp.e0));
            VDA_HIP(hipEventCreate(&smp.e1));
            VDA_HIP(hipEventRecord(smp.e0, s));
        }
        VDA_TRY(run());
        char kname[64] = "gemm_f32_kernel";
        if (rec) vda_gemm_launch_name(rec, kname, sizeof(kname));
        const std::string name = kname;
        auto& tot = pf.launches[name];
        tot.first += 1;
        tot.second += flops;
        if (timed) {
            VDA_HIP(hipEventRecord(smp.e1, s));
            smp.name = name;
            smp.flops = flops;
            pf.samples.push_back(smp);
        }
        return 0;
    }
    int dense(const void* A, const void* Wm, void* out, int epi, int M, int N, int K, const float* bias = nullptr, const void* res = nullptr,
              const float* gamma = nullptr, int ldc = 0, int m_plan = 0) {
        vda_gemm_args a = {};
        a.A = A, a.W = Wm, a.out = out, a.bias = bias, a.res = res, a.gamma = gamma;
        a.M = M, a.N = N, a.K = K, a.ldc = ldc, a.a_mode = VDA_A_DENSE, a.epilogue = epi;
        return gemm(a, m_plan);
    }
    int conv3x3(const void* x, const std::string& wname, void* out, int B, int H, int Wd, int Cin, int Cout, int epi, int stride,
                const float* bias, bool relu_in = false, const void* res = nullptr, const void* res2 = nullptr) {
        const int Ho = (H - 1) / stride + 1, Wo = (Wd - 1) / stride + 1;
        vda_gemm_args a = {};
        a.A = x, a.W = W(wname), a.out = out, a.bias = bias, a.res = res, a.res2 = res2;
        a.M = B * Ho * Wo, a.N = Cout, a.K = 9 * Cin, a.a_mode = VDA_A_CONV3X3, a.epilogue = epi, a.relu_in = relu_in ? 1 : 0;
        a.cB = B, a.cH = H, a.cW = Wd, a.cCin = Cin, a.cHo = Ho, a.cWo = Wo, a.cStride = stride;
        return gemm(a);
    }
    // resize_layers[i] (ConvTranspose2d, k == stride; dpt.py:71-82) on the ph x pw projection t -> out [B, k*ph, k*pw, C]
    int convt(const void* t, int i, void* out) {
        const std::string k = "resize" + std::to_string(i);
        const int B = g.BT, ph = g.ph, pw = g.pw, C = h->ocp[i], kk = i == 0 ? 4 : 2;
        vda_gemm_args a = {};
        a.A = t, a.W = W(k + ".w"), a.out = out, a.bias = V(k + ".b");
        a.M = B * ph * pw, a.N = kk * kk * C, a.K = C, a.ldc = C, a.a_mode = VDA_A_DENSE, a.epilogue = VDA_EPI_CONVT_F16;
        a.tK = kk, a.tH = ph, a.tW = pw, a.tCout = C;
        return gemm(a);
    }
    // Option convt_fold at level i: active on the fp16 path when the unfused layer{i+1}_rn conv (on the k*ph x k*pw map) would run on
    // the 8-phase 256 x 256 tile or the 128-row kernel - the two families the folded mode is built for. ViT-S's 64-channel convs run
    // in conv_lds.hip and stay unfused. A dry pass always lays out the unfused pair (the same buffers; the larger launch count).
    bool fold_level(int i) const {
        if (dry || prec != VDA_PREC_F16 || !h->convt_fold) return false;
        const int B = g.BT, C = h->ocp[i], Fe = g.Fe, kk = i == 0 ? 4 : 2, H = kk * g.ph, Wd = kk * g.pw;
        if ((long long)B * H * Wd * Fe >= (1ll << 31)) return false;
        vda_gemm_args a = {};
        a.M = B * H * Wd, a.N = Fe, a.K = 9 * C, a.lda = a.K, a.ldc = Fe, a.a_mode = VDA_A_CONV3X3, a.epilogue = VDA_EPI_BIAS_F16;
        a.cB = B, a.cH = H, a.cW = Wd, a.cCin = C, a.cHo = H, a.cWo = Wd, a.cStride = 1;
        vda_gemm_plan_t plan;
        if (vda_gemm_plan(&a, 0, 0, 1, &plan) != 0) return false;
        const vda_gemm_launch& r = plan.rec[0];
        return r.family == VDA_GEMM_FAM_128 || (r.family == VDA_GEMM_FAM_8P && r.bm == 256 && r.bn == 256);
    }
    // the folded pair: t [B, ph, pw, C] -> out [B, k*ph, k*pw, Fe] = layer{i+1}_rn(resize_layers[i](t)) in one implicit GEMM
    int convt_fold(const void* t, int i, void* out) {
        const std::string k = "rn" + std::to_string(i + 1) + ".fold";
        const int B = g.BT, ph = g.ph, pw = g.pw, C = h->ocp[i], Fe = g.Fe, kk = i == 0 ? 4 : 2;
        vda_gemm_args a = {};
        a.A = t, a.W = W(k + ".w"), a.out = out, a.bias = V(k + ".b");
        a.M = B * ph * pw, a.N = kk * kk * Fe, a.K = 9 * C, a.ldc = Fe, a.a_mode = VDA_A_CONV3X3, a.epilogue = VDA_EPI_CONVT_FOLD_F16;
        a.cB = B, a.cH = ph, a.cW = pw, a.cCin = C, a.cHo = ph, a.cWo = pw, a.cStride = 1;
        a.tK = kk, a.tH = ph, a.tW = pw, a.tCout = Fe;
        return gemm(a);
    }
    int layernorm(const float* x, void* out, const float* w, const float* b, float eps, int rows, int D, int group = 0, int skip = 0,
                  const float* pe = nullptr, int pe_rows = 0, int pe_steps = 0) {
        if (dry) return 0;
        return prec == VDA_PREC_F32 ? vda_layernorm_f32_f32(x, (float*)out, w, b, eps, rows, D, group, skip, pe, pe_rows, pe_steps, s)
                                    : vda_layernorm_f32_f16(x, out, w, b, eps, rows, D, group, skip, pe, pe_rows, pe_steps, s);
    }
    int bilinear(const void* x, void* out, int B, int hh, int ww, int H, int Wd, int C) {
        if (dry) return 0;
        return prec == VDA_PREC_F32 ? vda_bilinear_nhwc_f32((const float*)x, (float*)out, nullptr, B, hh, ww, H, Wd, C, s)
                                    : vda_bilinear_nhwc_f16(x, out, nullptr, B, hh, ww, H, Wd, C, s);
    }

    // motion_module.py:102-126,164-177 on token-major x [B*T*hw, C]; returns a new activation buffer
    int temporal(int m, const void* x, int hw, int Cc, const std::string& tag, void** result) {
        const std::string k = "tm" + std::to_string(m) + ".";
        const int B = g.B, T = g.T, BT = g.BT, rows = BT * hw;
        int chunks = (hw + 31) / 32;
        chunks = chunks < 1 ? 1 : (chunks > 16 ? 16 : chunks);
        float* part = f32(sp + "gn_partial", (size_t)BT * chunks * GN_GROUPS * 2);
        void* gn = act(sp + "tm_g", (size_t)rows * Cc);
        if (!dry)
            VDA_TRY(prec == VDA_PREC_F32 ? vda_groupnorm_nhwc_f32((const float*)x, (float*)gn, V(k + "gn.w"), V(k + "gn.b"), GN_EPS, BT, hw, Cc, GN_GROUPS, part, chunks, s)
                                         : vda_groupnorm_nhwc_f16(x, gn, V(k + "gn.w"), V(k + "gn.b"), GN_EPS, BT, hw, Cc, GN_GROUPS, part, chunks, s));
        float* hs = f32(sp + "tm_hs", (size_t)rows * Cc);
        VDA_TRY(dense(gn, W(k + "in.w"), hs, VDA_EPI_BIAS_F32, rows, Cc, Cc, V(k + "in.b")));
        void* n = act(sp + "tm_n", (size_t)rows * Cc);
        void* tqkv = act(sp + "tm_qkv", (size_t)rows * 3 * Cc);
        void* tao = act(sp + "tm_ao", (size_t)rows * Cc);
        for (int a = 0; a < 2; ++a) {
            const std::string ka = k + "a" + std::to_string(a) + ".";
            const bool rope = h->cfg.pe_rope != 0;                   // motion_module.py:221-224: no additive encoding, q and k rotated instead
            VDA_TRY(layernorm(hs, n, V(ka + "ln.w"), V(ka + "ln.b"), TMP_LN_EPS, rows, Cc, 0, 0, rope ? nullptr : V(ka + "pe"), hw, T));
            VDA_TRY(dense(n, W(ka + "qkv.w"), tqkv, VDA_EPI_BIAS_F16, rows, 3 * Cc, Cc));
            for (int b = 0; b < B && !dry; ++b) {
                const size_t r0 = (size_t)b * T * hw;
                if (rope)
                    VDA_TRY(prec == VDA_PREC_F32 ? vda_rope_qk_f32((float*)tqkv + r0 * 3 * Cc, T, hw, Cc, s) : vda_rope_qk_f16((h16*)tqkv + r0 * 3 * Cc, T, hw, Cc, s));
                VDA_TRY(prec == VDA_PREC_F32
                            ? vda_temporal_attention_f32((const float*)tqkv + r0 * 3 * Cc, (float*)tao + r0 * Cc, T, hw, Cc, TEMPORAL_HEADS, s)
                            : vda_temporal_attention_f16((const h16*)tqkv + r0 * 3 * Cc, (h16*)tao + r0 * Cc, T, hw, Cc, TEMPORAL_HEADS, s));
            }
            VDA_TRY(dense(tao, W(ka + "out.w"), hs, VDA_EPI_SCALE_RES_F32, rows, Cc, Cc, V(ka + "out.b"), hs));
        }
        VDA_TRY(layernorm(hs, n, V(k + "ffln.w"), V(k + "ffln.b"), TMP_LN_EPS, rows, Cc));
        void* gg = act(sp + "tm_gg", (size_t)rows * 4 * Cc);
        VDA_TRY(dense(n, W(k + "ff1.w"), gg, VDA_EPI_GEGLU_F16, rows, 8 * Cc, Cc, V(k + "ff1.b"), nullptr, nullptr, 4 * Cc));
        void* hh = act(sp + "tm_hh", (size_t)rows * Cc);
        VDA_TRY(dense(gg, W(k + "ff2.w"), hh, VDA_EPI_SCALE_RES_F32_H, rows, Cc, 4 * Cc, V(k + "ff2.b"), hs));
        void* out = act(tag, (size_t)rows * Cc);
        VDA_TRY(dense(hh, W(k + "out.w"), out, VDA_EPI_RES_F16, rows, Cc, Cc, V(k + "out.b"), x));
        *result = out;
        return 0;
    }

    // util/blocks.py:68-91: conv2(relu(conv1(relu(x)))) + x (+ res2: the fusion block's skip add)
    // rcu_conv1 is y = relu(conv1(relu(x))) alone. It reads x only, so option head_lanes runs it ahead on the lane stream for
    // resConfUnit1 of refinenets 3, 2, 1 and hands the result to rcu as y1 (!= nullptr: conv1 already done, here is y)
    int rcu_conv1(int i, int u, const void* x, void* y, int H, int Wd) {
        const std::string k = "ref" + std::to_string(i) + ".rcu" + std::to_string(u) + ".";
        return conv3x3(x, k + "c1.w", y, g.BT, H, Wd, g.Fe, g.Fe, VDA_EPI_BIAS_RELU_F16, 1, V(k + "c1.b"), true);
    }
    int rcu(int i, int u, const void* x, void* out, int H, int Wd, const void* res2 = nullptr, const void* y1 = nullptr) {
        const std::string k = "ref" + std::to_string(i) + ".rcu" + std::to_string(u) + ".";
        const void* y = y1;
        if (y1 == nullptr) {
            void* t = act(sp + "rcu_y", (size_t)g.BT * H * Wd * g.Fe);
            VDA_TRY(rcu_conv1(i, u, x, t, H, Wd));
            y = t;
        }
        VDA_TRY(conv3x3(y, k + "c2.w", out, g.BT, H, Wd, g.Fe, g.Fe, VDA_EPI_RES_F16, 1, V(k + "c2.b"), false, x, res2));
        return 0;
    }
    // util/blocks.py:135-162 with out_conv moved in front of the (commuting) bilinear resize
    // upsample = false: the caller's next conv does the resize itself (vda_conv3x3_up2_f16); *result is the out_conv output at H x Wd
    // y1: see rcu. no_out: stop after resConfUnit2 (never in a dry pass: it lays out and counts the whole block)
    int fusion(int i, const void* x0, const void* x1, int H, int Wd, int Ho, int Wo, const std::string& tag, void** result, bool upsample = true,
               const void* y1 = nullptr, bool no_out = false) {
        const int B = g.BT, Fe = g.Fe;
        const size_t rows = (size_t)B * H * Wd;
        const void* sm = x0;
        if (x1 != nullptr) {
            void* t = act(sp + "fus_s", rows * Fe);
            VDA_TRY(rcu(i, 1, x1, t, H, Wd, x0, y1));
            sm = t;
        }
        void* r = act(sp + "fus_r", rows * Fe);
        VDA_TRY(rcu(i, 2, sm, r, H, Wd));
        void* c = act(upsample ? sp + "fus_c" : tag, rows * Fe);
        if (no_out) {                          // option oc1_mix: out_conv lives in the composed weight, *result is resConfUnit2's output
            *result = r;
            return 0;
        }
        const std::string k = "ref" + std::to_string(i) + ".out.";
        VDA_TRY(dense(r, W(k + "w"), c, VDA_EPI_BIAS_F16, (int)rows, Fe, Fe, V(k + "b")));
        if (!upsample) {
            *result = c;
            return 0;
        }
        void* out = act(tag, (size_t)B * Ho * Wo * Fe);
        VDA_TRY(bilinear(c, out, B, H, Wd, Ho, Wo, Fe));
        *result = out;
        return 0;
    }

    // ---- streams. `sd`'s stream (created at first use) takes up behind this point of the launch stream. The joins stay explicit
    // hipEventRecord / hipStreamWaitEvent pairs where they are placed: with head_lanes their placement is the measured part.
    int fork(vda_model::Side& sd) {
        VDA_TRY(open_side(sd));
        VDA_HIP(hipEventRecord(sd.fork, s));
        VDA_HIP(hipStreamWaitEvent(sd.stream, sd.fork, 0));
        return 0;
    }
    // Options enc_split and head_lanes apply only while this forward is `alone`: not on a capturing stream, and not while a forward
    // of this handle on another caller stream is in flight (others_idle; vda_model::tails). head_lanes and head_overlap exclude
    // each other.
    bool want_lanes() const { return !dry && prec == VDA_PREC_F16 && h->head_lanes != 0 && !h->head_overlap; }
    bool others_idle() const {
        for (auto& kv : h->tails) {
            if (kv.first == s || kv.second == nullptr) continue;
            if (hipEventQuery(kv.second) != hipSuccess) {
                (void)hipGetLastError();      // (hipErrorNotReady: that forward is still running)
                return false;
            }
        }
        return true;
    }

    // ---- the state of one forward
    struct Part {             // frames [f0, f0 + nf) of the clip, launched on st
        int f0, nf;
        hipStream_t st;
    };
    Part parts[2] = {};       // the encoder's frame halves (option enc_split), or the whole clip as one part
    int nparts = 1;
    bool capturing = false, alone = true;
    bool fold = false, defer = false, mlp1 = false;      // the encoder's block form, chosen once per forward (encoder)
    bool xn_ready = false;                               // block_deferred: norm1 of block i already ran (fused with block i-1's fc2 residual)
    bool early_done = false;                             // head_early ran (or, dry pass, was laid out) under the encoder
    float *tok = nullptr, *lnpart = nullptr, *lnstat = nullptr;
    void *thi = nullptr, *tlo = nullptr, *xn = nullptr, *qkv = nullptr, *ao = nullptr, *hid = nullptr, *yb = nullptr;
    int32_t* ovf = nullptr;
    int ntap = 0;
    vda_model::Side *lane = nullptr, *side = nullptr;
    void *l1r = nullptr, *l2r = nullptr, *l3r = nullptr;   // head_early's results

    // fn(part) for every part, each on its own stream; the callers go op by op (A.qkv, B.qkv, A.attention, B.attention, ...) so
    // that neither queue runs dry on the host side
    template <typename Fn>
    int each(Fn&& fn) {
        for (int j = 0; j < nparts; ++j) {
            On on(*this, parts[j].st, sp);
            VDA_TRY(fn(parts[j]));
        }
        return 0;
    }
    int ln_gemm(const std::string& wk, void* out, int epi, int N, const Part& p) {   // LayerNorm(x) @ W^T + b on the hi plane
        const size_t r0 = (size_t)p.f0 * g.Nt;
        vda_gemm_args a = {};
        a.A = (const h16*)thi + r0 * g.D, a.W = W(wk + ".weight.ln"), a.out = (h16*)out + r0 * N, a.bias = V(wk + ".c2"), a.gamma = V(wk + ".c1");
        a.stats = lnstat + r0 * 2;
        a.M = p.nf * g.Nt, a.N = N, a.K = g.D, a.a_mode = VDA_A_DENSE, a.epilogue = epi;
        return gemm(a, nparts > 1 ? g.rows : 0);
    }
    int res_gemm(const void* A, const std::string& wk, const std::string& gk, int K, const Part& p) {   // x += gamma * (A @ W^T + b)
        const size_t r0 = (size_t)p.f0 * g.Nt;
        const int nr = p.nf * g.Nt, np = g.D / 64, D = g.D;
        vda_gemm_args a = {};
        a.A = (const h16*)A + r0 * K, a.W = W(wk + ".weight"), a.bias = V(wk + ".bias"), a.gamma = V(gk);
        a.out = (h16*)thi + r0 * D, a.out2 = (h16*)tlo + r0 * D, a.res = a.out, a.res2 = a.out2;
        a.stats = lnpart + r0 * np * 2;      // the part's own [np, nr, 2] block of partial statistics
        a.pos = lnstat + r0 * 2;             // re-centre by the mean the LayerNorm before this branch saw
        a.M = nr, a.N = D, a.K = K, a.a_mode = VDA_A_DENSE, a.epilogue = VDA_EPI_SCALE_RES_SPLIT;
        VDA_TRY(gemm(a, nparts > 1 ? g.rows : 0));
        // (after the last block nothing reads the statistics: that finalize runs for its overflow check alone, 5 us per clip. It
        // sees what this GEMM read back - a plane the last attn.proj saturated; what this GEMM itself saturates has finite
        // partials in the row-layout families and is reported by the reader of its planes: the next res_gemm, or tap_ln)
        if (!dry) VDA_TRY(vda_ln_stats_finalize(lnpart + r0 * np * 2, lnstat + r0 * 2, ENC_LN_EPS, nr, np, ovf, s));
        return 0;
    }
    // the encoder's final norm of the part's rows; out is the whole tensor (group > 0: compacted, group - skip rows per frame).
    // On the split stream it raises the forward's overflow flag for a saturated row it normalises: after the last block it is the
    // only reader of the planes, so a token that the last fc2 (or the fused MLP) pushed out of range is reported here or nowhere.
    int tap_ln(void* out, int group, int skip, const Part& p) {
        if (!fold) return layernorm(tok, out, V("norm.w"), V("norm.b"), ENC_LN_EPS, g.rows, g.D, group, skip);   // (one part: the clip)
        if (dry) return 0;
        const size_t r0 = (size_t)p.f0 * g.Nt, o0 = group > 0 ? (size_t)p.f0 * (g.Nt / group) * (group - skip) : r0;
        return vda_layernorm_split_check_f16((const h16*)thi + r0 * g.D, (const h16*)tlo + r0 * g.D, (h16*)out + o0 * g.D, V("norm.w"), V("norm.b"),
                                             ENC_LN_EPS, p.nf * g.Nt, g.D, group, skip, ovf, s);
    }
    int ln_res(const float* gamma, void* out, const float* w, const float* b, int group, int skip) {
        if (dry) return 0;
        return vda_layernorm_residual_f32_f16(tok, yb, gamma, out, w, b, ENC_LN_EPS, g.rows, g.D, group, skip, s);
    }
    int attention() {
        if (dry) return 0;
        return each([&](const Part& p) {
            const size_t r0 = (size_t)p.f0 * g.Nt;
            return prec == VDA_PREC_F32 ? vda_attention_f32((const float*)qkv + r0 * 3 * g.D, (float*)ao + r0 * g.D, p.nf, g.Nt, g.NH, s)
                                        : vda_attention_f16((const h16*)qkv + r0 * 3 * g.D, (h16*)ao + r0 * g.D, p.nf, g.Nt, g.NH, s);
        });
    }
    // use_clstoken (dpt_temporal.py:56-59): the tap becomes GELU(Linear([patch token, cls])); the tap's final norm dropped the cls
    // row, so norm the whole token matrix again (cls kept) and gather [patch | cls] rows for one K = 2D GEMM
    int readout(void* tp) {
        const int D = g.D, P = g.P;
        void* full = act("rd_full", (size_t)g.rows * D);
        void* cat = act("rd_cat", (size_t)g.BT * P * 2 * D);
        const std::string kr = "readout" + std::to_string(ntap);
        return each([&](const Part& p) -> int {
            const size_t r0 = (size_t)p.f0 * g.Nt, q0 = (size_t)p.f0 * P;      // (token rows, patch rows) before the part
            VDA_TRY(tap_ln(full, 0, 0, p));
            if (!dry)
                VDA_TRY(prec == VDA_PREC_F32 ? vda_readout_concat_f32((const float*)full + r0 * D, (float*)cat + q0 * 2 * D, p.nf, P, D, s)
                                             : vda_readout_concat_f16((const h16*)full + r0 * D, (h16*)cat + q0 * 2 * D, p.nf, P, D, s));
            return dense((const char*)cat + q0 * 2 * D * ab, W(kr + ".w"), (char*)tp + q0 * D * ab, VDA_EPI_BIAS_GELU_F16, p.nf * P, D, 2 * D,
                         V(kr + ".b"), nullptr, nullptr, 0, nparts > 1 ? g.BT * P : 0);
        });
    }

    // ---- one encoder block in each of its three forms; tp != nullptr: the block is a tap, tp takes its final norm (cls dropped)
    // Option ln_fold (fp16 path, default): no LayerNorm pass at all inside the encoder. The residual stream lives as two fp16
    // planes (x = hi + lo; VDA_EPI_SCALE_RES_SPLIT reads and writes both, 8 bytes per element like the fp32 stream, and leaves
    // per-row partial statistics); qkv / fc1 take the hi plane as their A operand with LayerNorm's affine folded into their
    // weights and apply rstd * (acc - mean * c1) + c2 in their epilogue (VDA_EPI_LN_*). Only the four taps still run a LayerNorm.
    // mlp1 (option mlp_fused; mlp.py:35-41 + block.py:106): the whole MLP branch in one kernel where vda_mlp_fused_f16 is built for
    // the width (ViT-S): hid stays in registers, one launch instead of two. Off by default: in-process A/B it loses to the two launches.
    int block_split(int i, void* tp) {
        const std::string k = "b" + std::to_string(i) + ".";
        const int D = g.D;
        VDA_TRY(each([&](const Part& p) { return ln_gemm(k + "attn.qkv", qkv, VDA_EPI_LN_BIAS_F16, 3 * D, p); }));
        VDA_TRY(attention());
        VDA_TRY(each([&](const Part& p) { return res_gemm(ao, k + "attn.proj", k + "ls1.gamma", D, p); }));
        if (mlp1) {
            if (!dry) {
                VDA_TRY(vda_mlp_fused_f16(thi, lnstat, W(k + "mlp.fc1.weight.ln"), V(k + "mlp.fc1.c1"), V(k + "mlp.fc1.c2"), W(k + "mlp.fc2.weight.perm"),
                                          V(k + "mlp.fc2.bias"), V(k + "ls2.gamma"), thi, tlo, lnpart, g.rows, D, 4 * D, g.rows, s));
                VDA_TRY(vda_ln_stats_finalize(lnpart, lnstat, ENC_LN_EPS, g.rows, D / 64, ovf, s));
            }
        } else {
            VDA_TRY(each([&](const Part& p) { return ln_gemm(k + "mlp.fc1", hid, VDA_EPI_LN_GELU_F16, 4 * D, p); }));
            VDA_TRY(each([&](const Part& p) { return res_gemm(hid, k + "mlp.fc2", k + "ls2.gamma", 4 * D, p); }));
        }
        if (tp != nullptr) VDA_TRY(each([&](const Part& p) { return tap_ln(tp, g.Nt, 1, p); }));
        return 0;
    }
    // The fp32 residual stream (ln_fold off, and the fp32 precision): the residual add of a block's two projections (attn.proj,
    // mlp.fc2) is the GEMM's own fp32 in-place epilogue (VDA_EPI_SCALE_RES_F32)
    int block_f32_stream(int i, void* tp) {
        const std::string k = "b" + std::to_string(i) + ".";
        const int D = g.D, rows = g.rows;
        VDA_TRY(layernorm(tok, xn, V(k + "norm1.weight"), V(k + "norm1.bias"), ENC_LN_EPS, rows, D));
        VDA_TRY(dense(xn, W(k + "attn.qkv.weight"), qkv, VDA_EPI_BIAS_F16, rows, 3 * D, D, V(k + "attn.qkv.bias")));
        VDA_TRY(attention());
        VDA_TRY(dense(ao, W(k + "attn.proj.weight"), tok, VDA_EPI_SCALE_RES_F32, rows, D, D, V(k + "attn.proj.bias"), tok, V(k + "ls1.gamma")));
        VDA_TRY(layernorm(tok, xn, V(k + "norm2.weight"), V(k + "norm2.bias"), ENC_LN_EPS, rows, D));
        VDA_TRY(dense(xn, W(k + "mlp.fc1.weight"), hid, VDA_EPI_BIAS_GELU_F16, rows, 4 * D, D, V(k + "mlp.fc1.bias")));
        VDA_TRY(dense(hid, W(k + "mlp.fc2.weight"), tok, VDA_EPI_SCALE_RES_F32, rows, D, 4 * D, V(k + "mlp.fc2.bias"), tok, V(k + "ls2.gamma")));
        if (tp != nullptr) VDA_TRY(tap_ln(tp, g.Nt, 1, parts[0]));
        return 0;
    }
    // Option residual_in_ln (fp16 path): the projection stores its bias-added output y as fp16 and x += gamma * y rides on the
    // LayerNorm that follows (vda_layernorm_residual_f32_f16). Measured on ViT-L 1x32x518x518: the projection GEMMs get 15 % faster
    // (1040 vs 902 TFLOP/s) but the LayerNorm doubles its bytes (12 B per element at 5.05 TB/s): +1.1 ms per clip net (57.9 vs
    // 56.8 ms). Kept as an A/B option, off.
    int block_deferred(int i, void* tp) {
        const std::string k = "b" + std::to_string(i) + ".";
        const int D = g.D, rows = g.rows;
        const bool last = i + 1 == h->cfg.depth;
        if (!xn_ready) VDA_TRY(layernorm(tok, xn, V(k + "norm1.weight"), V(k + "norm1.bias"), ENC_LN_EPS, rows, D));
        xn_ready = false;
        VDA_TRY(dense(xn, W(k + "attn.qkv.weight"), qkv, VDA_EPI_BIAS_F16, rows, 3 * D, D, V(k + "attn.qkv.bias")));
        VDA_TRY(attention());
        VDA_TRY(dense(ao, W(k + "attn.proj.weight"), yb, VDA_EPI_BIAS_F16, rows, D, D, V(k + "attn.proj.bias")));
        VDA_TRY(ln_res(V(k + "ls1.gamma"), xn, V(k + "norm2.weight"), V(k + "norm2.bias"), 0, 0));
        VDA_TRY(dense(xn, W(k + "mlp.fc1.weight"), hid, VDA_EPI_BIAS_GELU_F16, rows, 4 * D, D, V(k + "mlp.fc1.bias")));
        VDA_TRY(dense(hid, W(k + "mlp.fc2.weight"), yb, VDA_EPI_BIAS_F16, rows, D, 4 * D, V(k + "mlp.fc2.bias")));
        if (last && tp != nullptr) return ln_res(V(k + "ls2.gamma"), tp, V("norm.w"), V("norm.b"), g.Nt, 1);     // residual + final norm, cls dropped
        const std::string kn = "b" + std::to_string(last ? i : i + 1) + ".";                                       // residual + the next block's norm1
        VDA_TRY(ln_res(V(k + "ls2.gamma"), xn, V(kn + "norm1.weight"), V(kn + "norm1.bias"), 0, 0));
        xn_ready = true;
        if (tp != nullptr) VDA_TRY(tap_ln(tp, g.Nt, 1, parts[0]));
        return 0;
    }

    // patch embedding (dinov2.py:212-219): tok = the clip's token rows, fp32
    int embed(const float* x) {
        const int BT = g.BT, P = g.P, D = g.D;
        void* a0 = act("a0", (size_t)BT * P * KPATCH);
        if (!dry) {
            // the K padding (588 -> 640) must be zero: the buffer is shared with nothing else, but the block is caller memory
            VDA_HIP(hipMemsetAsync(a0, 0, (size_t)BT * P * KPATCH * ab, s));
            VDA_TRY(prec == VDA_PREC_F32 ? vda_patchify_f32_f32(x, (float*)a0, BT, g.H, g.W, KPATCH, s) : vda_patchify_f32_f16(x, a0, BT, g.H, g.W, KPATCH, s));
        }
        tok = f32("tok", (size_t)g.rows * D);
        const float* pos = dry ? nullptr : h->pos_cache.at({g.H, g.W});
        vda_gemm_args a = {};
        a.A = a0, a.W = W("patch.w"), a.out = tok, a.bias = V("patch.b"), a.pos = pos;
        a.M = BT * P, a.N = D, a.K = KPATCH, a.a_mode = VDA_A_DENSE, a.epilogue = VDA_EPI_PATCH_F32, a.P = P;
        VDA_TRY(gemm(a));
        if (!dry) VDA_TRY(vda_cls_rows_f32(tok, V("cls"), pos, BT, P, D, s));
        return 0;
    }
    // ---- encoder (dinov2.py:212-219, dinov2_layers/block.py:105-106) -> taps[0..3], the final-norm'd patch tokens of the tap blocks
    // Frame halves (option enc_split; fp16 ln_fold path). The encoder is exactly per frame: attention mixes the tokens of one frame
    // only and every GEMM / LayerNorm row is independent. So frames [0, F) and [F, BT) run as two launch chains, half A on the
    // caller's stream and half B on the handle's lane stream, and each chain's kernels fill the tail rounds, launch boundaries and
    // small launches the other leaves idle. Every op is a row range of the same buffers, and each GEMM half is dispatched as the
    // whole-clip GEMM would be (gemm's m_plan): the result is bit-identical to one chain. The head (its motion modules mix frames) runs
    // after the join at full T. A captured forward keeps one stream (a linear graph); the dry pass takes the uncaptured decision
    // (the larger launch count, which sizes the dynamic-schedule counters).
    int encoder(const float* x, void** taps) {
        const vda_config& c = h->cfg;
        const int BT = g.BT, D = g.D, rows = g.rows;
        VDA_TRY(embed(x));
        xn = act("xn", (size_t)rows * D);
        qkv = act("qkv", (size_t)rows * 3 * D);
        ao = act("ao", (size_t)rows * D);
        defer = prec == VDA_PREC_F16 && h->residual_in_ln != 0;
        fold = prec == VDA_PREC_F16 && h->ln_fold != 0 && !defer && D % 64 == 0;
        mlp1 = fold && h->mlp_fused != 0 && vda_mlp_fused_supported(D, 4 * D) != 0;
        hid = mlp1 ? nullptr : act("hid", (size_t)rows * 4 * D);      // (the fused MLP kernel makes it unnecessary)
        thi = fold ? buf("tok_hi", (size_t)rows * D, 2) : nullptr;
        tlo = fold ? buf("tok_lo", (size_t)rows * D, 2) : nullptr;
        lnpart = fold ? f32("ln_part", (size_t)rows * (D / 64) * 2) : nullptr;
        lnstat = fold ? f32("ln_stat", (size_t)rows * 2) : nullptr;
        // overflow flag of this forward (see vda_model::ovf_host): a token that moved further than 65 504 from its own mean saturates
        // the fp16 planes (hi = +-inf, lo = -+inf). Raised by whatever reads such a row back: vda_ln_stats_finalize after the next
        // residual GEMM (non-finite statistics), and the tap LayerNorm (tap_ln) for the rows it normalises
        ovf = fold ? (int32_t*)buf("overflow", 1, 4) : nullptr;
        yb = defer ? act("ybuf", (size_t)rows * D) : nullptr;
        if (fold && !dry) {
            VDA_HIP(hipMemsetAsync(ovf, 0, 4, s));
            // The planes hold every token RELATIVE TO ITS OWN MEAN: taken out here, and again by every residual epilogue (res_gemm's
            // a.pos: the mean the preceding LayerNorm statistics found), so the operand plane's fp16 rounding is relative to the
            // token's spread whatever offset the stream carries (tests/_outliers.py "offset": mean / sigma ~ 20 cost 15x the standalone
            // LayerNorm's error before this). Every reader of the stream is a LayerNorm - invariant to a per-row shift.
            VDA_TRY(vda_split_center_stats_f32(tok, thi, tlo, lnstat, ENC_LN_EPS, rows, D, s));
        }
        parts[0] = {0, BT, s};
        const bool want_split = fold && !mlp1 && h->enc_split != 0 && BT >= 2;
        alone = !capturing && (dry || !(want_split || want_lanes()) || others_idle());
        if (want_split && alone) {
            parts[0] = {0, BT / 2, s};
            parts[1] = {BT / 2, BT - BT / 2, s};
            nparts = 2;
            if (!dry) {
                lane = &h->lanes[s];
                VDA_TRY(fork(*lane));                                  // the centred token planes and their statistics exist
                parts[1].st = lane->stream;
            }
        }
        for (int i = 0; i < c.depth; ++i) {
            bool is_tap = false;
            for (int t = 0; t < 4; ++t) is_tap = is_tap || c.taps[t] == i;
            void* tp = (is_tap && ntap < 4) ? act("tap" + std::to_string(ntap), (size_t)BT * g.P * D) : nullptr;
            VDA_TRY(fold ? block_split(i, tp) : defer ? block_deferred(i, tp) : block_f32_stream(i, tp));
            if (tp == nullptr) continue;
            if (c.use_clstoken) VDA_TRY(readout(tp));
            taps[ntap++] = tp;
            if (ntap == 3 && i + 1 != c.depth) VDA_TRY(head_early_under_encoder(taps));
        }
        if (lane != nullptr) {                 // half B's encoder is done before anything later on the caller's stream
            VDA_HIP(hipEventRecord(lane->join, lane->stream));
            VDA_HIP(hipStreamWaitEvent(s, lane->join, 0));
        }
        return 0;
    }

    // ---- the part of the head that needs taps 0..2 only (dpt_temporal.py:55-69 for i = 0, 1, 2; :75 motion module 0 on layer_3;
    // :78-80 layer{1,2,3}_rn) -> l1r, l2r, l3r: 3.8 of the head's 12.5 TFLOP at ViT-L.
    // part: 1 = the tap 0 / tap 1 chains (-> l1r, l2r), 2 = the tap 2 chain (-> l3r), 3 = both, in the order of one chain. Its
    // motion module takes scratch blocks of its own ("e."): with option head_lanes motion module 1 runs beside it.
    int head_early(void* const* taps, int part) {
        On on(*this, s, "e.");
        const int BT = g.BT, ph = g.ph, pw = g.pw, P = g.P, D = g.D, Fe = g.Fe, h1 = g.h1, w1 = g.w1, h2 = g.h2, w2 = g.w2;
        const int* ocp = h->ocp;
        void* l1 = act("l1", (size_t)BT * h1 * w1 * ocp[0]);
        void* l2 = act("l2", (size_t)BT * h2 * w2 * ocp[1]);
        void* l3t = nullptr;
        // option convt_fold: a folded level skips its ConvTranspose here and runs the folded GEMM where layer{i+1}_rn stood
        const bool f0 = fold_level(0), f1 = fold_level(1);
        void *t0 = nullptr, *t1 = nullptr;
        if (part & 1) {
            if (!dry) h->folded[0] = f0, h->folded[1] = f1;
            t0 = act("t0", (size_t)BT * P * ocp[0]);
            VDA_TRY(dense(taps[0], W("proj0.w"), t0, VDA_EPI_BIAS_F16, BT * P, ocp[0], D, V("proj0.b")));
            if (!f0) VDA_TRY(convt(t0, 0, l1));
            t1 = act("t1", (size_t)BT * P * ocp[1]);
            VDA_TRY(dense(taps[1], W("proj1.w"), t1, VDA_EPI_BIAS_F16, BT * P, ocp[1], D, V("proj1.b")));
            if (!f1) VDA_TRY(convt(t1, 1, l2));
        }
        if (part & 2) {
            void* l3 = act("l3", (size_t)BT * P * ocp[2]);
            VDA_TRY(dense(taps[2], W("proj2.w"), l3, VDA_EPI_BIAS_F16, BT * P, ocp[2], D, V("proj2.b")));
            VDA_TRY(temporal(0, l3, P, ocp[2], "l3t", &l3t));              // dpt_temporal.py:75
        }
        if (part & 1) {
            l1r = act("l1r", (size_t)BT * h1 * w1 * Fe);
            if (f0) VDA_TRY(convt_fold(t0, 0, l1r));
            else VDA_TRY(conv3x3(l1, "rn1.w", l1r, BT, h1, w1, ocp[0], Fe, VDA_EPI_BIAS_F16, 1, nullptr));
            l2r = act("l2r", (size_t)BT * h2 * w2 * Fe);
            if (f1) VDA_TRY(convt_fold(t1, 1, l2r));
            else VDA_TRY(conv3x3(l2, "rn2.w", l2r, BT, h2, w2, ocp[1], Fe, VDA_EPI_BIAS_F16, 1, nullptr));
        }
        if (part & 2) {
            l3r = act("l3r", (size_t)BT * P * Fe);
            VDA_TRY(conv3x3(l3t, "rn3.w", l3r, BT, ph, pw, ocp[2], Fe, VDA_EPI_BIAS_F16, 1, nullptr));
        }
        return 0;
    }
    // Option head_overlap runs head_early on a SIDE stream as soon as tap 2 exists, under the remaining encoder blocks (ViT-L:
    // blocks 18-23), so that its kernels fill the tail rounds and epilogue bursts of theirs - what two clips in flight do for a
    // video, inside ONE clip. Same kernels, same arithmetic: bit-identical. Without the option head_early runs in head(); the dry
    // pass requests its buffers HERE, so that both orders of execution find them laid out.
    int head_early_under_encoder(void* const* taps) {
        if (!dry && !h->head_overlap) return 0;
        early_done = true;
        if (dry) return head_early(taps, 3);
        side = &h->sides[s];
        VDA_TRY(fork(*side));                                          // taps 0..2 are behind this point of the caller's stream
        if (lane != nullptr) {                                         // ... and of the lane's (enc_split: half B's tap rows)
            VDA_HIP(hipEventRecord(lane->join, lane->stream));
            VDA_HIP(hipStreamWaitEvent(side->stream, lane->join, 0));
        }
        {
            On on(*this, side->stream, sp);
            VDA_TRY(head_early(taps, 3));
        }
        VDA_HIP(hipEventRecord(side->join, side->stream));
        return 0;
    }
    // Option head_lanes: the lane stream's share of the head. Its order puts what refinenet 3 needs first: refinenet 3 waits for
    // that alone (join) and refinenet 2 for the rest (join2).
    int head_on_lane(void* const* taps, void* const* y1) {
        lane = &h->lanes[s];
        VDA_TRY(fork(*lane));                                          // behind the encoder's join: every tap row exists
        On on(*this, lane->stream, "e.");
        VDA_TRY(head_early(taps, 2));
        VDA_TRY(rcu_conv1(3, 1, l3r, y1[3], g.ph, g.pw));
        VDA_HIP(hipEventRecord(lane->join, lane->stream));
        VDA_TRY(head_early(taps, 1));
        VDA_TRY(rcu_conv1(2, 1, l2r, y1[2], g.h2, g.w2));
        VDA_TRY(rcu_conv1(1, 1, l1r, y1[1], g.h1, g.w1));
        VDA_HIP(hipEventRecord(lane->join2, lane->stream));
        return 0;
    }
    // ---- head: reassemble (dpt_temporal.py:55-69), temporal modules on layer_3 / layer_4 (:75-76), layer_rn (:78-81), refinenets
    // ---- option head_lanes: a TASK split of the head's DAG over the caller's stream and the lane stream (idle after the join).
    // The chain through tap 3 (proj3 -> resize3 -> motion module 1 -> rn4 -> refinenet 4 -> motion module 2) holds the head's
    // poorly filled launches: 19 x 19 maps, 18 .. 72 % of one round of 256 x 256 tiles, and the bandwidth-bound LayerNorm /
    // GroupNorm / temporal attention passes between them. Beside it the lane runs what does not depend on it and fills the
    // grid: head_early, and conv1 of resConfUnit1 of refinenets 3, 2, 1 (it reads l3r / l2r / l1r only; the other input of the
    // unit enters in conv2's epilogue). Every kernel keeps its rows, its tile plan and its arguments, and the two sides share no
    // scratch block (Run::sp, and y1[] for the hoisted convs): bit-identical to one chain. One join before refinenet 3 for all
    // of the lane's work measured 0.18 - 0.20 ms per ViT-L clip slower (profiles/r10/head_lanes/) and is not kept.
    int head(void* const* taps, float* depth) {
        const int BT = g.BT, ph = g.ph, pw = g.pw, P = g.P, Fe = g.Fe, h1 = g.h1, w1 = g.w1, h2 = g.h2, w2 = g.w2, h4 = g.h4, w4 = g.w4;
        const int* ocp = h->ocp;
        // (requested in every configuration: the layout does not depend on the option)
        void* y1[4] = {nullptr, act("ref1.y1", (size_t)BT * h1 * w1 * Fe), act("ref2.y1", (size_t)BT * h2 * w2 * Fe), act("ref3.y1", (size_t)BT * P * Fe)};
        const bool hlanes = want_lanes() && alone;
        if (hlanes) VDA_TRY(head_on_lane(taps, y1));
        else if (!early_done) VDA_TRY(head_early(taps, 3));
        else if (side != nullptr) VDA_HIP(hipStreamWaitEvent(s, side->join, 0));     // the side stream's part is done before anything reads it
        void* t3 = act("t3", (size_t)BT * P * ocp[3]);
        VDA_TRY(dense(taps[3], W("proj3.w"), t3, VDA_EPI_BIAS_F16, BT * P, ocp[3], g.D, V("proj3.b")));
        void* l4 = act("l4", (size_t)BT * h4 * w4 * ocp[3]);
        VDA_TRY(conv3x3(t3, "resize3.w", l4, BT, ph, pw, ocp[3], ocp[3], VDA_EPI_BIAS_F16, 2, V("resize3.b")));
        void* l4t = nullptr;
        VDA_TRY(temporal(1, l4, h4 * w4, ocp[3], "l4t", &l4t));
        void* l4r = act("l4r", (size_t)BT * h4 * w4 * Fe);
        VDA_TRY(conv3x3(l4t, "rn4.w", l4r, BT, h4, w4, ocp[3], Fe, VDA_EPI_BIAS_F16, 1, nullptr));
        void *p4 = nullptr, *p4t = nullptr, *p3 = nullptr, *p3t = nullptr, *p2 = nullptr, *p1 = nullptr;
        VDA_TRY(fusion(4, l4r, nullptr, h4, w4, ph, pw, "p4", &p4));
        VDA_TRY(temporal(2, p4, P, Fe, "p4t", &p4t));
        if (hlanes) VDA_HIP(hipStreamWaitEvent(s, lane->join, 0));                   // l3r and y1[3]
        VDA_TRY(fusion(3, p4t, l3r, ph, pw, h2, w2, "p3", &p3, true, hlanes ? y1[3] : nullptr));
        VDA_TRY(temporal(3, p3, h2 * w2, Fe, "p3t", &p3t));
        if (hlanes) VDA_HIP(hipStreamWaitEvent(s, lane->join2, 0));                    // l2r, l1r, y1[2], y1[1]
        VDA_TRY(fusion(2, p3t, l2r, h2, w2, h1, w1, "p2", &p2, true, hlanes ? y1[2] : nullptr));
        const Oc1 o = oc1_form();
        if (!dry) h->mixed = o.mix;
        VDA_TRY(fusion(1, p2, l1r, h1, w1, 2 * h1, 2 * w1, o.up_fused ? "p1c" : "p1", &p1, !o.up_fused, hlanes ? y1[1] : nullptr, o.mix));
        return output_convs(p1, depth);
    }
    // The form of output_conv1. up_fused: refinenet1's 2x upsample (util/blocks.py:156-160) is folded into output_conv1 on the fp16
    // path: path_1 at 8 ph x 8 pw (1.4 GB per ViT-L clip) never exists; "p1c" is refinenet1's out_conv output at 4 ph x 4 pw (bilinear
    // and the 1x1 conv commute). mix (option oc1_mix, where up_fused applies): the channel mixing of out_conv + output_conv1 as ONE
    // GEMM at h1 x w1 into z (9 * Fhp channels, pack-time weight vda_fold_oc1_weight) and the gather-and-add pass
    // vda_oc1_mix_combine_f16; refinenet1 stops after resConfUnit2 and "p1c" is never written. z of a whole ViT-L clip is 1.6 GB: the
    // pair runs per chunk of `frames` frames out of one z buffer. The dry pass lays out "p1c" and z and counts the launches of both
    // forms whatever the option says.
    struct Oc1 {
        bool up_fused, fits, mix;
        int frames, ldz;      // ldz: z's row, 9 * Fhp channels (tap, cout), padded where the GEMM planner then tiles better
    };
    Oc1 oc1_form() const {
        Oc1 o;
        o.up_fused = prec == VDA_PREC_F16 && h->oc1_fused != 0 && g.Fhp <= 128 && g.Fe % 16 == 0;
        o.frames = std::min(g.BT, h->oc1_mix_chunk > 0 ? h->oc1_mix_chunk : vda_oc1_mix_frames());
        o.ldz = vda_oc1_mix_ldz(g.Fhp);
        o.fits = (double)o.frames * g.h1 * g.w1 * o.ldz < 2147483647.0;
        o.mix = o.up_fused && !dry && h->oc1_mix != 0 && o.fits;
        return o;
    }
    // ---- output convs (dpt.py:117-124, dpt_temporal.py:93-100) on refinenet1's result p1 -> depth
    int output_convs(const void* p1, float* depth) {
        const Oc1 o = oc1_form();
        const int BT = g.BT, H = g.H, Wd = g.W, Fe = g.Fe, Fhp = g.Fhp, h1 = g.h1, w1 = g.w1, hh = 2 * h1, ww = 2 * w1;
        void* o1 = act("o1", (size_t)BT * hh * ww * Fhp);
        if (o.up_fused && o.fits && (o.mix || dry)) {
            void* z = act("oc1_z", (size_t)o.frames * h1 * w1 * o.ldz);
            for (int f0 = 0; f0 < BT; f0 += o.frames) {
                const int nf = std::min(o.frames, BT - f0);
                VDA_TRY(dense((const h16*)p1 + (size_t)f0 * h1 * w1 * Fe, W("oc1.mix.w"), z, VDA_EPI_BIAS_F16, nf * h1 * w1, o.ldz, Fe, V("oc1.mix.b")));
                if (!dry) VDA_TRY(vda_oc1_mix_combine_f16(z, V("oc1.b"), (h16*)o1 + (size_t)f0 * hh * ww * Fhp, nf, h1, w1, Fhp, o.ldz, s));
            }
        }
        if (o.up_fused) {
            if (!dry && !o.mix) VDA_TRY(vda_conv3x3_up2_f16(p1, W("oc1.w"), V("oc1.b"), o1, BT, h1, w1, Fe, Fhp, Fhp, s));
        } else
            VDA_TRY(conv3x3(p1, "oc1.w", o1, BT, hh, ww, Fe, Fhp, VDA_EPI_BIAS_F16, 1, V("oc1.b")));
        if (prec == VDA_PREC_F16) {
            // bilinear to (H,W) + output_conv2 (3x3 -> ReLU -> 1x1 -> ReLU) fused: the upsampled tensor never exists
            if (!dry) VDA_TRY(vda_depth_tail_f16(o1, W("oc2.w"), V("oc2.b"), V("oc3.w"), h->oc3_bias, depth, h->zero_page, BT, hh, ww, H, Wd, Fhp, s));
        } else {
            // fp32 operands: the same three steps unfused (speed is secondary on this path; 288 GB of HBM hold the 518^2 tensor)
            void* up = act("tail_up", (size_t)BT * H * Wd * Fhp);
            VDA_TRY(bilinear(o1, up, BT, hh, ww, H, Wd, Fhp));
            void* c2 = act("tail_c2", (size_t)BT * H * Wd * 32);
            VDA_TRY(conv3x3(up, "oc2.w", c2, BT, H, Wd, Fhp, 32, VDA_EPI_BIAS_RELU_F16, 1, V("oc2.b")));
            if (!dry) VDA_TRY(vda_head_out_f32_f32((const float*)c2, V("oc3.w"), h->oc3_bias, depth, (long long)BT * H * Wd, 32, s));
        }
        // video_depth.py:162-163: bilinear to (H,W) is the identity here (H == 14*ph) and the final ReLU is idempotent.
        if (fold && !dry) {
            hipLaunchKernelGGL(poison_on_overflow_kernel, dim3(256), dim3(256), 0, s, (const int*)ovf, depth, (long long)BT * H * Wd, (volatile int*)h->ovf_host);
            VDA_LAUNCH_CHECK();
        }
        return 0;
    }

    // One forward of the clip: x [B, T, 3, H, W] fp32 -> depth [B, T, H, W] fp32 (dry pass: the layout and the launch count)
    int forward(const float* x, float* depth) {
        if (!dry) {                          // (a captured forward stays one linear stream)
            hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
            if (hipStreamIsCapturing(s, &cs) != hipSuccess) {
                (void)hipGetLastError();          // (e.g. the legacy stream while another stream captures): treated as capturing
                cs = hipStreamCaptureStatusActive;
            }
            capturing = cs != hipStreamCaptureStatusNone;
        }
        // dynamic-schedule counters of every GEMM launch below: sized by the dry pass, zeroed here once per forward
        if (prec == VDA_PREC_F16 && h->dyn_sched) {
            const int cap = dry ? 4096 : lay->gemm_launches;
            sched = (int32_t*)buf("sched", (size_t)8 * (cap > 0 ? cap : 1), 4);
            if (!dry) VDA_HIP(hipMemsetAsync(sched, 0, (size_t)32 * lay->gemm_launches, s));
        }
        void* taps[4] = {nullptr, nullptr, nullptr, nullptr};
        VDA_TRY(encoder(x, taps));
        if (ntap != 4) {
            vda_set_error("vda_forward: the configuration's taps are not four distinct block indices below depth");
            return 1;
        }
        VDA_TRY(head(taps, depth));
        if (!dry && !capturing) {            // the end of the last forward enqueued on this caller stream (others_idle)
            hipEvent_t& tail = h->tails[s];
            if (tail == nullptr) VDA_HIP(hipEventCreateWithFlags(&tail, hipEventDisableTiming));
            VDA_HIP(hipEventRecord(tail, s));
        }
        return 0;
    }
    // vda_debug_copy: "l1" / "l2" of a forward that ran level lvl folded (option convt_fold) were never written: rebuilt here, into
    // their own block, from the level's projection with the ConvTranspose GEMM the unfused forward runs - same arguments, same
    // kernel, same bits
    int rebuild_level(int lvl) { return convt(act(lvl == 0 ? "t0" : "t1", 0), lvl, act(lvl == 0 ? "l1" : "l2", 0)); }
    // ... and "p1c" of a forward that ran option oc1_mix: rebuilt from resConfUnit2's output ("fus_r": refinenet1 is its last
    // writer) with the out_conv GEMM the unfused forward runs
    int rebuild_p1c() { return dense(act("fus_r", 0), W("ref1.out.w"), act("p1c", 0), VDA_EPI_BIAS_F16, g.BT * g.h1 * g.w1, g.Fe, g.Fe, V("ref1.out.b")); }
};

int get_layout(vda_model* h, int B, int T, int H, int W, int prec, Layout** out) {
    const std::array<int, 5> key = {B, T, H, W, prec};
    auto it = h->layouts.find(key);
    if (it == h->layouts.end()) {
        Layout lay;
        Run r(h, prec, true, &lay, nullptr, B, T, H, W);
        VDA_TRY(r.forward(nullptr, nullptr));
        lay.gemm_launches = r.nsched;
        size_t off = 0;
        for (const std::string& n : lay.order) {
            lay.bufs[n].first = off;
            off += lay.bufs[n].second;
        }
        lay.total = off;
        it = h->layouts.emplace(key, std::move(lay)).first;
    }
    *out = &it->second;
    return 0;
}

int check_shape(const vda_model* h, int B, int T, int H, int W, int prec) {
    VDA_REQUIRE(prec == VDA_PREC_F16 || prec == VDA_PREC_F32, "vda_forward: precision %d (VDA_PREC_F16 = 0, VDA_PREC_F32 = 1)", prec);
    VDA_REQUIRE(B > 0 && T > 0, "vda_forward: empty clip B=%d T=%d", B, T);
    VDA_REQUIRE(H > 0 && H % PATCH == 0, "Input image height %d is not a multiple of patch height %d", H, PATCH);       // patch_embed.py:73
    VDA_REQUIRE(W > 0 && W % PATCH == 0, "Input image width %d is not a multiple of patch width: %d", W, PATCH);         // patch_embed.py:74
    VDA_REQUIRE(T <= h->cfg.num_frames, "vda_forward: T=%d exceeds temporal_max_len=%d", T, h->cfg.num_frames);
    VDA_REQUIRE((long long)B * T * ((H / PATCH) * (W / PATCH) + 1) * 4 * h->cfg.embed_dim < (1ll << 31), "vda_forward: clip too large for 32-bit row offsets (B*T*tokens*4*embed_dim)");
    return 0;
}

// An on / off option's default from the environment (A/B through an unmodified caller; unset: on). Each default below reads its
// variable once per process.
int env_default(const char* var) {
    const char* e = getenv(var);
    return e == nullptr || atoi(e) != 0;
}
int enc_split_default(const vda_model*) { static const int v = env_default("VDA_ENC_SPLIT"); return v; }
int head_lanes_default(const vda_model*) { static const int v = env_default("VDA_HEAD_LANES"); return v; }
int convt_fold_default(const vda_model*) { static const int v = env_default("VDA_CONVT_FOLD"); return v; }
int oc1_mix_default(const vda_model* h) { return vda_oc1_mix_default(h->cfg.features); }

// vda_set_option: the tuning / A-B switches of the launch sequence (see Run). `flag`: the value is stored as value != 0, and where
// the option has a process default (`dflt`), value < 0 stores that; otherwise the value is stored as given. `relayout`: the
// workspace layout or the GEMM launch count (dynamic-schedule counters) depends on the option, so the layouts are dropped.
struct Option {
    const char* name;
    int vda_model::*field;
    bool flag, relayout;
    int (*dflt)(const vda_model*);
};
const Option OPTIONS[] = {
    // name            field                        flag   relayout  dflt                   default
    {"residual_in_ln", &vda_model::residual_in_ln, false, true, nullptr},                // 0
    {"ln_fold", &vda_model::ln_fold, false, true, nullptr},                              // 1
    {"dyn_sched", &vda_model::dyn_sched, false, true, nullptr},                          // 0
    {"oc1_fused", &vda_model::oc1_fused, false, true, nullptr},                          // 1
    {"mlp_fused", &vda_model::mlp_fused, true, true, nullptr},                           // 0 (hid is not allocated with it)
    {"head_overlap", &vda_model::head_overlap, true, false, nullptr},                    // 0
    {"enc_split", &vda_model::enc_split, true, true, enc_split_default},                 // 1, or VDA_ENC_SPLIT
    {"head_lanes", &vda_model::head_lanes, true, false, head_lanes_default},             // 1, or VDA_HEAD_LANES
    {"convt_fold", &vda_model::convt_fold, true, false, convt_fold_default},             // 1, or VDA_CONVT_FOLD
    {"oc1_mix", &vda_model::oc1_mix, true, false, oc1_mix_default},                      // vda_oc1_mix_default, or VDA_OC1_MIX
    {"oc1_mix_chunk", &vda_model::oc1_mix_chunk, false, true, nullptr},                  // 0: frames per z buffer (<= 0: vda_oc1_mix_frames())
};

// No exception crosses the C ABI: an entry point that can throw (std::map::at, std::string, std::vector) runs inside this
template <typename R, typename Fn>
R guarded(const char* entry, R on_throw, Fn&& fn) {
    try {
        return fn();
    } catch (const std::exception& e) {
        vda_set_error("%s: %s", entry, e.what());
        return on_throw;
    }
}

}  // namespace

extern "C" int vda_create(const vda_config* cfg, vda_model** out) {
    VDA_REQUIRE(cfg && out, "vda_create: null argument");
    VDA_REQUIRE(cfg->embed_dim > 0 && cfg->embed_dim % 64 == 0 && cfg->num_heads > 0 && cfg->embed_dim == cfg->num_heads * 64,
                "vda_create: embed_dim=%d must be num_heads=%d x 64 (the attention kernels are built for head dim 64)", cfg->embed_dim, cfg->num_heads);
    VDA_REQUIRE(cfg->depth > 0 && cfg->features > 0 && cfg->features % 64 == 0, "vda_create: depth=%d features=%d (features must be a multiple of 64)", cfg->depth, cfg->features);
    VDA_REQUIRE(cfg->num_frames > 0 && cfg->num_frames <= 32, "vda_create: num_frames=%d must be in 1..32", cfg->num_frames);
    VDA_REQUIRE((cfg->use_clstoken | cfg->use_bn | cfg->pe_rope) >> 1 == 0, "vda_create: use_clstoken / use_bn / pe_rope are 0 or 1");
    for (int i = 0; i < 4; ++i) {
        VDA_REQUIRE(cfg->out_channels[i] > 0 && cfg->out_channels[i] % 8 == 0, "vda_create: out_channels[%d]=%d must be a positive multiple of 8", i, cfg->out_channels[i]);
        VDA_REQUIRE(cfg->taps[i] >= 0 && cfg->taps[i] < cfg->depth && (i == 0 || cfg->taps[i] > cfg->taps[i - 1]), "vda_create: taps must be increasing block indices below depth");
    }
    VDA_REQUIRE(cfg->out_channels[2] % 64 == 0 && cfg->out_channels[3] % 64 == 0,
                "vda_create: out_channels[2..3] carry the temporal modules (GroupNorm over the true width): multiples of 64 only");
    vda_model* h = new vda_model();
    h->cfg = *cfg;
    if (hipGetDevice(&h->device) != hipSuccess) {
        delete h;
        vda_set_error("vda_create: no HIP device (this library has no CPU path)");
        return 2;
    }
    WeightTable table(h->cfg);                        // csrc/weight_table.h: one row per checkpoint tensor, and the padded widths
    for (int i = 0; i < 4; ++i) h->ocp[i] = table.ocp[i];
    h->Fhp = table.Fhp;
    h->table = std::move(table.rows);
    for (const WEntry& e : h->table) h->spec[e.name] = e.shape;
    if (dev_alloc(h, 256, &h->zero_page) != 0 || hipMemset(h->zero_page, 0, 256) != hipSuccess) {
        for (void* p : h->owned) (void)hipFree(p);
        delete h;
        vda_set_error("vda_create: device allocation failed");
        return 2;
    }
    void* ring = nullptr;
    if (hipHostMalloc(&ring, 64, hipHostMallocDefault) != hipSuccess) {
        for (void* p : h->owned) (void)hipFree(p);
        delete h;
        vda_set_error("vda_create: pinned host allocation failed");
        return 2;
    }
    memset(ring, 0, 64);
    h->ovf_host = (volatile int32_t*)ring;
    for (const Option& o : OPTIONS)
        if (o.dflt) h->*o.field = o.dflt(h);
    *out = h;
    return 0;
}

extern "C" int vda_destroy(vda_model* h) {
    if (h == nullptr) return 0;
    if (h->ovf_host) (void)hipHostFree((void*)h->ovf_host);
    for (auto& kv : h->tails)
        if (kv.second) (void)hipEventDestroy(kv.second);
    for (auto* m : {&h->sides, &h->lanes})
        for (auto& kv : *m) {
            if (kv.second.fork) (void)hipEventDestroy(kv.second.fork);
            if (kv.second.join) (void)hipEventDestroy(kv.second.join);
            if (kv.second.join2) (void)hipEventDestroy(kv.second.join2);
            if (kv.second.stream) (void)hipStreamDestroy(kv.second.stream);
        }
    for (void* p : h->owned) (void)hipFree(p);
    delete h;
    return 0;
}

extern "C" int vda_num_weights(const vda_model* h) { return h ? (int)h->spec.size() : 0; }

static int vda_load_weight_impl(vda_model* h, const char* name, const void* ptr, const int64_t* dims, int ndim, int dtype) {
    VDA_REQUIRE(h && name && ptr && (dims || ndim == 0), "vda_load_weight: null argument");
    VDA_REQUIRE(dtype == VDA_DTYPE_F32, "vda_load_weight(%s): dtype %d (only VDA_DTYPE_F32 = 0 checkpoints are defined, run.py:46)", name, dtype);
    VDA_TRY(require_device(h, "vda_load_weight"));
    auto it = h->spec.find(name);
    VDA_REQUIRE(it != h->spec.end(), "Unexpected key(s) in state_dict: \"%s\". ", name);
    const std::vector<int64_t>& want = it->second;
    bool same = (size_t)ndim == want.size();
    for (int i = 0; same && i < ndim; ++i) same = dims[i] == want[i];
    if (!same) {
        std::string got = "(", exp = "(";
        for (int i = 0; i < ndim; ++i) got += (i ? ", " : "") + std::to_string(dims[i]);
        for (size_t i = 0; i < want.size(); ++i) exp += (i ? ", " : "") + std::to_string(want[i]);
        vda_set_error("size mismatch for %s: copying a param with shape %s) from checkpoint, the shape in current model is %s).", name, got.c_str(), exp.c_str());
        return 1;
    }
    size_t n = 1;
    for (int64_t d : want) n *= (size_t)d;
    Raw& r = h->raw[name];
    if (r.d == nullptr) {
        void* p = nullptr;
        VDA_TRY(dev_alloc(h, n * sizeof(float), &p));
        r.d = (float*)p;
    }
    VDA_HIP(hipMemcpy(r.d, ptr, n * sizeof(float), hipMemcpyDefault));       // host or device source
    h->finalized = false;
    return 0;
}

static int vda_finalize_weights_impl(vda_model* h) {
    VDA_REQUIRE(h, "vda_finalize_weights: null handle");
    VDA_TRY(require_device(h, "vda_finalize_weights"));
    std::string missing;
    for (const auto& kv : h->spec)
        if (h->raw.find(kv.first) == h->raw.end()) missing += (missing.empty() ? "\"" : ", \"") + kv.first + "\"";
    if (!missing.empty()) {
        if (missing.size() > 400) missing = missing.substr(0, 400) + " ...";
        vda_set_error("Missing key(s) in state_dict: %s. ", missing.c_str());
        return 1;
    }
    // a re-load replaces every layout: drop the packed copies (their memory stays owned by the handle until vda_destroy)
    h->mat[0].clear();
    h->mat[1].clear();
    h->vec.clear();
    h->pos_cache.clear();
    h->packed[0] = h->packed[1] = false;
    VDA_HIP(hipMemcpy(&h->oc3_bias, h->raw.at("head.scratch.output_conv2.2.bias").d, sizeof(float), hipMemcpyDeviceToHost));
    VDA_TRY(pack_all<h16>(h, VDA_PREC_F16));
    h->finalized = true;
    return 0;
}

// Everything a forward of this shape / precision needs beyond the workspace: the fp32 weight pack (first fp32 use) and the
// positional embedding at this grid (dinov2.py:179-210). Called by vda_forward; callable up front to keep the first
// forward allocation-free.
static int vda_prepare_impl(vda_model* h, int B, int T, int H, int W, int precision) {
    VDA_REQUIRE(h && h->finalized, "vda_prepare: load every weight and call vda_finalize_weights first");
    VDA_TRY(require_device(h, "vda_prepare"));
    VDA_TRY(check_shape(h, B, T, H, W, precision));
    if (!h->packed[precision]) VDA_TRY(pack_all<float>(h, VDA_PREC_F32));
    const std::pair<int, int> key = {H, W};
    if (h->pos_cache.find(key) == h->pos_cache.end()) {
        const int ph = H / PATCH, pw = W / PATCH, D = h->cfg.embed_dim;
        const float* pe = h->raw.at("pretrained.pos_embed").d;
        void* p = nullptr;
        VDA_TRY(dev_alloc(h, (size_t)(1 + ph * pw) * D * sizeof(float), &p));
        if (ph * pw == POS_GRID * POS_GRID && H == W) {
            // dinov2.py:183-184. A device-to-device hipMemcpy may return before the copy has run, and the first forward reads the
            // cache on the caller's (non-blocking) stream: complete it here, as the resample branch does
            VDA_HIP(hipMemcpyAsync(p, pe, (size_t)(1 + ph * pw) * D * sizeof(float), hipMemcpyDeviceToDevice, nullptr));
        } else {
            VDA_TRY(vda_pos_embed_resample_f32(pe, (float*)p, POS_GRID, ph, pw, D, nullptr));
        }
        VDA_HIP(hipStreamSynchronize(nullptr));
        h->pos_cache[key] = (float*)p;
    }
    Layout* lay = nullptr;
    return get_layout(h, B, T, H, W, precision, &lay);
}

static int64_t vda_workspace_bytes_impl(vda_model* h, int B, int T, int H, int W, int precision) {
    if (h == nullptr || !h->finalized) {
        vda_set_error("vda_workspace_bytes: load every weight and call vda_finalize_weights first");
        return -1;
    }
    if (check_shape(h, B, T, H, W, precision) != 0) return -1;
    Layout* lay = nullptr;
    if (get_layout(h, B, T, H, W, precision, &lay) != 0) return -1;
    return (int64_t)lay->total;
}

extern "C" int vda_set_workspace(vda_model* h, void* ptr, int64_t bytes) {
    VDA_REQUIRE(h, "vda_set_workspace: null handle");
    VDA_REQUIRE(((uintptr_t)ptr & 255) == 0, "vda_set_workspace: the block must be 256-byte aligned");
    h->ws = ptr;
    h->ws_bytes = ptr ? bytes : 0;
    h->ws_owned = false;
    return 0;
}

// Overflow reports that have ARRIVED (their forward's stream work has completed): collected and cleared. A word still in flight
// reads 0 and is seen by a later call. Status 4 + a message naming the way out.
static int collect_overflow(vda_model* h, const char* who) {
    if (h->ovf_host[0] == 0) return 0;
    h->ovf_host[0] = 0;
    vda_set_error("%s: in a forward since the last check the split residual stream left fp16's range (a token further than 65504 from its own "
                  "mean): that forward's depth was overwritten with NaN. vda_set_option(h, \"ln_fold\", 0) keeps the stream in fp32 (the reference's "
                  "form, no such limit); fp32=True avoids it as well", who);
    return 4;
}

extern "C" int vda_forward_status(vda_model* h) {
    VDA_REQUIRE(h != nullptr, "vda_forward_status: null handle");
    return collect_overflow(h, "vda_forward_status");
}

static int vda_forward_impl(vda_model* h, const float* in, float* out, int B, int T, int H, int W, int precision, vda_stream_t stream) {
    VDA_REQUIRE(h && in && out, "vda_forward: null argument");
    VDA_REQUIRE(h->finalized, "vda_forward: load every weight and call vda_finalize_weights first");
    VDA_TRY(collect_overflow(h, "vda_forward"));          // an EARLIER forward's report, if nobody asked (never silent)
    VDA_TRY(vda_prepare(h, B, T, H, W, precision));
    Layout* lay = nullptr;
    VDA_TRY(get_layout(h, B, T, H, W, precision, &lay));
    if (h->ws == nullptr || (h->ws_owned && (size_t)h->ws_bytes < lay->total)) {
        // no caller block: the handle keeps one of its own, grown to the largest shape seen
        void* p = nullptr;
        VDA_HIP(hipMalloc(&p, lay->total));
        if (h->ws_owned && h->ws) {
            VDA_HIP(hipDeviceSynchronize());
            (void)hipFree(h->ws);
            for (auto& q : h->owned)
                if (q == h->ws) q = p;
        } else {
            h->owned.push_back(p);
        }
        h->ws = p;
        h->ws_bytes = (int64_t)lay->total;
        h->ws_owned = true;
    }
    VDA_REQUIRE((size_t)h->ws_bytes >= lay->total, "vda_forward: workspace of %lld bytes, this shape needs %lld (vda_workspace_bytes)",
                (long long)h->ws_bytes, (long long)lay->total);
    Run r(h, precision, false, lay, (hipStream_t)stream, B, T, H, W);
    h->last_key = {B, T, H, W, precision};
    return r.forward(in, out);
}

// Debug / parity hook: copy a named intermediate of the LAST forward (same workspace) into `dst`: "tap0".."tap3" (final-norm'd
// patch tokens), "l1", "l2", "l3t", "l4t" (reassembled + temporal layers), "p4t", "p3t", "p2", "p1" (fusion pyramid).
static int vda_debug_copy_impl(vda_model* h, const char* name, void* dst, int64_t bytes, vda_stream_t stream) {
    VDA_REQUIRE(h && name && dst, "vda_debug_copy: null argument");
    auto it = h->layouts.find(h->last_key);
    VDA_REQUIRE(it != h->layouts.end() && h->ws, "vda_debug_copy: no forward has run");
    auto b = it->second.bufs.find(name);
    VDA_REQUIRE(b != it->second.bufs.end(), "vda_debug_copy: no buffer named %s", name);
    VDA_REQUIRE(bytes > 0 && (size_t)bytes <= b->second.second, "vda_debug_copy: %s holds %lld bytes", name, (long long)b->second.second);
    // a stage that the last forward's options folded away is rebuilt first (Run::rebuild_level, Run::rebuild_p1c)
    const std::array<int, 5>& k = h->last_key;
    const int lvl = strcmp(name, "l1") == 0 ? 0 : strcmp(name, "l2") == 0 ? 1 : -1;
    const bool level = lvl >= 0 && h->folded[lvl], p1c = strcmp(name, "p1c") == 0 && h->mixed;
    if (k[4] == VDA_PREC_F16 && (level || p1c)) {
        VDA_TRY(require_device(h, "vda_debug_copy"));
        Run r(h, VDA_PREC_F16, false, &it->second, (hipStream_t)stream, k[0], k[1], k[2], k[3]);
        VDA_TRY(level ? r.rebuild_level(lvl) : r.rebuild_p1c());
    }
    VDA_HIP(hipMemcpyAsync(dst, (char*)h->ws + b->second.first, (size_t)bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

// The options, their value conventions and their defaults: the OPTIONS table above.
extern "C" int vda_set_option(vda_model* h, const char* name, int value) {
    VDA_REQUIRE(h && name, "vda_set_option: null argument");
    if (strcmp(name, "profile_min_gflop") == 0) {       // vda_profile_start brackets only launches of at least this many GFLOP
        h->prof.min_flops = 1e9 * value;
        return 0;
    }
    for (const Option& o : OPTIONS) {
        if (strcmp(name, o.name) != 0) continue;
        h->*o.field = !o.flag ? value : (value < 0 && o.dflt) ? o.dflt(h) : value != 0;
        if (o.relayout) h->layouts.clear();
        return 0;
    }
    vda_set_error("vda_set_option: unknown option %s", name);
    return 1;
}

// ---- bench.py's per-kernel timing of the GEMM / conv launches inside vda_forward
extern "C" int vda_profile_start(vda_model* h, int every) {
    VDA_REQUIRE(h && every > 0, "vda_profile_start: bad arguments");
    VDA_REQUIRE(h->prof.samples.empty(), "vda_profile_start: a profile is already open");
    const double keep = h->prof.min_flops;
    h->prof = Profile();
    h->prof.every = every;
    h->prof.min_flops = keep;
    return 0;
}

// Closes the profile and writes one JSON object {kernel name: {"launches", "flops", "timed", "timed_ms", "timed_flops"}} into
// `json` (NUL-terminated, at most `cap` bytes). Synchronises on the recorded events.
static int vda_profile_stop_impl(vda_model* h, char* json, int cap) {
    VDA_REQUIRE(h && json && cap > 2, "vda_profile_stop: bad arguments");
    Profile& pf = h->prof;
    struct Agg {
        long long timed = 0;
        double ms = 0.0, flops = 0.0;
    };
    std::map<std::string, Agg> agg;
    for (ProfSample& sm : pf.samples) {
        float ms = 0.f;
        hipError_t e = hipEventSynchronize(sm.e1);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, sm.e0, sm.e1);
        (void)hipEventDestroy(sm.e0);
        (void)hipEventDestroy(sm.e1);
        if (e != hipSuccess) continue;
        Agg& a = agg[sm.name];
        a.timed += 1;
        a.ms += ms;
        a.flops += sm.flops;
    }
    std::string out = "{";
    bool first = true;
    for (const auto& kv : pf.launches) {
        const Agg& a = agg[kv.first];
        char line[512];
        snprintf(line, sizeof(line), "%s\"%s\": {\"launches\": %lld, \"flops\": %.6e, \"timed\": %lld, \"timed_ms\": %.6f, \"timed_flops\": %.6e}",
                 first ? "" : ", ", kv.first.c_str(), kv.second.first, kv.second.second, a.timed, a.ms, a.flops);
        out += line;
        first = false;
    }
    out += "}";
    h->prof = Profile();
    VDA_REQUIRE((int)out.size() + 1 <= cap, "vda_profile_stop: the report needs %d bytes", (int)out.size() + 1);
    memcpy(json, out.c_str(), out.size() + 1);
    return 0;
}

extern "C" int vda_load_weight(vda_model* h, const char* name, const void* ptr, const int64_t* dims, int ndim, int dtype) {
    return guarded("vda_load_weight", 3, [&] { return vda_load_weight_impl(h, name, ptr, dims, ndim, dtype); });
}
extern "C" int vda_finalize_weights(vda_model* h) { return guarded("vda_finalize_weights", 3, [&] { return vda_finalize_weights_impl(h); }); }
extern "C" int vda_prepare(vda_model* h, int B, int T, int H, int W, int precision) {
    return guarded("vda_prepare", 3, [&] { return vda_prepare_impl(h, B, T, H, W, precision); });
}
extern "C" int vda_forward(vda_model* h, const float* in, float* out, int B, int T, int H, int W, int precision, vda_stream_t stream) {
    return guarded("vda_forward", 3, [&] { return vda_forward_impl(h, in, out, B, T, H, W, precision, stream); });
}
extern "C" int vda_debug_copy(vda_model* h, const char* name, void* dst, int64_t bytes, vda_stream_t stream) {
    return guarded("vda_debug_copy", 3, [&] { return vda_debug_copy_impl(h, name, dst, bytes, stream); });
}
extern "C" int vda_profile_stop(vda_model* h, char* json, int cap) {
    return guarded("vda_profile_stop", 3, [&] { return vda_profile_stop_impl(h, json, cap); });
}
extern "C" int64_t vda_workspace_bytes(vda_model* h, int B, int T, int H, int W, int precision) {
    return guarded("vda_workspace_bytes", (int64_t)-1, [&] { return vda_workspace_bytes_impl(h, B, T, H, W, precision); });
}
