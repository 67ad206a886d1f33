// The checkpoint's tensors, each described once: its name and shape in the flat fp32 state dict run.py:46 loads (dinov2.py:106-168,
// dpt.py:60-124, util/blocks.py:20-32,52-58,124-129, motion_module/motion_module.py:84-100,141-161,194, motion_module/attention.py:
// 81-91,333,374) and how the handle packs it for the kernels. csrc/host.hip loops over this table twice: name -> shape is the spec that
// vda_load_weight checks against, kind / key / paddings drive the pack kernels. True sizes are read from the shape, never restated.
// Plain C++17 without HIP: tests/weight_table_main.cpp prints the table on the host, tests/test_weight_table_host.py compares it with
// weights.state_dict_spec. Weights made of SEVERAL tensors (LayerNorm / BatchNorm / ConvTranspose / oc1_mix folds) are not rows here:
// host.hip builds them in pack_derived.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/vda.h"

constexpr int PATCH = 14, POS_GRID = 37, KPATCH = 640;
inline int pad64(int c) { return (c + 63) / 64 * 64; }
inline int weight_fhp(const vda_config& c) { return (c.features / 2 + 31) / 32 * 32; }      // output_conv1's width: only the depth tail (32-channel passes) consumes it

enum WKind {
    W_NONE,            // not packed from this row (read raw, unused, or an input of pack_derived)
    W_VEC,             // fp32 vector = one row of K elements, zero padded to kpad; packed once, shared by both precisions (as every *_BIAS kind)
    W_MAT,             // [N, K] -> [npad, kpad]
    W_ROWS,            // [N, K] -> rows row .. row + N of the key that several tensors share, [npad, kpad] as a whole
    W_CONV3,           // Conv2d [Co, Ci, 3, 3] -> [npad = Copad, (ky, kx, ci) = 9 * kpad]
    W_CONVT,           // ConvTranspose2d (k == stride) [Ci, Co, k, k] -> [(ky, kx, co) = k * k * npad, ci = kpad]
    W_CONVT_BIAS,      // its bias [Co], padded to kpad and repeated per tap: npad = k * k * kpad elements
    W_GEGLU,           // GEGLU proj [2n, K], rows [value | gate] -> interleaved [16 value | 16 gate] per 32 rows
    W_GEGLU_BIAS       // its bias [2n], interleaved alike
};

struct WEntry {
    std::string name;
    std::vector<int64_t> shape;
    WKind kind;
    std::string key;           // of Run::W() / Run::V()
    int npad, kpad, row;       // 0 in add(): the true size
    int64_t numel() const {
        int64_t n = 1;
        for (int64_t d : shape) n *= d;
        return n;
    }
    int N() const { return shape.size() < 2 ? 1 : (int)shape[0]; }        // a vector is a matrix of one row
    int K() const { return (int)(numel() / N()); }
    bool is_vec() const { return kind == W_VEC || kind == W_CONVT_BIAS || kind == W_GEGLU_BIAS; }
    size_t packed_elems() const {                                           // of the whole key
        const size_t kk = kind == W_CONV3 ? 9 : kind == W_CONVT ? (size_t)(shape[2] * shape[3]) : 1;
        return kind == W_CONVT_BIAS ? (size_t)npad : kk * npad * kpad;
    }
};

struct WeightTable {
    std::vector<WEntry> rows;
    int ocp[4], Fhp;
    void add(std::string name, std::vector<int64_t> shape, WKind kind = W_NONE, std::string key = "", int npad = 0, int kpad = 0, int row = 0) {
        rows.push_back(WEntry{std::move(name), std::move(shape), kind, std::move(key), npad, kpad, row});
        WEntry& e = rows.back();
        if (npad == 0) e.npad = e.N();
        if (kpad == 0) e.kpad = kind == W_CONV3 ? (int)e.shape[1] : e.K();
    }

    explicit WeightTable(const vda_config& c) {
        const int64_t D = c.embed_dim, F = c.features;
        const int* oc = c.out_channels;
        for (int i = 0; i < 4; ++i) ocp[i] = pad64(oc[i]);
        Fhp = weight_fhp(c);
        auto n = [](int i) { return std::to_string(i); };
        const std::string p = "pretrained.";
        add(p + "cls_token", {1, 1, D}, W_VEC, "cls");
        add(p + "pos_embed", {1, POS_GRID * POS_GRID + 1, D});                 // resampled per grid in vda_prepare
        add(p + "mask_token", {1, D});                                         // unused in inference
        add(p + "patch_embed.proj.weight", {D, 3, PATCH, PATCH}, W_MAT, "patch.w", 0, KPATCH);
        add(p + "patch_embed.proj.bias", {D}, W_VEC, "patch.b");
        for (int i = 0; i < c.depth; ++i) {
            const std::string b = p + "blocks." + n(i) + ".", k = "b" + n(i) + ".";
            add(b + "norm1.weight", {D}, W_VEC, k + "norm1.weight");
            add(b + "norm1.bias", {D}, W_VEC, k + "norm1.bias");
            add(b + "attn.qkv.weight", {3 * D, D}, W_MAT, k + "attn.qkv.weight");
            add(b + "attn.qkv.bias", {3 * D}, W_VEC, k + "attn.qkv.bias");
            add(b + "attn.proj.weight", {D, D}, W_MAT, k + "attn.proj.weight");
            add(b + "attn.proj.bias", {D}, W_VEC, k + "attn.proj.bias");
            add(b + "ls1.gamma", {D}, W_VEC, k + "ls1.gamma");
            add(b + "norm2.weight", {D}, W_VEC, k + "norm2.weight");
            add(b + "norm2.bias", {D}, W_VEC, k + "norm2.bias");
            add(b + "mlp.fc1.weight", {4 * D, D}, W_MAT, k + "mlp.fc1.weight");
            add(b + "mlp.fc1.bias", {4 * D}, W_VEC, k + "mlp.fc1.bias");
            add(b + "mlp.fc2.weight", {D, 4 * D}, W_MAT, k + "mlp.fc2.weight");
            add(b + "mlp.fc2.bias", {D}, W_VEC, k + "mlp.fc2.bias");
            add(b + "ls2.gamma", {D}, W_VEC, k + "ls2.gamma");
        }
        add(p + "norm.weight", {D}, W_VEC, "norm.w");
        add(p + "norm.bias", {D}, W_VEC, "norm.b");
        const std::string h = "head.";
        for (int i = 0; i < 4; ++i) {
            add(h + "projects." + n(i) + ".weight", {oc[i], D, 1, 1}, W_MAT, "proj" + n(i) + ".w", ocp[i]);
            add(h + "projects." + n(i) + ".bias", {oc[i]}, W_VEC, "proj" + n(i) + ".b", 1, ocp[i]);
        }
        for (int i = 0; i < 2; ++i) {                                            // ConvTranspose2d: [Cin, Cout, k, k]
            const int k = i == 0 ? 4 : 2;
            add(h + "resize_layers." + n(i) + ".weight", {oc[i], oc[i], k, k}, W_CONVT, "resize" + n(i) + ".w", ocp[i], ocp[i]);
            add(h + "resize_layers." + n(i) + ".bias", {oc[i]}, W_CONVT_BIAS, "resize" + n(i) + ".b", k * k * ocp[i], ocp[i]);
        }
        add(h + "resize_layers.3.weight", {oc[3], oc[3], 3, 3}, W_CONV3, "resize3.w", ocp[3], ocp[3]);
        add(h + "resize_layers.3.bias", {oc[3]}, W_VEC, "resize3.b", 1, ocp[3]);
        if (c.use_clstoken)                                                      // dpt.py:92-98
            for (int i = 0; i < 4; ++i) {
                add(h + "readout_projects." + n(i) + ".0.weight", {D, 2 * D}, W_MAT, "readout" + n(i) + ".w");
                add(h + "readout_projects." + n(i) + ".0.bias", {D}, W_VEC, "readout" + n(i) + ".b");
            }
        const std::string sc = h + "scratch.";
        for (int i = 0; i < 4; ++i) add(sc + "layer" + n(i + 1) + "_rn.weight", {F, oc[i], 3, 3}, W_CONV3, "rn" + n(i + 1) + ".w", 0, ocp[i]);
        // use_bn: a resConfUnit conv is packed with its BatchNorm folded in, by pack_derived
        const WKind conv = c.use_bn ? W_NONE : W_CONV3, bias = c.use_bn ? W_NONE : W_VEC;
        for (int i = 1; i <= 4; ++i) {
            const std::string r = sc + "refinenet" + n(i) + ".", k = "ref" + n(i) + ".";
            add(r + "out_conv.weight", {F, F, 1, 1}, W_MAT, k + "out.w");
            add(r + "out_conv.bias", {F}, W_VEC, k + "out.b");
            for (int u = 1; u <= 2; ++u)
                for (int cc = 1; cc <= 2; ++cc) {
                    const std::string rn = r + "resConfUnit" + n(u) + ".conv" + n(cc), kn = k + "rcu" + n(u) + ".c" + n(cc);
                    add(rn + ".weight", {F, F, 3, 3}, conv, c.use_bn ? "" : kn + ".w");
                    add(rn + ".bias", {F}, bias, c.use_bn ? "" : kn + ".b");
                    if (!c.use_bn) continue;                                     // util/blocks.py:60-62 (state_dict keys of nn.BatchNorm2d)
                    const std::string bn = r + "resConfUnit" + n(u) + ".bn" + n(cc) + ".";
                    for (const char* t : {"weight", "bias", "running_mean", "running_var"}) add(bn + t, {F});
                    add(bn + "num_batches_tracked", {});
                }
        }
        add(sc + "output_conv1.weight", {F / 2, F, 3, 3}, W_CONV3, "oc1.w", Fhp);
        add(sc + "output_conv1.bias", {F / 2}, W_VEC, "oc1.b", 1, Fhp);
        add(sc + "output_conv2.0.weight", {32, F / 2, 3, 3}, W_CONV3, "oc2.w", 0, Fhp);
        add(sc + "output_conv2.0.bias", {32}, W_VEC, "oc2.b");
        add(sc + "output_conv2.2.weight", {1, 32, 1, 1}, W_VEC, "oc3.w");
        add(sc + "output_conv2.2.bias", {1});                                    // read to the host in vda_finalize_weights
        const int64_t tc[4] = {oc[2], oc[3], F, F};                              // dpt_temporal.py:42-51 (vda_create: multiples of 64, never padded)
        for (int m = 0; m < 4; ++m) {
            const int64_t C = tc[m];
            const std::string t = h + "motion_modules." + n(m) + ".temporal_transformer.", tb = t + "transformer_blocks.0.", k = "tm" + n(m) + ".";
            add(t + "norm.weight", {C}, W_VEC, k + "gn.w");
            add(t + "norm.bias", {C}, W_VEC, k + "gn.b");
            add(t + "proj_in.weight", {C, C}, W_MAT, k + "in.w");
            add(t + "proj_in.bias", {C}, W_VEC, k + "in.b");
            for (int a = 0; a < 2; ++a) {
                const std::string ab = tb + "attention_blocks." + n(a) + ".", ka = k + "a" + n(a) + ".";
                int j = 0;
                for (const char* q : {"to_q.weight", "to_k.weight", "to_v.weight"})   // fused to one [3C, C]
                    add(ab + q, {C, C}, W_ROWS, ka + "qkv.w", 3 * (int)C, 0, (int)C * j++);
                add(ab + "to_out.0.weight", {C, C}, W_MAT, ka + "out.w");
                add(ab + "to_out.0.bias", {C}, W_VEC, ka + "out.b");
                if (!c.pe_rope) add(ab + "pos_encoder.pe", {1, c.num_frames, C}, W_VEC, ka + "pe");      // (rope: freqs_cis is not a buffer, motion_module.py:221-224)
                add(tb + "norms." + n(a) + ".weight", {C}, W_VEC, ka + "ln.w");
                add(tb + "norms." + n(a) + ".bias", {C}, W_VEC, ka + "ln.b");
            }
            add(tb + "ff.net.0.proj.weight", {8 * C, C}, W_GEGLU, k + "ff1.w");
            add(tb + "ff.net.0.proj.bias", {8 * C}, W_GEGLU_BIAS, k + "ff1.b");
            add(tb + "ff.net.2.weight", {C, 4 * C}, W_MAT, k + "ff2.w");
            add(tb + "ff.net.2.bias", {C}, W_VEC, k + "ff2.b");
            add(tb + "ff_norm.weight", {C}, W_VEC, k + "ffln.w");
            add(tb + "ff_norm.bias", {C}, W_VEC, k + "ffln.b");
            add(t + "proj_out.weight", {C, C}, W_MAT, k + "out.w");
            add(t + "proj_out.bias", {C}, W_VEC, k + "out.b");
        }
    }
};
