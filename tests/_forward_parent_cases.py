"""Cases and the recording routine of tests/golden/forward_parent.npz, shared by tools/record_forward_parent.py (writes the fixture
with the PARENT of a restructuring of csrc/host.hip built) and tests/test_forward_parent_gpu.py (replays it, for equality).

What a case pins of vda_forward's launch sequence: the workspace size in both precisions, the set of GEMM / conv launches (kernel
name -> launches, FLOPs; the handle's own profile at every = 1), and the SHA-256 of the depth and of every stage vda_debug_copy
can name. The cases are the smallest shapes at which each branch of the sequence still runs (see the table below). Only what the
Python handle exposes is used: set_option, forward, workspace_bytes, profile_start / profile_stop, vda_debug_copy."""
import ctypes as C
import functools
import hashlib
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "forward_parent.npz")

# every option at the library's default (< 0: the default of the options that have an environment default)
DEFAULTS = {"residual_in_ln": 0, "ln_fold": 1, "dyn_sched": 0, "oc1_fused": 1, "mlp_fused": 0, "head_overlap": 0, "enc_split": -1,
            "head_lanes": -1, "convt_fold": -1, "oc1_mix": -1, "oc1_mix_chunk": 0}

# model key -> (encoder, config keywords, golden that holds the seed and the input or None, seed otherwise)
MODELS = {"tiny": ("tiny", {}, "tiny_forward.npz", None), "clstoken": ("tiny", {"use_clstoken": True}, "tiny_clstoken_forward.npz", None),
          "bn": ("tiny", {"use_bn": True}, "tiny_bn_forward.npz", None), "rope": ("tiny", {"pe": "rope"}, "tiny_rope_forward.npz", None),
          "vits": ("vits", {}, None, 21)}

FP32 = {"fp32": 1}          # (not an option of the handle: the precision argument of the forward)


def _cases():
    out = []
    # 1. tiny, the golden's input: every option that changes the sequence
    for opts in ({}, FP32, {"ln_fold": 0}, {"ln_fold": 0, "residual_in_ln": 1}, {"enc_split": 0}, {"head_lanes": 0}, {"head_overlap": 1},
                 {"convt_fold": 0}, {"oc1_mix": 0}, {"oc1_mix": 1}, {"oc1_mix": 1, "oc1_mix_chunk": 1}, {"oc1_fused": 0}, {"dyn_sched": 1}):
        out.append(("tiny", None, opts))
    # 2. use_clstoken: the readout per part and whole
    for opts in ({}, {"enc_split": 0}, {"ln_fold": 0}, FP32):
        out.append(("clstoken", None, opts))
    # 3. use_bn, pe = 'rope'
    for model in ("bn", "rope"):
        for opts in ({}, FP32):
            out.append((model, None, opts))
    # 4. clip shapes: BT < 2 (no split), odd halves, the per-clip loop of temporal attention
    for shape in ((1, 1, 42, 56), (1, 3, 42, 56), (2, 2, 42, 56)):
        out.append(("tiny", shape, {}))
    # 5. ViT-S at the shapes of tests/test_head_lanes_gpu.py ("vits70", "vits70x98")
    for shape in ((1, 4, 70, 70), (1, 4, 70, 98)):
        for opts in ({}, {"mlp_fused": 1}, {"enc_split": 0}, {"head_lanes": 0}):
            out.append(("vits", shape, opts))
    return out


def case_id(c):
    model, shape, opts = c
    return ".".join([model] + (["x".join(map(str, shape))] if shape else []) + [f"{k}={v}" for k, v in opts.items()])


CASES = _cases()
IDS = [case_id(c) for c in CASES]


@functools.lru_cache(maxsize=None)
def model(key):
    from video_depth_anything_amd.config import get_config
    from video_depth_anything_amd.video_depth import VideoDepthAnything
    from video_depth_anything_amd.weights import synthetic_state_dict
    enc, kw, golden, seed = MODELS[key]
    if golden is not None:
        seed = int(np.load(os.path.join(GOLDEN, golden))["sd_seed"])
    cfg = get_config(enc, **kw)
    m = VideoDepthAnything(encoder=enc, features=cfg.features, out_channels=list(cfg.out_channels), **kw)
    m.load_state_dict(synthetic_state_dict(cfg, seed=seed), strict=True)
    return m.to("cuda").eval()


@functools.lru_cache(maxsize=None)
def clip(key, shape):
    if shape is None:
        return torch.from_numpy(np.load(os.path.join(GOLDEN, MODELS[key][2]))["x"]).cuda()
    B, T, H, W = shape
    return torch.randn(B, T, 3, H, W, generator=torch.Generator().manual_seed(1000 * B + 100 * T + H + W)).cuda()


def _sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def stage_hashes(m, x, fp32):
    """SHA-256 of every stage of the last forward that vda_debug_copy can name (sizes as in tests/test_head_lanes_gpu.py::stages)."""
    from video_depth_anything_amd._lib import lib
    cfg = m.cfg
    BT, ph, pw = x.shape[0] * x.shape[1], x.shape[3] // 14, x.shape[4] // 14
    P, Fe, D = ph * pw, cfg.features, cfg.embed_dim
    ocp = [(c + 63) // 64 * 64 for c in cfg.out_channels]
    Fhp = (Fe // 2 + 31) // 32 * 32
    h4, w4 = (ph - 1) // 2 + 1, (pw - 1) // 2 + 1
    elems = {"tap0": P * D, "tap1": P * D, "tap2": P * D, "tap3": P * D, "l1": 16 * P * ocp[0], "l2": 4 * P * ocp[1], "l3t": P * ocp[2],
             "l4t": h4 * w4 * ocp[3], "l1r": 16 * P * Fe, "l2r": 4 * P * Fe, "l3r": P * Fe, "l4r": h4 * w4 * Fe, "p4": P * Fe, "p4t": P * Fe,
             "p3": 4 * P * Fe, "p3t": 4 * P * Fe, "p2": 16 * P * Fe, "p1c": 16 * P * Fe, "p1": 64 * P * Fe, "o1": 64 * P * Fhp}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {}
    for k, n in elems.items():
        t = torch.empty(BT * n, dtype=torch.float32 if fp32 else torch.int16, device="cuda")
        rc = lib.vda_debug_copy(m.engine._h, k.encode(), C.c_void_p(t.data_ptr()), t.numel() * t.element_size(), stream)
        if rc != 0 and k in ("p1c", "p1"):
            continue                                     # refinenet1's output has one of the two names (option oc1_fused, precision)
        assert rc == 0, f"vda_debug_copy({k}): {lib.vda_last_error().decode()}"
        out[k] = _sha(t)
    assert ("p1c" in out) != ("p1" in out), sorted(out)
    return out


def record(c):
    """One case: the record that the fixture holds, as a dict of JSON-able values. Runs two forwards; the second hashes like the first."""
    key, shape, opts = c
    m, x = model(key), clip(key, shape)
    fp32 = bool(opts.get("fp32", 0))
    for k, v in {**DEFAULTS, **{k: v for k, v in opts.items() if k != "fp32"}}.items():
        m.engine.set_option(k, v)
    B, T, _, H, W = x.shape
    rec = {"workspace_f16": m.engine.workspace_bytes(B, T, H, W, False), "workspace_f32": m.engine.workspace_bytes(B, T, H, W, True)}
    m.engine.profile_start(1)                           # (before the stage copies: a stage that is rebuilt launches a GEMM of its own)
    d = m.forward(x, fp32=fp32)
    rec["profile"] = {k: [v["launches"], v["flops"]] for k, v in sorted(m.engine.profile_stop().items())}
    rec["depth"], rec["stages"] = _sha(d), stage_hashes(m, x, fp32)
    d2 = m.forward(x, fp32=fp32)
    again = (_sha(d2), stage_hashes(m, x, fp32))
    assert again == (rec["depth"], rec["stages"]), f"{case_id(c)}: the second forward does not hash like the first"
    torch.cuda.synchronize()
    for k, v in DEFAULTS.items():
        m.engine.set_option(k, v)
    return rec
