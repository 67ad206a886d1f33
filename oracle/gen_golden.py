"""Generate tests/golden/*.npz by running the REFERENCE's own modules.

Runs only in the build container (needs /root/reference, never shipped to the
GPU box). The reference is imported, not copied: we load our seeded synthetic
state dict into its modules with load_state_dict(strict=True) — which also
proves our key/shape inventory equals the reference's — run its forward /
infer_video_depth, and save inputs + outputs as data.

Harness shims (none of them replaces arithmetic on the pinned path):
  easydict     -> dict subclass (only used as **kwargs, dpt_temporal.py:35-48)
  torchvision  -> transforms.Compose = call each transform in turn
  cv2          -> INTER_* constants + resize() that asserts identity size
`VideoDepthAnything.__init__` is skipped (video_depth.py:60 is a network fetch);
the object is assembled as `pretrained = DINOv2(encoder)`, `head = DPTHeadTemporal(...)`,
which is what the commented upstream constructor at :59 and metric_depth/...:54 do.

Usage:  python oracle/gen_golden.py [--metric] [--check]
  --check   regenerate into a temporary directory and assert that every array equals the committed fixture bit for bit
            (tests/test_oracle_golden.py runs this when /root/reference is present).
"""
import argparse
import os
import sys
import types
from functools import partial

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "tests", "golden")


def install_shims():
    ed = types.ModuleType("easydict")

    class EasyDict(dict):
        pass

    ed.EasyDict = EasyDict
    sys.modules["easydict"] = ed

    tv = types.ModuleType("torchvision")
    tvt = types.ModuleType("torchvision.transforms")

    class Compose:
        def __init__(self, ts):
            self.ts = ts

        def __call__(self, x):
            for t in self.ts:
                x = t(x)
            return x

    tvt.Compose = Compose
    tv.transforms = tvt
    sys.modules["torchvision"] = tv
    sys.modules["torchvision.transforms"] = tvt

    cv2 = types.ModuleType("cv2")
    cv2.INTER_CUBIC, cv2.INTER_AREA, cv2.INTER_NEAREST = 2, 3, 0

    def resize(img, size, interpolation=None):
        assert (img.shape[1], img.shape[0]) == tuple(size), "golden generator only covers identity resize"
        return img

    cv2.resize = resize
    sys.modules["cv2"] = cv2


def build_reference(cfg, sd, ref_root):
    sys.path.insert(0, ref_root)
    # `utils` must resolve to the reference's namespace package (utils/util.py), not to this repo's utils/ directory:
    # drop anything cached under that name and let the import system merge the two directories (neither has __init__.py).
    for k in [k for k in sys.modules if k == "utils" or k.startswith("utils.")]:
        del sys.modules[k]
    import torch.nn as nn
    from video_depth_anything import video_depth as vd
    from video_depth_anything.dinov2 import DINOv2, DinoVisionTransformer
    from video_depth_anything.dinov2_layers import MemEffAttention, NestedTensorBlock as Block
    from video_depth_anything.dpt_temporal import DPTHeadTemporal

    m = vd.VideoDepthAnything.__new__(vd.VideoDepthAnything)
    nn.Module.__init__(m)
    m.intermediate_layer_idx = {cfg.name: list(cfg.taps)}
    m.encoder = cfg.name
    if cfg.name in ("vits", "vitl"):
        m.pretrained = DINOv2(model_name=cfg.name)
    else:
        m.pretrained = DinoVisionTransformer(
            img_size=518, patch_size=14, embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads,
            mlp_ratio=4, block_fn=partial(Block, attn_class=MemEffAttention), init_values=1.0, ffn_layer="mlp",
            block_chunks=0, num_register_tokens=0, interpolate_antialias=False, interpolate_offset=0.1)
    m.head = DPTHeadTemporal(m.pretrained.embed_dim, cfg.features, cfg.use_bn, out_channels=list(cfg.out_channels),
                             use_clstoken=cfg.use_clstoken, num_frames=cfg.num_frames, pe=cfg.pe)
    m.load_state_dict(sd, strict=True)
    return m.eval()


def sd_checksum(sd):
    return np.array([float(v.double().abs().sum()) for v in sd.values()], dtype=np.float64)


def capture_stages(model):
    """Forward hooks on the head's submodules, in the order dpt_temporal.py calls them."""
    store = {}
    hs = []

    def hook(name):
        def f(mod, inp, out):
            store[name] = out.detach().clone()
        return f

    h = model.head
    hs.append(h.resize_layers[0].register_forward_hook(hook("layer_1")))
    hs.append(h.resize_layers[1].register_forward_hook(hook("layer_2")))
    for i, n in enumerate(("layer_3", "layer_4", "path_4", "path_3")):
        hs.append(h.motion_modules[i].register_forward_hook(hook(n + "_bcthw")))
    hs.append(h.scratch.refinenet2.register_forward_hook(hook("path_2")))
    hs.append(h.scratch.refinenet1.register_forward_hook(hook("path_1")))
    return store, hs


def autocast_fp16(fn):
    """The reference's fp32=False path (video_depth.py:203-205) as far as a CPU can run it: its own modules under
    torch.autocast(fp16). This is the ANCHOR of the fp16 tolerance (tests/test_forward_gpu.py): how far the reference's own
    half-precision path is from its fp32 path on the same input and weights. (On the CPU the fp32 island of dpt_temporal.py:97-100
    - `autocast(device_type="cuda", enabled=False)` - is not entered, so output_conv2 runs in fp16 here too.)"""
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.float16):
        return fn()


def video_autocast_fp16(model, frames, input_size):
    """infer_video_depth(fp32=False): the reference opens torch.autocast(device_type=device) itself (video_depth.py:204); on the
    CPU that defaults to bfloat16, so the CPU autocast dtype is set to float16 around the call."""
    old = torch.get_autocast_dtype("cpu")
    torch.set_autocast_dtype("cpu", torch.float16)
    try:
        d, _ = model.infer_video_depth(frames, 24, input_size=input_size, device="cpu", fp32=False)
    finally:
        torch.set_autocast_dtype("cpu", old)
    return d.astype(np.float32)


class _NetworkSize(Exception):
    def __init__(self, size):
        self.size = size


def index_logic(model):
    """Integer / index host logic of infer_video_depth, taken from the reference's OWN code paths (bit-exact tier):
      sizes   [n, 5] = (H0, W0, input_size, H, W): the network size its aspect guard (video_depth.py:167-171) and
              Resize.get_size (util/transform.py:51-107) arrive at - read off the cv2.resize call the transform makes;
      win_<n> [windows, 32]: the SOURCE frame every slot of every window holds (video_depth.py:187-201: padding with the last
              frame, stride 22, key-frame refill from the previous window's input), obtained by running the reference's loop on
              a video whose frame i has the value i written into its pixels (base-256 digits over the three channels) and a
              stand-in forward that only records what it is handed.
    The model's arithmetic plays no part: `forward` is replaced by the recorder, depth is zeros."""
    import cv2
    from video_depth_anything import video_depth as vd
    out = {"KEYFRAMES": np.array(vd.KEYFRAMES, dtype=np.int32), "INFER_LEN": np.int32(vd.INFER_LEN), "OVERLAP": np.int32(vd.OVERLAP),
           "INTERP_LEN": np.int32(vd.INTERP_LEN)}
    real_resize, real_forward = cv2.resize, model.__dict__.get("forward")

    def raise_size(img, size, interpolation=None):
        raise _NetworkSize(size)

    cv2.resize = raise_size
    cases = []
    try:
        hs = (14, 100, 240, 360, 480, 518, 600, 720, 1080, 1440, 2160)
        ws = (14, 100, 320, 426, 518, 640, 854, 1000, 1280, 1920, 1930, 2000, 2560, 3840)
        grid = [(h, w, s) for s in (518, 392, 280, 1022) for h in hs for w in ws]
        # either side of the 1.78 guard, both orientations; sides just under / over the input size; odd multiples of 14
        grid += [(1000, w, 518) for w in (1776, 1777, 1778, 1779, 1780, 1781, 1782, 1790)] + [(h, 1000, 518) for h in (1779, 1780, 1781, 1790)]
        grid += [(517, 517, 518), (519, 519, 518), (511, 525, 518), (525, 511, 518), (7, 7, 518), (21, 700, 518), (700, 21, 518), (533, 947, 518)]
        for (h0, w0, size) in grid:
            try:
                model.infer_video_depth(np.zeros((1, h0, w0, 3), dtype=np.uint8), 24, input_size=size, device="cpu", fp32=True)
                raise AssertionError("the transform did not call cv2.resize")
            except _NetworkSize as e:
                cases.append((h0, w0, size, e.size[1], e.size[0]))
    finally:
        cv2.resize = real_resize
    out["sizes"] = np.array(cases, dtype=np.int32)

    mean, std = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
    seen = []

    def recorder(x):                                     # x [1, 32, 3, 14, 14], normalised
        px = x[0, :, :, 0, 0].double().numpy() * std + mean
        digits = np.rint(px * 255.0).astype(np.int64)
        seen.append(digits[:, 0] + 256 * digits[:, 1] + 65536 * digits[:, 2])
        return torch.zeros(1, x.shape[1], x.shape[3], x.shape[4])

    model.forward = recorder
    try:
        for n in (1, 5, 22, 23, 32, 33, 54, 55, 100, 1024):
            idx = np.arange(n)
            frames = np.stack([idx & 255, (idx >> 8) & 255, (idx >> 16) & 255], axis=-1).astype(np.uint8)[:, None, None, :]
            frames = np.ascontiguousarray(np.broadcast_to(frames, (n, 14, 14, 3)))
            seen.clear()
            d, _ = model.infer_video_depth(frames, 24, input_size=14, device="cpu", fp32=True)
            assert d.shape == (n, 14, 14)
            out[f"win_{n}"] = np.stack(seen).astype(np.int32)
    finally:
        if real_forward is None:
            del model.forward
        else:
            model.forward = real_forward
    return out


def compare_dirs(fresh, committed):
    """Every array of every freshly generated fixture must equal the committed one exactly."""
    bad = []
    for name in sorted(os.listdir(fresh)):
        a, b = np.load(os.path.join(fresh, name)), np.load(os.path.join(committed, name))
        if sorted(a.files) != sorted(b.files):
            bad.append(f"{name}: keys differ")
            continue
        for k in a.files:
            if a[k].shape != b[k].shape or a[k].dtype != b[k].dtype or not np.array_equal(a[k], b[k]):
                bad.append(f"{name}:{k}")
    if bad:
        raise SystemExit("golden fixtures differ from a fresh run of the reference: " + ", ".join(bad))
    print("check ok:", ", ".join(sorted(os.listdir(fresh))), "are bit-identical to tests/golden")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--metric", action="store_true", help="generate the metric_depth stitch golden instead")
    ap.add_argument("--check", action="store_true", help="regenerate to a temp dir and compare with tests/golden bit for bit")
    args = ap.parse_args()
    global OUT
    committed = OUT
    if args.check:
        import tempfile
        OUT = tempfile.mkdtemp(prefix="vda_golden_")
    install_shims()
    from video_depth_anything_amd.config import get_config
    from video_depth_anything_amd.weights import synthetic_state_dict

    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(8)

    if args.metric:
        # metric_depth/ carries its own copy of the package; run it in a process of its own.
        cfg = get_config("tiny")
        sd = synthetic_state_dict(cfg, seed=6)
        model = build_reference(cfg, sd, "/root/reference/metric_depth")
        rng = np.random.default_rng(13)
        frames = rng.integers(0, 256, (50, 42, 56, 3), dtype=np.uint8)
        depths, _ = model.infer_video_depth(frames, 24, input_size=42, device="cpu", fp32=True)
        np.savez_compressed(os.path.join(OUT, "tiny_metric_video.npz"), frames=frames, depths=depths.astype(np.float32),
                            depths_autocast_fp16=video_autocast_fp16(model, frames, 42), sd_seed=6, sd_checksum=sd_checksum(sd), input_size=42)
        print("tiny_metric_video", depths.shape, float(depths.mean()))
        if args.check:
            compare_dirs(OUT, committed)
        return

    # ---- 1. tiny config, non-square input, every stage tapped --------------------
    cfg = get_config("tiny")
    sd = synthetic_state_dict(cfg, seed=1)
    model = build_reference(cfg, sd, "/root/reference")
    g = torch.Generator().manual_seed(101)
    x = torch.randn(1, 4, 3, 42, 56, generator=g)
    store, hooks = capture_stages(model)
    with torch.no_grad():
        taps = model.pretrained.get_intermediate_layers(x.flatten(0, 1), list(cfg.taps), return_class_token=True)
        depth = model.forward(x)
    for h in hooks:
        h.remove()
    out = {"x": x.numpy(), "depth": depth.numpy(), "sd_seed": 1, "sd_checksum": sd_checksum(sd)}
    for i, (t, c) in enumerate(taps):
        out[f"tap{i}"] = t.numpy()
    for k, v in store.items():
        if k.endswith("_bcthw"):                        # [B,C,T,h,w] -> frame-major [(B T),C,h,w]
            v = v.permute(0, 2, 1, 3, 4).flatten(0, 1)
            k = k[:-6]
        out[k] = v.numpy()
    # the fp16 anchor of every array above (same hooks, the reference's modules under fp16 autocast)
    store16, hooks = capture_stages(model)
    taps16, depth16 = autocast_fp16(lambda: (model.pretrained.get_intermediate_layers(x.flatten(0, 1), list(cfg.taps), return_class_token=True),
                                             model.forward(x)))
    for h in hooks:
        h.remove()
    out["depth_autocast_fp16"] = depth16.float().numpy()
    for i, (t, c) in enumerate(taps16):
        out[f"tap{i}_autocast_fp16"] = t.float().numpy()
    for k, v in store16.items():
        if k.endswith("_bcthw"):
            v = v.permute(0, 2, 1, 3, 4).flatten(0, 1)
            k = k[:-6]
        out[k + "_autocast_fp16"] = v.float().numpy()
    np.savez_compressed(os.path.join(OUT, "tiny_forward.npz"), **out)
    print("tiny_forward", depth.shape, float(depth.mean()), {k: v.shape for k, v in out.items() if hasattr(v, "shape")})

    # ---- 2. tiny config: infer_video_depth, 3 windows ----------------------------
    sd = synthetic_state_dict(cfg, seed=2)
    model.load_state_dict(sd, strict=True)
    rng = np.random.default_rng(12)
    frames = rng.integers(0, 256, (50, 42, 56, 3), dtype=np.uint8)
    depths, fps = model.infer_video_depth(frames, 24, input_size=42, device="cpu", fp32=True)
    np.savez_compressed(os.path.join(OUT, "tiny_video.npz"), frames=frames, depths=depths.astype(np.float32),
                        depths_autocast_fp16=video_autocast_fp16(model, frames, 42), sd_seed=2, sd_checksum=sd_checksum(sd), input_size=42)
    # ---- 2b. integer / index host logic from the reference's own loop (no arithmetic of the model involved)
    np.savez_compressed(os.path.join(OUT, "index_logic.npz"), **index_logic(model))
    print("index_logic", "written")
    print("tiny_video", depths.shape, depths.dtype, float(depths.mean()), fps)

    # ---- 3. real ViT-S, small non-square clip ------------------------------------
    cfg = get_config("vits")
    sd = synthetic_state_dict(cfg, seed=0)
    model = build_reference(cfg, sd, "/root/reference")
    g = torch.Generator().manual_seed(102)
    x = torch.randn(1, 3, 3, 56, 70, generator=g)
    with torch.no_grad():
        depth = model.forward(x)
    np.savez_compressed(os.path.join(OUT, "vits_forward.npz"), x=x.numpy(), depth=depth.numpy(),
                        depth_autocast_fp16=autocast_fp16(lambda: model.forward(x)).float().numpy(), sd_seed=0, sd_checksum=sd_checksum(sd))
    print("vits_forward", depth.shape, float(depth.mean()))

    # ---- 3b. the same clip through the outlier state dicts of tests/_outliers.py: depth and its fp16 anchor per kind ----
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from _outliers import outlier_state_dict
    ref_root = os.path.dirname(os.path.dirname(os.path.abspath(sys.modules["video_depth_anything.video_depth"].__file__)))
    out = {}
    for kind in ("channels", "offset", "both"):
        osd = outlier_state_dict(cfg, seed=21, kind=kind)
        omodel = build_reference(cfg, osd, ref_root)                        # (section 4 goes on with `model` and `sd` above)
        with torch.no_grad():
            out[f"{kind}_depth"] = omodel.forward(x).numpy()
        out[f"{kind}_depth_autocast_fp16"] = autocast_fp16(lambda: omodel.forward(x)).float().numpy()
        out[f"{kind}_sd_checksum"] = sd_checksum(osd)
    np.savez_compressed(os.path.join(OUT, "vits_outlier_forward.npz"), x_seed=102, sd_seed=21, **out)
    print("vits_outlier_forward", ", ".join(f"{k} {float(v.mean())}" for k, v in out.items() if k.endswith("_depth")))

    # ---- 4. real ViT-S, one 518x518 frame (stored pos_embed path, 1370 tokens) ----
    g = torch.Generator().manual_seed(103)
    x = torch.randn(1, 1, 3, 518, 518, generator=g)
    with torch.no_grad():
        depth = model.forward(x)
    d = depth.numpy()
    d16 = autocast_fp16(lambda: model.forward(x)).float().numpy()
    np.savez_compressed(os.path.join(OUT, "vits_518.npz"), x_seed=103, depth_sub=d[..., ::7, ::7], depth_sub_autocast_fp16=d16[..., ::7, ::7],
                        row_sums_autocast_fp16=d16.sum(axis=-1).astype(np.float64),
                        depth_mean=float(d.mean()), depth_absmax=float(np.abs(d).max()),
                        row_sums=d.sum(axis=-1).astype(np.float64), sd_seed=0, sd_checksum=sd_checksum(sd))
    print("vits_518", depth.shape, float(depth.mean()))

    # ---- 4b. tiny config with use_clstoken=True (readout projections, dpt_temporal.py:56-59) -----------------------------
    cfg = get_config("tiny", use_clstoken=True)
    sd = synthetic_state_dict(cfg, seed=4)
    model = build_reference(cfg, sd, "/root/reference")
    x = torch.randn(1, 3, 3, 42, 56, generator=torch.Generator().manual_seed(104))
    store, hooks = capture_stages(model)
    with torch.no_grad():
        depth = model.forward(x)
    for h in hooks:
        h.remove()
    store16, hooks = capture_stages(model)
    depth16 = autocast_fp16(lambda: model.forward(x))
    for h in hooks:
        h.remove()
    np.savez_compressed(os.path.join(OUT, "tiny_clstoken_forward.npz"), x=x.numpy(), depth=depth.numpy(), layer_1=store["layer_1"].numpy(),
                        layer_2=store["layer_2"].numpy(), depth_autocast_fp16=depth16.float().numpy(),
                        layer_1_autocast_fp16=store16["layer_1"].float().numpy(), layer_2_autocast_fp16=store16["layer_2"].float().numpy(),
                        sd_seed=4, sd_checksum=sd_checksum(sd))
    print("tiny_clstoken_forward", depth.shape, float(depth.mean()))

    # ---- 4c / 4d. the two remaining constructor switches of video_depth.py:38-50 (no released configuration sets them): use_bn=True
    # (BatchNorm2d after each conv of the fusion blocks' ResidualConvUnits, util/blocks.py:60-62,80-86; eval mode, random running
    # statistics) and pe='rope' (rotary embedding of q and k in the temporal attention, motion_module.py:221-224,254-257)
    for tag, kw, sd_seed, x_seed in (("tiny_bn_forward", dict(use_bn=True), 6, 105), ("tiny_rope_forward", dict(pe="rope"), 7, 106)):
        cfg = get_config("tiny", **kw)
        sd = synthetic_state_dict(cfg, seed=sd_seed)
        model = build_reference(cfg, sd, "/root/reference")
        x = torch.randn(1, 4, 3, 42, 56, generator=torch.Generator().manual_seed(x_seed))
        store, hooks = capture_stages(model)
        with torch.no_grad():
            depth = model.forward(x)
        for h in hooks:
            h.remove()
        store16, hooks = capture_stages(model)
        depth16 = autocast_fp16(lambda: model.forward(x))
        for h in hooks:
            h.remove()
        frames_major = lambda v: v.permute(0, 2, 1, 3, 4).flatten(0, 1)          # [B,C,T,h,w] -> [(B T),C,h,w]
        np.savez_compressed(os.path.join(OUT, tag + ".npz"), x=x.numpy(), depth=depth.numpy(), path_2=store["path_2"].numpy(),
                            path_1=store["path_1"].numpy(), layer_3=frames_major(store["layer_3_bcthw"]).numpy(),
                            depth_autocast_fp16=depth16.float().numpy(), path_2_autocast_fp16=store16["path_2"].float().numpy(),
                            path_1_autocast_fp16=store16["path_1"].float().numpy(),
                            layer_3_autocast_fp16=frames_major(store16["layer_3_bcthw"]).float().numpy(), sd_seed=sd_seed,
                            sd_checksum=sd_checksum(sd))
        print(tag, depth.shape, float(depth.mean()))

    # ---- 5. stitcher maths directly (utils/util.py) -------------------------------
    from utils.util import compute_scale_and_shift, get_interpolate_frames
    rng = np.random.default_rng(14)
    pred = rng.random((2 * 30, 40), dtype=np.float32) * 5
    targ = (pred * 1.7 + 0.3 + rng.normal(0, 0.05, pred.shape)).astype(np.float32)
    s, t = compute_scale_and_shift(pred, targ, np.ones_like(targ) == 1)
    pre = [rng.random((6, 5), dtype=np.float32) for _ in range(8)]
    post = [rng.random((6, 5), dtype=np.float32) for _ in range(8)]
    mix = get_interpolate_frames(pre, post)
    np.savez_compressed(os.path.join(OUT, "stitch_math.npz"), pred=pred, targ=targ, scale=np.float64(s), shift=np.float64(t),
                        pre=np.stack(pre), post=np.stack(post), mix=np.stack(mix))
    print("stitch_math", s, t)
    if args.check:
        compare_dirs(OUT, committed)


if __name__ == "__main__":
    main()
