"""Depth videos as colour (or gray) frames: the mapping of the reference's utils/dc_utils.py save_video - the video's global range to
uint8, then matplotlib's 256-entry inferno table - with the bytes made on the device (csrc/visualize.hip).

The contract. For every pixel d (float32) and the range [d_min, d_max] (float32), every operation rounded to float32 once:

    span = d_max - d_min;  if not span > 0: span = 1e-12          a constant video maps to 0
    v    = ((d - d_min) / span) * 255                             the IEEE division, no reciprocal, no fused multiply-add
    k    = 0 if v is NaN or v < 0,  255 if v >= 255,  else v truncated
    out  = k (grayscale)  or  table[k] (three bytes, RGB)

For finite depth inside [d_min, d_max] this is the reference's `((d - d_min) / (d_max - d_min) * 255).astype(np.uint8)` followed by
`(colormap[norm] * 255).astype(np.uint8)`, which is `table[norm]` with table = (colormap * 255).astype(uint8) - one uint8 gather.
The clamp only defines what numpy's astype leaves to the machine (NaN, +-inf, values outside a range that was handed in).
`inferno_table()` is that table as the reference computes it from matplotlib; its 768 bytes ship in this module so that the
colours do not depend on matplotlib being installed (tests/golden/vis_frames.npz holds the table the reference used and the
frames its writer received; tests/test_visualize_numpy.py compares both).

The range, when not given, is the input's own minimum and maximum (they do not round): for numpy input the block-wise host
pass save_video has always made (numpy's min / max: a NaN in the input makes the range NaN and every pixel 0); for a CUDA tensor
vda_minmax_accum_f32 on the same stream, which never takes a NaN. A given range is rounded to float32.

`colorize_numpy` is the host twin: no GPU, the same bytes as `colorize`. Pixel counts past 2^31 in one call are untested.
"""
import numpy as np

from . import staging

_BLOCK_PIXELS = 1 << 25                       # pixels staged at a time by the numpy paths: 128 MB of depth, 96 MB of colour

_INFERNO = bytes.fromhex(
    "00000300000400000601000701010901010b02010e02021003021204031404031605041806041b07051d08061f0906210a07230b07260d08280e082a0f092d10"
    "092f120a32130a34140b36160b39170b3b190b3e1a0b401c0c431d0c451f0c47200c4a220b4c240b4e260b50270b52290b542b0a562d0a582e0a5a300a5c3209"
    "5d34095f3509603709613909623b09643c09653e0966400966410967430a68450a69460a69480b6a4a0b6a4b0c6b4d0c6b4f0d6c500d6c520e6c530e6d550f6d"
    "570f6d58106d5a116d5b116e5d126e5f126e60136e62146e63146e65156e66156e68166e6a176e6b176e6d186e6e186e70196e72196d731a6d751b6d761b6d78"
    "1c6d7a1c6d7b1d6c7d1d6c7e1e6c801f6b811f6b83206b85206a86216a88216a8922698b22698d23698e24689024689125679325679526669626669827659928"
    "649b28649c29639e2963a02a62a12b61a32b61a42c60a62c5fa72d5fa92e5eab2e5dac2f5cae305baf315bb1315ab23259b43358b53357b73456b83556ba3655"
    "bb3754bd3753be3852bf3951c13a50c23b4fc43c4ec53d4dc73e4cc83e4bc93f4acb4049cc4148cd4247cf4446d04544d14643d24742d44841d54940d64a3fd7"
    "4b3ed94d3dda4e3bdb4f3adc5039dd5238de5337df5436e05634e25733e35832e45a31e55b30e65c2ee65e2de75f2ce8612be9622aea6428eb6527ec6726ed68"
    "25ed6a23ee6c22ef6d21f06f1ff0701ef1721df2741cf2751af37719f37918f47a16f57c15f57e14f68012f68111f78310f7850ef8870df8880cf88a0bf98c09"
    "f98e08f99008fa9107fa9306fa9506fa9706fb9906fb9b06fb9d06fb9e07fba007fba208fba40afba60bfba80dfbaa0efbac10fbae12fbb014fbb116fbb318fb"
    "b51afbb71cfbb91efabb21fabd23fabf25fac128f9c32af9c52cf9c72ff8c931f8cb34f8cd37f7cf3af7d13cf6d33ff6d542f5d745f5d948f4db4bf4dc4ff3de"
    "52f3e056f3e259f2e45df2e660f1e864f1e968f1eb6cf1ed70f1ee74f1f079f1f27df2f381f2f485f3f689f4f78df5f891f6fa95f7fb99f9fc9dfafda0fcfea4")


def inferno_table():
    """uint8 [256,3]: (matplotlib's inferno colours * 255).astype(uint8), row k the RGB of level k. Read-only."""
    return np.frombuffer(_INFERNO, dtype=np.uint8).reshape(256, 3)


def _table(palette):
    if palette is None:
        return inferno_table()
    palette = np.asarray(palette.cpu() if hasattr(palette, "cpu") else palette)
    if palette.dtype != np.uint8 or palette.shape != (256, 3):
        raise ValueError(f"visualize: palette must be uint8 [256,3], got {palette.dtype} {palette.shape}")
    return np.ascontiguousarray(palette)


def _check(depths):
    if str(depths.dtype).replace("torch.", "") != "float32":
        raise ValueError(f"visualize: depths must be float32, got {depths.dtype}")
    shape = tuple(depths.shape)
    if len(shape) not in (2, 3) or 0 in shape:
        raise ValueError(f"visualize: depths must be [N,H,W] or [H,W] and not empty, got {shape}")
    return shape


def _blocks(n, px):
    b = staging.frames_per_block(n, px, _BLOCK_PIXELS)
    return [slice(i, min(i + b, n)) for i in range(0, n, b)]


def _host_range(frames, blocks, d_min, d_max):
    """(d_min, d_max) as float32; what is not given is the block-wise minimum / maximum of the input."""
    if d_min is None:
        d_min = min(frames[b].min() for b in blocks)
    if d_max is None:
        d_max = max(frames[b].max() for b in blocks)
    return np.float32(d_min), np.float32(d_max)


def _levels(block, lo, span):
    with np.errstate(invalid="ignore", over="ignore"):
        v = (block - lo) / span * np.float32(255)                  # float32 array with float32 scalars: three roundings
        assert v.dtype == np.float32
        v = np.where(v >= 0, v, np.float32(0))                     # NaN, or below the range
        v = np.where(v >= 255, np.float32(255), v)
    return v.astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- the host twin
def colorize_numpy(depths, d_min=None, d_max=None, grayscale=False, palette=None, device=None):
    """uint8 [N,H,W,3] (or [N,H,W] with grayscale; [H,W,3] / [H,W] for one frame) of float32 depths on the host. `device` is ignored."""
    depths = depths if isinstance(depths, np.ndarray) else np.asarray(depths)
    shape = _check(depths)
    table = None if grayscale else _table(palette)
    frames = depths.reshape((1,) + shape) if len(shape) == 2 else depths
    n, px = frames.shape[0], frames.shape[1] * frames.shape[2]
    blocks = _blocks(n, px)
    lo, hi = _host_range(frames, blocks, d_min, d_max)
    with np.errstate(invalid="ignore", over="ignore"):
        span = np.float32(hi - lo)
    if not span > 0:
        span = np.float32(1e-12)
    out = np.empty(frames.shape + (() if grayscale else (3,)), dtype=np.uint8)
    for b in blocks:
        k = _levels(np.asarray(frames[b]), lo, span)
        out[b] = k if grayscale else table[k]                      # one uint8 gather
    return out.reshape(shape + (() if grayscale else (3,)))


# ------------------------------------------------------------------------------------------------------------------ the device
def colorize(depths, d_min=None, d_max=None, grayscale=False, palette=None, device=None):
    """The same bytes as colorize_numpy, made by vda_depth_vis_u8. A CUDA tensor (float32 [N,H,W] or [H,W]) gives a CUDA uint8
    tensor on its device and stream; a range that is not given is found by vda_minmax_accum_f32 on that stream, with no host
    round trip. A numpy array or memory map gives a numpy array: the range is the host's block-wise min / max, and the frames go
    through one bounded pair of staging buffers a block at a time (`device`, default "cuda"), so a video that does not fit in
    memory or in one allocation still works."""
    import torch
    if not isinstance(depths, (torch.Tensor, np.ndarray)):
        depths = np.asarray(depths)
    shape = _check(depths)
    table = None if grayscale else _table(palette)
    is_tensor, dev = staging.placement(depths, device, "visualize", "colorize_numpy", "colorize")
    from . import ops
    ch = 1 if grayscale else 3
    out_shape = shape + (() if grayscale else (3,))
    with torch.cuda.device(dev):
        lut = None if grayscale else torch.from_numpy(np.array(table)).to(dev)
        if is_tensor:
            x = depths.contiguous()
            if d_min is None or d_max is None:
                minmax = torch.tensor([float("inf"), float("-inf")], dtype=torch.float32, device=dev)
                ops.minmax_accum(x, minmax)
                if d_min is not None:
                    minmax[0] = float(np.float32(d_min))
                if d_max is not None:
                    minmax[1] = float(np.float32(d_max))
            else:
                minmax = torch.tensor([float(np.float32(d_min)), float(np.float32(d_max))], dtype=torch.float32, device=dev)
            out = torch.empty(out_shape, dtype=torch.uint8, device=dev)
            ops.depth_vis(x, minmax, lut, out)
            return out
        frames = depths.reshape((1,) + shape) if len(shape) == 2 else depths
        n, px = frames.shape[0], frames.shape[1] * frames.shape[2]
        blocks = _blocks(n, px)
        lo, hi = _host_range(frames, blocks, d_min, d_max)
        minmax = torch.tensor([float(lo), float(hi)], dtype=torch.float32, device=dev)
        staged = staging.Staged(blocks[0].stop, frames.shape[1:], torch.float32, dev)
        host_out = torch.empty(staged.cap * px * ch, dtype=torch.uint8).pin_memory()
        dev_out = torch.empty(staged.cap * px * ch, dtype=torch.uint8, device=dev)
        out = np.empty(frames.shape + (() if grayscale else (3,)), dtype=np.uint8)
        flat_out = out.reshape(n, px * ch)
        for i, m, x in staged.blocks(frames):
            k = m * px * ch
            ops.depth_vis(x, minmax, lut, dev_out)
            host_out[:k].copy_(dev_out[:k], non_blocking=True)
            torch.cuda.current_stream().synchronize()
            np.copyto(flat_out[i:i + m].reshape(-1), host_out.numpy()[:k])
        return out.reshape(out_shape)
