"""vda_set_option("enc_split") (default on): the fp16 ln_fold encoder runs as two frame halves, half B on a handle-owned lane stream
forked after the token rows exist and joined back before the head. The encoder is exactly per frame and every half-GEMM is dispatched
as the whole-clip GEMM would be, so the split must be BIT-IDENTICAL to one launch chain: on the flagship clips, odd frame counts,
batches, the clstoken readout, two forwards in flight, a captured forward, and the overflow report."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def model_for(name, seed, **kw):
    from video_depth_anything_amd.config import get_config
    from video_depth_anything_amd.video_depth import VideoDepthAnything
    from video_depth_anything_amd.weights import synthetic_state_dict
    cfg = get_config(name, **kw)
    m = VideoDepthAnything(encoder=name, features=cfg.features, out_channels=list(cfg.out_channels), **kw)
    m.load_state_dict(synthetic_state_dict(cfg, seed=seed), strict=True)
    return m.to("cuda").eval()


def both(m, x):
    """(unsplit, split) depth of one input; the handle is left with the split on."""
    m.engine.set_option("enc_split", 0)
    a = m.forward(x, fp32=False).clone()
    m.engine.set_option("enc_split", 1)
    b = m.forward(x, fp32=False).clone()
    return a, b


def assert_same(a, b, what):
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} elements differ between the split and one chain"


@pytest.mark.parametrize("name", ["vitl", "vits"])
def test_split_full_clip_is_bit_identical(name):
    m = model_for(name, 0)
    x = torch.randn(1, 32, 3, 518, 518, generator=torch.Generator().manual_seed(3)).cuda()
    a, b = both(m, x)
    assert_same(a, b, f"{name} 1x32x518")
    if name == "vits":                                   # back to back: the lane's fork / join orders every forward after the last
        for i in range(20):
            assert_same(a, m.forward(x, fp32=False), f"{name} split forward {i}")


@pytest.mark.parametrize("B,T", [(1, 5), (2, 5), (1, 1), (2, 1)])
def test_split_odd_and_batched_shapes(B, T):
    m = model_for("vits", 5)
    x = torch.randn(B, T, 3, 70, 84, generator=torch.Generator().manual_seed(10 * B + T)).cuda()
    a, b = both(m, x)
    assert_same(a, b, f"vits B={B} T={T}")


@pytest.mark.parametrize("fixture,kw", [("tiny_forward.npz", {}), ("tiny_clstoken_forward.npz", {"use_clstoken": True})], ids=["tiny", "clstoken"])
def test_split_on_the_tiny_goldens(golden_dir, fixture, kw):
    z = np.load(os.path.join(golden_dir, fixture))
    m = model_for("tiny", int(z["sd_seed"]), **kw)
    x = torch.from_numpy(z["x"]).cuda()
    a, b = both(m, x)
    assert_same(a, b, fixture)
    s1 = m.engine.stage("path_2")[0].clone()
    m.engine.set_option("enc_split", 0)
    m.forward(x, fp32=False)
    assert_same(m.engine.stage("path_2")[0], s1, fixture + " path_2")


def test_split_two_forwards_in_flight_on_two_streams():
    """Two handles on two caller streams (four streams in all): the same results as one forward at a time."""
    ms = [model_for("vits", 7) for _ in range(2)]
    xs = [torch.randn(1, 8, 3, 518, 518, generator=torch.Generator().manual_seed(20 + i)).cuda() for i in range(2)]
    for m in ms:
        m.engine.set_option("enc_split", 0)
    ref = [m.forward(x, fp32=False).clone() for m, x in zip(ms, xs)]
    for m in ms:
        m.engine.set_option("enc_split", 1)
    torch.cuda.synchronize()
    st = [torch.cuda.Stream() for _ in range(2)]
    for s in st:
        s.wait_stream(torch.cuda.current_stream())
    outs = [[], []]
    for _ in range(3):
        for j in range(2):
            with torch.cuda.stream(st[j]):
                outs[j].append(ms[j].forward(xs[j], fp32=False).clone())
    torch.cuda.synchronize()
    for j in range(2):
        for i, d in enumerate(outs[j]):
            assert_same(ref[j], d, f"stream {j} forward {i}")


def test_one_handle_two_slots_in_flight():
    """One handle, two workspace slots on two caller streams (the video scheduler's mode, bench.py's two-clips pass): a forward issued
    while the other stream's is in flight runs unsplit, one issued after it finished splits - the same maps either way."""
    m = model_for("vits", 8)
    x = torch.randn(1, 8, 3, 518, 518, generator=torch.Generator().manual_seed(30)).cuda()
    m.engine.set_option("enc_split", 0)
    ref = m.engine.forward(x, fp32=False, slot=0)[0].clone()
    m.engine.set_option("enc_split", 1)
    torch.cuda.synchronize()
    st = [torch.cuda.Stream() for _ in range(2)]
    for s in st:
        s.wait_stream(torch.cuda.current_stream())
    outs = []
    for i in range(4):
        with torch.cuda.stream(st[i & 1]):
            outs.append(m.engine.forward(x, fp32=False, slot=i & 1)[0].clone())
    torch.cuda.synchronize()
    for i, d in enumerate(outs):
        assert_same(ref, d, f"slot {i & 1} forward {i}")


def test_split_captured_forward_replays_bit_identically():
    """A capturing stream keeps the one-stream sequence (a linear graph); its replay equals the eager split forward."""
    m = model_for("vits", 15)
    x = torch.randn(1, 4, 3, 70, 84, generator=torch.Generator().manual_seed(76)).cuda()
    a, ref = both(m, x)
    assert_same(a, ref, "eager")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())        # (one workspace slot: the forwards must not overlap)
    with torch.cuda.stream(side):
        m.forward(x, fp32=False)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = m.forward(x, fp32=False)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert_same(ref, out, "graph replay")


def test_split_stream_overflow_fails_loudly_with_the_split():
    """The outlier of test_split_stream_overflow_fails_loudly (3 frames: halves of 1 and 2): each half's statistics pass keeps its
    overflow check, the depth is NaN and the report names ln_fold."""
    from video_depth_anything_amd import _lib
    from video_depth_anything_amd.config import get_config
    from video_depth_anything_amd.video_depth import VideoDepthAnything
    from video_depth_anything_amd.weights import synthetic_state_dict
    cfg = get_config("tiny")
    sd = {k: v.clone() for k, v in synthetic_state_dict(cfg, seed=1).items()}
    sd["pretrained.blocks.1.attn.proj.bias"][5] = 3.0e5 / float(sd["pretrained.blocks.1.ls1.gamma"][5])
    m = VideoDepthAnything(encoder="tiny", features=cfg.features, out_channels=list(cfg.out_channels))
    m.load_state_dict(sd, strict=True)
    m = m.to("cuda").eval()
    m.engine.set_option("enc_split", 1)
    x = torch.randn(1, 3, 3, 42, 56, generator=torch.Generator().manual_seed(9)).cuda()
    d = m.forward(x, fp32=False)
    assert torch.isnan(d).all(), "a forward whose stream overflowed must not return numbers"
    with pytest.raises(_lib.VdaError, match="ln_fold"):
        m.engine.check()
    m.engine.check()                                     # reports are cleared once returned
