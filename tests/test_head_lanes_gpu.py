"""vda_set_option("head_lanes"): after the encoder's join the head's branches that do not depend on tap 3 (head_early, and conv1 of
resConfUnit1 in refinenets 3, 2, 1) run on the handle's lane stream beside proj3 .. motion module 2 on the caller's stream. It is a
split by TASK: every kernel keeps its rows, its tile plan and its arguments, and the two sides share no scratch block, so the result
must be BIT-IDENTICAL to one chain - the depth and every stage of the head - with
enc_split and dyn_sched on and off, forward after forward, and wherever the option must stand back (a captured forward, two forwards
in flight, head_overlap). No tolerance anywhere: every assertion is torch.equal against the option-off run of the same build.

A scratch race or a missing join shows at any shape, so the shapes are the smallest: the tiny golden, ViT-S T = 4 at 70x70 (5x5
patches: h4 = w4 = 3, the smallest map on which the stride-2 resize3 and motion module 1 still run) and at a non-square 70x98."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = ["tiny", "vits70", "vits70x98"]
STAGES = ["l1r", "l2r", "l3r", "l4r", "p4", "p4t", "p3", "p3t", "p2", "p1c", "o1"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def case(name):
    """(model, input) of a case, built once for the module; every test leaves the handle's options at their defaults."""
    from video_depth_anything_amd.config import get_config
    from video_depth_anything_amd.video_depth import VideoDepthAnything
    from video_depth_anything_amd.weights import synthetic_state_dict
    if name == "tiny":
        z = np.load(os.path.join(GOLDEN, "tiny_forward.npz"))
        enc, seed, x = "tiny", int(z["sd_seed"]), torch.from_numpy(z["x"])
    else:
        H, W = (70, 70) if name == "vits70" else (70, 98)
        enc, seed, x = "vits", 21, torch.randn(1, 4, 3, H, W, generator=torch.Generator().manual_seed(H + W))
    cfg = get_config(enc)
    m = VideoDepthAnything(encoder=enc, features=cfg.features, out_channels=list(cfg.out_channels))
    m.load_state_dict(synthetic_state_dict(cfg, seed=seed), strict=True)
    return m.to("cuda").eval(), x.cuda()


@pytest.fixture
def options():
    """set(model, **options); whatever a test set is back at the library's default afterwards."""
    touched = []

    def set_options(m, **kw):
        for k, v in kw.items():
            m.engine.set_option(k, v)
            touched.append((m, k))
    yield set_options
    torch.cuda.synchronize()
    for m, k in touched:
        m.engine.set_option(k, -1 if k in ("enc_split", "head_lanes") else 0)


def stages(m, x):
    """Every head stage buffer of the last forward that vda_debug_copy can name, as raw fp16 words."""
    from video_depth_anything_amd._lib import lib
    BT, ph, pw = x.shape[0] * x.shape[1], x.shape[3] // 14, x.shape[4] // 14
    Fe = m.cfg.features
    Fhp = (Fe // 2 + 31) // 32 * 32
    h4, w4 = (ph - 1) // 2 + 1, (pw - 1) // 2 + 1
    elems = {"l1r": 16 * ph * pw * Fe, "l2r": 4 * ph * pw * Fe, "l3r": ph * pw * Fe, "l4r": h4 * w4 * Fe, "p4": ph * pw * Fe, "p4t": ph * pw * Fe,
             "p3": 4 * ph * pw * Fe, "p3t": 4 * ph * pw * Fe, "p2": 16 * ph * pw * Fe, "p1c": 16 * ph * pw * Fe, "o1": 64 * ph * pw * Fhp}
    out = {}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for k in STAGES:
        t = torch.empty(BT * elems[k], dtype=torch.int16, device="cuda")
        rc = lib.vda_debug_copy(m.engine._h, k.encode(), C.c_void_p(t.data_ptr()), t.numel() * 2, stream)
        assert rc == 0, f"vda_debug_copy({k}): {lib.vda_last_error().decode()}"
        out[k] = t
    return out


def run(m, x):
    d = m.forward(x, fp32=False).clone()
    return d, stages(m, x)


def assert_same(ref, got, what):
    assert torch.equal(ref[0], got[0]), f"{what}: {int((ref[0] != got[0]).sum())} of {ref[0].numel()} depth values differ from one chain"
    for k in STAGES:
        assert torch.equal(ref[1][k], got[1][k]), f"{what}: stage {k} differs from one chain ({int((ref[1][k] != got[1][k]).sum())} of {got[1][k].numel()})"


@pytest.mark.parametrize("dyn_sched", [0, 1])
@pytest.mark.parametrize("enc_split", [0, 1])
@pytest.mark.parametrize("name", CASES)
def test_head_lanes_is_bit_identical_on_depth_and_every_stage(options, name, enc_split, dyn_sched):
    m, x = case(name)
    options(m, enc_split=enc_split, dyn_sched=dyn_sched, head_lanes=0)
    ref = run(m, x)
    options(m, head_lanes=1)
    assert_same(ref, run(m, x), f"{name} enc_split={enc_split} dyn_sched={dyn_sched} head_lanes=1")
    options(m, head_lanes=0)
    assert_same(ref, run(m, x), f"{name} enc_split={enc_split} dyn_sched={dyn_sched} back to one chain")


@pytest.mark.parametrize("name", CASES)
def test_twenty_forwards_with_head_lanes_are_all_the_first(options, name):
    """A scratch block shared by the two lanes, or a join that comes too late, shows as a difference here (never as a fault: both
    lanes only ever touch the forward's own workspace)."""
    m, x = case(name)
    options(m, head_lanes=0)
    ref = run(m, x)
    options(m, head_lanes=1)
    first = run(m, x)
    assert_same(ref, first, f"{name} head_lanes=1")
    for i in range(1, 20):
        d = m.forward(x, fp32=False)
        assert torch.equal(first[0], d), f"{name} head_lanes=1: forward {i} differs from the first"
    assert_same(first, (d, stages(m, x)), f"{name} head_lanes=1 forward 19")


def test_captured_forward_keeps_one_chain_and_equals_the_eager_one(options):
    m, x = case("vits70")
    options(m, head_lanes=1)
    ref = m.forward(x, fp32=False).clone()
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
    assert torch.equal(ref, out), "the captured forward differs from the eager one"
    assert torch.equal(ref, m.forward(x, fp32=False)), "the eager forward after the capture differs"


def test_two_forwards_in_flight_on_two_caller_streams(options):
    """One handle, workspace slots 0 and 1 on two caller streams: a forward issued while the other stream's is in flight keeps one
    chain, one issued after it finished uses the lanes - the same map either way."""
    m, x = case("vits70x98")
    options(m, head_lanes=0)
    ref = m.engine.forward(x, fp32=False, slot=0).clone()
    options(m, head_lanes=1)
    torch.cuda.synchronize()
    st = [torch.cuda.Stream() for _ in range(2)]
    for s in st:
        s.wait_stream(torch.cuda.current_stream())
    outs = []
    for i in range(6):
        with torch.cuda.stream(st[i & 1]):
            outs.append(m.engine.forward(x, fp32=False, slot=i & 1).clone())
    torch.cuda.synchronize()
    for i, d in enumerate(outs):
        assert torch.equal(ref, d), f"slot {i & 1} forward {i} differs from the single-stream result"


def test_head_overlap_wins_over_head_lanes(options):
    m, x = case("vits70")
    options(m, head_lanes=0, head_overlap=0)
    ref = run(m, x)
    options(m, head_lanes=1, head_overlap=1)
    for i in range(3):
        assert_same(ref, run(m, x), f"head_overlap + head_lanes, forward {i}")


@pytest.mark.parametrize("name", CASES)
def test_workspace_layout_does_not_depend_on_the_option(options, name):
    m, x = case(name)
    B, T, _, H, W = x.shape
    options(m, head_lanes=0)
    n0 = m.engine.workspace_bytes(B, T, H, W)
    ref = run(m, x)
    for v in (1, 0, 1):
        options(m, head_lanes=v)                         # toggled between forwards: nothing is prepared again
        assert m.engine.workspace_bytes(B, T, H, W) == n0, f"head_lanes={v} changes vda_workspace_bytes"
        assert_same(ref, run(m, x), f"{name} after toggling to head_lanes={v}")


def test_tiny_golden_with_head_lanes_on(options):
    """The reference-generated tiny golden with the option set explicitly, under the rule of tests/test_forward_gpu.py (the
    existing golden tests run through the library's default)."""
    from test_forward_gpu import check_map, golden_tol, nhwc_to_nchw
    z = np.load(os.path.join(GOLDEN, "tiny_forward.npz"))
    m, x = case("tiny")
    BT = x.shape[0] * x.shape[1]
    options(m, head_lanes=1)
    d = m.forward(x, fp32=False)
    tag = "tiny.head_lanes."
    for k in ("layer_3", "layer_4", "path_4", "path_3", "path_2"):
        t, h, w, Cp = m.engine.stage(k)
        C_ = z[k].shape[1]
        check_map(tag + k, nhwc_to_nchw(t, BT, h, w, Cp, C_), z[k], golden_tol(tag + k, z, k, False, stage=True), tail=False)
    check_map(tag + "depth", d.cpu().numpy(), z["depth"], golden_tol(tag + "depth", z, "depth", False))
