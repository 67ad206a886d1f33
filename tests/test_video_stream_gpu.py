"""infer_video_depth_stream on the MI355X: bit-identity with infer_video_depth for arrays, generators and ragged blocks, the running
depth range, bounded read-ahead and device memory, early exit, errors, the split-stream overflow, and the min/max kernel.

Tiny configuration, state-dict seeds, frame shape (42 x 56) and input size as tests/golden/tiny_video.npz and tiny_metric_video.npz;
the frames are seeded random uint8 so that any length can be drawn."""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H0, W0, INPUT = 42, 56, 42
SD_SEED = {False: 2, True: 6}                        # tiny_video.npz / tiny_metric_video.npz
PRECISIONS = [pytest.param(False, id="fp16"), pytest.param(True, id="fp32")]
VARIANTS = [pytest.param(False, id="relative"), pytest.param(True, id="metric")]
_models = {}


def model(metric=False):
    if metric not in _models:
        from video_depth_anything_amd.config import get_config
        from video_depth_anything_amd.video_depth import MetricVideoDepthAnything, VideoDepthAnything
        from video_depth_anything_amd.weights import synthetic_state_dict
        cfg = get_config("tiny")
        m = (MetricVideoDepthAnything if metric else VideoDepthAnything)(encoder="tiny", features=cfg.features, out_channels=list(cfg.out_channels))
        m.load_state_dict(synthetic_state_dict(cfg, seed=SD_SEED[metric]), strict=True)
        _models[metric] = m.to("cuda").eval()
    return _models[metric]


def video(n, seed=11, h=H0, w=W0):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def natural_pieces(n):
    """24 frames, then 22 per window, then the 8-frame tail, trimmed to n: [(first, count)]."""
    from video_depth_anything_amd.scheduler import plan_windows
    cuts = np.minimum(np.cumsum([0, 24] + [22] * (len(plan_windows(n)) - 1) + [8]), n)
    return [(int(a), int(b - a)) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]


def drain(stream, shape=(H0, W0)):
    """All pieces of a stream, checked for order, contiguity, dtype and ownership; returns the concatenation."""
    pieces, pos = [], 0
    for first, d in stream:
        assert first == pos and isinstance(d, np.ndarray) and d.dtype == np.float32 and d.shape[1:] == shape and d.shape[0] > 0
        assert d.flags.owndata and d.flags.writeable, "a piece is the caller's own array"
        pieces.append((first, d, d.copy()))
        pos += d.shape[0]
    for first, d, snap in pieces:
        assert np.array_equal(d, snap), f"the piece at frame {first} changed after it was handed out"
    assert stream.n_frames == pos
    return np.concatenate([d for _, d, _ in pieces]), [(f, d.shape[0]) for f, d, _ in pieces]


@pytest.mark.parametrize("fp32", PRECISIONS)
@pytest.mark.parametrize("metric", VARIANTS)
@pytest.mark.parametrize("n", [1, 5, 22, 23, 32, 33, 50, 100])
def test_array_input_is_bit_identical(n, metric, fp32):
    m = model(metric)
    frames = video(n)
    want, fps = m.infer_video_depth(frames, 24, input_size=INPUT, device="cuda", fp32=fp32)
    stream = m.infer_video_depth_stream(frames, 24, input_size=INPUT, device="cuda", fp32=fp32)
    got, cuts = drain(stream)
    assert got.shape == (n, H0, W0) and np.array_equal(got, want)
    assert cuts == natural_pieces(n)
    assert stream.n_frames == n and stream.fps == fps == 24
    assert stream.depth_min == want.min() and stream.depth_max == want.max()
    assert np.isfinite(want).all()


@pytest.mark.parametrize("fp32", PRECISIONS)
@pytest.mark.parametrize("metric", VARIANTS)
def test_iterables_are_bit_identical(metric, fp32):
    m = model(metric)
    n = 100
    frames = video(n, seed=12)
    want, _ = m.infer_video_depth(frames, 30, input_size=INPUT, device="cuda", fp32=fp32)

    def singles():
        for f in frames:
            yield f

    def ragged():
        rng, i = np.random.default_rng(3), 0
        while i < n:
            c = int(rng.integers(1, 41))
            yield frames[i] if c == 1 else frames[i:i + c]
            i += c

    def other_dtypes():                              # 8-bit values in other dtypes, a list and a strided block among them
        yield frames[:10].astype(np.float32)
        yield frames[10:35].astype(np.int64)
        yield [f for f in frames[35:40]]
        yield np.ascontiguousarray(frames[40:100][::-1])[::-1]

    for source in (singles(), ragged(), other_dtypes()):
        assert not hasattr(source, "__len__")
        stream = m.infer_video_depth_stream(source, 30, input_size=INPUT, fp32=fp32)
        got, cuts = drain(stream)
        assert np.array_equal(got, want) and cuts == natural_pieces(n)
        assert stream.n_frames == n and stream.fps == 30
        assert stream.depth_min == want.min() and stream.depth_max == want.max()


@pytest.mark.parametrize("fp32", PRECISIONS)
def test_resize_path_is_bit_identical(fp32):
    """Source frames that are not at the network size: the gather + bicubic resize kernel reads ring slots."""
    m = model()
    n, h, w = 60, 30, 52
    frames = video(n, seed=13, h=h, w=w)
    want, _ = m.infer_video_depth(frames, 24, input_size=INPUT, device="cuda", fp32=fp32)
    assert want.shape == (n, h, w)
    stream = m.infer_video_depth_stream((frames[i:i + 7] for i in range(0, n, 7)), 24, input_size=INPUT, fp32=fp32)
    got, _ = drain(stream, (h, w))
    assert np.array_equal(got, want)
    assert stream.depth_min == want.min() and stream.depth_max == want.max()


def test_read_ahead_is_bounded():
    """Frames drawn from the source when a piece is handed out: never more than those handed out plus the planner's named read-ahead
    (two windows in flight and one being uploaded: at most three windows)."""
    from video_depth_anything_amd.scheduler import READ_AHEAD
    assert READ_AHEAD <= 96
    m = model()
    n = 300
    frames = video(n, seed=14)
    drawn = [0]

    def source():
        for f in frames:
            drawn[0] += 1
            yield f

    stream = m.infer_video_depth_stream(source(), 24, input_size=INPUT)
    seen = []
    for first, d in stream:
        seen.append((first + d.shape[0], drawn[0]))
        assert drawn[0] <= first + d.shape[0] + READ_AHEAD, seen[-1]
    assert seen[-1][0] == n and drawn[0] == n
    assert max(dr - out for out, dr in seen) == READ_AHEAD, "the named read-ahead is the one the schedule has"


def test_device_memory_does_not_grow_with_the_video():
    m = model()
    frames = video(400, seed=15)

    def peak(n):
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        stream = m.infer_video_depth_stream((f for f in frames[:n]), 24, input_size=INPUT)
        total = sum(d.shape[0] for _, d in stream)
        assert total == n
        del stream
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated()

    peak(100)                                        # warm-up: workspaces, the allocator's pools
    p100, p400 = peak(100), peak(400)
    print(f"peak allocated: 100 frames {p100} B, 400 frames {p400} B, one source frame {H0 * W0 * 3} B")
    assert p400 - p100 < H0 * W0 * 3


def test_early_exit_restores_the_handle():
    m = model()
    frames = video(120, seed=16)
    before, _ = m.infer_video_depth(frames[:50], 24, input_size=INPUT, device="cuda")
    eng = m.engine
    for preset in (None, 1):
        if preset is not None:
            eng.set_option("enc_split", preset)
        was = eng.options.get("enc_split", -1)
        stream = m.infer_video_depth_stream(iter(frames), 24, input_size=INPUT)
        first, d = next(stream)
        assert first == 0 and d.shape == (24, H0, W0)
        assert eng.options.get("enc_split") == 0, "off for the duration"
        stream.close()
        torch.cuda.synchronize()
        assert eng.options.get("enc_split", -1) == was
        with pytest.raises(StopIteration):
            next(stream)
        stream.close()                               # idempotent
        assert np.array_equal(d, before[:24])
        # a break out of the loop and garbage collection
        for first, d in m.infer_video_depth_stream(iter(frames), 24, input_size=INPUT):
            break
        gc.collect()
        torch.cuda.synchronize()
        assert eng.options.get("enc_split", -1) == was
        # an exception in the consumer
        with pytest.raises(KeyError):
            stream = m.infer_video_depth_stream(iter(frames), 24, input_size=INPUT)
            try:
                for first, d in stream:
                    raise KeyError("consumer")
            finally:
                stream.close()
        assert eng.options.get("enc_split", -1) == was
        after, _ = m.infer_video_depth(frames[:50], 24, input_size=INPUT, device="cuda")
        assert np.array_equal(after, before)
    eng.set_option("enc_split", -1)


def test_errors():
    m = model()
    frames = video(40, seed=17)
    eng = m.engine
    was = eng.options.get("enc_split", -1)
    with pytest.raises(ValueError, match="empty video"):
        list(m.infer_video_depth_stream(iter([]), 24, input_size=INPUT))
    with pytest.raises(ValueError, match="empty video"):
        list(m.infer_video_depth_stream(frames[:0], 24, input_size=INPUT))
    with pytest.raises(ValueError):
        list(m.infer_video_depth_stream(iter([frames[:5], video(3, h=H0 + 2)]), 24, input_size=INPUT))
    with pytest.raises(ValueError):
        list(m.infer_video_depth_stream(iter([frames[0, :, :, :2]]), 24, input_size=INPUT))
    with pytest.raises(ValueError):
        m.infer_video_depth_stream(frames[..., :2], 24, input_size=INPUT)
    with pytest.raises(TypeError, match="8-bit"):
        list(m.infer_video_depth_stream(iter([frames[:5], frames[5:9].astype(np.float32) + 0.5]), 24, input_size=INPUT))
    with pytest.raises(TypeError, match="8-bit"):
        list(m.infer_video_depth_stream(frames.astype(np.float32) / 255.0, 24, input_size=INPUT))
    with pytest.raises(RuntimeError):
        m.infer_video_depth_stream(frames, 24, input_size=INPUT, device="cpu")
    # a bad block is raised when it is drawn: what lies before it has been delivered
    stream = m.infer_video_depth_stream(iter([frames, frames, frames[:4], video(3, h=H0 + 2)]), 24, input_size=INPUT)
    got = 0
    with pytest.raises(ValueError):
        for first, d in stream:
            got = first + d.shape[0]
    assert got >= 24
    torch.cuda.synchronize()
    assert eng.options.get("enc_split", -1) == was


def test_overflow_raises_and_never_delivers_nan():
    """The weights of test_split_stream_overflow_fails_loudly (one channel of block 1 jumps by 3e5: every fp16 window leaves the split
    stream's range): the stream raises RuntimeError, and no piece that holds frames of an overflowed window was handed out."""
    from video_depth_anything_amd.config import get_config
    from video_depth_anything_amd.video_depth import VideoDepthAnything
    from video_depth_anything_amd.weights import synthetic_state_dict
    cfg = get_config("tiny")
    sd = {k: v.clone() for k, v in synthetic_state_dict(cfg, seed=1).items()}
    sd["pretrained.blocks.1.attn.proj.bias"][5] = 3.0e5 / float(sd["pretrained.blocks.1.ls1.gamma"][5])
    m = VideoDepthAnything(encoder="tiny", features=cfg.features, out_channels=list(cfg.out_channels))
    m.load_state_dict(sd, strict=True)
    m = m.to("cuda").eval()
    frames = video(70, seed=18)
    delivered = []
    with pytest.raises(RuntimeError, match="ln_fold|65504"):
        for first, d in m.infer_video_depth_stream(iter(frames), 24, input_size=INPUT):
            delivered.append(d)
    assert not delivered, "window 0 overflowed: none of its frames may be handed out"
    torch.cuda.synchronize()
    try:
        m.engine.check()                             # a report that was still in flight when the stream raised
    except RuntimeError:
        pass
    # the fp32 path has no such limit: the same stream runs through
    got, _ = drain(m.infer_video_depth_stream(iter(frames), 24, input_size=INPUT, fp32=True))
    assert got.shape == (70, H0, W0) and np.isfinite(got).all()


def test_minmax_accum_kernel():
    from video_depth_anything_amd import ops
    rng = np.random.default_rng(21)
    mm = torch.tensor([float("inf"), float("-inf")], dtype=torch.float32, device="cuda")
    lo, hi = np.float32(np.inf), np.float32(-np.inf)
    for n in (1, 3, 5, 1023, 1024, 1025, 4099, 24 * H0 * W0 + 7, 1000003):
        x = (rng.standard_normal(n) * rng.uniform(0.1, 50)).astype(np.float32)
        t = torch.from_numpy(x).cuda()
        one = torch.tensor([float("inf"), float("-inf")], dtype=torch.float32, device="cuda")
        ops.minmax_accum(t, one)
        assert one.cpu().numpy().tolist() == [x.min(), x.max()], n
        ops.minmax_accum(t, mm)                                       # accumulates across calls
        lo, hi = min(lo, x.min()), max(hi, x.max())
        assert mm.cpu().numpy().tolist() == [lo, hi], n
    # an unaligned start, a length that is not a multiple of anything, only the first n elements
    x = rng.standard_normal(5000).astype(np.float32)
    t = torch.from_numpy(x).cuda()
    for off, n in ((1, 4097), (2, 777), (3, 4996)):
        one = torch.tensor([float("inf"), float("-inf")], dtype=torch.float32, device="cuda")
        ops.minmax_accum(t[off:], one, n)
        assert one.cpu().numpy().tolist() == [x[off:off + n].min(), x[off:off + n].max()], (off, n)
    # infinities
    x = rng.standard_normal(3001).astype(np.float32)
    x[17], x[2999] = np.inf, -np.inf
    one = torch.tensor([float("inf"), float("-inf")], dtype=torch.float32, device="cuda")
    ops.minmax_accum(torch.from_numpy(x).cuda(), one)
    assert one.cpu().numpy().tolist() == [-np.inf, np.inf]
    ops.minmax_accum(torch.from_numpy(x).cuda(), mm)
    assert mm.cpu().numpy().tolist() == [-np.inf, np.inf]
    with pytest.raises(ValueError):
        ops.minmax_accum(t, one, 0)
    with pytest.raises(ValueError):
        ops.minmax_accum(t, one, t.numel() + 1)


def test_stream_refuses_more_than_one_rank(monkeypatch):
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(NotImplementedError, match="infer_video_depth"):
        model().infer_video_depth_stream(video(5), 24, input_size=INPUT)
