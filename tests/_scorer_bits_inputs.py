"""The cases of tests/golden/scorer_bits.npz: the device scorers' OWN results (evaluate_depth, evaluate_tae, validation_loss, the
stitcher's ops.lsq_scale_shift), recorded bit for bit by tools/gen_scorer_bits_golden.py. They pin the order of every fp64 addition
of csrc/reduce64.h's pattern: more than 256 planes (the finishers' "thread t owns planes t, t + 256, ..." walk and a tree whose
entries above index 44 are not zero), several blocks per plane, chunk row offsets, a grid-stride loop that wraps.

The inputs come from the counter-based integer hash of _eval_inputs.py and IEEE float32 / float64 add, multiply and divide only, so
every platform produces the same bits; the fixture records their checksums, not the arrays. `run_cases` is shared by the recipe and
the test, so both flatten a result the same way: floats as float64, counts as int64."""
import hashlib

import numpy as np

from _eval_inputs import _hash24

f = np.float32


def _u01(n, stream):
    return _hash24(np.arange(n, dtype=np.uint64), stream << 32) * f(1.0 / (1 << 24))            # [0, 1), exact


def _depth_pair(shape, stream, far, zeros=0.1):
    """(pred, gt) float32: depth 0.4 .. 0.4 + far with `zeros` of the pixels 0 (invalid), pred = 1.7 / depth + 0.05 + noise."""
    n = int(np.prod(shape))
    u, v, w = (_u01(n, stream + s) for s in range(3))
    gt = f(0.4) + u * f(far)
    disp = f(1.0) / gt
    pred = f(1.7) * disp + f(0.05) + (v - f(0.5)) * f(2.0) * disp
    gt = np.where(w < f(zeros), f(0.0), gt).astype(np.float32)
    return np.ascontiguousarray(pred.reshape(shape)), np.ascontiguousarray(gt.reshape(shape))


def depth_many_frames():
    """300 frames of 7 x 9, float32 gt beyond max_depth in places, frame 123 without a valid pixel."""
    pred, gt = _depth_pair((300, 7, 9), 20, 75.0)
    gt[123] = f(0.0)
    return pred, gt, 70.0


def depth_many_blocks():
    """2 frames of 40 x 520 (82 blocks of 256 pixels per frame, 64 used), float64 gt = integer millimetres / 1000."""
    pred, gt = _depth_pair((2, 40, 520), 30, 75.0)
    return pred, np.floor(gt.astype(np.float64) * 1000.0) / 1000.0, 70.0


def tae_many_planes():
    """131 frames of 6 x 8 (260 planes), a mask, the camera moving by a constant step: (pred, gt, K, poses, mask, max_depth)."""
    N, H, W = 131, 6, 8
    pred, gt = _depth_pair((N, H, W), 40, 4.6)
    mask = (_u01(N * H * W, 43) < f(0.8)).astype(np.uint8).reshape(N, H, W)
    K = np.array([[10.0, 0.0, 3.5], [0.0, 10.0, 2.5], [0.0, 0.0, 1.0]])
    poses = np.tile(np.eye(4), (N, 1, 1))
    poses[:, :3, 3] = np.arange(N, dtype=np.float64)[:, None] * np.array([0.15, -0.1, 0.05])
    return pred, gt, K, poses, mask, 10.0


def _walk_pair(shape, stream):
    """(pred, y) float32 [B,N,H,W]: y walks by less than 0.1 per frame, about half the pixels of a pair static."""
    B, N, H, W = shape
    n = B * N * H * W
    u, v, w = (_u01(n, stream + s).reshape(B, N, H * W) for s in range(3))
    y = np.empty((B, N, H * W), dtype=np.float32)
    y[:, 0] = f(0.5) + u[:, 0] * f(3.0)
    for i in range(1, N):
        y[:, i] = y[:, i - 1] + (v[:, i] - f(0.5)) * f(0.2)
    pred = (y - f(0.3)) * f(0.6) + (w - f(0.5)) * f(0.2)
    return np.ascontiguousarray(pred.reshape(shape)), np.ascontiguousarray(y.reshape(shape))


def loss_many_planes():
    """[3,100,5,7]: 300 frame planes, 297 pair planes; ~70 % mask, frame (1, 37) without a valid pixel."""
    shape = (3, 100, 5, 7)
    pred, y = _walk_pair(shape, 50)
    mask = (_u01(int(np.prod(shape)), 53) < f(0.7)).astype(np.uint8).reshape(shape)
    mask[1, 37] = 0
    return pred, y, mask


def loss_wrap():
    """[1,2,130,257], no mask: 33 410 pixels per plane against 64 blocks x 256 threads - the grid-stride loop takes a third step."""
    pred, y = _walk_pair((1, 2, 130, 257), 60)
    return pred, y, None


STITCH_SIZES = (2 * 37 * 53, 2 * 518 * 518)


def stitch_pair(n):
    """(pred, target) float32 [n]: target = 0.8 * pred + 0.3 + noise."""
    u, v = _u01(n, 70), _u01(n, 71)
    pred = f(0.2) + u * f(5.0)
    return pred, pred * f(0.8) + f(0.3) + (v - f(0.5)) * f(0.1)


def checksum(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is not None:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def flatten(name, result):
    """A scorer's result dict as fixture entries `name.key`: float64 or int64 arrays, whatever Python type the scorer returned."""
    out = {}
    for k, v in result.items():
        a = np.asarray(v)
        out[f"{name}.{k}"] = np.ascontiguousarray(a.astype(np.int64 if a.dtype.kind in "iub" else np.float64))
    return out


def run_cases():
    """Every case on the device. Returns (results, input checksums, tae runs): `results` is what the fixture pins; the two TAE runs
    (chunk_pairs None and 50) are returned apart because they must agree with each other and share one record."""
    import torch
    from video_depth_anything_amd import ops
    from video_depth_anything_amd.evaluate import evaluate_depth, evaluate_tae
    from video_depth_anything_amd.losses import validation_loss

    res, sha = {}, {}
    pred, gt, md = depth_many_frames()
    sha["depth300"] = checksum(pred, gt)
    res.update(flatten("depth300.whole", evaluate_depth(pred, gt, md)))
    res.update(flatten("depth300.chunk64", evaluate_depth(pred, gt, md, chunk_frames=64)))
    pred, gt, md = depth_many_blocks()
    sha["depth_blocks"] = checksum(pred, gt)
    res.update(flatten("depth_blocks", evaluate_depth(pred, gt, md)))

    pred, gt, K, poses, mask, md = tae_many_planes()
    sha["tae"] = checksum(pred, gt, K, poses, mask)
    tae = [flatten("tae", evaluate_tae(pred, gt, K, poses, md, mask=mask, chunk_pairs=c)) for c in (None, 50)]
    res.update(tae[0])

    for name, make in (("loss300", loss_many_planes), ("loss_wrap", loss_wrap)):
        pred, y, mask = make()
        sha[name] = checksum(pred, y, mask)
        for variant in ("lsq", "mad"):
            res.update(flatten(f"{name}.{variant}", validation_loss(pred, y, mask, variant=variant)))

    work = torch.empty(4 * ops.LSQ_BLOCKS, dtype=torch.float64, device="cuda")
    for n in STITCH_SIZES:
        pred, target = stitch_pair(n)
        sha[f"stitch{n}"] = checksum(pred, target)
        ss = torch.empty(2, dtype=torch.float32, device="cuda")
        ops.lsq_scale_shift(torch.from_numpy(pred).cuda(), torch.from_numpy(target).cuda(), work, ss)
        res[f"stitch{n}.scale_shift"] = ss.cpu().numpy()
    return res, sha, tae
