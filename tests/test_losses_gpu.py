"""The device losses (csrc/losses.hip, video_depth_anything_amd/losses.py) on the MI355X against what the reference's modules
computed on the five cases of tests/golden/loss_metrics.npz, with the bounds of tests/test_losses_numpy.py, and against the numpy
twins; plus the properties a device reduction must have: exact medians, bit-identical repeats, host / device inputs, a non-default
stream, the [B,N,1,H,W] form, the drop-in modules, N = 1."""
import math

import numpy as np
import pytest
import torch

from _loss_inputs import CASES, SSI_TOL, VARIANTS, assert_within, load_case, tgm_tol

pytestmark = pytest.mark.gpu
_device, _twin = {}, {}


def device(golden_dir, name, variant):
    """validation_loss of a case on the device, computed once per (case, variant) and shared; nothing below writes into it."""
    from video_depth_anything_amd.losses import validation_loss
    if (name, variant) not in _device:
        pred, y, mask, _ = load_case(golden_dir, name)
        _device[name, variant] = validation_loss(pred, y, mask, variant=variant)
    return _device[name, variant]


def twin(golden_dir, name, variant):
    from video_depth_anything_amd.losses import validation_loss_numpy
    if (name, variant) not in _twin:
        pred, y, mask, _ = load_case(golden_dir, name)
        _twin[name, variant] = validation_loss_numpy(pred, y, mask, variant=variant)
    return _twin[name, variant]


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.asarray(a[k], dtype=np.float64).tobytes() == np.asarray(b[k], dtype=np.float64).tobytes(), (k, a[k], b[k])


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", CASES)
def test_device_losses_match_the_reference_and_the_twin(golden_dir, name, variant):
    pred, y, mask, exp = load_case(golden_dir, name)
    got, tw = device(golden_dir, name, variant), twin(golden_dir, name, variant)
    N = pred.shape[1]
    what = f"case {name} {variant}"
    bad = []
    for label, g, w, tol in ((f"{what} ssi vs the reference", got["ssi"], exp["ref64"][variant], SSI_TOL),
                             (f"{what} ssi vs the twin", got["ssi"], tw["ssi"], SSI_TOL),
                             (f"{what} tgm vs the reference", got["tgm"], exp["ref64"]["tgm"], tgm_tol(N)),
                             (f"{what} tgm vs the twin", got["tgm"], tw["tgm"], SSI_TOL),
                             (f"{what} loss vs the twin", got["loss"], tw["loss"], SSI_TOL)):
        try:
            assert_within(g, w, tol, label)
        except AssertionError as e:
            bad.append(str(e))
    pf = np.abs(got["ssi_per_frame"] - tw["ssi_per_frame"]) / np.where(tw["ssi_per_frame"] != 0, np.abs(tw["ssi_per_frame"]), 1.0)
    pp = np.abs(got["tgm_per_pair"] - tw["tgm_per_pair"]) / np.abs(tw["tgm_per_pair"])
    print(f"{what} ssi_per_frame vs the twin: worst rel {pf.max():.3e}; tgm_per_pair: worst rel {np.nanmax(pp) if np.isfinite(pp).any() else 0.0:.3e}")
    print(f"{what} n_static: got {got['n_static'].tolist()} want {exp['n_static'].tolist()}")
    assert not bad, bad
    assert pf.max() <= SSI_TOL
    assert np.array_equal(np.isnan(got["tgm_per_pair"]), np.isnan(tw["tgm_per_pair"])) and not (pp[np.isfinite(pp)] > SSI_TOL).any()
    assert got["n_static"].dtype == np.int64 and np.array_equal(got["n_static"], exp["n_static"])
    assert got["loss"] == 10.0 * got["tgm"] + 1.0 * got["ssi"]


@pytest.mark.parametrize("name", ["A", "C", "D"])
def test_device_medians_are_the_twins_bit_for_bit(golden_dir, name):
    from video_depth_anything_amd.losses import _masked_median, _masked_median_numpy
    pred, y, mask, _ = load_case(golden_dir, name)
    for label, x in (("pred", pred), ("y", y)):
        got, want = _masked_median(x, mask), _masked_median_numpy(x, mask)
        print(f"case {name} medians of {label}: got {got.ravel().tolist()} want {want.ravel().tolist()}")
        assert got.shape == want.shape == x.shape[:2] and got.dtype == np.float32
        assert got.tobytes() == want.tobytes()
    if name == "C":                                                     # the lower median of frame 1 lies among zeros of both signs
        assert _masked_median(pred)[0, 1] == 0.0


def test_single_tensor_and_pair_medians_agree_and_odd_counts(golden_dir):
    """The odd-count rule and planes a 1024-thread block does not fill: 1, 2, 3 and 1025 valid values."""
    from video_depth_anything_amd.losses import _masked_median, _masked_median_numpy
    rng = np.random.default_rng(3)
    x = rng.standard_normal((4, 33, 35)).astype(np.float32)             # 1155 values per plane
    m = np.zeros(x.shape, dtype=np.uint8)
    for f, n in enumerate((1, 2, 3, 1025)):
        m[f].reshape(-1)[rng.permutation(33 * 35)[:n]] = 1
    got, want = _masked_median(x, m), _masked_median_numpy(x, m)
    print(f"medians of 1 / 2 / 3 / 1025 valid values: got {got.tolist()} want {want.tolist()}")
    assert got.tobytes() == want.tobytes()
    got, want = _masked_median(torch.from_numpy(x).cuda()), _masked_median_numpy(x)
    assert got.tobytes() == want.tobytes()


def test_repeat_is_bit_identical(golden_dir):
    from video_depth_anything_amd.losses import validation_loss
    for name in ("A", "D"):
        pred, y, mask, _ = load_case(golden_dir, name)
        for variant in VARIANTS:
            same_bits(device(golden_dir, name, variant), validation_loss(pred, y, mask, variant=variant))


def test_device_tensors_and_host_arrays_agree_bit_for_bit(golden_dir):
    from video_depth_anything_amd.losses import ssi_loss, tgm_loss, validation_loss
    pred, y, mask, _ = load_case(golden_dir, "A")
    dp, dy = torch.from_numpy(pred.copy()).cuda(), torch.from_numpy(y.copy()).cuda()
    dm_u8, dm_bool = torch.from_numpy(mask.copy()).cuda(), torch.from_numpy(mask != 0).cuda()
    for variant in VARIANTS:
        host = device(golden_dir, "A", variant)
        same_bits(host, validation_loss(dp, dy, dm_u8, variant=variant))
        same_bits(host, validation_loss(dp, y, dm_bool, variant=variant))           # one of each, and a bool mask
        same_bits(host, validation_loss(pred, dy, mask != 0, variant=variant))
        assert ssi_loss(dp, dy, dm_u8, variant=variant) == host["ssi"]
    assert tgm_loss(dp, dy, dm_u8) == device(golden_dir, "A", "lsq")["tgm"]


def test_non_default_stream(golden_dir):
    from video_depth_anything_amd.losses import validation_loss
    pred, y, mask, _ = load_case(golden_dir, "A")
    s = torch.cuda.Stream()
    for variant in VARIANTS:
        with torch.cuda.stream(s):
            got = validation_loss(pred, y, mask, variant=variant)
        s.synchronize()
        same_bits(device(golden_dir, "A", variant), got)


def test_channel_axis_and_none_mask(golden_dir):
    from video_depth_anything_amd.losses import validation_loss
    pred, y, mask, _ = load_case(golden_dir, "E")
    for variant in VARIANTS:
        same_bits(device(golden_dir, "E", variant), validation_loss(pred[:, :, None], y[:, :, None], mask, variant=variant))
    pred, y, mask, _ = load_case(golden_dir, "D")
    assert mask is None
    same_bits(device(golden_dir, "D", "mad"), validation_loss(pred, y, np.ones(pred.shape, np.uint8), variant="mad"))


def test_drop_in_modules_return_the_validation_figures_as_float32(golden_dir):
    from utils import loss as loss_da
    from utils import loss_MiDas
    pred, y, mask, _ = load_case(golden_dir, "A")
    dp, dy = torch.from_numpy(pred.copy()).cuda()[:, :, None], torch.from_numpy(y.copy()).cuda()[:, :, None]     # [B,N,1,H,W]
    dm = torch.from_numpy(mask.astype(np.float32)).cuda()                                                        # any dtype: .bool()
    with torch.no_grad():
        for mod, key, variant in ((loss_MiDas.Loss_ssi(), "ssi", "lsq"), (loss_da.Loss_ssi(), "ssi", "mad"),
                                  (loss_MiDas.Loss_tgm(), "tgm", "lsq"), (loss_da.Loss_tgm(), "tgm", "mad")):
            out = mod(dp, dy, dm)
            want = np.float32(device(golden_dir, "A", variant)[key])
            print(f"{type(mod).__module__}.{type(mod).__name__}: {out.item()!r} want {want!r}")
            assert out.dtype == torch.float32 and out.dim() == 0 and out.device == dp.device
            assert np.float32(out.item()).tobytes() == want.tobytes()
        # the validation lines of train.py, unchanged
        loss_ssi, loss_tgm = loss_MiDas.Loss_ssi(), loss_MiDas.Loss_tgm()
        val = 10.0 * loss_tgm(dp, dy, dm) + 1.0 * loss_ssi(dp, dy, dm)
        assert val.dtype == torch.float32 and abs(val.item() - device(golden_dir, "A", "lsq")["loss"]) <= 4 * 2.0 ** -24 * abs(val.item())
        # eps is passed through to the kernels
        from video_depth_anything_amd.losses import ssi_loss_numpy
        for mod, variant in ((loss_MiDas.Loss_ssi(eps=1e-2), "lsq"), (loss_da.Loss_ssi(eps=1e-2), "mad")):
            assert_within(mod(dp, dy, dm).item(), float(np.float32(ssi_loss_numpy(pred, y, mask, variant=variant, eps=1e-2))), 2.0 ** -23,
                          f"{variant} with eps=1e-2")


def test_a_single_frame_gives_nan_for_tgm(golden_dir):
    from video_depth_anything_amd.losses import tgm_loss, validation_loss, validation_loss_numpy
    pred, y, mask, _ = load_case(golden_dir, "A")
    p1, y1, m1 = pred[:, :1], y[:, :1], mask[:, :1]
    assert math.isnan(tgm_loss(p1, y1, m1))
    r, t = validation_loss(p1, y1, m1), validation_loss_numpy(p1, y1, m1)
    assert math.isnan(r["tgm"]) and math.isnan(r["loss"]) and r["tgm_per_pair"].shape == (2, 0) and r["n_static"].shape == (2, 0)
    assert_within(r["ssi"], t["ssi"], SSI_TOL, "N = 1 ssi vs the twin")
