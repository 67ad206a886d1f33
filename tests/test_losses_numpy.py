"""The numpy twins of the device losses (video_depth_anything_amd/losses.py) against what the reference's own modules computed on
the five cases of tests/golden/loss_metrics.npz. CPU only; needs neither the library nor a GPU. The bounds are those of tests/_loss_inputs.py: both SSI
variants within 1e-12 relative of the reference's float64 run, TGM within (N + 3) * 2^-24 relative (the reference keeps its running
sum in a float32 scalar), n_static exact; the reference's float32 run only as a 1e-5 sanity bound on its own rounding."""
import os
import subprocess
import sys

import numpy as np
import pytest

from _loss_inputs import CASES, F32_SANITY_TOL, SSI_TOL, VARIANTS, assert_within, load_case, tgm_tol

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def losses():
    from video_depth_anything_amd import losses                         # the twins need neither the library nor a GPU
    return losses


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", CASES)
def test_ssi_twin_matches_the_reference(losses, golden_dir, name, variant):
    pred, y, mask, exp = load_case(golden_dir, name)
    got = losses.ssi_loss_numpy(pred, y, mask, variant=variant)
    assert_within(got, exp["ref64"][variant], SSI_TOL, f"case {name} ssi {variant} vs the reference's float64 run")
    assert_within(got, exp["ref32"][variant], F32_SANITY_TOL, f"case {name} ssi {variant} vs the reference's float32 run")


@pytest.mark.parametrize("name", CASES)
def test_tgm_twin_matches_the_reference(losses, golden_dir, name):
    pred, y, mask, exp = load_case(golden_dir, name)
    r = losses.validation_loss_numpy(pred, y, mask)
    N = pred.shape[1]
    assert_within(r["tgm"], exp["ref64"]["tgm"], tgm_tol(N), f"case {name} tgm vs the reference's float64 run")
    assert_within(r["tgm"], exp["ref32"]["tgm"], F32_SANITY_TOL, f"case {name} tgm vs the reference's float32 run")
    assert r["tgm"] == losses.tgm_loss_numpy(pred, y, mask)
    print(f"case {name} n_static: got {r['n_static'].tolist()} want {exp['n_static'].tolist()}")
    assert r["n_static"].dtype == np.int64 and np.array_equal(r["n_static"], exp["n_static"])
    assert np.array_equal(np.isnan(r["tgm_per_pair"]), exp["n_static"] == 0)            # skipped pairs, and only those, are NaN


def test_validation_loss_combines_the_parts(losses, golden_dir):
    pred, y, mask, exp = load_case(golden_dir, "E")
    for variant in VARIANTS:
        r = losses.validation_loss_numpy(pred, y, mask, variant=variant)
        assert r["loss"] == 10.0 * r["tgm"] + 1.0 * r["ssi"]
        assert r["ssi"] == losses.ssi_loss_numpy(pred, y, mask, variant=variant)
        assert r["ssi_per_frame"].shape == pred.shape[:2] and r["tgm_per_pair"].shape == (2, 3)
        assert abs(r["ssi_per_frame"].mean() - r["ssi"]) <= 1e-15 * max(r["ssi"], 1.0)
        r2 = losses.validation_loss_numpy(pred, y, mask, ratio_ssi=0.5, ratio_tgm=2.0, variant=variant)
        assert r2["loss"] == 2.0 * r["tgm"] + 0.5 * r["ssi"]
    # skipped pairs stay in the divisor: clip 0 has one skipped pair of three
    r = losses.validation_loss_numpy(pred, y, mask)
    clips = np.nansum(r["tgm_per_pair"], axis=1) / 3.0
    assert abs(clips.mean() - r["tgm"]) <= 1e-15


def test_channel_axis_none_mask_and_single_frame(losses, golden_dir):
    pred, y, mask, _ = load_case(golden_dir, "A")
    for variant in VARIANTS:
        assert losses.ssi_loss_numpy(pred[:, :, None], y[:, :, None], mask, variant=variant) == losses.ssi_loss_numpy(pred, y, mask, variant=variant)
        assert losses.ssi_loss_numpy(pred, y, None, variant=variant) == losses.ssi_loss_numpy(pred, y, np.ones(pred.shape, bool), variant=variant)
    assert np.isnan(losses.tgm_loss_numpy(pred[:, :1], y[:, :1], mask[:, :1]))          # N = 1: the reference's 0 / 0


def test_masked_median_twin_is_the_lower_median_of_the_keys(losses, golden_dir):
    pred, y, mask, _ = load_case(golden_dir, "C")
    med = losses._masked_median_numpy(pred)
    assert med.shape == (1, 3) and med.dtype == np.float32
    for f in range(3):
        s = np.sort(pred[0, f].ravel())
        assert med[0, f] == s[(s.size - 1) // 2]                                        # numerically torch.median's lower median
    # -0 sorts before +0: five values {-0, -0, +0, +0, 1} have the lower median +0; {-1, -0, -0, +0, +0}: -0
    a = np.array([[[1.0, 0.0, -0.0, 0.0, -0.0]]], dtype=np.float32)
    assert losses._masked_median_numpy(a).view(np.uint32)[0] == 0
    b = np.array([[[0.0, -0.0, -1.0, 0.0, -0.0]]], dtype=np.float32)
    assert losses._masked_median_numpy(b).view(np.uint32)[0] == 0x80000000
    m = np.array([[[0, 0, 0, 0, 0]]], dtype=np.uint8)
    assert losses._masked_median_numpy(a, m)[0] == 0.0                                  # no valid pixel
    v = np.array([3.5, -2.0, 0.0, -0.0, 1e-40, -1e-40, np.inf, -np.inf], dtype=np.float32)
    k = losses._keys(v)
    assert np.array_equal(np.argsort(k, kind="stable"), [7, 1, 5, 3, 2, 4, 0, 6])
    assert losses._values(k).tobytes() == v.tobytes()


def test_python_layer_refuses(losses):
    f32, f64 = np.zeros((1, 2, 3, 4), np.float32), np.zeros((1, 2, 3, 4), np.float64)
    for fn in (losses.ssi_loss_numpy, losses.tgm_loss_numpy, losses.validation_loss_numpy):
        with pytest.raises(ValueError, match="float32"):
            fn(f64, f32)
        with pytest.raises(ValueError, match="shape"):
            fn(f32, f32[:, :1])
        with pytest.raises(ValueError, match="mask"):
            fn(f32, f32, np.zeros((1, 2, 3, 5), bool))
        with pytest.raises(ValueError, match="mask"):
            fn(f32, f32, np.zeros((1, 2, 3, 4), np.float32))
    with pytest.raises(ValueError, match="variant"):
        losses.ssi_loss_numpy(f32, f32, variant="mse")


@pytest.mark.skipif(not os.path.isdir(os.environ.get("VDA_REFERENCE", "/root/reference")), reason="no reference checkout on this machine")
def test_fixture_regenerates_bit_for_bit():
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "gen_loss_golden.py"), "--reference",
                        os.environ.get("VDA_REFERENCE", "/root/reference"), "--check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "reproduced bit for bit" in r.stdout
