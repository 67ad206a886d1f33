"""CPU: the algebra of option "oc1_mix" in fp64 (tests/_oc1_mix_ref.py) against torch's conv2d(interpolate(conv1x1(r)))."""
import numpy as np
import pytest

import _oc1_mix_ref as R

B, FE, FH = 2, 64, 32


@pytest.mark.parametrize("grid", R.GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_composed_form_equals_torch(grid):
    h, w = grid
    r, W1, Wo, bo, b1 = R.inputs(B, h, w, FE, FH, seed=100 * h + w)
    got, _ = R.mix(r, W1, Wo, bo, b1)
    want = R.target(r, W1, Wo, bo, b1)
    assert got.shape == want.shape == (B, 2 * h, 2 * w, FH)
    assert np.abs(got - want).max() <= 1e-10 * max(1.0, np.abs(want).max())


def test_composed_weights_and_bias():
    _, W1, Wo, bo, _ = R.inputs(1, 1, 1, FE, FH, seed=3)
    Wz, bz = R.compose(W1, Wo, bo)
    assert Wz.shape == (9, FH, FE) and bz.shape == (9, FH)
    for tap in range(9):
        assert np.abs(Wz[tap] - W1.reshape(FH, FE, 9)[:, :, tap] @ Wo).max() <= 1e-12
        assert np.abs(bz[tap] - W1.reshape(FH, FE, 9)[:, :, tap] @ bo).max() <= 1e-12
    Wp, bp = R.pack(Wz, bz, 64)
    assert Wp.shape == (9 * 64, FE) and not Wp.reshape(9, 64, FE)[:, FH:].any() and not bp.reshape(9, 64)[:, FH:].any()
    assert np.array_equal(Wp.reshape(9, 64, FE)[:, :FH], Wz)


def test_single_pixel_grid_is_all_padding_but_the_inside_taps():
    """1 x 1: the scale is 0, every sample lands on pixel 0 with weight 1; output (Y, X) of the 2 x 2 map sums the taps whose q is inside."""
    g = np.random.default_rng(0)
    z = g.integers(-8, 9, size=(B, 1, 1, 9, FH)).astype(np.float64)
    out = R.gather(z)
    for Y in range(2):
        for X in range(2):
            want = sum(z[:, 0, 0, 3 * ky + kx] for ky in range(3) for kx in range(3) if 0 <= Y + ky - 1 < 2 and 0 <= X + kx - 1 < 2)
            assert np.array_equal(out[:, Y, X], want)


def test_no_sample_crosses_a_frame():
    """NaN in frame 0 stays out of frame 1."""
    r, W1, Wo, bo, b1 = R.inputs(B, 5, 7, FE, FH, seed=9)
    _, z = R.mix(r, W1, Wo, bo, b1)
    z[0] = np.nan
    out = R.gather(z, b1)
    assert np.isnan(out[0]).all() and np.isfinite(out[1]).all()


def test_last_grid_spans_two_tiles_unevenly():
    h, w = R.GRIDS[-1]
    assert R.TILE_ROWS < 2 * h < 2 * R.TILE_ROWS and (2 * h) % R.TILE_ROWS != 0
    for Fhp in (32, 128):
        assert 2 * w > R.tile_cols(Fhp) and (2 * w) % R.tile_cols(Fhp) != 0
