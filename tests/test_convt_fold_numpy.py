"""CPU: the algebra of the folded ConvTranspose2d(k == stride) + 3x3 conv (tests/_convt_fold_ref.py) against
conv2d(conv_transpose2d(x)) in fp64, border bias included."""
import pytest
import torch

import _convt_fold_ref as R

GRIDS = [(1, 1), (1, 3), (2, 3), (5, 7)]


def operands(k, seed, Ci=5, Cm=4, Co=3, B=2, H=1, W=1):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return rn(B, Ci, H, W), rn(Ci, Cm, k, k), rn(Cm), rn(Co, Cm, 3, 3)


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_composed_pair_equals_conv_of_conv_transpose(k, grid):
    t, wt, bt, wr = operands(k, 100 * k + grid[0] * 10 + grid[1], H=grid[0], W=grid[1])
    ref = R.unfused(t, wt, bt, wr, k)
    Wc, Bc = R.compose(wt, bt, wr)
    for name, got in (("in-image taps", R.apply(t, Wc, Bc, k)), ("class-bias table", R.apply_by_class(t, Wc, Bc, k))):
        assert got.shape == ref.shape == (2, 3, k * grid[0], k * grid[1])
        err = float((got - ref).abs().max())
        assert err <= 1e-10, f"k={k} grid={grid} ({name}): max abs difference {err:.3e}"


def test_bias_alone_depends_on_the_border_class():
    """t = 0: the output is the ConvTranspose's bias seen through the conv's zero padding - not constant over the image."""
    for k in (2, 4):
        t, wt, bt, wr = operands(k, 7, H=3, W=3)
        Wc, Bc = R.compose(wt, bt, wr)
        out = R.apply_by_class(torch.zeros_like(t), Wc, Bc, k)
        assert float((out - R.unfused(torch.zeros_like(t), wt, bt, wr, k)).abs().max()) <= 1e-10
        assert float((out[:, :, 0, 0] - out[:, :, k + 1, k + 1]).abs().max()) > 1e-3


@pytest.mark.parametrize("k,blocks", [(4, 36), (2, 16)])
def test_tap_counts(k, blocks):
    """Of the k*k*9 (phase, tap) blocks only 36 (k = 4) / 16 (k = 2) are ever reached: 2.25 / 4 taps per output instead of 9."""
    assert R.tap_blocks(k) == blocks
    _, wt, bt, wr = operands(k, 3)
    Wc, _ = R.compose(wt, bt, wr)
    assert R.tap_blocks(Wc) == blocks
    packed = R.pack(Wc, cin_pad=8)
    assert packed.shape == (k * k * 3, 9 * 8) and float(packed.reshape(k * k, 3, 9, 8)[..., 5:].abs().max()) == 0.0


def test_exact_inputs_stay_small_integers():
    """The GPU cases' operands: the fp16 intermediate of the unfused arm and every result are integers of magnitude <= 2048."""
    for k in (2, 4):
        t, wt, bt, wr = R.exact_inputs(k, 64, 64, 2, 5, 7, seed=k)
        l1 = torch.nn.functional.conv_transpose2d(t, wt, bt, stride=k)
        out = R.unfused(t, wt, bt, wr, k)
        for v in (l1, out):
            assert bool((v == v.round()).all()) and float(v.abs().max()) <= 2048
        assert int((wr != 0).sum(dim=1).max()) <= 3
