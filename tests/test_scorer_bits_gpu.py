"""The device scorers' results, byte for byte, against tests/golden/scorer_bits.npz (tools/gen_scorer_bits_golden.py: this project's
own outputs, recorded on an MI355X before csrc/reduce64.h replaced the kernels' private copies of the reduction). The order of the
fp64 additions is a checked contract: the other scorer tests hold the device against the reference and the numpy twins within a
tolerance and a run against itself bit for bit, which a changed summation order passes. The cases (tests/_scorer_bits_inputs.py) have
more than 256 planes, several blocks per plane, chunk row offsets and a wrapping grid-stride loop."""
import os

import numpy as np
import pytest

import _scorer_bits_inputs as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run(golden_dir):
    """(fixture, device results, input checksums, the two TAE runs): every case once, shared and never written to."""
    return (np.load(os.path.join(golden_dir, "scorer_bits.npz")),) + cases.run_cases()


def assert_same_bytes(fix, got, prefix):
    keys = sorted(k for k in fix.files if k.startswith(prefix + "."))
    assert keys and keys == sorted(k for k in got if k.startswith(prefix + ".")), (keys, sorted(got))
    bad = []
    for k in keys:
        same = got[k].dtype == fix[k].dtype and got[k].shape == fix[k].shape and got[k].tobytes() == fix[k].tobytes()
        if not same:
            differ = int((got[k].ravel().view(np.uint8) != fix[k].ravel().view(np.uint8)).sum()) if got[k].shape == fix[k].shape else -1
            print(f"{k}: got {got[k].ravel()[:4].tolist()!r} recorded {fix[k].ravel()[:4].tolist()!r} ({differ} bytes differ)")
            bad.append(k)
    assert not bad, f"results differ from the recorded bits: {bad}"


def test_inputs_are_the_recorded_ones(run):
    fix, _, sha, _ = run
    assert {f"sha256.{k}": v for k, v in sha.items()} == {k: str(fix[k]) for k in fix.files if k.startswith("sha256.")}


@pytest.mark.parametrize("case", ["depth300.whole", "depth300.chunk64", "depth_blocks"])
def test_evaluate_depth_bits(run, case):
    """300 frames of 7 x 9 (one without a valid pixel, float32 gt) whole and in chunks of 64 frames - two records, the chunkings may
    differ; 2 frames of 40 x 520 with float64 gt."""
    assert_same_bytes(run[0], run[1], case)


def test_evaluate_tae_bits(run):
    """131 frames of 6 x 8 with a mask: chunk_pairs None and 50 agree with each other and with the one record."""
    fix, _, _, tae = run
    for got in tae:
        assert_same_bytes(fix, got, "tae")


@pytest.mark.parametrize("variant", ["lsq", "mad"])
@pytest.mark.parametrize("case", ["loss300", "loss_wrap"])
def test_validation_loss_bits(run, case, variant):
    """[3,100,5,7] with a mask that empties a frame (300 frame planes, 297 pair planes); [1,2,130,257] where the grid-stride loop wraps."""
    assert_same_bytes(run[0], run[1], f"{case}.{variant}")


@pytest.mark.parametrize("n", cases.STITCH_SIZES)
def test_stitch_lsq_scale_shift_bits(run, n):
    assert run[1][f"stitch{n}.scale_shift"].dtype == np.float32
    assert_same_bytes(run[0], run[1], f"stitch{n}")
