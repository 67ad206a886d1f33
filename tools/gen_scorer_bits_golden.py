#!/usr/bin/env python
"""Write tests/golden/scorer_bits.npz: the bits THIS PROJECT's device scorers produce on the cases of tests/_scorer_bits_inputs.py
(evaluate_depth, evaluate_tae, validation_loss, ops.lsq_scale_shift), on one MI355X.

    python tools/gen_scorer_bits_golden.py [--check]

The fixture holds this project's own outputs, not the reference's: how close the scorers are to the reference is the business of
eval_metrics.npz, tae_metrics.npz and loss_metrics.npz and their tests. This one pins the order of the fp64 additions (the
determinism contract stated in csrc/reduce64.h): the results depend on the block counts and the chunking, never on timing, so a
change of a reduction that alters one bit of them is a change of the contract and must be made on purpose, by running this recipe
again and saying so. It was first recorded before csrc/reduce64.h existed, with every kernel still carrying its own copy.

Per case the fixture holds the result dictionaries as raw float64 / int64 arrays and the sha256 of the generated inputs.
--check regenerates everything and compares it with the committed file bit for bit. Needs a GPU."""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from _scorer_bits_inputs import run_cases  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "scorer_bits.npz")


def generate():
    res, sha, tae = run_cases()
    assert tae[0].keys() == tae[1].keys() and all(tae[0][k].tobytes() == tae[1][k].tobytes() for k in tae[0]), "evaluate_tae depends on chunk_pairs"
    # the cases are what they claim to be
    assert res["depth300.whole.n_frames_used"] == 299 and res["depth300.chunk64.n_frames_used"] == 299 and res["depth_blocks.n_frames_used"] == 2
    assert res["tae.pair_counts"].shape == (130, 2) and (res["tae.pair_counts"] > 0).sum() > 256
    for variant in ("lsq", "mad"):
        assert res[f"loss300.{variant}.ssi_per_frame"].shape == (3, 100) and res[f"loss300.{variant}.ssi_per_frame"][1, 37] == 0.0
        assert res[f"loss300.{variant}.n_static"].shape == (3, 99) and (res[f"loss300.{variant}.n_static"] > 0).sum() > 256
    out = dict(res)
    out.update({f"sha256.{k}": np.array(v) for k, v in sha.items()})
    for k in sorted(res):
        a = res[k]
        print(f"{k} {a.dtype}{list(a.shape)}: " + (repr(a.ravel()[:3].tolist()) + (" ..." if a.size > 3 else "")))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--check", action="store_true", help="compare with the committed fixture bit for bit instead of writing it")
    ap.add_argument("--out", default=OUT, help="where to write the fixture")
    args = ap.parse_args()
    new = generate()
    if args.check:
        old = np.load(OUT)
        assert sorted(old.files) == sorted(new), f"keys differ: {sorted(set(old.files) ^ set(new))}"
        bad = [k for k in new if np.asarray(new[k]).dtype != old[k].dtype or np.asarray(new[k]).tobytes() != old[k].tobytes()]
        if bad:
            sys.exit(f"fixture differs in {bad}")
        print(f"{OUT}: reproduced bit for bit")
    else:
        np.savez(args.out, **new)
        print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
