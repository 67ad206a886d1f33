#!/usr/bin/env python
"""Write tests/golden/forward_parent.npz: what vda_forward computes, requests and launches on the cases of
tests/_forward_parent_cases.py, on one MI355X.

    python tools/record_forward_parent.py [--check]

Run it with the PARENT of a change to the launch sequence (csrc/host.hip) built, never with the change itself: the fixture is the
parent's recorded behaviour, and tests/test_forward_parent_gpu.py holds the new code to it with no tolerance. Per case it holds
one JSON record: vda_workspace_bytes in both precisions, the handle's profile at every = 1 (kernel name -> launches, FLOPs), and
the SHA-256 of the depth and of every stage vda_debug_copy can name. It first recorded commit 09b6963, before Run::forward was
written as named stages. --check records again and compares with the committed file. Needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import _forward_parent_cases as F  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    got = {i: json.dumps(F.record(c), sort_keys=True) for i, c in zip(F.IDS, F.CASES)}
    if args.check:
        z = np.load(F.FIXTURE)
        bad = [i for i in got if i not in z.files or str(z[i]) != got[i]]
        print(f"{len(got) - len(bad)} of {len(got)} cases equal the committed fixture" + ("; differ: " + ", ".join(bad) if bad else ""))
        return 1 if bad else 0
    np.savez_compressed(F.FIXTURE, **{i: np.array(v) for i, v in got.items()})
    print(f"wrote {F.FIXTURE}: {len(got)} cases, {os.path.getsize(F.FIXTURE)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
