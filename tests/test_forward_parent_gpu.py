"""vda_forward against its own recorded past: tests/golden/forward_parent.npz was written by tools/record_forward_parent.py with the
commit BEFORE Run::forward (csrc/host.hip) was written as named stages. A restructuring of a launch sequence is right when the
parent's bits, workspace and launch set come back, so every comparison is for equality: the workspace size in both precisions, the
profile's (launches, FLOPs) per kernel name, and the SHA-256 of the depth and of every stage vda_debug_copy can name, on the
smallest shapes at which each branch of the sequence still runs (tests/_forward_parent_cases.py). Each case runs two forwards and
the second hashes like the first."""
import json

import numpy as np
import pytest

import _forward_parent_cases as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent():
    return np.load(F.FIXTURE)


@pytest.mark.parametrize("case", F.CASES, ids=F.IDS)
def test_forward_equals_the_parent_commit(parent, case):
    cid = F.case_id(case)
    want, got = json.loads(str(parent[cid])), json.loads(json.dumps(F.record(case)))
    assert got["workspace_f16"] == want["workspace_f16"] and got["workspace_f32"] == want["workspace_f32"], f"{cid}: vda_workspace_bytes changed"
    assert got["profile"] == want["profile"], f"{cid}: the set of GEMM / conv launches changed: " + ", ".join(
        f"{k}: {want['profile'].get(k)} -> {got['profile'].get(k)}" for k in sorted(set(want["profile"]) | set(got["profile"]))
        if want["profile"].get(k) != got["profile"].get(k))
    assert sorted(got["stages"]) == sorted(want["stages"]), f"{cid}: the stages that exist changed"
    bad = [k for k in want["stages"] if got["stages"][k] != want["stages"][k]]
    assert not bad, f"{cid}: stages differ from the parent's bits: {bad}"
    assert got["depth"] == want["depth"], f"{cid}: the depth differs from the parent's bits"
