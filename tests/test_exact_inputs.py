"""CPU proof that the exact-integer GPU tests (tests/test_kernels_f32_edges_gpu.py) can fail, and that their references are sound.

For every dense, conv3x3, ConvTranspose and patch-embed case of tests/_exact.py:
  1. the inputs meet the 2**24 condition (assert_exact_safe on the |operand| reference);
  2. torch's own fp32 CPU evaluation equals the fp64 reference exactly - the condition alone makes fp32 exact, whatever the order;
  3. four indexing mistakes a kernel could make, restated in plain torch, each break the equality on the case's inputs:
     one k index dropped, one conv tap shifted by a pixel, zero padding replaced by edge clamping, two adjacent output columns
     swapped. (Tap shift: conv3x3 and the patch embed's 14x14 window; padding: conv3x3, the only op that pads.)
A case whose inputs let a mistake through would make its GPU test vacuous for that mistake: the inputs are changed, not the check."""
import pytest
import torch

import _exact as E

F64 = torch.float64


def dbl(d):
    return {k: v.double() for k, v in d.items()}


def swapped(t, j, dim=-1):
    idx = list(range(t.shape[dim]))
    idx[j], idx[j + 1] = idx[j + 1], idx[j]
    return t.index_select(dim, torch.tensor(idx))


def differs(a, b, what):
    assert a.shape == b.shape
    assert not torch.equal(a, b), f"{what} goes unnoticed on these inputs"


# ------------------------------------------------------------------------------------------------ dense
@pytest.mark.parametrize("case", E.DENSE_CASES, ids=E.dense_id)
def test_dense_case_is_exact_and_sensitive(case):
    M, N, K, lda, ldc = case
    assert lda >= K and ldc >= N and K % 16 == 0 and N % 4 == 0 and lda % 4 == 0 and ldc % 4 == 0
    inp = E.dense_inputs(case)
    assert bool(inp["A"][:, K:].isnan().all()), "pad columns of A hold NaN"
    E.assert_exact_safe(*E.dense_bounds(inp, K))
    d = dbl(inp)
    ref = E.dense_lin(d["A"], d["W"], d["bias"], K)
    lin = E.dense_lin(inp["A"], inp["W"], inp["bias"], K)
    assert torch.equal(lin.double(), ref)
    assert torch.equal((inp["res"] + inp["gamma"] * lin).double(), d["res"] + d["gamma"] * ref)
    assert torch.equal((lin + inp["res"] + inp["res2"]).double(), ref + d["res"] + d["res2"])
    assert torch.equal(torch.relu(lin).double(), torch.relu(ref)) and bool((ref < 0).any()) and bool((ref > 0).any())

    for k in sorted({0, K // 2 + 1, K - 1}):
        A2 = d["A"].clone()
        A2[:, k] = 0
        differs(E.dense_lin(A2, d["W"], d["bias"], K), ref, f"dropping k = {k}")
    for j in sorted({0, N // 2 - 1, N - 2}):
        differs(swapped(ref, j), ref, f"swapping output columns {j} and {j + 1}")


# ------------------------------------------------------------------------------------------------ conv3x3
@pytest.mark.parametrize("case", E.CONV_CASES, ids=E.conv_id)
def test_conv_case_is_exact_and_sensitive(case):
    B, H, W, Cin, Cout, stride, relu_in = case
    inp = E.conv_inputs(case)
    a = {k: v.double().abs() for k, v in inp.items()}
    E.assert_exact_safe(E.conv_ref(a["x"], a["w"], a["bias"], stride, False) + a["res"])
    d = dbl(inp)
    ref = E.conv_ref(d["x"], d["w"], d["bias"], stride, relu_in)
    assert ref.shape == inp["res"].shape
    assert torch.equal(E.conv_ref(inp["x"], inp["w"], inp["bias"], stride, relu_in).double(), ref)
    assert torch.equal(E.conv_ref(inp["x"], inp["w"], None, stride, relu_in).double(), E.conv_ref(d["x"], d["w"], None, stride, relu_in))
    assert torch.equal(E.conv_by_taps(d["x"], d["w"], d["bias"], stride, relu_in), ref), "the tap-by-tap restatement is the convolution"
    if relu_in:
        differs(E.conv_ref(d["x"], d["w"], d["bias"], stride, False), ref, "ignoring relu_in")

    for ci in sorted({0, Cin // 2 + 1, Cin - 1}):          # k = (centre tap, ci): the one tap every output pixel has inside the image
        w2 = d["w"].clone()
        w2[:, ci, 1, 1] = 0
        differs(E.conv_ref(d["x"], w2, d["bias"], stride, relu_in), ref, f"dropping k = (tap 4, ci {ci})")
    differs(E.conv_by_taps(d["x"], d["w"], d["bias"], stride, relu_in, shift_tap=(1, 1)), ref, "shifting the centre tap by a pixel")
    differs(E.conv_by_taps(d["x"], d["w"], d["bias"], stride, relu_in, clamp_pad=True), ref, "edge clamping in place of zero padding")
    for j in sorted({0, Cout // 2 - 1, Cout - 2}):
        differs(swapped(ref, j), ref, f"swapping output channels {j} and {j + 1}")


# ------------------------------------------------------------------------------------------------ ConvTranspose
@pytest.mark.parametrize("k", E.CONVT_K)
@pytest.mark.parametrize("case", E.CONVT_CASES, ids=lambda c: "B%d-%dx%d-C%d-Cp%d" % c)
def test_convt_case_is_exact_and_sensitive(case, k):
    B, h, w, C, Cp = case
    inp = E.convt_inputs(case, k)
    a = {n: v.double().abs() for n, v in inp.items()}
    E.assert_exact_safe(E.convt_ref(a["x"], a["w"], a["bias"], k))
    d = dbl(inp)
    ref = E.convt_ref(d["x"], d["w"], d["bias"], k)
    assert ref.shape == (B, h * k, w * k, C)
    assert torch.equal(E.convt_ref(inp["x"], inp["w"], inp["bias"], k).double(), ref)

    for ci in sorted({0, C // 2 + 1, C - 1}):
        w2 = d["w"].clone()
        w2[ci] = 0
        differs(E.convt_ref(d["x"], w2, d["bias"], k), ref, f"dropping k = ci {ci}")
    for j in sorted({0, C - 2}):
        differs(swapped(ref, j), ref, f"swapping output channels {j} and {j + 1}")
    differs(swapped(ref, 0, dim=2), ref, "swapping two adjacent columns of the scatter (kx = 0 and 1 of the first input pixel)")
    differs(swapped(ref, 0, dim=1), ref, "swapping two adjacent rows of the scatter (ky = 0 and 1)")


# ------------------------------------------------------------------------------------------------ patch embed
@pytest.mark.parametrize("case", E.PATCH_CASES, ids=lambda c: "B%d-%dx%d-D%d" % c)
def test_patch_case_is_exact_and_sensitive(case):
    B, H, W, D = case
    inp = E.patch_inputs(case)
    a = {n: v.double().abs() for n, v in inp.items()}
    E.assert_exact_safe(E.patch_ref(a["x"], a["w"], a["bias"], a["pos"], a["cls"]))
    d = dbl(inp)
    ref = E.patch_ref(d["x"], d["w"], d["bias"], d["pos"], d["cls"])
    P = (H // 14) * (W // 14)
    assert ref.shape == (B, P + 1, D)
    assert torch.equal(E.patch_ref(inp["x"], inp["w"], inp["bias"], inp["pos"], inp["cls"]).double(), ref)

    def by_gemm(A, w588):        # the patch rows as the GEMM computes them
        return (A @ w588.t() + d["bias"]).reshape(B, P, D) + d["pos"][1:]

    A, w588 = E.unfold14(d["x"]), d["w"].reshape(D, 588)
    assert torch.equal(by_gemm(A, w588), ref[:, 1:]), "unfold + GEMM is the strided convolution"
    for kk in (0, 300, 587):
        w2 = w588.clone()
        w2[:, kk] = 0
        differs(by_gemm(A, w2), ref[:, 1:], f"dropping k = {kk}")
    A2 = A.clone()
    A2[:, 200] = A[:, 201]                                   # (c 1, ky 0, kx 4) reads pixel kx 5
    differs(by_gemm(A2, w588), ref[:, 1:], "shifting one tap of the 14x14 window by a pixel")
    for j in sorted({0, D // 2 - 1, D - 2}):
        differs(swapped(ref, j), ref, f"swapping output columns {j} and {j + 1}")
    if B > 1 or P > 1:
        differs(swapped(ref, 1, dim=1) if P > 1 else ref.flip(0), ref, "swapping two token rows")


def test_helpers_refuse_what_they_should():
    with pytest.raises(AssertionError, match="2\\*\\*24"):
        E.assert_exact_safe(torch.tensor([2.0 ** 24], dtype=F64))
    with pytest.raises(AssertionError, match="not integers"):
        E.assert_exact_safe(torch.tensor([0.5], dtype=F64))
    E.assert_exact_safe(torch.tensor([2.0 ** 24 - 1], dtype=F64))
    x = E.ints((1000,), -3, 3, 5)
    assert x.dtype == torch.float32 and float(x.min()) == -3 and float(x.max()) == 3 and torch.equal(x, E.ints((1000,), -3, 3, 5))
    assert bool(torch.tensor([E.SENTINEL_BITS], dtype=torch.int32).view(torch.float32).isnan().all()), "the sentinel is a NaN"
