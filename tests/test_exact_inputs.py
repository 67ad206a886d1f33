"""CPU proof that the exact-integer GPU tests (tests/test_kernels_f32_edges_gpu.py) can fail, and that their references are sound.

For every dense, conv3x3, ConvTranspose and patch-embed case of tests/_exact.py:
  1. the inputs meet the 2**24 condition (assert_exact_safe on the |operand| reference);
  2. torch's own fp32 CPU evaluation equals the fp64 reference exactly - the condition alone makes fp32 exact, whatever the order;
  3. four indexing mistakes a kernel could make, restated in plain torch, each break the equality on the case's inputs:
     one k index dropped, one conv tap shifted by a pixel, zero padding replaced by edge clamping, two adjacent output columns
     swapped. (Tap shift: conv3x3 and the patch embed's 14x14 window; padding: conv3x3, the only op that pads.)
A case whose inputs let a mistake through would make its GPU test vacuous for that mistake: the inputs are changed, not the check.

The second half of the file does the same for the fp16 GEMM's cases (tests/test_kernels_f16_edges_gpu.py), the last part for the fp16
attention kernels' exact-softmax inputs (tests/test_attention_edges_gpu.py), the part behind it for the fused upsample convolutions'
constant, selector and dyadic inputs (tests/test_upsample_edges_gpu.py), see there."""
import functools

import pytest
import torch
import torch.nn.functional as F

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


# ================================================================================================ the fp16 GEMM's cases
# The same three steps for tests/test_kernels_f16_edges_gpu.py, with the second condition (what is stored as fp16 is an fp16 value) and the
# mistakes the fp16 kernels could make: a dropped 64-wide K step, a staged row taken from min(m + 1, M - 1), the last 8-column row
# segment swapped with the one before it, a shifted tap, clamped padding.
F16 = torch.float16


def is_f16(t):
    return torch.equal(t.to(F16).to(t.dtype), t)


def next_row(t):
    """Row m of the result from row min(m + 1, M - 1) of the operand."""
    return t[torch.arange(1, t.shape[0] + 1).clamp_max(t.shape[0] - 1)]


def last_segments_swapped(t):
    N = t.shape[-1]
    return torch.cat((t[..., :N - 16], t[..., N - 8:], t[..., N - 16:N - 8]), dim=-1)


@pytest.mark.parametrize("case", E.DENSE16_CASES, ids=E.dense_id)
def test_dense16_case_is_exact_and_sensitive(case):
    M, N, K, lda, ldc = case
    assert lda >= K and ldc >= N and K % 64 == 0 and lda % 8 == 0 and N % 4 == 0 and ldc % 4 == 0
    assert (N % 8 == 0 and ldc % 8 == 0) or case == E.DENSE16_CASES[-1]
    inp = E.dense16_inputs(case)
    assert all(is_f16(v) for v in inp.values()), "every operand is its own fp16 rounding"
    ref = E.dense16_check(inp)                                  # both conditions, every exact epilogue
    f32 = E.dense16_refs(inp)                                   # torch's own fp32 evaluation, whatever its order
    assert set(ref) == set(e for e in E.dense16_epis(case) if e in E.DENSE16_EXACT)
    for k, r in ref.items():
        assert torch.equal(f32[k].double(), r), k
        if k not in E.DENSE16_F32_OUT:
            assert is_f16(r), f"{k}: stored as fp16"
    d = dbl(inp)
    Wf, c1, c2 = E.fold_ln(d)
    assert is_f16(Wf) and all(torch.equal(a.double(), b) for a, b in zip(E.fold_ln(inp), (Wf, c1, c2)))
    assert bool((ref["bias_f16"] < 0).any()) and bool((ref["bias_f16"] > 0).any()), "ReLU has something to do"
    assert len(set(inp["rstd"].tolist())) == (3 if M > 8 else 1) and (M == 1 or bool((inp["mean"] != 0).any()))

    for name in ("bias_f16", "ln_bias"):
        for kt in sorted({0, K // 128, K // 64 - 1}):           # a whole K step: what a pipeline that starts late or ends early loses
            d2 = dict(d, A=d["A"].clone())
            d2["A"][:, 64 * kt:64 * kt + 64] = 0
            differs(E.dense16_refs(d2)[name], ref[name], f"{name}: dropping K step {kt}")
        if M > 1:                                               # (M == 1 has no other row to take)
            differs(E.dense16_refs(dict(d, A=next_row(d["A"])))[name], ref[name], f"{name}: rows staged from min(m + 1, M - 1)")
    for name, r in ref.items():
        if N >= 16:                                             # (N == 8 has one segment)
            differs(last_segments_swapped(r), r, f"{name}: the last 8-column segment swapped with the one before")
    if "split" in ref:
        differs(ref["split_pos"], ref["split"], "ignoring the re-centring rows")
        sums = ref["split"].reshape(M, N // 64, 64).sum(-1)
        assert M == 1 or N == 64 or len(set(sums.flatten().tolist())) > 1, "the partial sums tell column blocks and rows apart"


@pytest.mark.parametrize("case", E.BROADCAST16_CASES + [E.walk16_case(256, N) for N in E.WALK16_N] + [E.split16_case(256), E.walk16_case(256, 2048)[:2] + (E.WALK16_BLOCKED_K,)], ids=lambda c: "M%d-N%d-K%d" % c)
def test_walk16_and_broadcast_cases_are_exact_and_sensitive(case):
    """(The broadcast case uses row 0 of the same inputs; the row-split case is checked on sampled rows, as on the GPU.)"""
    M, N, K = case
    inp = E.walk16_inputs(case)
    rows = torch.arange(0, M, 61)
    A = inp["A"][rows]
    d = dict(A=A.double(), W=inp["W"].double(), bias=inp["bias"].double())
    lin = d["A"] @ d["W"].t() + d["bias"]
    E.assert_exact_safe_f16([d["A"].abs() @ d["W"].abs().t() + d["bias"].abs()], [lin])
    assert torch.equal((A @ inp["W"].t() + inp["bias"]).double(), lin)
    A2 = d["A"].clone()
    A2[:, K - 64:] = 0
    differs(A2 @ d["W"].t() + d["bias"], lin, "dropping the last K step")
    differs(next_row(inp["A"].double())[rows] @ d["W"].t() + d["bias"], lin, "rows staged from min(m + 1, M - 1)")
    differs(last_segments_swapped(lin), lin, "the last two 8-column segments swapped")
    # a tile computed for the wrong place: tile (i, j) of 256 x 256 holds other values than its neighbours
    assert not torch.equal(lin[:, :256], lin[:, 256:512]) if N >= 512 else True


@pytest.mark.parametrize("case", E.PATCH16_CASES + E.SEAM_PATCH16_CASES, ids=lambda c: "fr%d-P%d-N%d-K%d-ldc%d" % c)
def test_patch16_case_is_exact_and_sensitive(case):
    fr, P, N, K, ldc = case
    inp = E.patch16_inputs(case)
    d, a = dbl(inp), {k: v.double().abs() for k, v in inp.items()}
    E.assert_exact_safe(E.patch16_ref(a, P))                    # fp32 out: the first condition alone
    ref = E.patch16_ref(d, P)
    assert all(is_f16(inp[k]) for k in ("A", "W")) and torch.equal(E.patch16_ref(inp, P).double(), ref)
    differs(E.patch16_ref(dict(d, A=next_row(d["A"])), P), ref, "rows staged from min(m + 1, M - 1)")
    differs(last_segments_swapped(ref), ref, "the last two 8-column segments swapped")
    if P > 1:
        differs(swapped(ref, 0, dim=1), ref, "two patch rows of a frame swapped")
    differs(ref.flip(0), ref, "frames in the wrong order")


@pytest.mark.parametrize("k", E.CONVT_K)
@pytest.mark.parametrize("case", E.CONVT16_CASES + E.SEAM_CONVT16_CASES, ids=lambda c: "B%d-%dx%d-C%d-Cp%d" % c)
def test_convt16_case_is_exact_and_sensitive(case, k):
    B, h, w, C, Cp = case
    inp = E.convt16_inputs(case, k)
    d, a = dbl(inp), {n: v.double().abs() for n, v in inp.items()}
    ref = E.convt_ref(d["x"], d["w"], d["bias"], k)
    E.assert_exact_safe_f16([E.convt_ref(a["x"], a["w"], a["bias"], k)], [ref])
    assert Cp % 64 == 0 and all(is_f16(v) for v in inp.values())
    assert torch.equal(E.convt_ref(inp["x"], inp["w"], inp["bias"], k).double(), ref)
    w2 = d["w"].clone()
    w2[C - 1] = 0
    differs(E.convt_ref(d["x"], w2, d["bias"], k), ref, "dropping the last input channel")
    differs(swapped(ref, 0, dim=2), ref, "two adjacent columns of the scatter swapped")
    differs(swapped(ref, 0, dim=1), ref, "two adjacent rows of the scatter swapped")
    differs(last_segments_swapped(ref), ref, "the last two 8-channel segments swapped")


@pytest.mark.parametrize("case", E.CONV16_CASES + E.SEAM_CONV16_CASES, ids=E.conv16_id)
def test_conv16_case_is_exact_and_sensitive(case):
    B, H, W, Cin, Cout, stride, relu_in, ldc = case
    assert Cin % 64 == 0 and Cout % 8 == 0 and ldc % 8 == 0 and ldc >= Cout
    inp = E.conv16_inputs(case)
    assert all(is_f16(v) for v in inp.values())
    ref = E.conv16_check(case, inp)
    f32 = E.conv16_refs(inp, stride, relu_in)
    for k, r in ref.items():
        assert torch.equal(f32[k].double(), r) and is_f16(r), k
    d = dbl(inp)
    lin = ref["bias_f16"]
    assert lin.shape == inp["res"].shape
    assert torch.equal(E.conv_by_taps(d["x"], d["w"], d["bias"], stride, relu_in), lin), "the tap-by-tap restatement is the convolution"
    if relu_in:
        differs(E.conv_ref(d["x"], d["w"], d["bias"], stride, False), lin, "ignoring relu_in")
    for kt in sorted({0, Cin // 64 - 1}):                       # a K step = 64 input channels of one tap; the centre tap is inside the image for every pixel
        w2 = d["w"].clone()
        w2[:, 64 * kt:64 * kt + 64, 1, 1] = 0
        differs(E.conv_ref(d["x"], w2, d["bias"], stride, relu_in), lin, f"dropping the K step (tap 4, channels {64 * kt}..)")
    differs(E.conv_by_taps(d["x"], d["w"], d["bias"], stride, relu_in, shift_tap=(1, 1)), lin, "shifting the centre tap by a pixel")
    differs(E.conv_by_taps(d["x"], d["w"], d["bias"], stride, relu_in, clamp_pad=True), lin, "edge clamping in place of zero padding")
    flat = lin.reshape(-1, Cout)
    if flat.shape[0] > 1:
        differs(next_row(flat), flat, "output pixel m computed from the window of min(m + 1, M - 1)")
    if Cout >= 16:
        differs(last_segments_swapped(lin), lin, "the last two 8-channel segments swapped")


@pytest.mark.parametrize("Cc", E.TAIL16_C)
@pytest.mark.parametrize("case", E.TAIL16_CASES, ids=lambda c: "B%d-%dx%d" % c)
def test_tail16_case_is_exact_and_sensitive(case, Cc):
    inp = E.tail16_inputs(case, Cc)
    b3 = inp.pop("b3")
    assert all(is_f16(inp[k]) for k in ("x", "w2"))
    d, a = dbl(inp), {k: v.double().abs() for k, v in inp.items()}
    E.assert_exact_safe(E.tail16_ref(a, abs(b3)), F.conv2d(a["x"], a["w2"], a["b2"], padding=1))
    ref = E.tail16_ref(d, b3)
    assert torch.equal(E.tail16_ref(inp, b3).double(), ref) and bool((ref > 0).any())
    w2 = d["w2"].clone()
    w2[:, Cc - 64:, 1, 1] = 0
    differs(E.tail16_ref(dict(d, w2=w2), b3), ref, "dropping the centre tap's last K step")
    y = F.conv2d(d["x"], d["w2"], d["b2"], padding=1)
    differs(F.relu((y * d["w3"].view(1, 32, 1, 1)).sum(1) + b3), ref, "no ReLU between the two convolutions")
    xc = F.pad(d["x"], (1, 1, 1, 1), mode="replicate")
    differs(F.relu((F.relu(F.conv2d(xc, d["w2"], d["b2"])) * d["w3"].view(1, 32, 1, 1)).sum(1) + b3), ref, "edge clamping in place of zero padding")


def test_f16_helpers_refuse_what_they_should():
    ok = torch.tensor([2048.0, -3.0], dtype=F64)
    E.assert_exact_safe_f16([ok], [ok])
    with pytest.raises(AssertionError, match="> 2048"):
        E.assert_exact_safe_f16([ok], [torch.tensor([2049.0], dtype=F64)])
    with pytest.raises(AssertionError, match="multiple"):
        E.assert_exact_safe_f16([ok], [torch.tensor([0.5], dtype=F64)])
    E.assert_exact_safe_f16([ok], [torch.tensor([1023.5], dtype=F64)], step=0.5)
    with pytest.raises(AssertionError, match="> 2048"):
        E.assert_exact_safe_f16([ok], [torch.tensor([1024.5], dtype=F64)], step=0.5)
    with pytest.raises(AssertionError, match="2\\*\\*24"):
        E.assert_exact_safe_f16([torch.tensor([2.0 ** 24], dtype=F64)], [ok])
    assert E.FP16_EXACT_LIMIT == 2048.0
    assert bool(torch.tensor([E.SENTINEL16_BITS], dtype=torch.int16).view(F16).isnan().all()), "the fp16 sentinel is a NaN"
    from video_depth_anything_amd import _lib
    assert all(getattr(_lib, "EPI_" + k) == v for k, v in E.EPI.items()) and len(E.EPI) == 13
    assert _lib.EPI_CONVT_FOLD_F16 == E.EPI_CONVT_FOLD_F16


# ================================================================================================ tile seams: a persistent workgroup's later tiles
# tests/test_kernels_f16_edges_gpu.py runs the seam cases of tests/_exact.py under vda_set_max_wgs(8 or 16). Here, without a GPU: the
# walk model says of every case what it is there for (two full rounds and a partial one, the partial row tile in a later round, ...),
# the planner gives every built large tile its launches, the exactness preconditions hold, and a tile of round >= 1 computed with
# something its workgroup's PREVIOUS tile left behind - bias, residual / statistics / pos rows, the first K step's A or W rows, the
# conv row origin, the column of an unrotated fold round - or without its second K step differs from the reference inside that tile.
@pytest.fixture(scope="module")
def L():
    from video_depth_anything_amd import _lib
    yield _lib
    _lib.lib.vda_gemm_set_variant(-1)


def test_tile_walk_model():
    """The restatement against hand-walked launches: 19 tiles on 8 workgroups, one column tile (dealt: the last round's three tiles go
    to XCDs 0, 1, 2); 21 tiles in three columns (plain: XCDs 0..4); 36 tiles in two columns on 16 (dealt by row panel); the folded
    rotation is a bijection of every round's tiles and moves round 1 by FOLD_ROT columns."""
    w = E.tile_walk(19 * 256 - 37, 256, 256, 256, 8)
    assert (w["full_rounds"], w["rem"], w["deal_last"]) == (2, 3, True) and w["tiles"] == [[b, 8 + b] + ([16 + b] if b < 3 else []) for b in range(8)]
    w = E.tile_walk(7 * 256 - 37, 520, 256, 256, 8)
    assert (w["nbn"], w["full_rounds"], w["rem"], w["deal_last"]) == (3, 2, 5, False) and w["tiles"][4] == [4, 12, 20] and w["tiles"][5] == [5, 13]
    w = E.tile_walk(18 * 256 - 37, 264, 256, 256, 16)
    assert (w["per_xcd"], w["rem"], w["deal_last"]) == (2, 4, True)
    assert [len(m) for m in w["tiles"]] == [3, 3] + [2] * 6 + [3, 3] + [2] * 6 and w["tiles"][0] == [0, 16, 32] and w["tiles"][8] == [1, 17, 33] and w["tiles"][1] == [2, 18, 34]
    for nbn in (2, 4):
        plain, fold = E.tile_walk(2400, nbn * 256, 256, 256, 8), E.tile_walk(2400, nbn * 256, 256, 256, 8, fold=True)
        for r in range(3):
            a, b = [m[r] for m in plain["tiles"] if len(m) > r], [m[r] for m in fold["tiles"] if len(m) > r]
            assert sorted(a) == sorted(b) and (a == b) == (r * E.FOLD_ROT % nbn == 0 or r == 0)
        assert fold["tiles"][0][1] == 8 + E.FOLD_ROT % nbn


@functools.lru_cache(maxsize=None)
def seam_dense(case):
    inp = E.dense16_inputs(case)
    return inp, E.dense16_check(inp), dbl(inp)


def seam_index(w, a, b):
    """Rows / columns of tile b, and those that tile a's origin gives the same places of the tile (clamped as the kernels clamp)."""
    r0, r1, c0, c1 = E.tile_box(w, b)
    p0, _, q0, _ = E.tile_box(w, a)
    return slice(r0, r1), slice(c0, c1), (p0 + torch.arange(r1 - r0)).clamp_max(w["M"] - 1), (q0 + torch.arange(c1 - c0)).clamp_max(w["N"] - 1)


@pytest.mark.parametrize("spec", E.SEAM16_SPECS, ids=E.seam16_id)
def test_seam16_case_is_exact_and_sensitive(L, spec):
    bm, bn, per_cu, cap, case = spec
    M, N, K, lda, ldc = case
    w = E.assert_seam16(case, bm, bn, per_cu * cap)
    # the planner: every epilogue some family builds on this tile reaches it on this case under some forced variant
    launches = E.seam16_launches(L, spec)
    built = {e for e in E.dense16_epis(case) if any(L.lib.vda_gemm_built(fam, bm, bn, per_cu, 0, E.EPI[E.EPI_OF[e]]) for fam in (L.FAM_256, L.FAM_256S, L.FAM_8P))}
    assert {e for _, e, _, _ in launches} == built and built, sorted(built - {e for _, e, _, _ in launches})
    assert all(fam == L.FAM_8P for _, _, fam, dyn in launches if dyn)
    assert any(dyn for *_, dyn in launches) == bool(L.lib.vda_gemm_built(L.FAM_8P, bm, bn, per_cu, 0, 0))
    inp, ref, d = seam_dense(case)                       # (dense16_check: both exactness conditions for every exact epilogue)
    assert all(is_f16(v) for v in inp.values())
    Wf, c1, c2 = E.fold_ln(d)
    A, W, lin = d["A"], d["W"], ref["bias_f16"]
    pairs = E.seam_pairs(w)
    assert len(pairs) == w["nwg"] + w["rem"]
    nbn, seen_col = w["nbn"], False
    for a, b in pairs:
        rows, cols, prow, pcol = seam_index(w, a, b)
        what = f"tile {b} after tile {a}"
        assert a // nbn != b // nbn, "every seam changes the row panel"
        blk = lin[rows, cols]
        # rows: residual, (mean, rstd) and pos rows of the previous tile
        assert not torch.equal(d["res"][rows, cols], d["res"][prow][:, cols]) and not torch.equal(d["mean"][rows], d["mean"][prow]) and not torch.equal(d["rstd"][rows], d["rstd"][prow])
        differs(blk + d["res"][prow][:, cols], ref["res"][rows, cols], f"{what}: the previous tile's residual rows")
        differs(d["res"][prow][:, cols] + d["gamma"][cols] * blk, ref["scale_res_in_place_gamma"][rows, cols], f"{what}: the previous tile's residual rows (LayerScale)")
        ln = lambda mean, rstd, k1, k2: rstd[:, None] * (A[rows] @ Wf[cols].t() - mean[:, None] * k1) + k2      # noqa: E731
        assert torch.equal(ln(d["mean"][rows], d["rstd"][rows], c1[cols], c2[cols]), ref["ln_bias"][rows, cols])
        differs(ln(d["mean"][prow], d["rstd"][rows], c1[cols], c2[cols]), ref["ln_bias"][rows, cols], f"{what}: the previous tile's mean rows")
        differs(ln(d["mean"][rows], d["rstd"][prow], c1[cols], c2[cols]), ref["ln_bias"][rows, cols], f"{what}: the previous tile's rstd rows")
        if "split" in ref:
            stream = lambda res, res2: res + res2 + d["gamma"][cols] * blk      # noqa: E731
            differs(stream(d["res"][prow][:, cols], d["res2"][rows, cols]), ref["split"][rows, cols], f"{what}: the previous tile's hi plane rows")
            differs(stream(d["res"][rows, cols], d["res2"][prow][:, cols]), ref["split"][rows, cols], f"{what}: the previous tile's lo plane rows")
            differs(ref["split"][rows, cols] - d["mean"][prow][:, None], ref["split_pos"][rows, cols], f"{what}: the previous tile's pos rows")
        # K steps: the first one from the previous tile's A rows, the second one missing
        differs(blk + (A[prow, :64] - A[rows, :64]) @ W[cols, :64].t(), blk, f"{what}: K step 0 from the previous tile's A rows")
        differs(blk - A[rows, 64:128] @ W[cols, 64:128].t(), blk, f"{what}: K step 1 missing")
        # columns: bias (c1, c2 of the LayerNorm-folded epilogues) and W rows of the previous tile, where the workgroup changes column
        if a % nbn != b % nbn:
            seen_col = True
            assert not torch.equal(d["bias"][cols], d["bias"][pcol]) and not torch.equal(c2[cols], c2[pcol]) and not torch.equal(c1[cols], c1[pcol])
            differs(blk - d["bias"][cols] + d["bias"][pcol], blk, f"{what}: the previous tile's bias")
            differs(ln(d["mean"][rows], d["rstd"][rows], c1[pcol], c2[cols]), ref["ln_bias"][rows, cols], f"{what}: the previous tile's c1")
            differs(ln(d["mean"][rows], d["rstd"][rows], c1[cols], c2[pcol]), ref["ln_bias"][rows, cols], f"{what}: the previous tile's c2")
            differs(blk + A[rows, :64] @ (W[pcol, :64] - W[cols, :64]).t(), blk, f"{what}: K step 0 from the previous tile's W rows")
    assert seen_col == (nbn > 1 and w["nwg"] % nbn != 0), "a workgroup changes its column tile at a seam exactly where nbn does not divide the grid"


def test_seam16_specs_cover_what_is_stated(L):
    """Every large dense tile in all three walk modes with both K-step counts; lda > K and ldc > N once per tile at least; the tiles are
    the ones vda_gemm_built lists."""
    built = {(bm, bn, pc) for fam in (1, 2, 3) for bm in (192, 256) for bn in (128, 256, 384) for pc in (1, 2) if any(L.lib.vda_gemm_built(fam, bm, bn, pc, 0, e) for e in range(13))}
    assert built == set(E.SEAM16_TILES)
    for tile in E.SEAM16_TILES:
        mine = [s for s in E.SEAM16_SPECS if s[:3] == tile]
        walks = [E.tile_walk(s[4][0], s[4][1], s[0], s[1], s[2] * s[3]) for s in mine]
        assert {(w["nbn"], w["deal_last"]) for w in walks} == {(1, True), (3, False), (2, True)}
        assert {s[4][2] // 64 for s in mine} == {5, 9}
        assert any(s[4][3] > s[4][2] and s[4][4] > s[4][1] for s in mine)
        assert any(s[4][1] % 64 == 0 for s in mine) and (tile[1] == 384 or any(s[4][1] % 64 == 8 for s in mine))


def seam_walks(L, fields, variants, fold=False):
    """{(bm, bn, nwg): walk} over the variants' launches of one conv / patch / ConvTranspose / folded seam case (E.pick_cap)."""
    out = {}
    for v in variants:
        L.lib.vda_gemm_set_variant(v)
        got = E.pick_cap(L, fields, fold)
        if got is not None:
            cap, r, w = got
            assert w["ntiles"] > 2 * r.per_cu * cap
            out[(r.family, r.bm, r.bn, w["nwg"])] = w
    L.lib.vda_gemm_set_variant(-1)
    return out


@pytest.mark.parametrize("case", E.SEAM_CONV16_CASES[:-1], ids=E.conv16_id)
def test_seam_conv16_case_reaches_the_seams(L, case):
    """(Exactness and the tap / pad / K-step mistakes: test_conv16_case_is_exact_and_sensitive runs on these cases too.)"""
    B, H, W, Cin, Cout, stride, relu_in, ldc = case
    kw = E.conv16_kw(case)
    M, hw = kw["M"], kw["M"] // B
    walks = seam_walks(L, E.gemm16_fields(epi=E.EPI["BIAS_F16"], **kw), E.SEAM_CONV16_VARIANTS)
    assert {k[:3] for k in walks} >= {(L.FAM_256, 256, 256), (L.FAM_256, 256, 128), (L.FAM_256S, 256, 256), (L.FAM_256S, 256, 128), (L.FAM_8P, 256, 256), (L.FAM_8P, 256, 128)}
    inp = E.conv16_inputs(case)
    lin = E.conv16_refs(dbl(inp), stride, relu_in)["bias_f16"].reshape(M, Cout)
    bias = inp["bias"].double()
    for key, w in walks.items():
        later = {b for _, b in E.seam_pairs(w)}
        cross = [b for b in later for f in range(1, B) if E.tile_box(w, b)[0] < f * hw < E.tile_box(w, b)[1]]
        assert cross, f"{key}: no frame border inside a tile of round >= 1"
        for a, b in E.seam_pairs(w):
            rows, cols, prow, pcol = seam_index(w, a, b)
            differs(lin[prow][:, cols], lin[rows, cols], f"{key} tile {b}: rows decoded with the (b, y, x) origin of tile {a}")
            if a % w["nbn"] != b % w["nbn"]:
                differs(lin[rows, cols] - bias[cols] + bias[pcol], lin[rows, cols], f"{key} tile {b}: the bias of tile {a}")


def test_seam_c64_case(L):
    """27 tiles of 8 x 32 on the 8 workgroups of vda_set_max_wgs(8): conv3x3_c64_kernel gives XCD x the tiles [27 x / 8, 27 (x + 1) / 8) -
    three or four each, so both patch buffers and the residual prefetch are reused, by an odd and an even count."""
    B, H, W, Cin, Cout, stride, relu_in, ldc = E.SEAM_C64_CASE
    assert (Cin, stride) == (64, 1) and 32 < Cout <= 64
    ntiles = B * -(-H // 8) * -(-W // 32)
    shares = [ntiles * (x + 1) // 8 - ntiles * x // 8 for x in range(8)]
    assert ntiles == 27 and sorted(set(shares)) == [3, 4]
    L.lib.vda_gemm_set_variant(-1)
    rc, recs = E.plan16(L, E.gemm16_fields(epi=E.EPI["RES_F16"], **E.conv16_kw(E.SEAM_C64_CASE)), ncu=8)
    assert rc == 0 and L.launch_name(recs[0]) == "conv3x3_lds_kernel<2>"


@pytest.mark.parametrize("case", E.SEAM_PATCH16_CASES, ids=lambda c: "fr%d-P%d-N%d-K%d-ldc%d" % c)
def test_seam_patch16_case_reaches_the_seams(L, case):
    fr, P, N, K, ldc = case
    walks = seam_walks(L, E.gemm16_fields(epi=E.EPI["PATCH_F32"], **E.patch16_kw(case)), E.SEAM_CONV16_VARIANTS)
    assert {k[0] for k in walks} == {L.FAM_256, L.FAM_256S, L.FAM_8P} and {k[1] for k in walks} == {256}
    d = dbl(E.patch16_inputs(case))
    ref = E.patch16_ref(d, P).reshape(fr * P, N)
    lin = d["A"] @ d["W"].t() + d["bias"]
    for key, w in walks.items():
        for rnd in (1, 2):
            tiles = [m[rnd] for m in w["tiles"] if len(m) > rnd]
            assert any(E.tile_box(w, t)[0] % P != 0 and E.tile_box(w, t)[0] // P != (E.tile_box(w, t)[1] - 1) // P for t in tiles), f"{key}: no frame boundary inside a tile of round {rnd}"
        for a, b in E.seam_pairs(w):
            rows, cols, prow, pcol = seam_index(w, a, b)
            m = torch.arange(rows.start, rows.stop)
            assert torch.equal(lin[rows, cols] + d["pos"][1 + m % P][:, cols], ref[rows, cols])
            differs(lin[rows, cols] + d["pos"][1 + prow % P][:, cols], ref[rows, cols], f"{key} tile {b}: the pos rows of tile {a}")


@pytest.mark.parametrize("case,k", E.SEAM_CONVT16, ids=lambda c: "B%d-%dx%d-C%d-Cp%d" % c if isinstance(c, tuple) else "k%d" % c)
def test_seam_convt16_case_reaches_the_seams(L, case, k):
    B, h, w_, C, Cp = case
    walks = seam_walks(L, E.gemm16_fields(epi=E.EPI["CONVT_F16"], **E.convt16_kw(case, k)), E.SEAM_CONV16_VARIANTS)
    assert {key[0] for key in walks} == {L.FAM_256, L.FAM_256S, L.FAM_8P}
    d = dbl(E.convt16_inputs(case, k))
    ref = E.convt_ref(d["x"], d["w"], d["bias"], k)                              # [B, h k, w k, C]
    G = ref.reshape(B, h, k, w_, k, C).permute(0, 1, 3, 2, 4, 5).reshape(B * h * w_, k * k, C)     # one row per input pixel: what a GEMM row scatters
    for key, w in walks.items():
        moves = [(a, b) for a, b in E.seam_pairs(w) if a // w["nbn"] != b // w["nbn"]]       # (16 column tiles on 8 workgroups: every other seam stays in its row panel)
        assert len(moves) >= w["nwg"]
        assert any(E.tile_box(w, b)[0] < f * h * w_ < E.tile_box(w, b)[1] for _, b in moves for f in range(1, B)), f"{key}: no frame border inside a tile of round >= 1"
        for a, b in moves:
            r0, r1, _, _ = E.tile_box(w, b)
            p0 = E.tile_box(w, a)[0]
            prow = (p0 + torch.arange(r1 - r0)).clamp_max(B * h * w_ - 1)
            differs(G[prow], G[r0:r1], f"{key} tile {b}: scattered with the row map of tile {a}")


@pytest.mark.parametrize("case", E.SEAM_FOLD_CASES, ids=lambda c: "k%d-Cin%d-Fe%d-B%d-%dx%d" % c)
def test_seam_fold_case_reaches_the_seams(L, case):
    k, Cin, Fe, B, H, W = case
    f = E.fold_fields(case)
    walks = seam_walks(L, f, (-1, 5), fold=True)
    assert {key[:3] for key in walks} == {(L.FAM_8P, 256, 256)} and all(w["full_rounds"] >= 2 and w["nwg"] == 8 for w in walks.values())
    w = next(iter(walks.values()))
    plain = E.tile_walk(f["M"], f["N"], 256, 256, 8)
    t, Wc, Bc, ref = E.seam_fold_data(case)
    G = E.fold_as_gemm(ref, k)
    moved = [(p, q) for mp, mq in zip(plain["tiles"], w["tiles"]) for p, q in list(zip(mp, mq))[1:] if p != q]
    assert bool(moved) == (w["nbn"] > 1), "a rotated round moves tiles exactly where there is more than one column tile"
    for p, q in moved:
        (r0, r1, c0, c1), (_, _, u0, u1) = E.tile_box(w, q), E.tile_box(w, p)
        differs(G[r0:r1, u0:u1], G[r0:r1, c0:c1], f"tile {q}: the column tile of the unrotated round ({p})")


# ================================================================================================ the fp16 attention kernels' cases
# tests/test_attention_edges_gpu.py: the selector and counting inputs meet their preconditions on every case, their fp64 reference IS
# the closed form, and a tiled restatement of attention with one mistake built in fails the GPU test's own assertion.

ATTN_ALL_CASES = E.ATTN_CASES + [E.ATTN_BIG_CASE]


@functools.lru_cache(maxsize=None)
def selector_case(case):
    B, N, H = case
    qkv, pi = E.attn_selector_inputs(B, N, H, E.attn_seed(case))
    return qkv, pi, E.selector_expected(qkv, pi, B, N, H)


def test_attention_case_list_is_the_one_stated():
    assert [c[1] for c in E.ATTN_CASES[:15]] == [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 321, 449]
    assert all(c[0] == 1 and c[2] == 1 for c in E.ATTN_CASES[:15])
    assert E.ATTN_CASES[15:] == [(3, 129, 1), (1, 129, 3), (2, 65, 4), (3, 193, 3)] and E.ATTN_BIG_CASE == (1, 1370, 2)
    assert [-(-n // 128) * b * h for b, n, h in E.ATTN_CASES[15:]] == [6, 6, 8, 18], "workgroups: remainder arm twice, quotient arm, both"
    assert sorted(E.ATTN_VARIANTS) == [-1, 0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11] and E.ATTN_STRADDLE_N == [129, 160, 192, 449]


@pytest.mark.parametrize("case", ATTN_ALL_CASES, ids=E.attn_case_id)
def test_attention_selector_case_is_exact(case):
    B, N, H = case
    qkv, pi, expect = selector_case(case)
    assert qkv.shape == (B, N, 3 * H * 64) and pi.shape == (B, H, N)
    assert all(sorted(pi[b][h].tolist()) == list(range(N)) for b in range(B) for h in range(H)), "pi is a permutation per (frame, head)"
    assert B * H == 1 or N == 1 or len({tuple(pi[b][h].tolist()) for b in range(B) for h in range(H)}) == B * H, "drawn separately"
    E.assert_selector_safe(qkv, pi, B, N, H)
    for log2_q in (False, True):
        ref = E.attn_ref64(qkv, B, N, H, log2_q)
        assert float((ref - expect).abs().max()) <= 2.0 ** -26
        assert E.selector_mismatch(ref.to(F16), expect) is None, "the fp64 reference, rounded to fp16, is V[pi]"
    assert E.selector_mismatch(E.tiled_attention(qkv, B, N, H).to(F16), expect) is None, "the tiled restatement is attention"
    k = qkv.reshape(B, N, 3, H, 64)[0, :, 1, 0]
    agree = (k @ k.t() / 144).fill_diagonal_(0)
    assert float(agree.max()) <= 2, "two keys agree in at most two digits"
    tiles = {int(j) // 64 for j in pi[0][0].tolist()}
    assert tiles == set(range(-(-N // 64))), "winners fall in every tile, the last partial one included"
    v = qkv.reshape(B, N, 3, H, 64)[:, :, 2]
    rows = v.permute(0, 2, 1, 3).reshape(B * H, N, 64)          # (31 is a unit mod the prime 2039 > N: no two keys of a head share a row)
    assert all(len({tuple(r.tolist()) for r in rows[g]}) == N for g in range(B * H)), "every key of a (frame, head) has a V row of its own"
    assert all(not bool((rows[g] == rows[g2]).all(-1).any()) for g in range(B * H) for g2 in range(g)), "the same key differs between heads and frames"


@pytest.mark.parametrize("case", ATTN_ALL_CASES, ids=E.attn_case_id)
def test_attention_counting_case_is_exact(case):
    B, N, H = case
    qkv = E.attn_counting_inputs(B, N, H, E.attn_seed(case))
    assert is_f16(qkv)
    q, k, v = qkv.reshape(B, N, 3, H, 64).unbind(2)
    assert not bool(q.any()) and (N < 4 or bool(k.any())) and float(v.sum(1).max()) < E.EXACT_LIMIT
    expect = E.counting_expected(B, N, H)
    ref = E.attn_ref64(qkv, B, N, H)
    assert float((ref - expect).abs().max()) <= 1e-15, "the fp64 reference is the counts over N"
    for y in (ref.to(F16), E.tiled_attention(qkv, B, N, H).to(F16), expect.float().to(F16)):
        ok, worst = E.counting_check(y, B, N, H)
        assert ok and worst <= 1
    if B * H > 1:
        rows = expect.reshape(B, N, H, 64)[:, 0].reshape(B * H, 64)
        assert all(not torch.equal(rows[g], rows[g + 1]) for g in range(B * H - 1)), "neighbouring heads / frames differ in scale"


# which family's own assertion must fail for which mistake. The selector is blind to a key counted twice (softmax normalises the
# winner's doubled weight away) and the counting inputs to anything that permutes keys 64 apart or queries (every row is the same;
# heads and frames differ by their scale 1 + (b H + h) % 3 only, which is not relied on);
# between them every mistake is seen wherever it can occur.
SEEN_BY_SELECTOR = {"drop_last", "mask_moved", "stale_v", "heads", "frames", "queries"}
SEEN_BY_COUNTING = {"drop_last", "dup_last", "mask_moved"}


@pytest.mark.parametrize("mutation", E.ATTN_MUTATIONS)
@pytest.mark.parametrize("case", ATTN_ALL_CASES, ids=E.attn_case_id)
def test_attention_equalities_can_fail(case, mutation):
    B, N, H = case
    if not E.attn_mutation_applies(mutation, B, N, H):
        for fam in ("selector", "counting"):                     # the mistake cannot occur at this shape: the restatement is unchanged
            qkv = selector_case(case)[0] if fam == "selector" else E.attn_counting_inputs(B, N, H, E.attn_seed(case))
            assert torch.equal(E.tiled_attention(qkv, B, N, H, mutation), E.tiled_attention(qkv, B, N, H))
        return
    seen = set()
    qkv, pi, expect = selector_case(case)
    if E.selector_mismatch(E.tiled_attention(qkv, B, N, H, mutation).to(F16), expect) is not None:
        seen.add("selector")
    ok, _ = E.counting_check(E.tiled_attention(E.attn_counting_inputs(B, N, H, E.attn_seed(case)), B, N, H, mutation).to(F16), B, N, H)
    if not ok:
        seen.add("counting")
    want = ({"selector"} if mutation in SEEN_BY_SELECTOR else set()) | ({"counting"} if mutation in SEEN_BY_COUNTING else set())
    assert want and want <= seen, f"{mutation} goes unnoticed by {sorted(want - seen)} on these inputs"


def test_selector_mismatch_names_the_key():
    case = (1, 65, 1)
    qkv, pi, expect = selector_case(case)
    y = E.tiled_attention(qkv, 1, 65, 1, "stale_v").to(F16)
    msg = E.selector_mismatch(y, expect, qkv.reshape(1, 65, 3, 1, 64)[:, :, 2])
    i = pi[0][0].tolist().index(64)
    assert msg is not None and msg.startswith("1/65 ") and f"query {i} head 0" in msg and "(0, 0)" in msg, msg


@pytest.mark.parametrize("N", E.ATTN_STRADDLE_N)
def test_attention_straddle_margins(N):
    """Both row sums at least 8 % from SUM_LIMIT under either q scaling; the fp16 rounding of q * log2(e) / 8 moves the fp64 result by
    less than a third of the GPU test's bound."""
    qkv = E.attn_straddle_inputs(N, 9900 + N)
    assert is_f16(qkv) and float(qkv[..., 128:].min()) >= 1
    for log2_q in (False, True):
        even, odd = E.straddle_tile_sums(qkv, log2_q)
        assert even <= E.ATTN_SUM_LIMIT * 0.92 and odd >= E.ATTN_SUM_LIMIT * 1.08, (even, odd)
        assert abs(even - 64 * 2.718281828459045 ** 3.25) < 5 and abs(odd - 64 * 2.718281828459045 ** 3.65625) < 8
    ref, ref2 = E.attn_ref64(qkv, 1, N, 1), E.attn_ref64(qkv, 1, N, 1, log2_q=True)
    err = (ref2 - ref).abs() / (1 + ref.abs())
    assert float(err.max()) <= E.ATTN_TOL / 3, float(err.max())
    assert float((E.tiled_attention(qkv, 1, N, 1) - ref).abs().max()) < 1e-9


@pytest.mark.parametrize("C,heads", E.TATTN_SELECTOR_GEOM)
def test_temporal_selector_cases_are_exact(C, heads):
    for T in E.TATTN_T:
        for hw in E.TATTN_HW:
            qkv, pi = E.tattn_selector_inputs(T, hw, C, heads, E.tattn_seed(T, hw, C, heads))
            assert qkv.shape == (T * hw, 3 * C) and pi.shape == (hw, heads, T)
            E.assert_tattn_selector_safe(qkv, pi, T, hw, C, heads)
            expect = E.tattn_selector_expected(qkv, pi, T, hw, C, heads)
            ref = E.tattn_ref64(qkv, T, hw, C, heads)
            assert torch.equal(ref.to(F16).double(), expect), "the fp64 reference, rounded to fp16, is V[pi]"
            if T > 1:
                differs(expect.reshape(T, hw * C).flip(0), expect.reshape(T, hw * C), "frames in the wrong order")
            if hw > 1:
                differs(expect.reshape(T, hw, C).flip(1), expect.reshape(T, hw, C), "pixels in the wrong order")
            if heads > 1:
                differs(expect.reshape(T * hw, heads, C // heads).flip(1), expect.reshape(T * hw, heads, C // heads), "heads in the wrong order")


def test_temporal_selector_needs_nonzero_values():
    """With a zero in V the d = 128 case's real result next to it is a nonzero fp16 subnormal: the precondition refuses it."""
    T, hw, C, heads = 32, 1, 1024, 8
    qkv, pi = E.tattn_selector_inputs(T, hw, C, heads, 1)
    bad = qkv.clone()
    bad[int(pi[0][0][0]), 2 * C] = 0.0                          # V of query 0's winner, head 0, channel 0
    with pytest.raises(AssertionError, match="nonzero"):
        E.assert_tattn_selector_safe(bad, pi, T, hw, C, heads)
    assert float(E.tattn_ref64(bad, T, hw, C, heads)[0, 0].to(F16)) != 0.0


def test_attention_helpers_refuse_what_they_should():
    B, N, H = 1, 65, 1
    qkv, pi = E.attn_selector_inputs(B, N, H, 3)
    weak = qkv.clone().reshape(B, N, 3, H, 64)
    weak[:, :, 0] *= 0.5                                         # a lead of 18 natural units: weights of e^-18 are not nothing
    with pytest.raises(AssertionError, match="2\\*\\*-40"):
        E.assert_selector_safe(weak.reshape(B, N, 192), pi, B, N, H)
    big = qkv.clone()
    big[0, 0, 128] = 1020.0
    with pytest.raises(AssertionError, match="1019"):
        E.assert_selector_safe(big, pi, B, N, H)
    wrong = pi.clone()
    wrong[0, 0, :2] = pi[0, 0, :2].flip(0)
    with pytest.raises(AssertionError, match="winner"):
        E.assert_selector_safe(qkv, wrong, B, N, H)
    assert E.counting_check(E.counting_expected(1, 64, 1).to(F16), 1, 64, 1) == (True, 0.0)
    off = E.counting_expected(1, 65, 1).to(F16)
    nudged = (off.view(torch.int16) + 2).view(F16)              # two fp16 steps: refused; one: allowed
    assert not E.counting_check(nudged, 1, 65, 1)[0] and E.counting_check((off.view(torch.int16) + 1).view(F16), 1, 65, 1)[0]


# ================================================================================================ the fused upsample convolutions' cases
# tests/test_upsample_edges_gpu.py: every case reaches the branch it is listed for (window extents, tile counts, store path, tap x
# k-step x chunk coverage, the tail's kernel), every reference equals an fp32 / fp16 emulation of the kernel's own operation order (or
# bounds it, for the selector family), and a restatement with one mistake built in (E.FUSED_MUTATIONS) fails the GPU test's assertion.

def test_up2_cases_reach_their_branches():
    g = [E.up2_geometry(c) for c in E.UP2_CASES]
    assert len(E.UP2_CASES) == 10 and all(c[3] % 16 == 0 and c[4] % 4 == 0 and c[5] % 4 == 0 and c[5] >= c[4] for c in E.UP2_CASES)
    assert E.ac_coords(1, 2)[3] == 0.0 and (g[0]["nk"], g[0]["wide"], g[0]["idle"], g[0]["ntiles"]) == (1, False, 7, 1)
    assert (g[1]["ntiles"], 2 * E.UP2_CASES[1][1], 2 * E.UP2_CASES[1][2]) == (1, E.UP2_TH, E.UP2_TW)
    assert (g[2]["ntiles"], g[2]["idle"], g[2]["wide"], g[2]["partial_block"], g[2]["nk"]) == (8, 0, True, True, 2) and 18 % E.UP2_TH == 2 and 34 % E.UP2_TW == 2
    assert (g[3]["ntiles"], g[3]["grid"], g[3]["per_xcd"], g[3]["CB"], g[3]["partial_block"], g[3]["wide"], g[3]["nk"]) == (12, 16, 2, 2, True, False, 3)
    assert (g[4]["CB"], g[4]["wide"], g[4]["rows"], g[4]["cols"]) == (4, True, 10, 18)
    assert (g[5]["CB"], g[5]["wide"], g[5]["partial_block"], g[5]["rows"], g[5]["cols"]) == (4, False, True, 10, 18)
    assert (g[6]["rows"], g[7]["cols"]) == (1, 1) and E.UP2_CASES[6][1] == 1 and E.UP2_CASES[7][2] == 1
    assert E.UP2_CASES[8][1] == 148 and E.UP2_CASES[9][2] == 148 and int(E.ac_coords(148, 296)[1].max()) == 147
    assert all(x["rows"] <= E.UP2_SH and x["cols"] <= E.UP2_SW for x in g)
    assert [c for c in E.UP2_CASES if 9 * c[3] % 64 == 0] == [E.UP2_CASES[4]], "the cases the conv GEMM can take"
    assert all(not E.up2_geometry(c)["wide"] or c is E.UP2_CASES[2] for c in E.UP2_OFFSET_CASES)
    # 17 and 33 are the smallest sizes whose windows reach 10 rows / 18 columns, and no size up to 299 needs the 11th row / 19th column
    rows = {n: E.src_window_extent(n, 2 * n, E.UP2_TH) for n in range(1, 300)}
    cols = {n: E.src_window_extent(n, 2 * n, E.UP2_TW) for n in range(1, 300)}
    assert min(n for n, e in rows.items() if e == 10) == 17 and max(rows.values()) == 10 < E.UP2_SH
    assert min(n for n, e in cols.items() if e == 18) == 33 and max(cols.values()) == 18 < E.UP2_SW


@pytest.mark.parametrize("case", E.UP2_CASES, ids=E.up2_id)
def test_up2_selector_sets_cover_every_tap_kstep_and_chunk(case):
    C, N = case[3], case[4]
    assert E.up2_selector_coverage(case) == {(t, k, c) for t in range(9) for k in range(C // 16) for c in range(2)}
    for w, picks in E.up2_selector_sets(case):
        assert bool((w.sum((1, 2, 3)) == 1).all()) and bool(((w == 0) | (w == 1)).all()) and len(picks) == N
        assert all(picks[n] != picks[n + 32] for n in range(N - 32)), "a cout block shifted by 32 selects something else"
    x = E.up2_selector_x(case)
    assert float(x.abs().max()) <= 64 and bool((x == x.round()).all()) and torch.equal(x.to(torch.float16).float(), x)


def fused_seen(mut, ref, bound=None):
    """Does the mistaken result fail the GPU test's assertion: inequality (bound None) or an error above the bound after the fp16 store."""
    if bound is None:
        return not torch.equal(mut, ref)
    return bool(((mut.to(torch.float16).double() - ref).abs() > bound).any())


@pytest.mark.parametrize("case", E.UP2_CASES + [(1, 3, 3, 256, 128, 128)], ids=E.up2_id)
def test_up2_constant_case_is_exact_and_sensitive(case):
    """(The last case is no GPU case: the value ranges hold the preconditions at C = 256, the model's width, too.)"""
    B, h, w, C, N, ldc = case
    H, W = 2 * h, 2 * w
    inp = E.up2_const_inputs(case)
    ref = E.up2_const_ref(case, inp)
    d = dbl(inp)
    for contracted in (False, True):
        assert torch.equal(E.fused_emulate(inp["x"], d["w"], H, W, "sum4_f32", contracted=contracted) + d["bias"], ref), "the kernel's operation order gives the reference"
    assert torch.equal(E.fused_emulate(inp["x"], d["w"], H, W, "sum4_f32", "row_off") + d["bias"], ref), "(a constant image cannot see a wrong source row: the selector family does)"
    for m in E.FUSED_MUTATIONS[1:]:
        if E.fused_mutation_applies(m, B, h, H, W, C, N, (E.UP2_TH, E.UP2_TW), E.UP2_KC):
            assert fused_seen(E.fused_emulate(inp["x"], d["w"], H, W, "sum4_f32", m) + d["bias"], ref), f"{m} goes unnoticed on these inputs"
    differs(E.fused_emulate(inp["x"], d["w"], H, W, "sum4_f32") + d["bias"].roll(1), ref, "bias on the wrong cout")


SELECTOR_GEOM = [(17, 33), (148, 5), (5, 148), (148, 148), (1, 7)]


def selector_ratio(x, H, W):
    """Worst error / bound of two fp32 evaluation orders (conv_up.hip's four-weight sum on plain and on contracted coordinates,
    torch's own F.interpolate) against the fp64 definition on plain and on contracted coordinates."""
    h, w = x.shape[2:]
    amax = float(x.abs().max())
    ys = [E.interp_image(x, H, W, "sum4_f32"), E.interp_image(x, H, W, "sum4_f32", contracted=True),
          F.interpolate(x, size=(H, W), mode="bilinear", align_corners=True).to(torch.float16).double()]
    worst = 0.0
    for contracted in (False, True):
        r = E.interp_image(x, H, W, "f64", contracted)
        bound = E.up2_selector_bound(r, h, w, amax)
        worst = max([worst] + [float(((y - r).abs() / bound).max()) for y in ys])
    return worst


@pytest.mark.parametrize("h,w", SELECTOR_GEOM)
def test_selector_bound_holds_at_the_stated_geometries(h, w):
    worst = selector_ratio(E.up2_selector_x((1, h, w, 16, 4, 4)), 2 * h, 2 * w)
    assert worst <= 1.0, worst


@pytest.mark.parametrize("case", E.UP2_CASES, ids=E.up2_id)
def test_up2_selector_case_is_bounded_and_sensitive(case):
    B, h, w, C, N, ldc = case
    H, W = 2 * h, 2 * w
    x = E.up2_selector_x(case)
    assert selector_ratio(x, H, W) <= 1.0
    amax = float(x.abs().max())
    seen = set()
    for wsel, picks in E.up2_selector_sets(case):
        wd = wsel.double()
        ref = E.fused_emulate(x, wd, H, W, "f64")
        bound = E.up2_selector_bound(ref, h, w, amax)
        assert float(bound.max()) < 0.05, "the bound is a few hundredths"
        # the reference is a gather of the interpolated image: cout n holds the image at (tap, channel), zero outside
        img = F.pad(E.interp_image(x, H, W, "f64"), (1, 1, 1, 1))
        for n in (0, N - 1):
            tap, ch = picks[n]
            assert torch.equal(ref[..., n], img[:, ch, tap // 3:tap // 3 + H, tap % 3:tap % 3 + W])
        for contracted in (False, True):
            assert not fused_seen(E.fused_emulate(x, wd, H, W, "sum4_f32", contracted=contracted), ref, bound), "the kernel's operation order stays inside the bound"
        for m in E.FUSED_MUTATIONS:
            if E.fused_mutation_applies(m, B, h, H, W, C, N, (E.UP2_TH, E.UP2_TW), E.UP2_KC) and fused_seen(E.fused_emulate(x, wd, H, W, "sum4_f32", m), ref, bound):
                seen.add(m)
    for m in E.FUSED_MUTATIONS:
        if E.fused_mutation_applies(m, B, h, H, W, C, N, (E.UP2_TH, E.UP2_TW), E.UP2_KC):
            assert m in seen, f"{m} stays inside the bound on these inputs"


def test_every_fused_mutation_fails_in_a_listed_case():
    """The per-case tests above assert that every mutation that APPLIES to a case fails there (selector family: all seven; constant
    family: all but the wrong source row); here: each applies to several listed cases."""
    for m in E.FUSED_MUTATIONS:
        hit = [c for c in E.UP2_CASES if E.fused_mutation_applies(m, c[0], c[1], 2 * c[1], 2 * c[2], c[3], c[4], (E.UP2_TH, E.UP2_TW), E.UP2_KC)]
        assert len(hit) >= 2, m


# ------------------------------------------------------------------------------------------------ the resizing depth tail, dyadic scales
TAILUP_ALL = E.TAILUP_CASES + [E.tailup_many_tiles_case(256)]


def test_tailup_cases_run_the_kernel_they_are_listed_for():
    names = [E.tailup_kernel(c) for c in E.TAILUP_CASES]
    assert names == [E.TAIL_KERNELS[2]] * 5 + [E.TAIL_KERNELS[1]] * 2 + [E.TAIL_KERNELS[2]]
    assert all(E.tailup_kernel(c, 1) == E.TAIL_KERNELS[1] for c in TAILUP_ALL) and E.tailup_kernel((1, 5, 7, 5, 7)) == E.TAIL_KERNELS[0]
    assert E.tail_src_extent(17, 17, 16) * E.tail_src_extent(17, 33, 32) > E.TAIL_SRC_ROWS
    assert E.tail_src_extent(33, 17, 16) * E.tail_src_extent(65, 33, 32) > E.TAIL_SRC_ROWS
    B, h, w, H, W = E.TAILUP_CASES[1]
    assert (-(-H // 16), -(-W // 32), H % 16, W % 32) == (2, 2, 1, 1)
    for ncu in (8, 64, 256, 304):
        c = E.tailup_many_tiles_case(ncu)
        assert c[0] * -(-c[3] // 16) * -(-c[4] // 32) > ncu and E.tailup_kernel(c) == E.TAIL_KERNELS[2]
    scales = {(E.ac_coords(c[1], c[3])[3], E.ac_coords(c[2], c[4])[3]) for c in E.TAILUP_CASES}
    assert scales == {(0.0, 0.0), (0.5, 0.5), (0.25, 0.25), (0.5, 0.25), (1.0, 0.25), (1.0, 0.5), (2.0, 2.0), (1.5, 0.5)}


@pytest.mark.parametrize("case,Cc", [(c, Cc) for c in E.TAILUP_CASES for Cc in E.TAILUP_C] + [(TAILUP_ALL[-1], 32), (E.SEAM_TAILUP_CASE, 32)],
                         ids=lambda v: E.tailup_id(v) if isinstance(v, tuple) else str(v))
def test_tailup_case_is_exact_and_sensitive(case, Cc):
    B, h, w, H, W = case
    inp = E.tailup_inputs(case, Cc)
    b3 = inp.pop("b3")
    assert all(is_f16(inp[k]) for k in ("x", "w2"))
    ref = E.tailup_ref(case, inp, b3)
    assert bool((ref > 0).any()), "something survives the last ReLU"
    d = dbl(inp)
    tile = (16, 32) if E.tailup_kernel(case) == E.TAIL_KERNELS[2] else (8, 32)
    emu = lambda m=None: E.tail_epilogue(E.fused_emulate(inp["x"], d["w2"], H, W, "pk_f16", m, tile, 32), d, b3)      # noqa: E731
    assert torch.equal(emu(), ref), "bilinear8's packed-fp16 chain gives the reference"
    assert torch.equal(E.tail_epilogue(E.fused_emulate(inp["x"], d["w2"], H, W, "pk_f16", None, tile, 32).float(), {k: v.float() for k, v in d.items()}, b3).double(), ref)
    for m in E.FUSED_MUTATIONS:
        if m != "cout_shift" and E.fused_mutation_applies(m, B, h, H, W, Cc, 32, tile, 32):
            differs(emu(m), ref, m)


def test_upsample_helpers_refuse_what_they_should():
    with pytest.raises(AssertionError, match="scale"):
        E.assert_dyadic(9, 17, 16, 33)
    E.assert_dyadic(7, 5, 5, 9)
    case = E.UP2_CASES[1]
    inp = E.up2_const_inputs(case)
    with pytest.raises(AssertionError):
        E.up2_const_ref(case, dict(inp, x=inp["x"] * 400))                       # outputs past 2048
    bad = inp["x"].clone()
    bad[0, 0, 0, 0] += 1
    with pytest.raises(AssertionError):
        E.up2_const_ref(case, dict(inp, x=bad))                                  # not a constant image
    from video_depth_anything_amd import _lib
    assert _lib.lib.vda_depth_tail_last_kernel() in (b"",) + tuple(k.encode() for k in E.TAIL_KERNELS)


# ------------------------------------------------------------------------------------------------ vda_bilinear_nhwc at dyadic scales
@pytest.mark.parametrize("Cc", E.BILINEAR_DYADIC_C)
@pytest.mark.parametrize("case", E.TAILUP_CASES, ids=E.tailup_id)
def test_bilinear_dyadic_case_is_exact_and_sensitive(case, Cc):
    B, h, w, H, W = case
    inp = E.bilinear_dyadic_inputs(case, Cc)
    up, both = E.bilinear_dyadic_refs(case, inp)
    lerp = E.interp_image(inp["x"], H, W, "lerp_f32").permute(0, 2, 3, 1)
    assert torch.equal(lerp, up), "the kernel's nested fp32 lerp gives the reference"
    add = inp["add"].permute(0, 2, 3, 1)
    assert torch.equal((lerp.float() + add).to(torch.float16).double(), both) and torch.equal((lerp.float() + add).double(), both)
    differs(both, up, "forgetting the addend")
    if h > 1:
        differs(E.interp_image(inp["x"], H, W, "lerp_f32", row_off=H // 2).permute(0, 2, 3, 1), up, "a source row off by one")
