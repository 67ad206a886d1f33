"""relu_in of the fp16 3x3 convolution as a compile-time property: both values on both conv kernels.

The 8-phase 256 x 256 kernel (vda_gemm_set_variant(5)) and the 128-row kernel (variant 0) each have two conv instantiations: one
applies max(x, threshold) to every A fragment (the threshold is 0 with relu_in, -65504 without), the other - what a launch without
relu_in runs - has no max in its K loop. Which of the two a launch ran is not visible from outside (vda_gemm_last_kernel reports the
family's kernel for both); what is visible is the result, so every case runs relu_in = 0 and 1 and three things are asserted:

  * exact-integer operands (tests/_exact.py's conditions, asserted here): the output EQUALS the numpy definition, conv(relu(x)) or
    conv(x), element for element;
  * random fp16 operands with negative values and -65504 among them (the one finite value at which an identity max could differ from
    no max): within the error bound below of the fp64 numpy definition;
  * on |x| - where relu changes nothing - the launch without relu_in (the instantiation without the max) gives the BITS of the
    launch with it (the instantiation every conv ran before, whose max is then an identity on every element): same K order, same
    accumulators, same epilogue.

Error bound of the random cases, per element, with T = sum |x| |w| + |bias| over the element's 9 * Cin terms: the kernels accumulate
exact fp16 products in fp32 in some order, K + 1 roundings of at most 2**-24 relative to a partial sum that never exceeds T, so
|acc - ref| <= (K + 1) * 2**-24 * T; the store rounds to fp16: 2**-11 relative to |acc| <= |ref| + that, and 2**-25 absolute in
the subnormal range. Nothing in it is measured."""
import functools

import numpy as np
import pytest
import torch

import _exact as E
from _exact import check_sentinel, guarded, sentinel_out_f16
from test_kernels_gpu import ops  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
KERNELS = {5: "gemm8p_kernel<256, 1, %d, 1, 256, false>", 0: "gemm_kernel<128, %d, 1>"}      # forced variant -> the kernel it names
# (B, H, W, Cin, Cout): one pixel (eight taps are padding); a few rows; 323 rows = one 256-row tile + 67, two 128-row tiles + 67
CASES = [(1, 1, 1, 64, 64), (1, 3, 5, 64, 256), (1, 17, 19, 64, 64), (1, 17, 19, 64, 256)]
case_id = lambda c: "B%d-%dx%d-Cin%d-Cout%d" % c      # noqa: E731


@pytest.fixture(scope="module")
def L(ops):
    from video_depth_anything_amd import _lib
    yield _lib
    _lib.lib.vda_gemm_set_variant(-1)


def conv_np(x, w, bias, relu_in):
    """The definition, in fp64: x [B, H, W, Cin], w [Cout, Cin, 3, 3], bias [Cout] -> [B * H * W, Cout]; stride 1, zero padding 1."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    if relu_in:
        x = np.maximum(x, 0.0)
    B, H, W, _ = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    out = np.zeros((B, H, W, w.shape[0]))
    for ky in range(3):
        for kx in range(3):
            out += np.einsum("bhwc,oc->bhwo", xp[:, ky:ky + H, kx:kx + W], w[:, :, ky, kx])
    return (out + np.asarray(bias, np.float64)).reshape(B * H * W, -1)


@functools.lru_cache(maxsize=None)
def data(case, kind):
    """Host operands of one case, shared by the kernels and relu_in values: x NHWC fp16, w [Cout, Cin, 3, 3] fp16 values, bias fp32."""
    B, H, W, Cin, Cout = case
    seed = 9100 + 7 * CASES.index(case)
    if kind == "ints":
        x = E.ints((B, H, W, Cin), -3, 3, seed)                     # negative values make relu_in matter
        w, bias = E.ints((Cout, Cin, 3, 3), -2, 2, seed + 1), E.ints((Cout,), -4, 4, seed + 2)
        bound = torch.from_numpy(conv_np(x.abs(), w.abs(), bias.abs(), False))
        refs = [torch.from_numpy(conv_np(x, w, bias, r)) for r in (False, True)]
        E.assert_exact_safe_f16([bound], refs)
    else:
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(B, H, W, Cin, generator=g).to(F16).float()
        hit = torch.rand(B, H, W, Cin, generator=g) < 1.0 / 64          # about one element of every pixel's 64 channels
        x[hit] = -65504.0
        x[0, 0, 0, 0] = -65504.0                                        # (the one-pixel case has it for certain)
        w = (torch.randn(Cout, Cin, 3, 3, generator=g) * (9 * Cin) ** -0.5 / 16).to(F16).float()     # |w| ~ 2.6e-3: sums of -65504 w stay finite in fp16
        bias = torch.randn(Cout, generator=g)
    return x, w, bias


def run(ops, L, case, x, w, bias, relu_in, variant):
    B, H, W, Cin, Cout = case
    M = B * H * W
    from video_depth_anything_amd import ops as o
    out = sentinel_out_f16(M, Cout, Cout)
    L.lib.vda_gemm_set_variant(variant)
    ops.gemm(guarded(x.to(F16), pad_elems=(W + 2) * Cin), guarded(o.pack_conv3x3(w)), out, L.EPI_BIAS_F16, M=M, N=Cout, K=9 * Cin, bias=guarded(bias),
             relu_in=relu_in, conv=(B, H, W, Cin, H, W, 1))
    got = L.lib.vda_gemm_last_kernel().decode()
    want = KERNELS[variant] % (L.EPI_BIAS_F16 if variant == 5 else (64 if Cout <= 64 else 128))
    assert got == want, f"variant {variant} ran {got}"
    check_sentinel(out, M, Cout, f"conv {case_id(case)} relu_in={relu_in} variant {variant}")
    return out[:M].cpu()


@pytest.mark.parametrize("variant", [5, 0], ids=["8phase", "128row"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_conv_relu_in_exact_integers(ops, L, case, variant):
    x, w, bias = data(case, "ints")
    for relu_in in (False, True):
        y = run(ops, L, case, x, w, bias, relu_in, variant)
        ref = torch.from_numpy(conv_np(x, w, bias, relu_in))
        bad = y.double() != ref
        assert not bool(bad.any()), f"relu_in={relu_in}: {int(bad.sum())}/{bad.numel()} elements differ from the definition, first at {bad.nonzero()[0].tolist()}"
    assert not torch.equal(torch.from_numpy(conv_np(x, w, bias, False)), ref), "the two definitions differ on this case: relu_in is visible"


@pytest.mark.parametrize("variant", [5, 0], ids=["8phase", "128row"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_conv_relu_in_random_fp16_with_the_most_negative_value(ops, L, case, variant):
    x, w, bias = data(case, "random")
    assert float(x.min()) == -65504.0 and bool((x > 0).any())
    K = 9 * case[3]
    T = conv_np(x.abs(), w.abs(), bias.abs(), False)
    for relu_in in (False, True):
        y = run(ops, L, case, x, w, bias, relu_in, variant).double().numpy()
        ref = conv_np(x, w, bias, relu_in)
        acc_err = (K + 1) * 2.0 ** -24 * (T if not relu_in else conv_np(np.maximum(x.numpy(), 0), w.abs(), bias.abs(), False))
        bound = acc_err + 2.0 ** -11 * (np.abs(ref) + acc_err) + 2.0 ** -25
        err = np.abs(y - ref)
        print(f"{case_id(case)} variant {variant} relu_in={int(relu_in)}: max err / bound {float((err / bound).max()):.3f}, max |ref| {float(np.abs(ref).max()):.1f}")
        assert np.isfinite(y).all() and float(np.abs(ref).max()) < 65504.0
        assert bool((err <= bound).all()), f"relu_in={relu_in}: {int((err > bound).sum())} elements past the bound, worst {float((err / bound).max()):.2f} x"
    assert float(np.abs(conv_np(x, w, bias, False) - ref).max()) > 1.0, "-65504 inputs move the relu_in = 0 result: the identity max would be seen"


@pytest.mark.parametrize("variant", [5, 0], ids=["8phase", "128row"])
@pytest.mark.parametrize("kind", ["ints", "random"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_conv_without_relu_in_gives_the_bits_of_the_relu_kernel_on_nonnegative_inputs(ops, L, case, kind, variant):
    x, w, bias = data(case, kind)
    xa = x.abs()
    plain, relu = (run(ops, L, case, xa, w, bias, r, variant) for r in (False, True))
    assert torch.equal(plain.view(torch.int16), relu.view(torch.int16)), f"{int((plain.view(torch.int16) != relu.view(torch.int16)).sum())} elements differ in bits"
