"""tests/gemm_matrix_ref.py checked without a GPU: every grid row reaches the kernel form its comment
names (through the library's own plan functions), the exact cases are exact (float32 on the CPU gives
the float64 reference's bits, so any summation order does), and the GELU arguments stay inside the
range the documented error bounds hold on."""
import pytest
import torch

import gemm_matrix_ref as R
from count_pipnet_amd import _lib
from count_pipnet_amd import kernels as K

_EPIS = [_lib.EPI_NONE, _lib.EPI_BIAS, _lib.EPI_BIAS_GELU, _lib.EPI_RESID, _lib.EPI_MUL, _lib.EPI_BIAS_RELU,
         _lib.EPI_BIAS_RESID_RELU, _lib.EPI_RESID_ROWSCALE, _lib.EPI_GELU_BWD]


@pytest.mark.parametrize("m,n,k,variant,npad", R.DENSE_ROWS)
def test_dense_rows_reach_their_variant(m, n, k, variant, npad):
    assert K.splitk_factor(m, n, k) == 1
    for epi in _EPIS:
        if variant == 5 and epi == _lib.EPI_GELU_BWD:
            assert K.gemm_variant(m, n, k, epi, 0) == 2          # not dispatched on the wide tile
            continue
        assert K.gemm_variant(m, n, k, epi, 0) == variant, epi
    assert npad == (variant == 2 and n % 128 != 0)
    name = K.gemm_kernel_name(m, n, k, _lib.EPI_NONE, 0)
    if variant == 2:
        assert name.endswith("true>" if npad else "false>")
    assert k <= 16384 and R.rows_per_scale(m, n, k) * R.dense_case(m, n, k)["row_scale"].numel() >= m


def test_dense_grid_covers_every_kernel_form():
    forms = {(v, npad) for _, _, _, v, npad in R.DENSE_ROWS}
    assert forms == {(0, False), (1, False), (2, False), (2, True), (3, False), (5, False)}
    m, n, k = R.WIDE
    assert -(-m // 192) == 101 and m - 100 * 192 == 5 and m % R.WIDE_ROWS_PER_SCALE != 0


@pytest.mark.parametrize("m,n,k,slabs", R.SPLITK_ROWS)
def test_splitk_rows_reach_their_slab_count(m, n, k, slabs):
    assert K.splitk_factor(m, n, k) == slabs
    assert k % 32 == 0 and n % 4 == 0 and slabs <= k // 32
    if slabs == 1:
        assert m == K.SPLITK_MAX_M + 1 and K.splitk_factor(m - 1, n, k) > 1
        assert K.gemm_variant(m, n, k) == 2


def test_splitk_slab_ranges_are_uneven():
    ranges = lambda tiles, s: [tiles * (y + 1) // s - tiles * y // s for y in range(s)]  # noqa: E731
    assert ranges(544 // 32, 2) == [8, 9] and ranges(800 // 32, 3) == [8, 8, 9] and ranges(16384 // 32, 64) == [8] * 64


@pytest.mark.parametrize("b,h,w,cin,cout,kh,kw,stride,pad,variant,tap_walk", R.CONV_ROWS)
def test_conv_rows_reach_their_variant(b, h, w, cin, cout, kh, kw, stride, pad, variant, tap_walk):
    oh, ow = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    assert h != w and oh != ow
    pointwise = kh == 1 and kw == 1 and stride == 1 and pad == 0
    for epi in (_lib.EPI_NONE, _lib.EPI_BIAS, _lib.EPI_BIAS_RELU, _lib.EPI_BIAS_RESID_RELU):
        assert K.gemm_variant(b * oh * ow, cout, kh * kw * cin, epi, 0 if pointwise else 2) == variant
    if variant == 0 or pointwise:
        assert tap_walk is None
    else:
        assert tap_walk == (cin % (16 if variant == 1 else 32) == 0)
        assert (kh * kw * cin) % (16 if variant == 1 else 32) == 0


def test_conv_grid_covers_both_loader_paths():
    seen = {(v, t) for *_, v, t in R.CONV_ROWS if t is not None}
    assert seen == {(1, True), (1, False), (2, True), (2, False), (3, True), (3, False)}


@pytest.mark.parametrize("b,h,w,cin,cout,stride,variant", R.CONV2X2_ROWS)
def test_conv2x2_rows_reach_their_variant(b, h, w, cin, cout, stride, variant):
    oh, ow = (h - 2) // stride + 1, (w - 2) // stride + 1
    assert h != w and oh != ow and cin % 32 == 0
    for epi in (_lib.EPI_NONE, _lib.EPI_BIAS):
        assert K.gemm_variant(b * oh * ow, cout, 4 * cin, epi, 1) == variant


def _all_dense():
    return [r[:3] for r in R.DENSE_ROWS] + [r[:3] for r in R.SPLITK_ROWS]


@pytest.mark.parametrize("m,n,k", _all_dense())
def test_dense_exact_cases_are_exact_in_float32(m, n, k):
    for mode in R.EXACT_MODES:
        ref = R.dense_ref(mode, m, n, k)
        assert ref.dtype == torch.float64 and float(ref.abs().max()) < 2 ** 24
        assert torch.equal(ref, ref.round())
        assert torch.equal(ref.float(), R.dense_ref(mode, m, n, k, torch.float32)), mode
    c = R.dense_case(m, n, k)
    # every intermediate the kernels may form, not only the final value, is an integer below 2^24
    top = (c["a"].abs() @ c["w"].abs().t() + c["bias"].abs()) * c["scale"].abs().clamp(min=1) * 2 + c["r"].abs()
    assert float(top.max()) < 2 ** 24


@pytest.mark.parametrize("row", R.CONV_ROWS)
def test_conv_exact_cases_are_exact_in_float32(row):
    shape = row[:9]
    for mode in R.CONV_EPILOGUES:
        ref = R.conv_ref(mode, *shape)
        assert float(ref.abs().max()) < 2 ** 24 and torch.equal(ref, ref.round())
        assert torch.equal(ref.float(), R.conv_ref(mode, *shape, dtype=torch.float32)), mode


@pytest.mark.parametrize("b,h,w,cin,cout,stride,variant", R.CONV2X2_ROWS)
def test_conv2x2_exact_cases_are_exact_in_float32(b, h, w, cin, cout, stride, variant):
    for mode in ("none", "bias"):
        ref = R.conv_ref(mode, b, h, w, cin, cout, 2, 2, stride, 0)
        assert torch.equal(ref.float(), R.conv_ref(mode, b, h, w, cin, cout, 2, 2, stride, 0, dtype=torch.float32))


@pytest.mark.parametrize("m,n,k,variant,form", R.GELU_ROWS)
def test_gelu_rows(m, n, k, variant, form):
    if variant == "splitk":
        assert K.splitk_factor(m, n, k) > 1
    else:
        assert K.splitk_factor(m, n, k) == 1 and K.gemm_variant(m, n, k, _lib.EPI_BIAS_GELU, 0) == variant
        assert R.epilogue_form(variant, n) == form
        if variant != 5:
            assert K.gemm_variant(m, n, k, _lib.EPI_GELU_BWD, 0) == variant
    c = R.gelu_case(m, n, k)
    assert float(c["arg"].abs().max()) < R.GELU_ARG_RANGE["scalar"] <= R.GELU_ARG_RANGE[form]
    assert float(c["arg"].abs().max()) >= 3.0                  # and the draw fills a good part of it
    # the scaled operands and the argument are exact in fp32: the float32 product has the same bits
    arg32 = c["a"].float() @ c["w"].float().t() + c["bias"].float()
    assert torch.equal(arg32.double(), c["arg"])
    assert torch.equal(c["h"].float().double(), c["h"])


def test_gelu_grid_covers_both_forms_on_every_variant():
    seen = {(v, f) for *_, v, f in R.GELU_ROWS}
    # the K-tail kernel (variant 0) has no float4 epilogue; the wide tile and split-K no scalar one
    assert seen == {(0, "scalar"), (1, "vector"), (1, "scalar"), (2, "vector"), (2, "scalar"), (3, "vector"),
                    (3, "scalar"), (5, "vector"), ("splitk", "vector")}


def test_gelu_references():
    x = torch.linspace(-6, 6, 1001, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.gelu(x)
    # torch forms 1 + erf, which cancels in the negative tail; erfc does not: absolute agreement there
    torch.testing.assert_close(R.gelu_erf(x.detach()), y.detach(), rtol=1e-14, atol=2e-15)
    (g,) = torch.autograd.grad(y.sum(), x)
    torch.testing.assert_close(R.gelu_grad(x.detach()), g, rtol=1e-13, atol=2e-15)


@pytest.mark.parametrize("m,n,k,variant,npad", R.RANDOM_ROWS)
def test_random_rows(m, n, k, variant, npad):
    if variant == "splitk":
        assert K.splitk_factor(m, n, k) > 1
    else:
        assert K.splitk_factor(m, n, k) == 1 and K.gemm_variant(m, n, k) == variant
        assert npad == (variant == 2 and n % 128 != 0)


def test_bitwise_claim_rows():
    # gemm_f32.hip, wide short-K rule: 128-row tiles above 64 rows, 64-row tiles up to 64
    assert K.gemm_variant(200, 1024, 192) == 3 and K.gemm_variant(64, 1024, 192) == 2
    assert K.splitk_factor(200, 1024, 192) == 1 and K.splitk_factor(64, 1024, 192) == 1
