"""The fp32 MFMA GEMM at every kernel form, epilogue, A-loader, epilogue form and ragged edge.

Grid, data and references: tests/gemm_matrix_ref.py (checked without a GPU by test_gemm_matrix_cpu.py).
The core is exact: small-integer operands make every sum exact in fp32 in any order, so the result must
equal the float64 reference bit for bit -- a wrong index, a transposed fragment, a missed tap, a wrong
K-slab range or an epilogue applied to the wrong row cannot pass.  Every result is written into a
sentinel-filled buffer whose guard rows, guard columns and leading bytes must come back untouched.

Of the four mutations the grid was sized against: swapping t_kx / t_ky in a_src fails the twelve tap-walk
cases of test_conv2d_exact (3 x 3 taps on non-square images) and loading the bias under EPI_MUL in the
scalar epilogue fails the six "mul" cases of the scalar-epilogue rows, which pass a non-zero bias (both run
once against a scratch build: exactly those 18 exact cases failed, every other one passed); offsetting kt_begin by one
K-tile fails every LDS-DMA row (from the case list, not run).  Dropping the min(m, M - 1) clamp of
the row-scale lookup changes no stored value (rows >= M are never stored): it only reads up to one tile
past ``row_scale``, which no output comparison can see.
"""
import functools

import pytest
import torch

import gemm_matrix_ref as R
from count_pipnet_amd import _lib
from count_pipnet_amd import kernels as K

pytestmark = pytest.mark.gpu

SENTINEL = -77777.0


class Guarded:
    """An (m, n) result view inside a sentinel-filled buffer: ``rows`` guard rows above and below, ``left`` /
    ``right`` guard columns (ldc = left + n + right), the whole buffer ``offset`` floats past a 16-byte
    boundary."""

    def __init__(self, m, n, dev, rows=4, left=0, right=0, offset=0):
        self.m, self.n, self.rows, self.left = m, n, rows, left
        ld = left + n + right
        self.flat = torch.full((offset + (m + 2 * rows) * ld,), SENTINEL, device=dev, dtype=torch.float32)
        self.grid = self.flat[offset:].view(m + 2 * rows, ld)
        self.view = self.grid[rows:rows + m, left:left + n]
        assert self.view.data_ptr() % 16 == 4 * ((offset + rows * ld + left) % 4)

    def check(self, ref, what):
        """The view equals ``ref`` (float32, any device) bit for bit and nothing else was written."""
        got = self.view.clone()
        self.view.fill_(SENTINEL)
        stray = int((self.flat != SENTINEL).sum())
        assert stray == 0, f"{what}: {stray} floats written outside the {self.m} x {self.n} result"
        ref = ref.to(got.device)
        assert ref.dtype == torch.float32 and ref.shape == got.shape
        if not torch.equal(got, ref):
            bad = (got != ref).nonzero()
            i, j = (int(v) for v in bad[0])
            raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} values differ, first at [{i}, {j}]: "
                                 f"got {float(got[i, j])}, want {float(ref[i, j])}; rows "
                                 f"{sorted(set(bad[:, 0].tolist()))[:8]}, columns {sorted(set(bad[:, 1].tolist()))[:8]}")


def _dev(t, gpu):
    return t.float().to(gpu)


@functools.lru_cache(maxsize=None)
def _dense_dev(m, n, k, gpu):
    """The row's operands on the device (read-only: shared by every case of the row)."""
    return {key: _dev(v, gpu) for key, v in R.dense_case(m, n, k).items() if key != "acc"}


def _wider(t, extra, left=0):
    """The same values as a column slice of a sentinel-filled buffer ``extra`` columns wider."""
    buf = torch.full((t.shape[0], t.shape[1] + extra), SENTINEL, device=t.device, dtype=t.dtype)
    view = buf[:, left:left + t.shape[1]]
    view.copy_(t)
    return view


def _offset1(t):
    """The same values one float past a 16-byte boundary (contiguous)."""
    flat = torch.full((t.numel() + 1,), SENTINEL, device=t.device, dtype=t.dtype)
    flat[1:].copy_(t.reshape(-1))
    view = flat[1:].view(t.shape)
    assert view.data_ptr() % 16 == 4
    return view


FORMS = ["lda", "interior_out", "ldr", "out+1", "r+1", "bias+1"]


def _run_exact(gpu, mode, m, n, k, form="plain"):
    epi, has_bias, has_scale, inplace = R.EXACT_MODES[mode]
    c = _dense_dev(m, n, k, gpu)
    a, w, r = c["a"], c["w"], c["r"]
    bias = c["bias"] if has_bias else None
    scale = c["scale"] if has_scale else None
    g = Guarded(m, n, gpu)
    if form == "lda":
        a = _wider(a, 8, left=4)
        assert a.stride(0) == k + 8 and a.data_ptr() % 16 == 0
    elif form == "interior_out":
        g = Guarded(m, n, gpu, rows=2, left=4, right=4)
    elif form == "ldr":
        r = _wider(r, 4)
    elif form == "out+1":
        g = Guarded(m, n, gpu, offset=1)
    elif form == "r+1":
        r = _offset1(r)
    elif form == "bias+1":
        bias = _offset1(bias)
    else:
        assert form == "plain"
    out = g.view
    if inplace:
        out.copy_(r)
        r = out
    if mode == "rowscale":
        ret = K.linear_rowscale(a, w, bias, scale, out, c["row_scale"], R.rows_per_scale(m, n, k))
    else:
        ret = K.linear(a, w, bias, epi, scale=scale, r=r, out=out)
    assert ret is out
    g.check(R.dense_ref(mode, m, n, k).float(), f"{mode} {m} x {n} x {k} ({form})")


# ---------------------------------------------------------------------------------------------------
# 1 + 2. exact cases, nothing written outside the result
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(R.EXACT_MODES))
@pytest.mark.parametrize("m,n,k,variant,npad", R.DENSE_ROWS)
def test_dense_exact(gpu, m, n, k, variant, npad, mode):
    _run_exact(gpu, mode, m, n, k)


@pytest.mark.parametrize("mode", R.LINEAR_MODES)
@pytest.mark.parametrize("m,n,k,slabs", R.SPLITK_ROWS)
def test_splitk_exact(gpu, m, n, k, slabs, mode):
    assert K.splitk_factor(m, n, k) == slabs
    _run_exact(gpu, mode, m, n, k)


_FORM_ROWS = [(130, 132, 36), (129, 96, 128), (130, 388, 224), R.WIDE]      # variants 0, 2 NPAD, 3, 5


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("m,n,k", _FORM_ROWS)
def test_operand_forms_exact(gpu, m, n, k, form):
    """Strided and offset operands: lda > K, out as an interior view, ldr != ldc, and out / r / bias one
    float off 16-byte alignment, which must take the scalar epilogue (on the wide row: fall back from the
    192 x 384 tile to the 64-row tile) and still be exact."""
    _run_exact(gpu, "resid", m, n, k, form)
    if (m, n, k) == R.WIDE:
        _run_exact(gpu, "rowscale", m, n, k, form if form != "r+1" else "out+1")


_CONV_EPI = {"none": _lib.EPI_NONE, "bias": _lib.EPI_BIAS, "bias_relu": _lib.EPI_BIAS_RELU,
             "bias_resid_relu": _lib.EPI_BIAS_RESID_RELU}


@pytest.mark.parametrize("mode", R.CONV_EPILOGUES)
@pytest.mark.parametrize("row", R.CONV_ROWS, ids=lambda r: "-".join(str(v) for v in r))
def test_conv2d_exact(gpu, row, mode):
    b, h, w, cin, cout, kh, kw, stride, pad = row[:9]
    c = {key: _dev(v, gpu) for key, v in R.conv_case(*row[:9]).items()}
    ref = R.conv_ref(mode, *row[:9]).float()
    epi = _CONV_EPI[mode]
    y = K.conv2d_nhwc(c["x"], c["wp"], c["bias"], stride, pad, epi, c["r"])
    assert y.shape == ref.shape
    assert torch.equal(y.cpu(), ref), f"conv2d_nhwc {row} {mode}: {int((y.cpu() != ref).sum())} values differ"
    # the same launch into a guarded buffer (the wrapper allocates its own result)
    m = ref.numel() // cout
    g = Guarded(m, cout, gpu)
    _lib.call("pipnet_conv2d_nhwc_f32", c["x"].data_ptr(), b, h, w, cin, c["wp"].data_ptr(), c["bias"].data_ptr(),
              cout, kh, kw, stride, pad, c["r"].data_ptr(), epi, g.view.data_ptr(),
              torch.cuda.current_stream(gpu).cuda_stream)
    g.check(ref.view(m, cout), f"conv2d {row} {mode}")


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("b,h,w,cin,cout,stride,variant", R.CONV2X2_ROWS)
def test_conv2x2_exact(gpu, b, h, w, cin, cout, stride, variant, with_bias):
    shape = (b, h, w, cin, cout, 2, 2, stride, 0)
    c = {key: _dev(v, gpu) for key, v in R.conv_case(*shape).items()}
    ref = R.conv_ref("bias" if with_bias else "none", *shape).float()
    bias = c["bias"] if with_bias else None
    y = K.conv2x2(c["x"], c["wp"], bias, stride)
    assert y.shape == ref.shape
    assert torch.equal(y.cpu(), ref), f"conv2x2: {int((y.cpu() != ref).sum())} values differ"
    m = ref.numel() // cout
    g = Guarded(m, cout, gpu)
    _lib.call("pipnet_conv2x2_f32", c["x"].data_ptr(), b, h, w, cin, c["wp"].data_ptr(),
              None if bias is None else bias.data_ptr(), cout, stride, g.view.data_ptr(),
              torch.cuda.current_stream(gpu).cuda_stream)
    g.check(ref.view(m, cout), f"conv2x2 {shape} bias={with_bias}")


# ---------------------------------------------------------------------------------------------------
# 3. GELU epilogues on exact arguments
# ---------------------------------------------------------------------------------------------------
def _report(what, err, tol):
    ratio = float((err / tol).max())
    print(f"{what}: max |err| {float(err.max()):.3e}, worst err / tolerance {ratio:.3f}")
    return ratio


@pytest.mark.parametrize("m,n,k,variant,form", R.GELU_ROWS)
def test_bias_gelu_exact_argument(gpu, m, n, k, variant, form):
    """acc + bias is exact, so this tests the GELU of each epilogue form alone, against float64 erf-GELU
    within the bound its source documents (gemm_matrix_ref.gelu_tol quotes both) plus one fp32 rounding.

    Measured on the MI355X, worst err / tolerance per row.  Vector epilogue (gelu_pk16): 0.36 (129 x 132 x 48),
    0.37 (70 x 128 x 64), 0.49 (129 x 96 x 128), 0.37 (130 x 388 x 224), 0.49 / 0.31 (split-K), 0.48 (wide
    tile).  Scalar epilogue: 0.28 (70 x 37 x 20), 0.31 (130 x 132 x 36), 0.30 (65 x 197 x 64, 70 x 130 x 64,
    130 x 390 x 224).

    This test found the one fault of the matrix.  With gelu_fast inside the scalar epilogue these five rows
    were 1.23, 1.23, 1.26, 1.26 and 1.36 times outside the bound gelu_fast documents (max |err| 2.8e-7):
    "1.4e-8 absolute, 1.2e-7 relative" are the Chebyshev fit's errors in exact arithmetic (the formula in
    float64: max |err| 1.38e-8), and its fp32 evaluation, even with every operation correctly rounded, is
    up to 1.8x outside 1.4e-8 + 1.2e-7 |gelu| + one rounding.  The scalar-epilogue path now stores
    A W^T + b and takes the GELU in a second pass in double (csrc/gemm_f32.hip gelu_rows_kernel), which
    leaves the one rounding; the bound is the documented one, unchanged."""
    c = R.gelu_case(m, n, k)
    assert float(c["arg"].abs().max()) < R.GELU_ARG_RANGE[form]       # inside the documented range
    ref = R.gelu_erf(c["arg"])
    g = Guarded(m, n, gpu)
    K.linear(_dev(c["a"], gpu), _dev(c["w"], gpu), _dev(c["bias"], gpu), _lib.EPI_BIAS_GELU, out=g.view)
    got = g.view.double().cpu()
    g.check(g.view.clone(), "BIAS_GELU guard")
    ratio = _report(f"BIAS_GELU {form} {m} x {n} x {k} (variant {variant})", (got - ref).abs(), R.gelu_tol(form, ref))
    assert ratio <= 1.0


@pytest.mark.parametrize("offset,left,right", [(1, 0, 0), (0, 3, 5)], ids=["out+1", "interior+3"])
@pytest.mark.parametrize("m,n,k", [(70, 37, 20), (130, 388, 224)])
def test_bias_gelu_scalar_form_strided_out(gpu, m, n, k, offset, left, right):
    """The scalar form's second pass (gelu_rows_kernel) on a misaligned and on an interior, misaligned ``out``
    (ldc > N): the scalar bound, and nothing written outside the view."""
    c = R.gelu_case(m, n, k)
    ref = R.gelu_erf(c["arg"])
    g = Guarded(m, n, gpu, rows=2, left=left, right=right, offset=offset)
    assert g.view.data_ptr() % 16 != 0
    K.linear(_dev(c["a"], gpu), _dev(c["w"], gpu), _dev(c["bias"], gpu), _lib.EPI_BIAS_GELU, out=g.view)
    got = g.view.double().cpu()
    g.check(g.view.clone(), "BIAS_GELU strided guard")
    ratio = _report(f"BIAS_GELU scalar {m} x {n} x {k} (out +{offset}, columns {left}:{left + n} of {left + n + right})",
                    (got - ref).abs(), R.gelu_tol("scalar", ref))
    assert ratio <= 1.0


@pytest.mark.parametrize("m,n,k,variant,form", [r for r in R.GELU_ROWS if r[3] != 5])
def test_gelu_bwd_exact_product(gpu, m, n, k, variant, form):
    """out = (A W^T) * gelu'(R) with an exact product: the rtol / atol of
    test_gpu_backward.test_gelu_forward_and_backward_epilogue."""
    c = R.gelu_case(m, n, k)
    ref = c["acc"] * R.gelu_grad(c["h"])
    g = Guarded(m, n, gpu)
    K.linear(_dev(c["a"], gpu), _dev(c["w"], gpu), None, _lib.EPI_GELU_BWD, r=_dev(c["h"], gpu), out=g.view)
    got = g.view.double().cpu()
    g.check(g.view.clone(), "GELU_BWD guard")
    ratio = _report(f"GELU_BWD {form} {m} x {n} x {k} (variant {variant})", (got - ref).abs(),
                    1e-5 + 1e-5 * ref.abs())
    assert ratio <= 1.0


# ---------------------------------------------------------------------------------------------------
# 4. random values: low-order bits
# ---------------------------------------------------------------------------------------------------
# (linear_rowscale never splits K: no ROWSCALE case on the split-K row)
_RANDOM_CASES = [row + (mode,) for row in R.RANDOM_ROWS for mode in ("none", "bias", "resid", "mul", "rowscale")
                 if not (mode == "rowscale" and row[3] == "splitk")]


@pytest.mark.parametrize("m,n,k,variant,npad,mode", _RANDOM_CASES)
def test_dense_random(gpu, m, n, k, variant, npad, mode):
    """randn operands against float64 within the bounds this suite already uses: test_gpu_kernels._gemm_tol
    for NONE, the 4e-6 form of test_linear_epilogues otherwise (|row_scale| folded into the scale term)."""
    epi = R.EXACT_MODES[mode][0]
    c = R.random_case(m, n, k)
    rps = R.rows_per_scale(m, n, k)
    ref = R.epilogue_ref(epi, c["acc"], c["bias"], c["scale"], c["r"], c["row_scale"], rps)
    if mode == "none":
        tol = 2e-6 * c["absacc"] + 1e-6
    else:
        s = c["scale"].abs()
        if mode == "rowscale":
            s = s * c["row_scale"].repeat_interleave(rps)[:m].view(-1, 1).abs()
        tol = 4e-6 * (1 + ref.abs()) + 4e-6 * (c["absacc"] * (1 + s + c["r"].abs()))
    g = Guarded(m, n, gpu)
    a, w, bias, scale = (_dev(c[key], gpu) for key in ("a", "w", "bias", "scale"))
    if mode == "rowscale":
        g.view.copy_(_dev(c["r"], gpu))
        K.linear_rowscale(a, w, bias, scale, g.view, _dev(c["row_scale"], gpu), rps)
    else:
        K.linear(a, w, bias, epi, scale=scale, r=_dev(c["r"], gpu), out=g.view)
    got = g.view.double().cpu()
    g.check(g.view.clone(), "random guard")
    ratio = _report(f"random {mode} {m} x {n} x {k} (variant {variant}{' NPAD' if npad else ''})",
                    (got - ref).abs(), tol)
    assert ratio <= 1.0


# ---------------------------------------------------------------------------------------------------
# 5. a bit-equality the source claims
# ---------------------------------------------------------------------------------------------------
def test_wide_short_k_rows_bitwise_equal_64row_tile(gpu):
    """gemm_f32.hip on the wide short-K rule (128-row tiles for M > 64, 64-row tiles up to 64): "Same K
    order: bitwise equal"."""
    gen = torch.Generator().manual_seed(2024)
    a = torch.randn(200, 192, generator=gen).to(gpu)
    w = torch.randn(1024, 192, generator=gen).to(gpu)
    assert K.gemm_variant(200, 1024, 192) == 3 and K.gemm_variant(64, 1024, 192) == 2
    full, head = K.linear(a, w), K.linear(a[:64], w)
    assert torch.equal(full[:64], head), f"{int((full[:64] != head).sum())} of {head.numel()} values differ"
    ref = a.double() @ w.double().t()
    assert torch.all((full.double() - ref).abs() <= 2e-6 * (a.double().abs() @ w.double().abs().t()) + 1e-6)


# ---------------------------------------------------------------------------------------------------
# 6. wrapper validation
# ---------------------------------------------------------------------------------------------------
def test_linear_rejects_bad_operands(gpu):
    m, n, k = 8, 12, 16
    a, w = torch.ones(m, k, device=gpu), torch.ones(n, k, device=gpu)
    vec, mat = torch.ones(n, device=gpu), torch.ones(m, n, device=gpu)
    wide = torch.ones(m, 2 * n, device=gpu)
    bad = [
        dict(out=mat.double()), dict(out=mat.cpu()), dict(out=torch.ones(m, n + 1, device=gpu)),
        dict(out=torch.ones(m * n, device=gpu)), dict(out=wide[:, ::2]), dict(out=mat.t().contiguous().t()),
        dict(r=mat.double()), dict(r=mat.cpu()), dict(r=wide[:, ::2]), dict(r=torch.ones(m + 1, n, device=gpu)),
        dict(r=torch.ones(1, n, device=gpu).expand(m, n)),
        dict(bias=vec[:-1]), dict(bias=vec.double()), dict(bias=vec.cpu()), dict(bias=torch.ones(2 * n, device=gpu)[::2]),
        dict(scale=vec[:-1], epilogue=_lib.EPI_RESID, r=mat), dict(scale=vec.half(), epilogue=_lib.EPI_RESID, r=mat),
        dict(epilogue=_lib.EPI_RESID), dict(epilogue=_lib.EPI_MUL), dict(epilogue=_lib.EPI_BIAS_RESID_RELU, bias=vec),
        dict(epilogue=_lib.EPI_GELU_BWD),
    ]
    for kw in bad:
        with pytest.raises(RuntimeError):
            K.linear(a, w, **kw)
    with pytest.raises(RuntimeError):                      # lda % 4 != 0
        K.linear(torch.ones(m, k + 2, device=gpu)[:, :k], w)
    with pytest.raises(RuntimeError):                      # a not 16-byte aligned
        K.linear(_offset1(a), w)
    with pytest.raises(RuntimeError):                      # w not 16-byte aligned
        K.linear(a, _offset1(w))
    with pytest.raises(RuntimeError):                      # non-unit column stride of a
        K.linear(torch.ones(m, 2 * k, device=gpu)[:, ::2], w)

    rs = torch.ones(2, device=gpu)
    bad_rowscale = [
        dict(r=mat.double()), dict(r=wide[:, ::2]), dict(r=torch.ones(m, n + 1, device=gpu)), dict(r=mat.cpu()),
        dict(r=None), dict(bias=vec[:-1]), dict(scale=vec[:-1]), dict(scale=vec.double()),
        dict(row_scale=rs[:1]), dict(rows_per_scale=0),
    ]
    for kw in bad_rowscale:
        args = dict(bias=vec, scale=vec, r=mat.clone(), row_scale=rs, rows_per_scale=4)
        args.update(kw)
        with pytest.raises(RuntimeError):
            K.linear_rowscale(a, w, args["bias"], args["scale"], args["r"], args["row_scale"], args["rows_per_scale"])

    # and the well-formed calls still go through
    assert torch.equal(K.linear(a, w, vec, _lib.EPI_RESID, scale=vec, r=mat), torch.full((m, n), k + 2.0, device=gpu))
    assert torch.equal(K.linear_rowscale(a, w, None, None, mat.clone(), rs * 2, 4),
                       torch.full((m, n), 2.0 * k + 1.0, device=gpu))
