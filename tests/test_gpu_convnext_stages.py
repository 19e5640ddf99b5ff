"""The ConvNeXt forward producers -- MFMA stem, depthwise 7x7 + LayerNorm, row LayerNorm -- at every tile
variant, output form and edge, through ``count_pipnet_amd.kernels``.

Grids, data, float64 references and the tolerance: tests/convnext_stage_ref.py (checked without a GPU by
tests/test_convnext_stage_ref_cpu.py).  Every fp32 result must satisfy |out - ref| <= F_BOUND * bound
elementwise, where ``bound`` is the first-order worst case of an fp32 evaluation and F_BOUND = 0.677 is 8 x what
torch's own float32 CPU evaluation needs over the same grids (never measured against these kernels; a ratio
above 1 here is a finding about the kernel, not a reason to raise it).  The largest err / bound per kernel
family is printed when the module finishes (``pytest -s``); profiles/convnext_stages/gpu_ratios.txt records an
MI355X run.

Around that: every fp32 result is written through ``out=`` into the middle of a sentinel-filled buffer with one
guard image (row) in front and one behind, which must come back untouched, and every input is the middle of a
NaN-filled buffer, so a read outside the images shows as NaN in the result (all inside one allocation: nothing
here can fault; the stem has no ``out=``, so only its input is guarded).  The split-plane and bf16 forms must
equal ``split_planes(fp32)`` and ``fp32.to(bfloat16)`` bit for bit at every case.  Crops of a map that take
another tile variant, and one image of a batch run alone, must reproduce the same pixels bit for bit: the claim
of csrc/convnext_ops.hip that every tile sums the same 49 products in the same order.

Mutants.  The grids and the bound were sized against five wrong lines.  Each was first run as a float32 torch
evaluation on the CPU (tests/test_convnext_stage_ref_cpu.py: 4x or more outside F_BOUND * bound on the cases it
names), then once on the MI355X against a scratch build of the library with that one line changed in the
kernels; only ``*_reference`` tests failed (and ``test_layernorm_forms`` where the result was NaN):
  * one-pass variance E[y^2] - E[y]^2 in all four LayerNorm bodies: all 8 depthwise ``offset`` cases, the stem's
    (3, 36, 20) ``offset`` case, 69 of the 70 row LayerNorm ``offset`` cases and 34 of its ``flat`` cases (a variance
    below zero: NaN).  No ``normal`` case sees it.  CPU: depthwise (96, 9, 16), (96, 9, 57), (192, 7, 29),
    (384, 8, 15), (768, 7, 14) as (C, H, W); row LayerNorm (65, 517), (192, 517), (2048, 5) as (C, rows).
  * eps outside the square root: all 8 depthwise ``ripple`` and all 8 ``flat`` cases, 49 of the 70 row LayerNorm
    ``flat`` cases.  A flat case shows it only where the fp32 mean of the constant is inexact: the kernels' sum *
    (1 / C) is, in float32 torch the depthwise flat cases (96, 9, 57) and (192, 7, 29) are not, which is why
    ``ripple`` exists.  CPU: every ``ripple`` case, six ``flat`` cases, row LayerNorm ``flat`` (65, 5), (769, 517), (2048, 3).
  * tap (ky, kx) = (0, 0), or (6, 6), multiplied by zero: the 59 ``normal`` cases with H >= 4 and W >= 4, all 8
    ``offset`` cases, all 8 ``impulse_interior`` cases and the 8 ``impulse_corner`` cases for (0, 0), the 8
    ``impulse_edge`` cases for (6, 6).  No case with H <= 3 can see either tap.  CPU: the ``normal`` case of every
    variant at H >= 7.
  * kx and ky swapped in the weight index: all 24 ``impulse`` cases, 110 ``normal`` and the 8 ``offset`` cases.
    CPU: the three ``impulse`` cases of every variant (eight non-square maps).
  * row LayerNorm mean over 64 * NJ lane slots instead of C: all 135 cases whose C is not 64 * NJ (C = 1, 63, 64, 65,
    129, 193, 385, 769, 1000).  CPU: C = 65 at every row count.

The Python wrappers refuse no C in 1..2048 for the split-plane or bf16 row LayerNorm that include/pipnet_amd.h
allows, so every C of the grid runs in all three forms.
"""
import functools

import pytest
import torch

import convnext_stage_ref as R
from count_pipnet_amd import kernels as K

pytestmark = pytest.mark.gpu

SENTINEL = -77777.0
_WORST = {"dwconv7_ln": (0.0, "-"), "layernorm": (0.0, "-"), "stem": (0.0, "-")}


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    for family, (ratio, what) in _WORST.items():
        print(f"\nconvnext stages: {family:<11} max err / bound = {ratio:.5f} of F_BOUND {R.F_BOUND} allowed ({what})")


def _within_bound(family, out, expect, what):
    ratio = R.worst_ratio(out.cpu(), expect)
    if ratio > _WORST[family][0]:
        _WORST[family] = (ratio, what)
    assert ratio <= R.F_BOUND, f"{family} {what}: err / bound = {ratio:.4f} > F_BOUND = {R.F_BOUND}"


def _inside_nan(t, gpu):
    """``t`` on the device as the middle slice [1:1+n] of a NaN-filled buffer with one guard image (row) each side."""
    buf = torch.full((t.shape[0] + 2,) + tuple(t.shape[1:]), float("nan"), device=gpu, dtype=torch.float32)
    view = buf[1:1 + t.shape[0]]
    view.copy_(t)
    assert view.is_contiguous()
    return view


class GuardedOut:
    """An fp32 result view buf[1:1+n] of a sentinel-filled buffer with one guard image (row) in front and behind."""

    def __init__(self, shape, gpu):
        self.n = shape[0]
        self.buf = torch.full((self.n + 2,) + tuple(shape[1:]), SENTINEL, device=gpu, dtype=torch.float32)
        self.view = self.buf[1:1 + self.n]
        assert self.view.is_contiguous()

    def check(self, what):
        stray = int((self.buf[0] != SENTINEL).sum()) + int((self.buf[1 + self.n:] != SENTINEL).sum())
        assert stray == 0, f"{what}: {stray} floats written outside the result"
        assert not bool(torch.isnan(self.view).any()), f"{what}: NaN in the result (a read outside the input)"
        unwritten = int((self.view == SENTINEL).sum())
        assert unwritten == 0, f"{what}: {unwritten} floats of the result never written"


def _params(gpu, d, *names):
    return [d[k].to(gpu) for k in names]


def _id(case):
    return "-".join(str(v) for v in case)


# ---------------------------------------------------------------------------------------------------
# depthwise 7x7 + LayerNorm
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dw_dev(case, gpu):
    d = R.dw_data(case)
    return (_inside_nan(d["x"], gpu),) + tuple(_params(gpu, d, "w", "bias", "ln_w", "ln_b"))


def _dw_f32(case, gpu):
    args = _dw_dev(case, gpu)
    g = GuardedOut(args[0].shape, gpu)
    ret = K.dwconv7_ln(*args, out=g.view)
    assert ret is g.view
    g.check("dwconv7_ln " + _id(case))
    return g.view


def _check_forms(f32, s3, bf16, what):
    c = f32.shape[-1]
    assert s3.dtype == bf16.dtype == torch.bfloat16
    assert s3.shape == f32.shape[:-1] + (2 * c,) and bf16.shape == f32.shape
    assert torch.equal(s3, K.split_planes(f32)), f"{what}: split planes differ from split_planes(fp32)"
    assert torch.equal(bf16, f32.to(torch.bfloat16)), f"{what}: bf16 form differs from fp32.to(bfloat16)"
    assert torch.equal(bf16, s3[..., :c]), f"{what}: bf16 form differs from the hi plane"


@pytest.mark.parametrize("case", R.DW_CASES, ids=_id)
def test_dwconv7_ln_reference(gpu, case):
    """fp32 form: within F_BOUND * bound of the float64 reference, guards untouched, no NaN read."""
    _within_bound("dwconv7_ln", _dw_f32(case, gpu), R.dw_expect(case), _id(case))


@pytest.mark.parametrize("case", R.DW_CASES, ids=_id)
def test_dwconv7_ln_forms(gpu, case):
    args = _dw_dev(case, gpu)
    _check_forms(_dw_f32(case, gpu), K.dwconv7_ln_s3(*args), K.dwconv7_ln_bf16(*args), "dwconv7_ln " + _id(case))


def _dw_all_forms(x, rest):
    return K.dwconv7_ln(x, *rest), K.dwconv7_ln_s3(x, *rest), K.dwconv7_ln_bf16(x, *rest)


@pytest.mark.parametrize("c,full_w,crops", [(96, 40, ((8, 28, (4, 4)), (10, 26, (7, 1)))),
                                            (192, 24, ((4, 20, (4, 2)), (8, 16, (7, 1))))])
def test_dwconv7_ln_tile_independence(gpu, c, full_w, crops):
    """Column crops of an H = 12 map, which take another tile variant than the full map's (7, 2): every crop
    column at least 3 in from both crop edges sees the same 49 inputs as in the full map and must come out with
    the same bits, in all three output forms."""
    h = 12
    d = R.dw_data((c, 2, h, full_w, R.NORMAL))
    x, *rest = _params(gpu, d, "x", "w", "bias", "ln_w", "ln_b")
    assert R.dw_variant(c, full_w) == (7, 2)
    full = _dw_all_forms(x, rest)
    for lo, hi, tile in crops:
        assert R.dw_variant(c, hi - lo) == tile
        crop = _dw_all_forms(x[:, :, lo:hi].contiguous(), rest)
        for form, a, b in zip(("fp32", "s3", "bf16"), crop, full):
            assert torch.equal(a[:, :, 3:hi - lo - 3], b[:, :, lo + 3:hi - 3]), \
                f"C = {c}: columns [{lo + 3}, {hi - 3}) differ between the W = {full_w} map and its W = {hi - lo} crop ({form})"


@pytest.mark.parametrize("c,h,w", [(v[0],) + v[7] for v in R.DW_VARIANTS])
def test_dwconv7_ln_batch_invariance(gpu, c, h, w):
    """Image 1 alone equals image 1 of a batch of 3, bit for bit (one ragged case per variant)."""
    d = R.dw_data((c, 3, h, w, R.NORMAL))
    x, *rest = _params(gpu, d, "x", "w", "bias", "ln_w", "ln_b")
    for form, a, b in zip(("fp32", "s3", "bf16"), _dw_all_forms(x[1:2], rest), _dw_all_forms(x, rest)):
        assert torch.equal(a[0], b[1]), f"C = {c}, {h} x {w}: image 1 depends on its batch ({form})"


def _offset1(t):
    """The same values one float past a 16-byte boundary (contiguous)."""
    flat = torch.zeros(t.numel() + 1, device=t.device, dtype=t.dtype)
    flat[1:].copy_(t.reshape(-1))
    view = flat[1:].view(t.shape)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def test_dwconv7_ln_refusals(gpu):
    for fn in (K.dwconv7_ln, K.dwconv7_ln_s3, K.dwconv7_ln_bf16):
        for c in (48, 100, 1536):                                 # C outside {96, 192, 384, 768}
            x = torch.zeros((1, 4, 4, c), device=gpu)
            with pytest.raises(RuntimeError):
                fn(x, torch.zeros((49, c), device=gpu), *(torch.zeros(c, device=gpu) for _ in range(3)))
        c = 96
        x = torch.zeros((1, 4, 5, c), device=gpu)
        good = [torch.zeros((49, c), device=gpu)] + [torch.zeros(c, device=gpu) for _ in range(3)]
        fn(x, *good)                                              # the baseline every refusal departs from
        for i in range(4):
            for wrong in (torch.zeros(good[i].numel() - 1, device=gpu),            # wrong size
                          torch.zeros(good[i].numel() + c, device=gpu),
                          good[i].cpu(),                                           # a CPU operand
                          _offset1(good[i])):                                      # a misaligned view
                args = list(good)
                args[i] = wrong
                with pytest.raises(RuntimeError):
                    fn(x, *args)
        with pytest.raises(RuntimeError):
            fn(x.cpu(), *good)
        with pytest.raises(RuntimeError):
            fn(_offset1(x), *good)
        with pytest.raises(RuntimeError):
            fn(x[:, :, 1:], *good)                                # not contiguous
        with pytest.raises(RuntimeError):
            fn(x[0], *good)                                       # not 4-D
    with pytest.raises(RuntimeError):
        K.dwconv7_ln(x, *good, out=torch.zeros((1, 4, 4, c), device=gpu))
    with pytest.raises(RuntimeError):
        K.dwconv7_ln(x, *good, out=_offset1(torch.zeros_like(x)))


# ---------------------------------------------------------------------------------------------------
# row LayerNorm
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ln_dev(case, gpu):
    d = R.ln_data(case)
    return (_inside_nan(d["x"], gpu),) + tuple(_params(gpu, d, "ln_w", "ln_b"))


def _ln_f32(case, gpu):
    args = _ln_dev(case, gpu)
    g = GuardedOut(args[0].shape, gpu)
    ret = K.layernorm(*args, out=g.view)
    assert ret is g.view
    g.check("layernorm " + _id(case))
    return g.view


@pytest.mark.parametrize("case", R.LN_CASES, ids=_id)
def test_layernorm_reference(gpu, case):
    _within_bound("layernorm", _ln_f32(case, gpu), R.ln_expect(case), _id(case))


@pytest.mark.parametrize("case", R.LN_CASES, ids=_id)
def test_layernorm_forms(gpu, case):
    args = _ln_dev(case, gpu)
    _check_forms(_ln_f32(case, gpu), K.layernorm_s3(*args), K.layernorm_bf16(*args), "layernorm " + _id(case))


@pytest.mark.parametrize("c", [1, 96, 2048])
def test_layernorm_no_rows(gpu, c):
    w, b = torch.ones(c, device=gpu), torch.zeros(c, device=gpu)
    x = torch.empty((0, c), device=gpu)
    out = K.layernorm(x, w, b)
    assert out.shape == (0, c) and out.dtype == torch.float32
    assert K.layernorm_s3(x, w, b).shape == (0, 2 * c)
    assert K.layernorm_bf16(x, w, b).shape == (0, c)
    g = GuardedOut((0, c), gpu)                                   # an empty slice of a real buffer
    assert K.layernorm(x, w, b, out=g.view) is g.view
    g.check(f"layernorm 0 x {c}")


def test_layernorm_refusals(gpu):
    for fn in (K.layernorm, K.layernorm_s3, K.layernorm_bf16):
        with pytest.raises(RuntimeError):                         # the C ABI stops at C = 2048
            fn(torch.zeros((3, 2049), device=gpu), torch.ones(2049, device=gpu), torch.zeros(2049, device=gpu))
        c = 65
        x, w, b = torch.zeros((3, c), device=gpu), torch.ones(c, device=gpu), torch.zeros(c, device=gpu)
        fn(x, w, b)
        for args in ((x, w[:-1], b), (x, w, torch.zeros(c + 1, device=gpu)), (x.cpu(), w, b), (x, w.cpu(), b),
                     (x, w, b.cpu()), (x[:, 1:], w[1:], b[1:])):
            with pytest.raises(RuntimeError):
                fn(*args)
    with pytest.raises(RuntimeError):
        K.layernorm(x, w, b, out=torch.zeros((3, c + 1), device=gpu))


# ---------------------------------------------------------------------------------------------------
# stem
# ---------------------------------------------------------------------------------------------------
def _stem_run(case, gpu, images=None):
    d = R.stem_data(case)
    x = d["x"] if images is None else d["x"][images]
    return K.convnext_stem(_inside_nan(x, gpu), *_params(gpu, d, "w", "bias", "ln_w", "ln_b"))


@pytest.mark.parametrize("case", R.STEM_CASES, ids=_id)
def test_stem_reference(gpu, case):
    """The 7 x 448 x 452 case has 2,769 tiles for 2,048 waves: 721 waves take a second trip through the persistent
    loop on their prefetched tile, one of them the ragged last tile of 16 pixels."""
    out = _stem_run(case, gpu)
    assert not bool(torch.isnan(out).any()), "NaN in the result (a read outside the input)"
    _within_bound("stem", out, R.stem_expect(case), _id(case))


@pytest.mark.parametrize("case,image", [((3, 36, 20, R.NORMAL), 1), (R.STEM_BIG, 0)], ids=["3-36-20", "big"])
def test_stem_batch_invariance(gpu, case, image):
    alone = _stem_run(case, gpu, slice(image, image + 1))
    assert torch.equal(alone[0], _stem_run(case, gpu)[image]), f"image {image} depends on its batch"


def test_stem_refusals(gpu):
    d = R.stem_data((1, 4, 8, R.NORMAL))
    good = _params(gpu, d, "w", "bias", "ln_w", "ln_b")
    K.convnext_stem(torch.zeros((1, 3, 4, 8), device=gpu), *good)
    for shape in ((1, 3, 6, 8), (1, 3, 8, 6), (1, 3, 8, 9), (1, 3, 2, 8), (1, 3, 0, 8), (1, 3, 8, 2),   # H, W % 4, < 4
                  (1, 1, 8, 8), (1, 4, 8, 8), (3, 8, 8)):                                             # C != 3, not 4-D
        with pytest.raises(RuntimeError):
            K.convnext_stem(torch.zeros(shape, device=gpu), *good)
    x = torch.zeros((1, 3, 8, 8), device=gpu)
    for i in range(4):
        for wrong in (torch.zeros(good[i].numel() - 1, device=gpu), good[i].cpu(), _offset1(good[i])):
            args = list(good)
            args[i] = wrong
            with pytest.raises(RuntimeError):
                K.convnext_stem(x, *args)
    with pytest.raises(RuntimeError):
        K.convnext_stem(x.cpu(), *good)
    with pytest.raises(RuntimeError):
        K.convnext_stem(_offset1(x), *good)
