"""The ConvNeXt stage matrix (tests/test_gpu_convnext_stages.py): float64 references, data, case grids and the
tolerance of the three forward producers of csrc/convnext_ops.hip / csrc/convnext_dw.hpp -- the MFMA stem,
the depthwise 7x7 + LayerNorm kernel and the row LayerNorm.  tests/test_convnext_stage_ref_cpu.py checks
everything here without a GPU.

References.  ``stem_ref``, ``dwconv7_ln_ref`` and ``layernorm_ref`` are explicit tap loops over shifted slices
in float64 (no library convolution, no library layer norm, none of the kernels' index arithmetic): eps 1e-6
inside the square root, biased two-pass variance.  Each returns a ``Ref``: the output and the float64
intermediates of the tolerance -- pre-norm ``y``, ``A`` = sum |x||w| + |bias| (|x| for the row LayerNorm),
``d`` = y - mean and ``r`` = rstd.

Tolerance.  Per element, with u = 2^-24 (``bound``):

    E     = 2 max_c(k u A_c) + 20 u max_c |y_c|
    bound = |g| r E (1 + |d| r) + 4 u (|d r g| + |beta|)

k = 50 for the depthwise kernel (a 49-FMA chain plus the bias), 49 for the stem, and k u A is u |x| for the row
LayerNorm.  This is the first-order worst case of an fp32 evaluation: the error of y, of the mean and variance
reductions, and what the perturbed rstd does to d r g.  A test asserts ``err <= F_BOUND * bound``.

F_BOUND is measured, not chosen: 8 times the largest err / bound that torch's own float32 CPU evaluation
(F.conv2d + F.layer_norm in float32, ``torch_f32``) reaches over every case of the three grids below; the
factor 8 covers another fp32 summation order (FMA chains, shuffle trees), which moves the error by small
multiples, not by an order of magnitude.  It was never measured against the HIP kernels.  ``python
tests/convnext_stage_ref.py`` prints the per-family maxima; profiles/convnext_stages/bound_check.txt holds
that output:

    dwconv7_ln  max err / bound = 0.02046  (C=192 B=3 H=7 W=29 offset; 158 cases)
    layernorm   max err / bound = 0.08468  (C=192 rows=517 offset; 210 cases)
    stem        max err / bound = 0.02012  (B=7 H=448 W=452 normal; 9 cases)
    F_BOUND = 8 * 0.08468 = 0.677

Data.  Seeded by the case tuple; every value is an fp32 number before the float64 reference sees it.  ``normal``:
N(0,1) x, 0.2 N w, N bias, ln_w = 1 + 0.1 N, ln_b = 0.1 N.  ``offset``: bias + 1000 (x + 1000 for the row
LayerNorm), mean >> std: a one-pass variance drowns.  ``flat``: all-zero x under a constant bias (constant rows
for the row LayerNorm), variance 0: the output must be ln_b to within the bound.  A misplaced eps shows there only
where the fp32 mean of the constant happens to be inexact (d != 0).  The row LayerNorm has a constant of its own in
every row, so some rows always show it; the depthwise kernel has one constant per launch, so ``ripple`` goes with
its ``flat``: the same with one seeded channel 2^-21 (4 ulps) up.  Its variance is still far below eps, d is a few ulps in any arithmetic, and r
must stay at 1000: eps outside the square root makes it about 1e6 and the output wrong in the first digit.
``impulse_*``: x is zero but for one pixel per image -- seeded in the interior, the corner (0, 0), or one pixel in
from the right and bottom edges -- so every output pixel within 3 of it sees exactly one tap.

Nothing here calls ``count_pipnet_amd``.
"""
import collections
import functools
import zlib

import torch
import torch.nn.functional as F

EPS = 1e-6
U = 2.0 ** -24
F_BOUND = 0.677          # 8 x the largest torch-float32 err / bound (module docstring; bound_check.txt)

Ref = collections.namedtuple("Ref", "out y A d r")


# ---------------------------------------------------------------------------------------------------
# float64 references
# ---------------------------------------------------------------------------------------------------
def _norm(y, A, g, beta):
    mean = y.sum(-1, keepdim=True) / y.shape[-1]
    d = y - mean
    var = (d * d).sum(-1, keepdim=True) / y.shape[-1]
    r = 1.0 / torch.sqrt(var + EPS)
    return Ref(d * r * g.double() + beta.double(), y, A, d, r)


def layernorm_ref(x, w, b):
    """Row LayerNorm over the last dimension of x [..., C]."""
    x = x.double()
    return _norm(x, x.abs(), w, b)


def dwconv7_ln_ref(x_nhwc, w49c, bias, ln_w, ln_b):
    """Depthwise 7x7, pad 3 (cross-correlation, as torch): y[b, i, j, c] = bias[c] + sum over (ky, kx) of
    x[b, i + ky - 3, j + kx - 3, c] * w49c[7 ky + kx, c], zero outside the image; then LayerNorm over c."""
    x, w = x_nhwc.double(), w49c.double()
    bsz, h, wd, c = x.shape
    xp = torch.zeros((bsz, h + 6, wd + 6, c), dtype=torch.float64)
    xp[:, 3:3 + h, 3:3 + wd] = x
    y = bias.double().expand(bsz, h, wd, c).clone()
    A = bias.double().abs().expand(bsz, h, wd, c).clone()
    for ky in range(7):
        for kx in range(7):
            win = xp[:, ky:ky + h, kx:kx + wd]
            y += win * w[7 * ky + kx]
            A += win.abs() * w[7 * ky + kx].abs()
    return _norm(y, A, ln_w, ln_b)


def stem_ref(x, w, b, ln_w, ln_b):
    """Conv2d(3, 96, k 4, stride 4) on NCHW x, then LayerNorm over the 96 channels; NHWC result."""
    x, w = x.double(), w.double()
    bsz, cin, h, wd = x.shape
    cout = w.shape[0]
    y = b.double().expand(bsz, h // 4, wd // 4, cout).clone()
    A = b.double().abs().expand(bsz, h // 4, wd // 4, cout).clone()
    for ci in range(cin):
        for ky in range(4):
            for kx in range(4):
                px = x[:, ci, ky::4, kx::4].unsqueeze(-1)
                y += px * w[:, ci, ky, kx]
                A += px.abs() * w[:, ci, ky, kx].abs()
    return _norm(y, A, ln_w, ln_b)


def bound(ref, g, beta, k):
    """The per-element fp32 bound (module docstring); k = 50 depthwise, 49 stem, 1 row LayerNorm (A = |x|)."""
    g, beta = g.double().abs(), beta.double().abs()
    E = 2 * k * U * ref.A.amax(-1, keepdim=True) + 20 * U * ref.y.abs().amax(-1, keepdim=True)
    return g * ref.r * E * (1 + ref.d.abs() * ref.r) + 4 * U * ((ref.d * ref.r).abs() * g + beta)


K_DW, K_STEM, K_LN = 50, 49, 1


# ---------------------------------------------------------------------------------------------------
# the grids
# ---------------------------------------------------------------------------------------------------
NORMAL, OFFSET, FLAT, RIPPLE = "normal", "offset", "flat", "ripple"
RIPPLE_STEP = 2.0 ** -21          # 4 fp32 ulps of the constant, on one seeded channel
IMPULSES = ("impulse_interior", "impulse_corner", "impulse_edge")

# Depthwise variants: (C, (TX, TY), NP = pixels of a column tile, every W of the variant, H of the every-W row,
# the two W that take every H: a whole number of column tiles where the variant's W range holds one (of the
# TX-pixel group tiles otherwise) and a ragged one, every H, the ragged (H, W) of the offset / flat / impulse
# cases).  The largest W of a C is three column tiles wide.
DW_VARIANTS = [
    (96, (7, 1), 56, (1, 3, 6, 7, 8, 16), 9, (7, 16), (1, 2, 3, 4, 5, 7, 9), (9, 16)),
    (96, (4, 4), 32, (17, 31, 32), 9, (32, 17), (1, 2, 3, 4, 5, 7, 9), (9, 31)),
    (96, (7, 2), 56, (33, 56, 57, 113), 9, (56, 57), (1, 2, 3, 4, 5, 7, 9), (9, 57)),
    (192, (7, 1), 28, (1, 7, 8), 7, (7, 8), (1, 2, 3, 4, 7), (7, 8)),
    (192, (4, 2), 16, (9, 15, 16), 7, (16, 9), (1, 2, 3, 4, 7), (7, 15)),
    (192, (7, 2), 28, (17, 28, 29, 57), 7, (28, 29), (1, 2, 3, 4, 7), (7, 29)),
    (384, (7, 3), 14, (1, 6, 13, 14, 15, 29), 8, (14, 15), (1, 2, 3, 4, 7, 8), (8, 15)),
    (768, (13, 1), 13, (1, 12, 13, 14, 27), 7, (13, 14), (1, 2, 4, 7), (7, 14)),
]


def dw_variant(c, w):
    """(TX, TY) of the grid row a (C, W) case belongs to (the table above, not the library)."""
    rows = [v for v in DW_VARIANTS if v[0] == c and min(v[3]) <= w <= max(v[3])]
    assert len(rows) == 1, (c, w)
    return rows[0][1]


def _dw_cases():
    cases, special = [], []
    for c, _tile, _np, ws, h_all, w_pair, hs, (sh, sw) in DW_VARIANTS:
        rows = [(h_all, w) for w in ws] + [(h, w) for w in w_pair for h in hs]
        for h, w in dict.fromkeys(rows):                            # B = 3 where H + W is odd, 1 elsewhere
            cases.append((c, 3 if (h + w) % 2 else 1, h, w, NORMAL))
        special += [(c, 3 if c < 768 else 1, sh, sw, kind) for kind in (OFFSET, FLAT, RIPPLE) + IMPULSES]
    return cases, special


DW_NORMAL_CASES, DW_SPECIAL_CASES = _dw_cases()
DW_CASES = DW_NORMAL_CASES + DW_SPECIAL_CASES            # (C, B, H, W, kind)

LN_CHANNELS = (1, 63, 64, 65, 128, 129, 192, 193, 384, 385, 768, 769, 1000, 2048)
LN_ROWS = (1, 3, 4, 5, 517)
LN_CASES = [(c, rows, kind) for c in LN_CHANNELS for rows in LN_ROWS for kind in (NORMAL, OFFSET, FLAT)]

STEM_BIG = (7, 448, 452, NORMAL)     # 88,592 pixels = 2,769 32-pixel tiles over 2,048 waves, ragged last tile
STEM_CASES = [(2, 224, 224, NORMAL), (2, 64, 64, NORMAL), (2, 128, 128, NORMAL), (3, 36, 20, NORMAL),
              (1, 4, 8, NORMAL), (5, 68, 132, NORMAL), STEM_BIG, (1, 4, 4, NORMAL), (3, 36, 20, OFFSET)]


# ---------------------------------------------------------------------------------------------------
# data (float32 tensors on the CPU; read-only, shared)
# ---------------------------------------------------------------------------------------------------
def _gen(family, case):
    return torch.Generator().manual_seed(zlib.crc32(repr((family,) + tuple(case)).encode()))


def _randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, dtype=torch.float32) * scale


def _affine(g, c):
    return 1 + _randn(g, c, scale=0.1), _randn(g, c, scale=0.1)


def impulse_positions(case):
    """(py, px) of the one non-zero pixel of every image of an impulse case."""
    _c, bsz, h, w, kind = case
    if kind == "impulse_corner":
        return [(0, 0)] * bsz
    if kind == "impulse_edge":
        return [(h - 2, w - 2)] * bsz
    g = _gen("impulse", case)
    lo_y, hi_y, lo_x, hi_x = min(3, h // 2), max(h - 4, h // 2), min(3, w // 2), max(w - 4, w // 2)
    draw = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))  # noqa: E731
    return [(draw(lo_y, hi_y), draw(lo_x, hi_x)) for _ in range(bsz)]


@functools.lru_cache(maxsize=None)
def dw_data(case):
    c, bsz, h, w, kind = case
    g = _gen("dw", case)
    x = _randn(g, bsz, h, w, c)
    w49c, bias = _randn(g, 49, c, scale=0.2), _randn(g, c)
    ln_w, ln_b = _affine(g, c)
    if kind == OFFSET:
        bias = bias + 1000
    elif kind in (FLAT, RIPPLE):
        x = torch.zeros_like(x)
        bias = torch.full((c,), float(torch.rand(1, generator=g)) + 0.5)
        if kind == RIPPLE:
            bias[int(torch.randint(c, (1,), generator=g))] *= 1 + RIPPLE_STEP
    elif kind in IMPULSES:
        pix = x[:, 0, 0].clone()
        x = torch.zeros_like(x)
        for i, (py, px) in enumerate(impulse_positions(case)):
            x[i, py, px] = pix[i]
    else:
        assert kind == NORMAL
    return dict(x=x, w=w49c, bias=bias, ln_w=ln_w, ln_b=ln_b)


@functools.lru_cache(maxsize=None)
def ln_data(case):
    c, rows, kind = case
    g = _gen("ln", case)
    x = _randn(g, rows, c)
    ln_w, ln_b = _affine(g, c)
    if kind == OFFSET:
        x = x + 1000
    elif kind == FLAT:
        x = _randn(g, rows, 1, scale=3.0).expand(rows, c).contiguous()
    else:
        assert kind == NORMAL
    return dict(x=x, ln_w=ln_w, ln_b=ln_b)


@functools.lru_cache(maxsize=2)
def stem_data(case):
    bsz, h, w, kind = case
    g = _gen("stem", case)
    x = _randn(g, bsz, 3, h, w)
    wt, bias = _randn(g, 96, 3, 4, 4, scale=0.2), _randn(g, 96)
    ln_w, ln_b = _affine(g, 96)
    if kind == OFFSET:
        bias = bias + 1000
    else:
        assert kind == NORMAL
    return dict(x=x, w=wt, bias=bias, ln_w=ln_w, ln_b=ln_b)


# ---------------------------------------------------------------------------------------------------
# per case: (float64 reference output, per-element bound), computed once
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dw_expect(case):
    d = dw_data(case)
    ref = dwconv7_ln_ref(d["x"], d["w"], d["bias"], d["ln_w"], d["ln_b"])
    return ref.out, bound(ref, d["ln_w"], d["ln_b"], K_DW)


@functools.lru_cache(maxsize=None)
def ln_expect(case):
    d = ln_data(case)
    ref = layernorm_ref(d["x"], d["ln_w"], d["ln_b"])
    return ref.out, bound(ref, d["ln_w"], d["ln_b"], K_LN)


@functools.lru_cache(maxsize=2)
def stem_expect(case):
    d = stem_data(case)
    ref = stem_ref(d["x"], d["w"], d["bias"], d["ln_w"], d["ln_b"])
    return ref.out, bound(ref, d["ln_w"], d["ln_b"], K_STEM)


def worst_ratio(out, expect):
    """max err / bound of ``out`` (any float dtype, CPU) against ``expect`` = (reference, bound); NaN counts as inf."""
    ref, bnd = expect
    assert out.shape == ref.shape, (out.shape, ref.shape)
    ratio = (out.double() - ref).abs() / bnd
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    return float(ratio.max()) if ratio.numel() else 0.0


# ---------------------------------------------------------------------------------------------------
# torch's own float32 evaluation on the CPU: what F_BOUND is measured against
# ---------------------------------------------------------------------------------------------------
def w49c_to_torch(w49c):
    """[49, C] -> the Conv2d weight [C, 1, 7, 7]."""
    return w49c.t().reshape(-1, 1, 7, 7).contiguous()


def dw_torch_f32(case):
    d = dw_data(case)
    c = d["x"].shape[-1]
    y = F.conv2d(d["x"].permute(0, 3, 1, 2), w49c_to_torch(d["w"]), d["bias"], padding=3, groups=c)
    return F.layer_norm(y.permute(0, 2, 3, 1), (c,), d["ln_w"], d["ln_b"], EPS)


def ln_torch_f32(case):
    d = ln_data(case)
    return F.layer_norm(d["x"], (d["x"].shape[-1],), d["ln_w"], d["ln_b"], EPS)


def stem_torch_f32(case):
    d = stem_data(case)
    y = F.conv2d(d["x"], d["w"], d["bias"], stride=4).permute(0, 2, 3, 1)
    return F.layer_norm(y, (96,), d["ln_w"], d["ln_b"], EPS)


FAMILIES = {
    "dwconv7_ln": (DW_CASES, dw_torch_f32, dw_expect, "C=%d B=%d H=%d W=%d %s"),
    "layernorm": (LN_CASES, ln_torch_f32, ln_expect, "C=%d rows=%d %s"),
    "stem": (STEM_CASES, stem_torch_f32, stem_expect, "B=%d H=%d W=%d %s"),
}


def measure():
    """Per family: (largest err / bound of the torch float32 evaluation, the case that reaches it)."""
    worst = {}
    for name, (cases, f32, expect, fmt) in FAMILIES.items():
        ratios = [(worst_ratio(f32(case), expect(case)), fmt % case) for case in cases]
        worst[name] = max(ratios)
    return worst


if __name__ == "__main__":
    torch.manual_seed(0)
    found = measure()
    for fam, (ratio, what) in found.items():
        print(f"{fam:<11} max err / bound = {ratio:.5f}  ({what}; {len(FAMILIES[fam][0])} cases)")
    top = max(r for r, _ in found.values())
    print(f"F_BOUND = 8 * {top:.5f} = {8 * top:.3f}   (committed: {F_BOUND})")
