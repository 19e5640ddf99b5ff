"""The fp32 GEMM test matrix (tests/test_gpu_gemm_matrix.py) and its plain-torch reference.

Exact data.  A and W are integers in {-4..4}; bias, scale and R in {-3..3}; row_scale in {0, 1, 2}.
With K <= 16384 every product, partial sum and epilogue value is an integer below 2^24, so fp32
arithmetic is exact in ANY summation order (the MFMA's k order, the split-K slab order, an fma or a
separate multiply and add).  The float64 reference cast to float32 is then the one correct answer and
the GPU tests compare with ``torch.equal``.  tests/test_gemm_matrix_cpu.py proves the claim from the
reference alone (float32 on the CPU gives the same bits) and checks every row against the library's
own plan (``kernels.gemm_variant`` / ``kernels.splitk_factor``): a row that does not reach the variant
it names gets another shape, never another expectation.

Nothing here calls ``count_pipnet_amd.kernels``; only the epilogue codes of ``_lib`` are shared.
"""
import functools

import torch
import torch.nn.functional as F

from count_pipnet_amd import _lib

# ---------------------------------------------------------------------------------------------------
# the grid
# ---------------------------------------------------------------------------------------------------
WIDE = (19205, 384, 768)         # 101 wide (192 x 384) tiles, the last holds 5 rows
WIDE_ROWS_PER_SCALE = 193        # row groups straddle the 192-row tiles, the last group is partial

# (M, N, K, variant, NPAD column skip): dense products through kernels.linear / linear_rowscale
DENSE_ROWS = [
    (70, 37, 20, 0, False),       # K tail of 20, N % 4 != 0
    (130, 132, 36, 0, False),     # two tiles each way, 2-row / 4-column remainders
    (40, 72, 48, 0, False),       # K % 16 == 0 but M <= 64
    (129, 132, 48, 1, False),     # BK16 via the K % 32 rule
    (65, 197, 64, 1, False),      # BK16 via the K <= 96 rule, scalar epilogue
    (200, 260, 96, 1, False),     # three column tiles, the last 4 wide
    (130, 260, 16, 1, False),     # one K-tile of 16 under 3 LDS stages (fewer tiles than prologue stages)
    (70, 128, 64, 2, False),      # plain 64-row tile
    (65, 36, 64, 2, True),        # wave column counts jl = 2 and 0
    (129, 96, 128, 2, True),      # jl = 2 and 1, the last row tile holds one row
    (64, 160, 32, 2, True),       # second column tile jl = 1 and 0; one K-tile under 3 LDS stages
    (3, 516, 224, 2, True),       # M = 3, five column tiles
    (70, 130, 64, 2, True),       # scalar epilogue on the NPAD tile
    (130, 388, 224, 3, False),    # ragged both ways, vector epilogue
    (130, 390, 224, 3, False),    # scalar epilogue on the 128-row tile
    (65, 1024, 128, 3, False),    # wide short-K rule (K <= 96 goes to BK16 first, so 2 LDS stages never
                                  # see a single K-tile: four here)
    WIDE + (5, False),
]

# (M, N, K, K slabs): split-K through kernels.linear
SPLITK_ROWS = [
    (3, 8, 544, 2),               # 17 K-tiles over 2 slabs (8 / 9)
    (37, 132, 800, 3),            # 25 K-tiles over 3 slabs (8 / 8 / 9), N = 132
    (1, 4, 16384, 64),            # the maximum 64 slabs
    (512, 128, 512, 2),           # the last M that splits
    (513, 128, 512, 1),           # must not split
]

# (B, H, W, Cin, Cout, KH, KW, stride, pad, variant, tap_walk): kernels.conv2d_nhwc, all non-square.
# tap_walk (Cin % BK == 0 of the LDS-DMA kernels, BK = 16 for variant 1 and 32 otherwise) is None for the
# K-tail kernel and for the pointwise row, which takes the dense loader.
CONV_ROWS = [
    (2, 5, 7, 4, 40, 3, 3, 1, 1, 0, None),       # K-tail kernel on the conv loader
    (5, 9, 6, 16, 40, 3, 3, 2, 1, 1, True),      # tap walk, stride 2
    (4, 6, 5, 8, 196, 2, 2, 1, 1, 1, False),     # per-lane addresses (Cin 8 under BK 16)
    (2, 6, 5, 8, 40, 2, 2, 1, 1, 2, False),      # per-lane addresses (Cin 8 under BK 32), NPAD
    (2, 7, 9, 32, 48, 3, 3, 2, 1, 2, True),
    (2, 7, 9, 32, 388, 3, 3, 1, 1, 3, True),
    (2, 8, 6, 16, 388, 4, 4, 1, 2, 3, False),    # pad 2
    (3, 5, 9, 64, 40, 1, 1, 1, 0, 2, None),      # pointwise: dense loader
]
CONV_EPILOGUES = ["none", "bias", "bias_relu", "bias_resid_relu"]

# (B, H, W, Cin, Cout, stride, variant): kernels.conv2x2
CONV2X2_ROWS = [
    (3, 5, 8, 32, 40, 1, 2),      # NPAD
    (6, 6, 9, 64, 388, 2, 3),     # odd W under stride 2
]

# exact epilogue cases: name -> (epilogue code, bias given, scale given, R aliases C).  bias, scale and r
# are passed in every case that does not withhold them, also where the epilogue must ignore them.
EXACT_MODES = {
    "none": (_lib.EPI_NONE, True, True, False),
    "bias": (_lib.EPI_BIAS, True, True, False),
    "bias_nullbias": (_lib.EPI_BIAS, False, True, False),
    "resid": (_lib.EPI_RESID, True, True, False),
    "resid_inplace": (_lib.EPI_RESID, True, True, True),
    "resid_nullbias_nullscale": (_lib.EPI_RESID, False, False, False),
    "mul": (_lib.EPI_MUL, True, True, False),
    "bias_relu": (_lib.EPI_BIAS_RELU, True, True, False),
    "bias_resid_relu": (_lib.EPI_BIAS_RESID_RELU, True, True, False),
    "rowscale": (_lib.EPI_RESID_ROWSCALE, True, True, True),
}
LINEAR_MODES = [m for m in EXACT_MODES if m != "rowscale"]       # what kernels.linear takes

# GELU rows: (M, N, K, variant or "splitk", epilogue form)
GELU_ROWS = [
    (70, 37, 20, 0, "scalar"),
    (130, 132, 36, 0, "scalar"),      # the K-tail kernel has the scalar epilogue only
    (129, 132, 48, 1, "vector"),
    (65, 197, 64, 1, "scalar"),
    (70, 128, 64, 2, "vector"),
    (129, 96, 128, 2, "vector"),
    (70, 130, 64, 2, "scalar"),
    (130, 388, 224, 3, "vector"),
    (130, 390, 224, 3, "scalar"),
    (37, 132, 800, "splitk", "vector"),
    (3, 8, 544, "splitk", "vector"),
    WIDE + (5, "vector"),             # BIAS_GELU only: the wide tile is not dispatched for GELU_BWD
]

# random-valued rows: (M, N, K, variant or "splitk", NPAD)
RANDOM_ROWS = [
    (130, 132, 36, 0, False),
    (200, 260, 96, 1, False),
    (70, 128, 64, 2, False),
    (129, 96, 128, 2, True),
    (130, 388, 224, 3, False),
    (37, 132, 800, "splitk", False),
    WIDE + (5, False),
]

FP32_EPS = 2.0 ** -24           # one rounding to fp32, relative


def rows_per_scale(m, n, k):
    """Row groups of the ROWSCALE cases: 7 rows (no divisor of any tile height, so groups straddle the
    64- / 128-row tiles and the last group is partial), 193 on the wide row."""
    return WIDE_ROWS_PER_SCALE if (m, n, k) == WIDE else 7


def epilogue_form(variant, n, aligned=True):
    """Which epilogue the library runs: the K-tail kernel (variant 0) has the scalar one only; the
    LDS-DMA kernels take the float4 epilogue when N % 4 == 0 and every operand is 16-byte friendly."""
    return "vector" if variant != 0 and n % 4 == 0 and aligned else "scalar"


# ---------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------
def _ints(gen, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


@functools.lru_cache(maxsize=None)
def dense_case(m, n, k):
    """Integer operands of an M x N x K product (float64) and their exact product ``acc``."""
    g = torch.Generator().manual_seed(1000003 * m + 1009 * n + k)
    c = {"a": _ints(g, -4, 4, m, k), "w": _ints(g, -4, 4, n, k), "bias": _ints(g, -3, 3, n),
         "scale": _ints(g, -3, 3, n), "r": _ints(g, -3, 3, m, n)}
    rps = rows_per_scale(m, n, k)
    c["row_scale"] = _ints(g, 0, 2, -(-m // rps))
    c["acc"] = c["a"] @ c["w"].t()
    return c


@functools.lru_cache(maxsize=None)
def conv_case(b, h, w, cin, cout, kh, kw, stride, pad):
    """NHWC integer operands of a convolution: x [B,H,W,Cin], wp [Cout,KH,KW,Cin], r [B,OH,OW,Cout]."""
    g = torch.Generator().manual_seed(((((b * 31 + h) * 31 + w) * 31 + cin) * 31 + cout) * 31 + kh * 7 + stride)
    oh, ow = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    return {"x": _ints(g, -4, 4, b, h, w, cin), "wp": _ints(g, -4, 4, cout, kh, kw, cin),
            "bias": _ints(g, -3, 3, cout), "r": _ints(g, -3, 3, b, oh, ow, cout)}


def gelu_scale_exp(m, n, k):
    """e with max |acc + bias| * 2^-e < 6 on the row's integer draw: inside |x| < 6, where gelu_fast's
    bound is documented, and inside gelu_pk16's [-10, 10]."""
    c = dense_case(m, n, k)
    top = float((c["acc"] + c["bias"]).abs().max())
    e = 0
    while top * 2.0 ** -e >= 6.0:
        e += 1
    return e


def gelu_case(m, n, k):
    """The integer draw with A and bias scaled by 2^-e: ``arg`` = A W^T + bias is still exact in fp32
    (an integer below 2^24 times a power of two).  ``h`` is the GELU_BWD pre-activation (random, O(3))."""
    c = dense_case(m, n, k)
    s = 2.0 ** -gelu_scale_exp(m, n, k)
    g = torch.Generator().manual_seed(77 + 1000003 * m + 1009 * n + k)
    a, bias = c["a"] * s, c["bias"] * s
    return {"a": a, "w": c["w"], "bias": bias, "acc": c["acc"] * s, "arg": c["acc"] * s + bias,
            "h": (torch.randn(m, n, generator=g, dtype=torch.float64) * 3).float().double()}


@functools.lru_cache(maxsize=None)
def random_case(m, n, k):
    g = torch.Generator().manual_seed(555 + 1000003 * m + 1009 * n + k)
    # drawn and scaled in float32, so the float64 reference sees the very operands the kernel gets
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).double()  # noqa: E731
    c = {"a": rn(m, k), "w": rn(n, k, scale=0.05), "bias": rn(n), "scale": rn(n), "r": rn(m, n)}
    rps = rows_per_scale(m, n, k)
    c["row_scale"] = ((torch.rand(-(-m // rps), generator=g) < 0.7).float() / 0.7).double()
    c["acc"] = c["a"] @ c["w"].t()
    c["absacc"] = c["a"].abs() @ c["w"].abs().t()
    return c


# ---------------------------------------------------------------------------------------------------
# references (dtype-generic: float64 is the reference, float32 the CPU proof that the data is exact)
# ---------------------------------------------------------------------------------------------------
def epilogue_ref(epi, acc, bias=None, scale=None, r=None, row_scale=None, rps=0):
    """What include/pipnet_amd.h defines for each exact epilogue; a withheld bias is 0, a withheld scale 1."""
    b = 0 if bias is None else bias
    s = 1 if scale is None else scale
    if epi == _lib.EPI_NONE:
        return acc.clone()
    if epi == _lib.EPI_BIAS:
        return acc + b
    if epi == _lib.EPI_RESID:
        return r + s * (acc + b)
    if epi == _lib.EPI_MUL:
        return acc * r
    if epi == _lib.EPI_BIAS_RELU:
        return torch.relu(acc + b)
    if epi == _lib.EPI_BIAS_RESID_RELU:
        return torch.relu(acc + b + r)
    if epi == _lib.EPI_RESID_ROWSCALE:
        rows = row_scale.repeat_interleave(rps)[:acc.shape[0]].view(-1, 1)
        return r + rows * (s * (acc + b))
    raise ValueError(epi)


def dense_ref(mode, m, n, k, dtype=torch.float64):
    """Reference of exact case ``mode`` on row (m, n, k) in ``dtype`` (the product is redone in float32)."""
    epi, has_bias, has_scale, _ = EXACT_MODES[mode]
    c = dense_case(m, n, k)
    t = lambda x: x.to(dtype)  # noqa: E731
    acc = c["acc"] if dtype == torch.float64 else t(c["a"]) @ t(c["w"]).t()
    return epilogue_ref(epi, acc, t(c["bias"]) if has_bias else None, t(c["scale"]) if has_scale else None,
                        t(c["r"]), t(c["row_scale"]), rows_per_scale(m, n, k))


def conv_ref(mode, b, h, w, cin, cout, kh, kw, stride, pad, dtype=torch.float64):
    """F.conv2d on NCHW in ``dtype``, permuted to NHWC, then the epilogue."""
    c = conv_case(b, h, w, cin, cout, kh, kw, stride, pad)
    t = lambda x: x.to(dtype)  # noqa: E731
    y = F.conv2d(t(c["x"]).permute(0, 3, 1, 2), t(c["wp"]).permute(0, 3, 1, 2), None, stride=stride, padding=pad)
    y = y.permute(0, 2, 3, 1)
    if mode != "none":
        y = y + t(c["bias"])
    if mode == "bias_resid_relu":
        y = y + t(c["r"])
    if mode in ("bias_relu", "bias_resid_relu"):
        y = torch.relu(y)
    return y.contiguous()


def gelu_erf(x):
    """x Phi(x), float64."""
    return 0.5 * x * torch.special.erfc(-x * 0.70710678118654752440)


def gelu_grad(x):
    """d gelu_erf / dx = Phi(x) + x phi(x), float64."""
    return 0.5 * torch.special.erfc(-x * 0.70710678118654752440) + \
        x * torch.exp(-0.5 * x * x) * 0.39894228040143267794


# BIAS_GELU bounds, from the comments above the two device functions, plus one fp32 rounding of the result.
#   vector epilogue, gelu_pk16 (csrc/common.hpp): "|GELU error| < 1e-6 on [-10, 10] (fp32 emulation)"
#   scalar epilogue, gelu_fast (csrc/gemm_f32_impl.hpp): "Max |error| vs the erf-GELU of torch: 1.4e-8
#   absolute, 1.2e-7 relative for |x| < 6" -- the accuracy promised for that form; the library meets it by
#   taking the scalar form's GELU in a second pass in double (csrc/gemm_f32.hip gelu_rows_kernel)
GELU_ARG_RANGE = {"vector": 10.0, "scalar": 6.0}


def gelu_tol(form, ref):
    if form == "vector":
        return 1e-6 + FP32_EPS * ref.abs()
    return 1.4e-8 + (1.2e-7 + FP32_EPS) * ref.abs()
