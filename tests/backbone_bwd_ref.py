"""The backbone-backward / BatchNorm test matrix (tests/test_gpu_backbone_bwd.py) and its plain-torch
float64 references, for the kernels of csrc/backward_ops.hip and csrc/bn_ops.hip.

Exact data.  A, B, x, w, dy are integers in {-4..4}; the layer scale and the accumulate bases in {-3..3};
row_scale in {0, 1, 2}.  The longest reduction has 65570 rows, so every product, partial sum and result is
an integer below 16 * 65570 + 3 < 2^24 and fp32 arithmetic is exact in ANY summation order (the MFMA's
row order, the slab order, an fma or a separate multiply and add).  The float64 reference cast to float32
is then the one correct answer and the GPU tests compare with ``torch.equal``.
tests/test_backbone_bwd_cpu.py proves the claim from the references alone (float32 on the CPU gives the
same bits), and checks every row against the library's own plan (``pipnet_wgrad_workspace_bytes``,
``pipnet_bn_slabs``): a row that does not reach the slab count it names gets another shape, never another
expectation.

Every output the caller allocates is handed to the kernel as the interior of a sentinel-filled buffer
(``Framed``), 16-byte aligned, and the frame must come back untouched.

Nothing here calls ``count_pipnet_amd.kernels``.
"""
import functools

import torch
import torch.nn.functional as F

from count_head_ref import align_term
from oracle import train_ref

SENTINEL = -7777.0          # the frame's fill; only the frame is compared with it, the interior with the reference
FRAME = 16                  # floats of sentinel before and after the interior: 64 bytes, keeps 16-byte alignment


def share(got, ref, rtol, atol):
    """Worst |got - ref| / (atol + rtol |ref|): the part of an assert_close tolerance a result uses."""
    got, ref = got.double(), ref.double()
    if got.numel() == 0:
        return 0.0
    return float(((got - ref).abs() / (atol + rtol * ref.abs())).max())


# ---------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------
def ints(shape, lo, hi, seed):
    """Seeded integers lo..hi as float64."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).double()


def leaf(t, dtype):
    """A fresh autograd leaf of ``dtype`` (the cached case tensors are never touched)."""
    return t.detach().to(dtype).clone().requires_grad_(True)


def randn(shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(tuple(shape), generator=g) * scale + shift).double()    # float32 values, held in float64


class Framed:
    """A float32 view of ``shape`` (row stride ``ld`` for a 2-D shape, else contiguous) inside a
    sentinel-filled buffer; ``base`` (same shape) is copied in for the accumulate cases."""

    def __init__(self, shape, device, base=None, ld=None):
        shape = tuple(shape)
        n = 1
        for s in shape:
            n *= s
        if ld is not None:
            assert len(shape) == 2 and ld >= shape[1]
            n = shape[0] * ld
        self.buf = torch.full((2 * FRAME + n,), SENTINEL, device=device, dtype=torch.float32)
        inner = self.buf[FRAME:FRAME + n]
        self.view = inner.view(shape[0], ld)[:, :shape[1]] if ld is not None else inner.view(shape)
        assert self.view.data_ptr() % 16 == 0
        if base is not None:
            self.view.copy_(base.to(device=device, dtype=torch.float32))

    def intact(self):
        """True when everything outside the view still holds the sentinel."""
        probe = self.buf.clone()
        inner = probe[FRAME:probe.numel() - FRAME]
        if self.view.dim() == 2 and self.view.stride(0) != self.view.shape[1]:
            inner.view(self.view.shape[0], self.view.stride(0))[:, :self.view.shape[1]].fill_(SENTINEL)
        else:
            inner.fill_(SENTINEL)
        return bool((probe == SENTINEL).all())

    def untouched(self):
        """True when the view itself was not written either (a rejected call)."""
        return bool((self.buf == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------
# wgrad: C[N1, N2] (+)= A[M, N1]^T B[M, N2]
# ---------------------------------------------------------------------------------------------------
WBK = 32                    # rows per K-tile (backward_ops.hip)

# (M, N1, N2, slabs, K-tiles per slab): the slab counts are wgrad_splits', the per-slab lists follow from
# mchunk = ceil(ktiles / slabs) * 32 rows per slab -- trailing slabs run short, then empty.
WGRAD_ROWS = [
    (5, 4, 8, 1, [1]),                               # one K-tile, direct; one-slab workspace path with accumulate
    (255, 128, 132, 1, [8]),                         # 8 K-tiles, the last a row short; a 4-column N2 tile
    (256, 128, 132, 1, [8]),
    (257, 128, 132, 1, [9]),                         # the ninth K-tile holds one row
    (544, 260, 124, 2, [9, 8]),                      # uneven slabs, a 4-row N1 tile
    (2081, 4, 4, 8, [9] * 7 + [3]),                  # the last slab short
    (4100, 128, 128, 16, [9] * 14 + [3, 0]),         # the last slab empty
    (9000, 768, 768, 14, [21] * 13 + [9]),           # 36 tiles: the 3 % rule picks 14, not the 35 allowed
    (65570, 128, 128, 249, [9] * 227 + [7] + [0] * 21),
    (0, 8, 8, 0, []),                                # no rows: zero, or C unchanged with accumulate
]

# (M, N1, N2, accumulate, strided A / B, extra out row stride)
WGRAD_CASES = (
    [(m, n1, n2, False, False, 0) for m, n1, n2, _, _ in WGRAD_ROWS]
    + [(m, n1, n2, True, False, 0) for m, n1, n2 in [(5, 4, 8), (255, 128, 132), (256, 128, 132), (257, 128, 132),
                                                     (0, 8, 8), (544, 260, 124), (4100, 128, 128)]]
    + [(257, 128, 132, False, True, 0), (2081, 4, 4, True, True, 0)]
    + [(256, 128, 132, False, False, 8), (544, 260, 124, True, False, 12)]
)


def slab_ktiles(m, slabs):
    """K-tiles of each slab under the launcher's mchunk rule."""
    if slabs == 0:
        return []
    ktiles = -(-m // WBK)
    mchunk = -(-ktiles // slabs) * WBK
    return [max(0, -(-(min(m, (s + 1) * mchunk) - s * mchunk) // WBK)) for s in range(slabs)]


@functools.lru_cache(maxsize=None)
def wgrad_case(m, n1, n2, strided):
    """dict(a, b[, big]) float64 integers; strided: A and B are column slices of one [M, N1 + N2 + 8] matrix at
    offsets 4 and N1 + 8."""
    seed = 1000 + m + 3 * n1 + 7 * n2
    if strided:
        big = ints((m, n1 + n2 + 8), -4, 4, seed)
        return dict(big=big, a_cols=(4, 4 + n1), b_cols=(n1 + 8, n1 + 8 + n2), a=big[:, 4:4 + n1],
                    b=big[:, n1 + 8:n1 + 8 + n2], base=ints((n1, n2), -3, 3, seed + 1))
    return dict(a=ints((m, n1), -4, 4, seed), b=ints((m, n2), -4, 4, seed + 2), base=ints((n1, n2), -3, 3, seed + 1))


def wgrad_ref(m, n1, n2, accumulate, strided, dtype=torch.float64):
    c = wgrad_case(m, n1, n2, strided)
    out = c["a"].to(dtype).t() @ c["b"].to(dtype)
    return out + c["base"].to(dtype) if accumulate else out


# ---------------------------------------------------------------------------------------------------
# conv weight gradients (wgrad_conv, wgrad_conv2x2), always H != W and OH != OW
# ---------------------------------------------------------------------------------------------------
# (B, H, W, Cin, Cout, k, stride, pad, accumulate, slabs)
WGRAD_CONV_ROWS = [
    (2, 5, 7, 4, 132, 3, 1, 1, False, 1),            # 3x3 s1 p1; K = 36: every 4 columns another tap
    (2, 7, 10, 132, 4, 3, 2, 1, True, 1),            # 3x3 s2 p1, odd x even image; the tap boundary inside a tile
    (3, 5, 8, 4, 4, 1, 2, 0, False, 1),              # strided 1x1
    (1, 9, 12, 4, 132, 7, 2, 3, False, 1),           # 7x7 s2 p3: taps hang over every edge
    (2, 10, 14, 4, 4, 4, 4, 0, True, 1),             # the ConvNeXt stem's 4x4 / 4; rows 8-9, columns 12-13 never read
    (4, 12, 13, 4, 4, 3, 1, 1, True, 2),             # 624 output pixels: two slabs
]

# (B, H, W, Cin, Cout, stride, accumulate)
WGRAD_CONV2X2_ROWS = [
    (2, 5, 8, 4, 8, 1, False),
    (3, 7, 10, 8, 132, 2, True),                     # odd H under stride 2: the last row is never read
]


def conv_out_hw(h, w, k, s, p):
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


@functools.lru_cache(maxsize=None)
def conv_case(b, h, w, cin, cout, k, s, p):
    """dict(x [B,H,W,Cin], dy [B,OH,OW,Cout], base [Cout, k*k*Cin]) float64 integers, NHWC."""
    seed = 2000 + 31 * h + w + 5 * cin + 11 * cout + k + s
    oh, ow = conv_out_hw(h, w, k, s, p)
    return dict(x=ints((b, h, w, cin), -4, 4, seed), dy=ints((b, oh, ow, cout), -4, 4, seed + 1),
                base=ints((cout, k * k * cin), -3, 3, seed + 2))


def conv_wgrad_ref(b, h, w, cin, cout, k, s, p, accumulate, dtype=torch.float64):
    """Packed [Cout, k*k*Cin] (tap-major, channel-minor) weight gradient by autograd through F.conv2d."""
    c = conv_case(b, h, w, cin, cout, k, s, p)
    wt = torch.zeros(cout, cin, k, k, dtype=dtype, requires_grad=True)
    y = F.conv2d(c["x"].to(dtype).permute(0, 3, 1, 2), wt, stride=s, padding=p)
    y.backward(c["dy"].to(dtype).permute(0, 3, 1, 2))
    out = wt.grad.permute(0, 2, 3, 1).reshape(cout, k * k * cin)
    return out + c["base"].to(dtype) if accumulate else out


# ---------------------------------------------------------------------------------------------------
# colsum
# ---------------------------------------------------------------------------------------------------
# (M, N, strided row view)
COLSUM_ROWS = [(0, 8, False), (1, 4, False), (63, 260, False), (64, 256, False), (65, 300, True), (70000, 8, False)]


@functools.lru_cache(maxsize=None)
def colsum_case(m, n, strided):
    """strided: the matrix is columns 4 .. 4 + N of an [M, N + 8] one."""
    big = ints((m, n + 8 if strided else n), -4, 4, 3000 + m + n)
    return dict(big=big, a=big[:, 4:4 + n] if strided else big, base=ints((n,), -3, 3, 3001 + m + n))


def colsum_ref(m, n, strided, accumulate, dtype=torch.float64):
    c = colsum_case(m, n, strided)
    out = c["a"].to(dtype).sum(0)
    return out + c["base"].to(dtype) if accumulate else out


# ---------------------------------------------------------------------------------------------------
# resid_scale / ls_backward / ln_backward: rows [M, C]
# ---------------------------------------------------------------------------------------------------
WIDTHS = [4, 100, 256, 260, 512, 516, 768, 772, 1024, 1028, 2048]      # at 37 rows
WIDTH_ROWS = 37
ROW_COUNTS = [1, 4, 2048, 2049, 4100]                                  # at C = 8 and C = 260
SWEEP_ROWS = 2048                                                      # TB_G * 4 rows per grid sweep
RPS = 16


def nj4(c):
    """The PIPNET_BY_NJ4 instantiation of a width (float4 chunks per lane), None when rejected."""
    for top, nj in ((256, 1), (512, 2), (768, 3), (1024, 4), (2048, 8)):
        if c <= top:
            return nj
    return None


# (M, C, rows_per_scale, row_scale given, accumulate)
LS_CASES = (
    [(WIDTH_ROWS, c, RPS, True, c in (260, 1028)) for c in WIDTHS]
    + [(m, c, RPS, True, m == 2049) for m in ROW_COUNTS for c in (8, 260)]
    + [(50, 8, 16, True, False), (50, 8, 16, False, True)]
)

# (M, C, want_dz, accumulate)
LN_CASES = (
    [(WIDTH_ROWS, c, c not in (512, 772), c in (260, 1028)) for c in WIDTHS]
    + [(m, c, not (m == 2049 and c == 8), m == 4100) for m in ROW_COUNTS for c in (8, 260)]
)


@functools.lru_cache(maxsize=None)
def ls_case(m, c, rps, with_rs):
    seed = 4000 + 13 * m + c
    return dict(x=ints((m, c), -4, 4, seed), y2=ints((m, c), -4, 4, seed + 1), dy=ints((m, c), -4, 4, seed + 2),
                ls=ints((c,), -3, 3, seed + 3), rs=ints((-(-m // rps),), 0, 2, seed + 4) if with_rs else None,
                base_ls=ints((c,), -3, 3, seed + 5), base_b2=ints((c,), -3, 3, seed + 6))


def ls_ref(m, c, rps, with_rs, accumulate, dtype=torch.float64):
    """dict(out = resid_scale, dy2, d_ls, d_b2) of out = x + r[m // rps] * (ls * y2), by autograd."""
    k = ls_case(m, c, rps, with_rs)
    r = (k["rs"].to(dtype).repeat_interleave(rps)[:m] if with_rs else torch.ones(m, dtype=dtype)).view(-1, 1)
    ls = leaf(k["ls"], dtype)
    b2 = torch.zeros(c, dtype=dtype, requires_grad=True)
    y2 = leaf(k["y2"], dtype)
    out = k["x"].to(dtype) + r * (ls * (y2 + b2))
    out.backward(k["dy"].to(dtype))
    d_ls, d_b2 = ls.grad, b2.grad
    if accumulate:
        d_ls, d_b2 = d_ls + k["base_ls"].to(dtype), d_b2 + k["base_b2"].to(dtype)
    return dict(out=out.detach(), dy2=y2.grad, d_ls=d_ls, d_b2=d_b2)


LN_EPS = 1e-6


@functools.lru_cache(maxsize=None)
def ln_case(m, c):
    """z = 0.5 + 2 randn, gamma = 1 + 0.1 randn (float32 values); dt integers, so d_beta is exact."""
    seed = 5000 + 17 * m + c
    return dict(z=randn((m, c), seed, 2.0, 0.5), dt=ints((m, c), -4, 4, seed + 1), gamma=randn((c,), seed + 2, 0.1, 1.0),
                base_g=ints((c,), -3, 3, seed + 3), base_b=ints((c,), -3, 3, seed + 4))


def ln_ref(m, c, accumulate, dtype=torch.float64):
    """dict(dz, d_gamma, d_beta) by autograd through F.layer_norm (eps 1e-6)."""
    k = ln_case(m, c)
    z, gamma = leaf(k["z"], dtype), leaf(k["gamma"], dtype)
    beta = torch.zeros(c, dtype=dtype, requires_grad=True)
    F.layer_norm(z, (c,), gamma, beta, LN_EPS).backward(k["dt"].to(dtype))
    dg, db = gamma.grad, beta.grad
    if accumulate:
        dg, db = dg + k["base_g"].to(dtype), db + k["base_b"].to(dtype)
    return dict(dz=z.grad, d_gamma=dg, d_beta=db)


# (rtol, atol) of the inexact outputs: the sibling tests' own (test_gpu_backward.py, test_gpu_resnet_train.py)
TOL = {
    "ln_dz": (1e-4, 1e-5),
    "head": (2e-4, 1e-6),
    "bn_apply": (1e-5, 2e-5),
    "bn_dx": (1e-4, 1e-5),              # atol times max |dx|
    "bn_stats": (1e-5, 1e-6),           # mean, invstd and the running statistics
    "gelu": (1e-6, 1e-6),
    "colsum_rtol": 1e-4,                # d_gamma of LN and BN, with colsum_atol(M)
    "large_mean": 1e-3,                 # invstd / running_var of the x = 1000 + randn row: torch's float32 variance
                                        # is 6e-8 off there, a one-pass E[x^2] - E[x]^2 0.15
}


def colsum_atol(m):
    """Column sums over M rows: the siblings' 1e-4 up to 1000 rows, a random walk's growth above."""
    return 1e-4 * max(1.0, (m / 1000.0) ** 0.5)


# ---------------------------------------------------------------------------------------------------
# depthwise 7x7
# ---------------------------------------------------------------------------------------------------
DWCONV_ROWS = [(1, 1, 1, 4), (2, 2, 3, 8), (1, 3, 8, 260), (1, 7, 7, 100), (2, 9, 11, 96)]     # (B, H, W, C)


@functools.lru_cache(maxsize=None)
def dw_case(b, h, w, c):
    seed = 6000 + 100 * b + 10 * h + w + c
    return dict(x=ints((b, h, w, c), -4, 4, seed), wt=ints((c, 1, 7, 7), -4, 4, seed + 1), bias=ints((c,), -3, 3, seed + 2),
                dz=ints((b, h, w, c), -4, 4, seed + 3), base_x=ints((b, h, w, c), -3, 3, seed + 4),
                base_w=ints((49, c), -3, 3, seed + 5), base_b=ints((c,), -3, 3, seed + 6))


def pack_dw(wt):
    """[C, 1, 7, 7] -> the kernels' [49, C]."""
    return wt.reshape(wt.shape[0], 49).t().contiguous()


def dw_ref(b, h, w, c, dtype=torch.float64):
    """dict(y = forward with bias, dx = base_x + input gradient, dw [49, C], db, and dw / db on their bases),
    NHWC, by autograd through F.conv2d(groups = C)."""
    k = dw_case(b, h, w, c)
    x, wt, bias = leaf(k["x"].permute(0, 3, 1, 2), dtype), leaf(k["wt"], dtype), leaf(k["bias"], dtype)
    y = F.conv2d(x, wt, bias, padding=3, groups=c)
    y.backward(k["dz"].to(dtype).permute(0, 3, 1, 2))
    dw, db = pack_dw(wt.grad), bias.grad
    return dict(y=y.detach().permute(0, 2, 3, 1), dx=k["base_x"].to(dtype) + x.grad.permute(0, 2, 3, 1), dw=dw, db=db,
                dw_acc=dw + k["base_w"].to(dtype), db_acc=db + k["base_b"].to(dtype))


# ---------------------------------------------------------------------------------------------------
# max-pool head backward
# ---------------------------------------------------------------------------------------------------
HEAD_WIDTHS = [4, 100, 260, 768, 1000, 2048]         # on a 3 x 5 map, two images per view
HEAD_MAP = (3, 5)
HEAD_SWEEP = (2, 42, 50, 8)                          # (Bh, H, W, P): 4200 pixel pairs, 4096 per grid sweep
HEAD_CLASSES = 5
HEAD_WEIGHTS = (5.0, 2.0, 2.0)                       # align, tanh, class
# (w_align, w_tanh, classifier term)
HEAD_MODES = {"align": (HEAD_WEIGHTS[0], 0.0, False), "tanh": (0.0, HEAD_WEIGHTS[1], False), "cls": (0.0, 0.0, True),
              "all": (HEAD_WEIGHTS[0], HEAD_WEIGHTS[1], True), "all_no_dout": (HEAD_WEIGHTS[0], HEAD_WEIGHTS[1], False)}
TIE_KINDS = ["first_last", "middle", "constant", "saturated"]
TIE_SHAPE = (1, 3, 5, 8)                             # (Bh, H, W, P)
TIE_MIDDLE = (5, 9)                                  # the two tied pixels of the "middle" fixture


@functools.lru_cache(maxsize=None)
def head_proto(bh, h, w, p, tie=None):
    """float32 proto NHWC [2 Bh, H, W, P] = softmax(3 randn) over P, or a tie fixture built from it in float32:
    first_last: every column's maximum copied to pixels 0 and HW - 1;  middle: a value above the maximum at
    pixels 5 and 9;  constant: every even prototype constant over the map;  saturated: softmax(40 randn),
    whose winners round to exactly 1.0f."""
    g = torch.Generator().manual_seed(7000 + 100 * bh + 10 * h + w + p)
    logits = torch.randn(2 * bh, h, w, p, generator=g)
    proto = torch.softmax(logits * (40.0 if tie == "saturated" else 3.0), dim=-1)
    cols = proto.view(2 * bh, h * w, p)
    top = cols.max(dim=1).values
    if tie == "first_last":
        cols[:, 0] = top
        cols[:, -1] = top
    elif tie == "middle":
        for i in TIE_MIDDLE:
            cols[:, i] = (top + 1.0) / 2.0
    elif tie == "constant":
        cols[:, :, 0::2] = 0.125
    return proto.contiguous()


@functools.lru_cache(maxsize=None)
def head_params(bh, p):
    g = torch.Generator().manual_seed(7500 + bh + p)
    return dict(w=torch.randn(HEAD_CLASSES, p, generator=g), ys=torch.randint(0, HEAD_CLASSES, (bh,), generator=g),
                mult=2.0)


def head_ref(bh, h, w, p, mode, tie=None, dtype=torch.float64):
    """dict(proto f32 NHWC, pooled f32, d_out f32 or None, w f32, d_logits NHWC ``dtype``).  The float32 proto is
    the leaf; g = d loss / d proto by autograd through adaptive_max_pool2d (the first maximum of a tie), the
    relu(W) classifier and the align / tanh terms, and d logits = y (g - <g, y>), the softmax backward."""
    w_align, w_tanh, cls = HEAD_MODES[mode]
    proto32 = head_proto(bh, h, w, p, tie)
    prm = head_params(bh, p)
    y = leaf(proto32.permute(0, 3, 1, 2), dtype)                              # NCHW leaf
    pooled = F.adaptive_max_pool2d(y, (1, 1)).flatten(1)
    out = pooled @ torch.relu(prm["w"].to(dtype)).t()
    pooled32 = pooled.detach().float()
    d_out = train_ref.d_out(out.detach().float(), prm["ys"], prm["mult"], True, HEAD_WEIGHTS[2]) if cls else None
    terms = train_ref.loss_terms(y, pooled, out, prm["ys"], prm["mult"])
    loss = w_align * align_term(y) + w_tanh * terms["tanh"]
    if cls:
        loss = loss + (out * d_out.to(dtype)).sum()
    (g,) = torch.autograd.grad(loss, y)
    yd = y.detach()
    d_logits = yd * (g - (g * yd).sum(dim=1, keepdim=True))
    return dict(proto=proto32, pooled=pooled32, d_out=d_out, w=prm["w"], d_logits=d_logits.permute(0, 2, 3, 1),
                g=g.permute(0, 2, 3, 1))


# ---------------------------------------------------------------------------------------------------
# BatchNorm (train mode) on rows [M, C]
# ---------------------------------------------------------------------------------------------------
BN_EPS, BN_MOMENTUM = 1e-5, 0.1
# (M, C, slabs G, residual, relu, running statistics, want_dx, want_masked)
BN_ROWS = [
    (2, 4, 1, False, False, True, False, True),              # no dx: with two rows xhat = +-1 and dx is the residue
                                                             # of a cancellation (torch float32 is 500 tolerances off)
    (3, 320, 1, True, True, True, True, False),              # 80 channel quads: the second workgroup is ragged
    (17, 128, 1, False, True, False, True, True),
    (784, 64, 3, True, False, True, True, True),
    (70000, 4, 17, True, True, False, True, False),          # G > 16: a finish lane takes two slabs
    (4161, 320, 65, False, False, True, True, True),         # G > 64: a second round of the finish loop; ragged
    (4200, 1024, 65, True, True, True, True, True),          # and 1 075 200 float4: a second elementwise sweep
    (65600, 256, 1024, False, True, False, True, False),     # the BN_GMAX clamp (65600 / 64 = 1025)
]
BN_LARGE_MEAN = (784, 64, 3)                                 # x = 1000 + randn
BN_ELEM_SWEEP = 4096 * 256                                   # float4 per sweep of the elementwise kernels


@functools.lru_cache(maxsize=None)
def bn_case(m, c, large_mean=False):
    seed = 8000 + 7 * m + c
    x = randn((m, c), seed, 1.0, 1000.0) if large_mean else randn((m, c), seed, 2.0, 0.7)
    g = torch.Generator().manual_seed(seed + 1)
    return dict(x=x, gamma=(torch.rand(c, generator=g) + 0.5).double(), beta=randn((c,), seed + 2),
                res=randn((m, c), seed + 3), dy=ints((m, c), -4, 4, seed + 4),
                rm=randn((c,), seed + 5), rv=(torch.rand(c, generator=g) + 0.5).double())


def bn_ref(m, c, residual, relu, large_mean=False, dtype=torch.float64, mask=None):
    """dict(mean, invstd, running_mean, running_var, y, dx, masked, d_gamma, d_beta) through F.batch_norm(training)
    and autograd.  The ReLU's backward is the mask y > 0 applied to dy, as the kernel takes it from the saved
    output; ``mask`` replaces this pass's own (the float32 pass is given the float64 one, so that a sign that
    differs at an output next to zero is not counted as a rounding error of the sums)."""
    k = bn_case(m, c, large_mean)
    x, gamma, beta = leaf(k["x"], dtype), leaf(k["gamma"], dtype), leaf(k["beta"], dtype)
    rm, rv = k["rm"].to(dtype).clone(), k["rv"].to(dtype).clone()
    pre = F.batch_norm(x, rm, rv, gamma, beta, training=True, momentum=BN_MOMENTUM, eps=BN_EPS)
    if residual:
        pre = pre + k["res"].to(dtype)
    y = torch.relu(pre.detach()) if relu else pre.detach()
    masked = k["dy"].to(dtype)
    if relu:
        masked = masked * ((y > 0) if mask is None else mask)
    pre.backward(masked)
    xd = x.detach()
    mean, var = xd.mean(0), xd.var(0, unbiased=False)
    return dict(mean=mean, invstd=(var + BN_EPS).rsqrt(), running_mean=rm, running_var=rv, y=y, dx=x.grad,
                masked=masked, d_gamma=gamma.grad, d_beta=beta.grad)


# ---------------------------------------------------------------------------------------------------
# the rest
# ---------------------------------------------------------------------------------------------------
GELU_N = 8192 * 256 * 4 + 4             # one float4 more than a full sweep of the capped grid
CLAMP_SIZES = [1, 255, 2 ** 20 + 3]
SCATTER_ROWS = [(2, 3, 5, 4, 3, 5, 1, False), (2, 3, 5, 4, 3, 5, 1, True), (1, 2, 3, 8, 4, 7, 3, True)]
#               (B, OH, OW, C, H, W, stride, accumulate)


def gelu_ref(x):
    return F.gelu(x)


def scatter_ref(b, oh, ow, c, h, w, s, accumulate, dtype=torch.float64):
    x, base = ints((b, oh, ow, c), -4, 4, 9000 + oh + c).to(dtype), ints((b, h, w, c), -3, 3, 9001 + h).to(dtype)
    out = base.clone() if accumulate else torch.zeros(b, h, w, c, dtype=dtype)
    out[:, 0:oh * s:s, 0:ow * s:s] += x
    return dict(x=x, base=base, out=out)


# ---------------------------------------------------------------------------------------------------
# operand checks of the wrappers
# ---------------------------------------------------------------------------------------------------
def bad_calls(K, z):
    """(name, call) pairs on the wrappers of ``K`` (count_pipnet_amd.kernels, handed in: this module does not
    import it), each with one operand of the wrong shape; z(*shape) makes a float32 tensor."""
    return [
        ("colsum transposed", lambda: K.colsum(z(8, 4).t())),
        ("colsum out", lambda: K.colsum(z(4, 8), out=z(4))),
        ("resid_scale branch", lambda: K.resid_scale(z(6, 8), z(6, 4), z(8), None, 1)),
        ("resid_scale ls", lambda: K.resid_scale(z(6, 8), z(6, 8), z(4), None, 1)),
        ("resid_scale row_scale", lambda: K.resid_scale(z(6, 8), z(6, 8), z(8), z(2), 2)),
        ("ls_backward y2", lambda: K.ls_backward(z(6, 8), z(5, 8), z(8), None, 1, z(8), z(8))),
        ("ls_backward ls", lambda: K.ls_backward(z(6, 8), z(6, 8), z(12), None, 1, z(8), z(8))),
        ("ls_backward d_ls", lambda: K.ls_backward(z(6, 8), z(6, 8), z(8), None, 1, z(4), z(8))),
        ("ls_backward d_b2", lambda: K.ls_backward(z(6, 8), z(6, 8), z(8), None, 1, z(8), z(4))),
        ("ls_backward row_scale", lambda: K.ls_backward(z(50, 8), z(50, 8), z(8), z(3), 16, z(8), z(8))),
        ("ln_backward dt", lambda: K.ln_backward(z(6, 8), z(6, 4), z(8), z(8), z(8))),
        ("ln_backward gamma", lambda: K.ln_backward(z(6, 8), z(6, 8), z(4), z(8), z(8))),
        ("ln_backward d_gamma", lambda: K.ln_backward(z(6, 8), z(6, 8), z(8), z(4), z(8))),
        ("ln_backward d_beta", lambda: K.ln_backward(z(6, 8), z(6, 8), z(8), z(8), z(16))),
        ("dwconv7_plain weight", lambda: K.dwconv7_plain(z(1, 3, 3, 8), z(49, 4), None)),
        ("dwconv7_plain bias", lambda: K.dwconv7_plain(z(1, 3, 3, 8), z(49, 8), z(4))),
        ("dwconv7_plain out", lambda: K.dwconv7_plain(z(1, 3, 3, 8), z(49, 8), None, out=z(1, 3, 2, 8))),
        ("dwconv7_wgrad dz", lambda: K.dwconv7_wgrad(z(1, 3, 2, 8), z(1, 3, 3, 8), z(49, 8), z(8))),
        ("dwconv7_wgrad dw", lambda: K.dwconv7_wgrad(z(1, 3, 3, 8), z(1, 3, 3, 8), z(48, 8), z(8))),
        ("dwconv7_wgrad db", lambda: K.dwconv7_wgrad(z(1, 3, 3, 8), z(1, 3, 3, 8), z(49, 8), z(4))),
        ("wgrad_conv2x2 dy", lambda: K.wgrad_conv2x2(z(1, 3, 3, 8), z(1, 5, 6, 4), 1, z(8, 16))),
        ("wgrad_conv2x2 out", lambda: K.wgrad_conv2x2(z(1, 4, 5, 8), z(1, 5, 6, 4), 1, z(8, 8))),
        ("head_backward odd batch", lambda: K.head_backward(z(3, 1, 1, 16), z(3, 16), None, None, 1.0, 1.0)),
        ("head_backward pooled", lambda: K.head_backward(z(2, 1, 1, 16), z(2, 20), None, None, 1.0, 1.0)),
        ("head_backward w", lambda: K.head_backward(z(2, 1, 1, 16), z(2, 16), z(2, 5), z(5, 20), 1.0, 1.0)),
        ("head_backward d_out", lambda: K.head_backward(z(2, 1, 1, 16), z(2, 16), z(2, 4), z(5, 16), 1.0, 1.0)),
        ("bn_stats running_mean", lambda: K.bn_stats(z(8, 16), 1e-5, 0.1, z(8), z(16))),
        ("bn_stats one running", lambda: K.bn_stats(z(8, 16), 1e-5, 0.1, z(16), None)),
        ("bn_apply mean", lambda: K.bn_apply(z(8, 16), z(8), z(16), z(16), z(16))),
        ("bn_apply invstd", lambda: K.bn_apply(z(8, 16), z(16), z(8), z(16), z(16))),
        ("bn_apply gamma", lambda: K.bn_apply(z(8, 16), z(16), z(16), z(8), z(16))),
        ("bn_apply beta", lambda: K.bn_apply(z(8, 16), z(16), z(16), z(16), z(8))),
        ("bn_apply residual", lambda: K.bn_apply(z(8, 16), z(16), z(16), z(16), z(16), residual=z(4, 16))),
        ("bn_backward dy", lambda: K.bn_backward(z(8, 16), z(8, 8), z(16), z(16), z(16))),
        ("bn_backward mean", lambda: K.bn_backward(z(8, 16), z(8, 16), z(8), z(16), z(16))),
        ("bn_backward gamma", lambda: K.bn_backward(z(8, 16), z(8, 16), z(16), z(16), z(32))),
        ("bn_backward relu_out", lambda: K.bn_backward(z(8, 16), z(8, 16), z(16), z(16), z(16), relu_out=z(16, 8))),
        ("clamp_min_ strided", lambda: K.clamp_min_(z(8, 4).t(), 0.0)),
    ]
