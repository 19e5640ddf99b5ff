"""The first three kernels of csrc/explain.hip restated on the CPU (float64 torch / numpy), and the
seeded inputs of their GPU grid (tests/test_gpu_explain_matrix.py, tests/test_explain_ref_cpu.py;
tests/test_gpu_topk.py imports the helpers it used to define).

  two_step_loc     the reference's location rule as it writes it                (util/vis_pipnet.py:235-238)
  first_rank_loc   the same rule without torch.max's tie behaviour: the smallest w * H + h among the
                   pixels that equal the maximum
  located_pool     softmax + max-pool in float64 with the pixels that may hold the maximum
  topk_expected    the k best by (score descending, dataset index ascending)    (vis_pipnet.py:248-274)
  reference_lists  that loop replayed literally, one image at a time            (vis_pipnet.py:227-274 / :698-754)
  abstained        torch.amax(out, dim=1) == 0.                                 (vis_pipnet.py:217-219)

The case builders are lru_cached: an input or a reference is computed once, shared by the tests that
need it and never written to."""
import functools

import numpy as np
import torch

POOL_RTOL, POOL_ATOL = 1e-5, 1e-7        # POOLED_TOL[0] of tests/test_gpu_head_matrix.py
PIX_PER_BLOCK = 32                       # pixels of one workgroup of pool_argmax_kernel (head_common.hpp)
WAVES = 4                                # waves of a workgroup: wave w takes the pixels w, w + 4, ...


# ---- location ------------------------------------------------------------------------------
def two_step_loc(proto_nchw):
    """vis_pipnet.py:235-238 for every (image, prototype) of a CPU [B,P,H,W] map -> (h_idx, w_idx)."""
    max_h, h_idx = torch.max(proto_nchw, dim=2)          # over H: [B,P,W]
    _, w_idx = torch.max(max_h, dim=2)                   # over W: [B,P]
    return h_idx.gather(2, w_idx.unsqueeze(-1)).squeeze(-1), w_idx


def pixel_rank(h, w):
    """[h, w] int64: the column-first rank w_idx * h + h_idx of every pixel."""
    return torch.arange(w)[None, :] * h + torch.arange(h)[:, None]


def first_rank_loc(map_nhwc, skip_nan=False):
    """[B,H,W,P] (NHWC, the kernels' layout) -> loc [B,P] int64 = h_idx * W + w_idx of the pixel with the
    smallest rank w_idx * H + h_idx among those equal to the map's maximum.  A map in which no pixel
    equals the maximum (torch's amax of a map holding NaN is NaN) gives 0.  ``skip_nan``: the rule
    explain.hip documents for map_argmax -- NaN pixels are passed over, the maximum is that of the
    others (-inf when there are none)."""
    b, h, w, p = map_nhwc.shape
    x = map_nhwc.double()
    valid = ~torch.isnan(x) if skip_nan else torch.ones_like(x, dtype=torch.bool)
    xm = torch.where(valid, x, torch.full_like(x, -float("inf"))) if skip_nan else x
    hit = (xm == xm.amax(dim=(1, 2), keepdim=True)) & valid
    rank = torch.where(hit, pixel_rank(h, w)[None, :, :, None], torch.tensor(h * w)).amin(dim=(1, 2))
    w_idx = rank // h
    return torch.where(rank < h * w, (rank - w_idx * h) * w + w_idx, torch.zeros_like(rank))


def max_skip_nan(map_nhwc):
    """[B,H,W,P] -> float64 [B,P]: the maximum of the non-NaN pixels, -inf where every pixel is NaN."""
    x = map_nhwc.double()
    return torch.where(torch.isnan(x), torch.full_like(x, -float("inf")), x).amax(dim=(1, 2))


def located_pool(x):
    """x [B,H,W,P] float32 logits -> float64 (proto [B,H,W,P], pooled [B,P], tol [B,H,W,P], cand
    [B,H,W,P] bool).  tol = atol + rtol |proto| is what a float32 evaluation may be off by (the bound of
    tests/test_gpu_head_matrix.py); a pixel is a candidate for the location where its upper bound
    proto + tol reaches the maximum's lower bound (the scheme of head_ref.candidates)."""
    proto = torch.softmax(x.double(), dim=-1)
    pooled = proto.amax(dim=(1, 2))
    tol = POOL_ATOL + POOL_RTOL * proto
    top = pooled[:, None, None, :]
    return proto, pooled, tol, (proto + tol) >= (top - (POOL_ATOL + POOL_RTOL * top))


# ---- streaming top-k -----------------------------------------------------------------------
def topk_expected(score, loc, k, groups=None, g=0, min_score=None, i0=0):
    """score [n,P] float32, loc [n,P] int32 (numpy) -> (score [P,k] float32, index [P,k] int64, loc [P,k]
    int32): the k best of group ``g`` by (score descending, dataset index i0 + i ascending), padded with
    0 / -1 / -1.  ``groups`` [n] (None: every image in group 0): an image goes to the list of its id, so
    an id outside the lists asked for goes nowhere; ``min_score`` drops score < float32(min_score),
    a score equal to it stays.  No NaN scores: the reference's sort is undefined on them."""
    score, loc = np.asarray(score, np.float32), np.asarray(loc, np.int32)
    n, p = score.shape
    assert not np.isnan(score).any()
    in_g = np.full(n, g == 0) if groups is None else np.asarray(groups) == g
    out = np.broadcast_to(~in_g[:, None], (n, p)).copy()                            # True: not in this list
    if min_score is not None:
        out |= score < np.float32(min_score)
    idx = np.broadcast_to(np.arange(n)[:, None], (n, p))
    order = np.lexsort((idx, -score.astype(np.float64), out), axis=0)[:k]           # last key first
    kept = ~np.take_along_axis(out, order, axis=0)
    pad = k - order.shape[0]
    s = np.where(kept, np.take_along_axis(score, order, axis=0), np.float32(0))
    i = np.where(kept, order.astype(np.int64) + np.int64(i0), np.int64(-1))
    l = np.where(kept, np.take_along_axis(loc, order, axis=0), np.int32(-1))
    s, i, l = (np.pad(a, ((0, pad), (0, 0)), constant_values=c) for a, c in ((s, 0), (i, -1), (l, -1)))
    return (np.ascontiguousarray(s.T, np.float32), np.ascontiguousarray(i.T, np.int64),
            np.ascontiguousarray(l.T, np.int32))


def reference_lists(outputs, k, protos, min_score=None, groups=None):
    """The reference loop (vis_pipnet.py:227-274 / :698-754), one image at a time on CPU copies of a
    forward's outputs: outputs[i] = (proto [1,P,H,W], pooled [1,P], out [1,K]); groups[i] selects the
    list an image goes to.  Returns ({(p, group): [(score, index, h_idx, w_idx), ...]}, abstained)."""
    lists, abstained = {}, 0
    for i, (proto, pooled, out) in enumerate(outputs):
        if torch.amax(out, dim=1)[0].item() == 0.0:
            abstained += 1
        for p in protos:
            score = pooled.squeeze(0)[p].item()
            if min_score is not None and score < min_score:
                continue
            fmap = proto.squeeze(0)[p]
            max_h, h_idx = torch.max(fmap, dim=0)
            _, w_idx = torch.max(max_h, dim=0)
            item = (score, i, h_idx[w_idx].item(), w_idx.item())
            lst = lists.setdefault((p, None if groups is None else groups[i]), [])
            if len(lst) < k:
                lst.append(item)
                lst.sort(key=lambda t: t[0], reverse=True)
            elif score > lst[-1][0]:
                lst[-1] = item
                lst.sort(key=lambda t: t[0], reverse=True)
    return lists, abstained


def abstained(out):
    """out [B,K] float32 logits -> [B] bool: torch.amax(out, dim=1) == 0. of the reference, NaN
    propagating through amax as torch does (NaN == 0 is False)."""
    return torch.amax(out, dim=1) == 0.


# ---- sentinel frames -----------------------------------------------------------------------
FRAME_BYTE = 0xA5


class Framed:
    """A contiguous view of ``shape`` / ``dtype`` (float32, int32, int64: backbone_bwd_ref.Framed holds
    float32 only) in the middle of a buffer of 0xA5 bytes, ``frame`` elements wide on either side."""

    def __init__(self, shape, dtype, device, frame=64, base=None):
        shape = tuple(shape)
        n = int(np.prod(shape)) if shape else 1
        self.isz = torch.empty((), dtype=dtype).element_size()
        frame = -(-frame // 4) * 4                       # keeps the view 16-byte aligned
        self.lo, self.hi = frame * self.isz, (frame + n) * self.isz
        assert frame >= 4
        self.buf = torch.full((self.hi + self.lo,), FRAME_BYTE, device=device, dtype=torch.uint8)
        self.view = self.buf[self.lo:self.hi].view(dtype).view(shape)
        assert self.view.data_ptr() % 16 == 0 and self.view.is_contiguous()
        if base is not None:
            self.view.copy_(base.to(device=device, dtype=dtype))

    def fill_bytes(self, byte):
        self.buf[self.lo:self.hi] = byte
        return self

    def intact(self):
        """True when every byte outside the view still holds the sentinel."""
        return bool((self.buf[:self.lo] == FRAME_BYTE).all()) and bool((self.buf[self.hi:] == FRAME_BYTE).all())


# ---- (a) pool_argmax: the grid and its planted pixels ----------------------------------------
# (P, H, W): P at both edges of every nj_bucket (NJ = 1, 2, 4, 8, 12, 16, 32)
POOL_ROWS = [
    (1, 1, 1),           # NJ 1: one lane of one wave busy, HW = 1
    (63, 1, 9),          # NJ 1: H = 1
    (64, 9, 1),          # NJ 1: W = 1
    (65, 5, 7),          # NJ 2: two workgroups
    (128, 7, 5),         # NJ 2: H > W
    (129, 6, 6),         # NJ 4
    (256, 4, 8),         # NJ 4: exactly one full pixel block
    (257, 8, 4),         # NJ 8
    (512, 13, 13),       # NJ 8: six workgroups
    (513, 3, 11),        # NJ 12: 33 pixels, a second block of one pixel
    (768, 11, 3),        # NJ 12
    (769, 8, 9),         # NJ 16
    (1024, 2, 17),       # NJ 16
    (1025, 17, 2),       # NJ 32
    (2048, 7, 7),        # NJ 32 full: 64 KiB of LDS
]
POOL_B = 2
SATURATED, DEAD = 40.0, -200.0


def planted_pixels(h, w):
    """Three pixels (h_idx, w_idx) that get one logit vector, for maps of at least four pixels: flat pixel
    1, the first pixel of row 1 and the last pixel.  On a map with H, W > 1 the column-first winner is
    (1, 0), not the flat-first (0, 1); the last pixel lies in another workgroup than both wherever the
    map has more than one (HW > 32), else in another wave.  With H = 1 or W = 1 rank and flat order are
    the same order: flat pixels 1, 2 and the last, in three waves, and the winner is flat pixel 1."""
    assert h * w >= 4
    if h == 1 or w == 1:
        flat = [1, 2, h * w - 1]
        return [(f // w, f % w) for f in flat]
    return [(0, 1), (1, 0), (h - 1, w - 1)]


@functools.lru_cache(maxsize=None)
def pool_case(p, h, w):
    """One row of the grid: dict(x [2,h,w,p] float32 = 3 randn (seed 1000 + p) with the planted pixels,
    proto / pooled / tol / cand of located_pool, planted = {channel: (pooled value, loc)} judged
    exactly, free = [p] bool, the channels judged by candidates).

    Planted where HW >= 4: one vector (3 randn, channel p - 1 at +40: softmax exactly 1.0f) at the three
    planted_pixels -- an exact tie of every channel there, decided for channel p - 1; channel p // 2 at
    -200 in every pixel: softmax exactly 0.0f, pooled 0, location (0, 0)."""
    g = torch.Generator().manual_seed(1000 + p)
    x = torch.randn(POOL_B, h, w, p, generator=g) * 3
    planted = {}
    if h * w >= 4:
        sat, dead = p - 1, p // 2
        row = torch.randn(p, generator=g) * 3
        row[sat] = SATURATED
        pix = planted_pixels(h, w)
        for hh, ww in pix:
            x[:, hh, ww] = row
        x[..., dead] = DEAD
        win = min(pix, key=lambda t: t[1] * h + t[0])
        planted = {sat: (1.0, win[0] * w + win[1]), dead: (0.0, 0)}
    free = torch.ones(p, dtype=torch.bool)
    free[list(planted)] = False
    proto, pooled, tol, cand = located_pool(x)
    return dict(x=x, proto=proto, pooled=pooled, tol=tol, cand=cand, planted=planted, free=free)


@functools.lru_cache(maxsize=None)
def ones_case():
    """P = 1 on a 5 x 7 map: the softmax of one channel is exactly 1.0 in every pixel of both
    workgroups; pooled 1, location (0, 0)."""
    return torch.randn(POOL_B, 5, 7, 1, generator=torch.Generator().manual_seed(57)) * 3


# ---- (b) map_argmax --------------------------------------------------------------------------
MAP_P = [1, 63, 64, 65, 128, 129, 2048]
MAP_HW = [(1, 1), (1, 3), (3, 1), (5, 7), (7, 5), (16, 16), (2, 9)]      # (1,3), (3,1): a wave without a pixel
MAP_ROWS = [(p, *MAP_HW[i]) for i, p in enumerate(MAP_P)]
MAP_KINDS = ["random", "negative", "sparse", "constant", "neg_inf", "pos_inf"]
INF = float("inf")


@functools.lru_cache(maxsize=None)
def map_case(p, h, w, kind):
    """[B,h,w,p] float32 NHWC map of one kind; B = 3 at P = 2048, else 2."""
    b = 3 if p == 2048 else 2
    g = torch.Generator().manual_seed(17 + 31 * p + h + 7 * (MAP_KINDS + ["nan"]).index(kind))
    if kind == "random":                                   # any sign
        return torch.randn(b, h, w, p, generator=g)
    if kind == "negative":
        return -torch.rand(b, h, w, p, generator=g) - 0.5
    if kind == "sparse":                                   # the CountPIPNet 0/1 map
        m = (torch.rand(b, h, w, p, generator=g) < 0.1).float()
        m[0, :, :, 0] = 0.0                                # an all-zero map: value 0 at (0, 0)
        m[1, :, :, p - 1] = 0.0
        m[1, h - 1, w - 1, p - 1] = 1.0                    # a single 1 at the last pixel
        return m
    if kind == "constant":                                 # every pixel ties: (0, 0)
        return torch.randn(b, 1, 1, p, generator=g).expand(b, h, w, p).contiguous()
    if kind == "neg_inf":
        return torch.full((b, h, w, p), -INF)
    if kind == "pos_inf":                                  # ties at +inf
        m = torch.randn(b, h, w, p, generator=g)
        m[torch.rand(b, h, w, p, generator=g) < 0.15] = INF
        return m
    assert kind == "nan"
    m = torch.randn(b, h, w, p, generator=g)
    m[torch.rand(b, h, w, p, generator=g) < 0.3] = float("nan")
    m[0, :, :, 0] = float("nan")                           # all NaN: (-inf, 0)
    if p > 1 and h * w > 1:
        m[1, :, :, 1] = -INF                               # NaN at the first pixel, -inf elsewhere: the first -inf
        m[1, 0, 0, 1] = float("nan")
    return m


# ---- (c) topk_update -------------------------------------------------------------------------
TOPK_N = 70
LEVELS = [0.0, 0.1, 0.25, 0.5, 1.0]
MIN_AT = 0.25                                                        # a score level: scores equal to it stay
MIN_BELOW = float(np.nextafter(np.float32(0.25), np.float32(0)))     # one float below it
I0S = [0, 2 ** 31 - 3, 2 ** 40]                                      # the second crosses int32 inside a batch
TOPK_SPLITS = {"ones": [1] * 70, "sevens": [7] * 10, "eights": [8] * 8 + [6], "nines": [9] * 7 + [7], "whole": [70]}
TOPK_KINDS = ["levels", "continuous", "negative", "zeros", "inf"]
# (P, G, k, kind, i0, min_score): G * P a multiple of 64 at (64, 1), (64, 5), (768, 1), (768, 5), (2048, 1),
# (2048, 3); every P, G, k, kind, i0 occurs; k = 32 meets P = 2048 and G = 3.
TOPK_ROWS = [
    (1, 1, 1, "levels", 0, None),
    (1, 3, 10, "continuous", 2 ** 40, None),
    (63, 3, 2, "continuous", 2 ** 31 - 3, None),
    (63, 1, 31, "levels", 2 ** 40, MIN_AT),
    (64, 1, 10, "negative", 2 ** 40, None),
    (64, 5, 2, "levels", 2 ** 31 - 3, MIN_BELOW),
    (65, 5, 31, "zeros", 0, None),
    (65, 3, 1, "inf", 2 ** 31 - 3, None),
    (65, 1, 32, "levels", 0, MIN_AT),
    (768, 1, 32, "inf", 2 ** 31 - 3, None),
    (768, 5, 10, "levels", 0, MIN_BELOW),
    (2048, 1, 1, "negative", 0, None),
    (2048, 3, 32, "levels", 2 ** 40, MIN_AT),
]


@functools.lru_cache(maxsize=None)
def topk_inputs(n, p, kind, groups):
    """(score [n,p] float32, loc [n,p] int32 in [0, 64), group [n] int32 in [-1, groups] or None where
    ``groups`` is 0).  Ids -1 and ``groups`` are outside the lists: those images are skipped."""
    g = torch.Generator().manual_seed(n * 131 + p * 7 + TOPK_KINDS.index(kind) + 1000 * groups)
    lv = torch.tensor(LEVELS)[torch.randint(0, 5, (n, p), generator=g)]
    if kind == "levels":                                   # five tied levels
        score = lv
    elif kind == "continuous":
        score = torch.rand(n, p, generator=g)
    elif kind == "negative":                               # tied levels below zero: the 0.0 of an empty slot is larger
        score = -lv - 0.125
    elif kind == "zeros":                                  # +0.0 and -0.0 tie; a few scores above them
        score = torch.where(torch.rand(n, p, generator=g) < 0.5, torch.tensor(0.0), torch.tensor(-0.0))
        score = torch.where(torch.rand(n, p, generator=g) < 0.1, lv, score)
    else:                                                  # ties at +inf
        score = torch.where(torch.rand(n, p, generator=g) < 0.1, torch.tensor(INF), lv)
    loc = torch.randint(0, 64, (n, p), generator=g, dtype=torch.int32)
    group = None
    if groups:
        group = torch.randint(-1, groups + 1, (n,), generator=g, dtype=torch.int32)
        group[0], group[n // 2] = -1, groups               # both kinds of id without a list occur
    return score, loc, group


@functools.lru_cache(maxsize=None)
def topk_case(p, n_groups, k, kind, i0, min_score, n=TOPK_N):
    """One row: dict(score, loc, group (None at G = 1 with an even k), expected = [per group (score,
    index, loc)], fill [G,P])."""
    score, loc, group = topk_inputs(n, p, kind, 0 if n_groups == 1 and k % 2 == 0 else n_groups)
    gnp = None if group is None else group.numpy()
    expected = [topk_expected(score.numpy(), loc.numpy(), k, gnp, gi, min_score, i0) for gi in range(n_groups)]
    fill = np.stack([(e[1] >= 0).sum(axis=1) for e in expected]).astype(np.int32)
    return dict(score=score, loc=loc, group=group, expected=expected, fill=fill)


ABSTAIN_K = [1, 9, 64, 65, 200, 1000]
ABSTAIN_B = [1, 7, 8, 9, 17]
ABSTAIN_KINDS = ["zero", "neg_zero", "subnormal", "negative", "nan", "positive"]
SUBNORMAL = float(np.float32(2.0 ** -149))


@functools.lru_cache(maxsize=None)
def abstain_case(b, k, shift):
    """out [b,k] float32: negative logits, row r made the kind (r + shift) % 6 with its decisive entry
    in the last column (behind the first 64 wherever K > 64):
      zero       maximum +0.0                                          abstained
      neg_zero   maximum -0.0                                          abstained
      subnormal  maximum 2^-149 beside a +0.0                          not abstained
      negative   every logit below zero                                not abstained
      nan        zeros and one NaN (amax is NaN)                       not abstained
      positive   one logit above zero                                  not abstained"""
    g = torch.Generator().manual_seed(b * 1009 + k * 13 + shift)
    out = -torch.rand(b, k, generator=g) - 0.1
    for r in range(b):
        kind = ABSTAIN_KINDS[(r + shift) % 6]
        if kind == "zero":
            out[r, k - 1] = 0.0
        elif kind == "neg_zero":
            out[r, k - 1] = -0.0
        elif kind == "subnormal":
            out[r, 0] = 0.0
            out[r, k - 1] = SUBNORMAL
        elif kind == "nan":
            out[r] = 0.0
            out[r, k - 1] = float("nan")
        elif kind == "positive":
            out[r, k - 1] = 0.5
    return out
