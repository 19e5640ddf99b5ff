"""The inference heads restated in float64 torch on the CPU, and the seeded inputs of their GPU
grids (tests/test_gpu_head_matrix.py, tests/test_gpu_eval_matrix.py, tests/test_head_ref_cpu.py).

Each function restates one module path in the kernels' own layout (NHWC maps, [B, P] rows); inputs
are the float32 (or bf16) values the kernel reads, widened -- nothing is rounded to float32 on the
way.  tests/test_head_ref_cpu.py pins every one of them to the module it restates:

  softmax_pool    nn.Softmax(dim=1) + AdaptiveMaxPool2d(1) / spatial sum            (pipnet.py:33-34)
  nonneg_linear   where(x < 0.1, 0, x) of PIPNet.forward(inference=True) + NonNegLinear (pipnet.py:36-37, 70-71)
  hard_head       GumbelSoftmax(...).eval() on an injected draw                     (count_pipnet_utils.py:7-38)
  count_finish    STE_Round + ClampSTE forwards                                     (count_pipnet.py:90-97)
  count_encode    create_modified_encoding / LinearIntermediate forwards            (count_pipnet_utils.py)

The case builders are lru_cached: a reference is computed once, shared by the tests that need it
and never written to."""
import functools

import torch

F32_EPS = 2.0 ** -24          # unit roundoff of float32


# ---- references ----------------------------------------------------------------------------
def softmax_pool(x, mode):
    """x [B, h, w, P] float32 / bf16 logits -> float64 (proto [B, h, w, P], pooled [B, P]);
    mode 0 = max over the pixels, 1 = their sum."""
    proto = torch.softmax(x.double(), dim=-1)
    flat = proto.reshape(proto.shape[0], -1, proto.shape[-1])
    return proto, (flat.amax(dim=1) if mode == 0 else flat.sum(dim=1))


def nonneg_linear(x, w, bias, thresh):
    """x [B, D], w [K, D], bias [K] or None, all float32 -> float64 (x', out, abs_sum): x' = x with
    the entries below float32(thresh) zeroed (thresh None: x), out = x' relu(w)^T + bias, and
    abs_sum = |x'| relu(w)^T, the magnitude a summation-error bound scales with.  The comparison
    is the module's: a float32 tensor against the float32 value of the scalar."""
    xd = x.double()
    if thresh is not None:
        xd = torch.where(x < torch.tensor(thresh, dtype=torch.float32), torch.zeros_like(xd), xd)
    wp = torch.relu(w.double())
    out = xd @ wp.t()
    if bias is not None:
        out = out + bias.double()
    return xd, out, xd.abs() @ wp.t()


def hard_head(x, log_e, tau):
    """x [B, h, w, P] float32 logits, log_e float64 log of the Exp(1) draw in the same layout ->
    (z = (x - log_e) / tau, top = first argmax over the channels, tol): tol = 1e-6 (1 + |x| +
    |log_e|) / tau is the per-element allowance for the kernel's three float32 roundings (log,
    subtract, scale by 1 / tau), some 8 float32 ulps of the larger operand."""
    xd = x.double()
    z = (xd - log_e) / tau
    tol = 1e-6 * (1 + xd.abs() + log_e.abs()) / tau
    return z, first_argmax(z), tol


def first_argmax(z):
    """Lowest index of the maximum over the last dimension (written out: no reliance on a tie
    rule of torch.argmax)."""
    p = z.shape[-1]
    idx = torch.arange(p).expand(z.shape)
    return torch.where(z == z.amax(dim=-1, keepdim=True), idx, torch.full_like(idx, p)).amin(dim=-1)


def candidates(z, tol, top):
    """[..., P] bool: the channels whose upper bound z + tol reaches the top's lower bound."""
    z_top = torch.gather(z, -1, top[..., None])
    tol_top = torch.gather(tol, -1, top[..., None])
    return (z + tol) >= (z_top - tol_top)


def round_half_even(c):
    """torch.round on float64 values, written out."""
    f = torch.floor(c)
    d = c - f
    up = (d > 0.5) | ((d == 0.5) & (torch.remainder(f, 2.0) == 1.0))
    return f + up.to(c.dtype)


def count_finish(values, max_count, do_round):
    """values [B, P] (int32 histogram or float32 sums) -> float64 (raw, clamped): raw = the values
    as float32, clamped = clamp(round half to even (raw), 0, max_count) (no rounding without
    ``do_round``)."""
    raw = values.float().double()
    r = round_half_even(raw) if do_round else raw
    return raw, r.clamp(0.0, float(max_count))


def count_encode(x, c, kind, do_round, w=None):
    """x [B, P] float32 counts -> float64 [B, P * c] (prototype-major).  kind 0: one-hot at
    clamp(trunc(v) - 1, 0, c - 1) where v > float32(0.1), v = the (rounded) count; kind 1:
    x[..., None] * w with w [c] (exact: a product of two float32 fits float64)."""
    v = x.double()
    if kind == 1:
        return (v[..., None] * w.double()).reshape(x.shape[0], -1)
    if do_round:
        v = round_half_even(v)
    present = v > float(torch.tensor(0.1, dtype=torch.float32))
    slot = (torch.trunc(v) - 1).clamp(0, c - 1).long()
    enc = torch.zeros(*x.shape, c, dtype=torch.float64)
    enc.scatter_(2, slot[..., None], present.double()[..., None])
    return enc.reshape(x.shape[0], -1)


# ---- seeded inputs -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pool_case(b, hw, p, bf16=False):
    """(logits [b, 1, hw, p] float32 or bf16 = 4 randn, float64 proto, pooled max, pooled sum)."""
    x = torch.randn(b, 1, hw, p, generator=torch.Generator().manual_seed(b * 1000 + hw * 7 + p)) * 4
    if bf16:
        x = x.to(torch.bfloat16)
    proto, pmax = softmax_pool(x, 0)
    return x, proto, pmax, softmax_pool(x, 1)[1]


THRESH = 0.1
AT_THRESH = torch.tensor(THRESH, dtype=torch.float32)
BELOW_THRESH = torch.nextafter(AT_THRESH, torch.tensor(0.0))


@functools.lru_cache(maxsize=None)
def linear_case(b, d, k):
    """(x [b, d] in [0, 0.3) with every 7th element exactly float32(0.1) and, three further on, the
    float just below it; w [k, d] = randn; bias [k] = randn)."""
    g = torch.Generator().manual_seed(b * 100003 + d * 17 + k)
    x = torch.rand(b, d, generator=g) * 0.3
    flat = x.view(-1)
    flat[0::7] = AT_THRESH
    flat[3::7] = BELOW_THRESH
    return x, torch.randn(k, d, generator=g), torch.randn(k, generator=g)


@functools.lru_cache(maxsize=None)
def encode_counts(c, b, p):
    """[b, p] float32 counts cycling through 0, 0.1, the float above 0.1, 2.9, c, c + 2, 0.5, 1.5
    (the last two round to even)."""
    at = torch.tensor(0.1)
    vals = torch.stack([torch.tensor(0.0), at, torch.nextafter(at, torch.tensor(1.0)), torch.tensor(2.9),
                        torch.tensor(float(c)), torch.tensor(c + 2.0), torch.tensor(0.5), torch.tensor(1.5)])
    return vals.repeat(b * p // len(vals) + 1)[:b * p].view(b, p).contiguous()


@functools.lru_cache(maxsize=None)
def finish_values(b, p):
    """[b, p] float32 sums cycling through negatives, the exact .5 ties 0.5, 1.5, 2.5, -0.5, 3.5, the
    floats adjacent to each, and values above every max_count of the grid."""
    base = torch.tensor([-2.0, -0.5, 0.0, 0.1, 0.5, 1.5, 2.5, 3.5, 2.9, 3.0, 7.49, 9.0, 6.5, 7.5])
    lo, hi = torch.tensor(-1e9), torch.tensor(1e9)
    vals = torch.cat([base, torch.nextafter(base, lo), torch.nextafter(base, hi)])
    return vals.repeat(b * p // len(vals) + 1)[:b * p].view(b, p).contiguous()


# (B, HW, P, tau) of the hard Gumbel head: the smallest shape that reaches each branch
GUMBEL_GRID = [
    (2, 1, 4, 1.0),        # bucket 1: one lane, one pixel, three idle waves
    (2, 17, 16, 1.0),      # bucket 1: the second workgroup holds one pixel (ragged block, prefetch guard)
    (2, 15, 100, 0.5),     # bucket 2: partly filled workgroup, lanes >= 25 idle
    (1, 33, 128, 2.0),     # bucket 2: its upper edge, a third workgroup of one pixel
    (2, 37, 260, 2.0),     # bucket 8 / NJ4 = 2: the second chunk holds one lane
    (1, 16, 512, 0.1),     # bucket 8 full, one full workgroup
    (1, 16, 768, 1.0),     # bucket 12 / NJ4 = 3
    (3, 33, 1000, 0.5),    # bucket 16 / NJ4 = 4, ragged last chunk
    (1, 17, 1028, 0.5),    # bucket 32 / NJ4 = 8 with chunks 5..7 empty, the fifth holds one lane
    (1, 17, 2048, 0.5),    # bucket 32 full
    (2, 64, 2048, 1.0),    # C5's width, four workgroups per image
]
GUMBEL_EXTRA = [(2, 19, 132, 1.0), (2, 19, 256, 1.0)]      # bucket 4 (ceil(P / 64) = 3, 4), which the grid skips


@functools.lru_cache(maxsize=None)
def gumbel_logits(b, hw, p):
    """[b, hw, 1, p] float32 NHWC logits = 2 randn."""
    g = torch.Generator().manual_seed(b * 1000 + hw * 7 + p)
    return torch.randn(b, hw, 1, p, generator=g) * 2


@functools.lru_cache(maxsize=None)
def gumbel_case(b, hw, p, tau):
    """Injected-noise case of one grid row: dict(x NHWC logits, e float32 NCHW Exp(1) draw, z, top,
    tol, cand [b, hw, 1, p], single [b, hw, 1] = exactly one candidate)."""
    x = gumbel_logits(b, hw, p)
    g = torch.Generator().manual_seed(77 + b * 1000 + hw * 7 + p)
    e = torch.empty(b, p, hw, 1).exponential_(generator=g)
    return dict(x=x, e=e, **judge(x, e.double().log().permute(0, 2, 3, 1), tau))


def judge(x, log_e, tau):
    """hard_head and its candidate sets."""
    z, top, tol = hard_head(x, log_e, tau)
    cand = candidates(z, tol, top)
    return dict(z=z, top=top, tol=tol, cand=cand, single=cand.sum(-1) == 1)


TIE_ROWS = [(8, 1.0), (260, 0.5), (1000, 1.0), (2048, 0.5)]      # (P, tau)


@functools.lru_cache(maxsize=None)
def tie_case(p, tau):
    """Exact ties of the hard head: integer logits (background {0, 1}, the maximum 2 planted at two
    or more channels of every pixel), E = 1.  -> (x [2, hw, 1, p], first = lowest planted index
    [2, hw, 1]).  Per image, four pixels of every way the width allows -- the same lane (c, c + 1),
    two lanes of one 256-channel chunk, one lane in two chunks (c, c + 256), a lower lane holding the
    higher index (the cross-lane reduction must compare indices, not lanes), first and last channel,
    every channel -- so that 17+ pixels also cross a workgroup (16 pixels)."""
    g = torch.Generator().manual_seed(p)
    plants = []
    for r in range(4):
        c = 4 * ((5 * r + 3) % (p // 4))
        plants.append((c, c + 1))                                  # one lane, adjacent elements
        lo = (c // 256) * 256
        other = lo + (c - lo + 4 * (7 + r) + 2) % min(256, p - lo)
        if other // 4 != c // 4:
            plants.append((c + 3, other))                          # two lanes of one chunk
        if p > 256:
            c1 = 256 + (4 * (2 + r) + r) % min(p - 256, 200)       # second chunk, lane < 50
            plants.append((c1 - 256, c1))                          # one lane, two chunks
            plants.append((4 * (60 - r) + 1, c1))                  # lanes 57..60 hold the lower index
        if p > 512:
            last = ((p - 1) // 256) * 256
            cl = last + (4 * (3 + r) + 2) % (p - last)
            plants.append((cl - last, cl))                         # one lane, first and last chunk
        plants.append((0, p - 1))                                  # first and last channel
        plants.append(tuple(range(p)))                             # every channel
    hw = len(plants)
    x = torch.randint(0, 2, (2, hw, 1, p), generator=g).float()
    first = torch.empty(2, hw, 1, dtype=torch.long)
    for b in range(2):
        for i, chans in enumerate(plants[b:] + plants[:b]):        # image 1: the same ways, rotated
            x[b, i, 0, list(chans)] = 2.0
            first[b, i, 0] = min(chans)
    return x, first


# (B, P, K) of the eval-metric grid
EVAL_GRID = [
    (1, 4, 2),             # one image, one lane busy
    (5, 100, 3),           # K < 64, P < 256
    (64, 768, 200),        # C2's shape: K in every wave
    (300, 260, 257),       # B > 256 (eval_reduce_kernel's strided loop), K > 256, P = 256 + 4
    (3, 6144, 9),          # C5's shape
]
EVAL_THR = 1e-3
THR_F32 = torch.tensor(EVAL_THR, dtype=torch.float32)
ABOVE_THR = torch.nextafter(THR_F32, torch.tensor(1.0))
EVAL_BATCHES = 3


@functools.lru_cache(maxsize=None)
def eval_case(b, p, k):
    """Three synthetic eval batches of one row: dict(w [k, p] >= 0 sparse, batches = [(pooled, out,
    w, ys)] as oracle.ref_cpu.eval_loop takes them, planted = what was planted where).

    pooled in [0, 1] with ~70 % exact zeros, out = pooled w^T in float32 (at most ~30).  Planted:
      * threshold: prototype 0 has w[0, 0] = 1 and pooled = float32(1e-3) (the product equals the
        threshold: not counted) in image 0, the next float above it (counted) in image b - 1
        (b = 1: batches 0, 1 at the threshold, batch 2 above it);
      * prototypes per class: prototype 1 carries weight for class k - 1 only and is non-zero only
        in the last image of each batch (eval_class_kernel's early-exit scan must reach it);
      * abstain: image 0 of batch 1 has pooled = 0, so out = 0 (prediction 0, abstain counted);
      * argmax ties, written into ``out`` after the product (the kernel reads out, it does not
        recompute it): the row maximum + 1 duplicated at two indices of one wave (1, 2), at 3 and
        k - 1 and, for k >= 200, in two waves (3 and 70; 70 and 199, neither in wave 0), one pair
        per image from the last image down; ``planted['ties']`` lists (batch, image, first index).
    Labels run through the classes in turn: every class occurs wherever 3 b >= k (all rows but
    64 x 768 x 200, whose 192 images cannot)."""
    g = torch.Generator().manual_seed(b * 7919 + p * 31 + k)
    w = torch.rand(k, p, generator=g) * (torch.rand(k, p, generator=g) < 0.1).float()
    w *= min(1.0, 60.0 / max(1.0, 0.05 * p))          # keeps out = pooled w^T within the goldens' range
    w[:, :2] = 0.0
    w[0, 0] = 1.0
    w[k - 1, 1] = 0.5
    batches, ties = [], []
    for i in range(EVAL_BATCHES):
        pooled = torch.rand(b, p, generator=g) * (torch.rand(b, p, generator=g) < 0.3).float()
        pooled[:, 0] = 0.0
        if b > 1:
            pooled[0, 0], pooled[b - 1, 0] = THR_F32, ABOVE_THR
        else:
            pooled[0, 0] = ABOVE_THR if i == 2 else THR_F32
        pooled[:, 1] = 0.0
        pooled[b - 1, 1] = 0.75
        if i == 1:
            pooled[0] = 0.0
        out = pooled @ w.t()
        pairs = [(0, 1)] if k < 4 else [(1, 2), (3, k - 1)] + ([(3, 70), (70, 199)] if k > 199 else [])
        assert b >= len(pairs)
        for j, (a, c) in enumerate(pairs):
            img = b - 1 - j
            if i == 1 and img == 0:
                continue
            top = out[img].max() + 1.0
            out[img, a] = top
            out[img, c] = top
            ties.append((i, img, a))
        ys = (torch.arange(b) + i * b) % k
        batches.append((pooled, out, w, ys))
    return dict(w=w, batches=batches, planted=dict(ties=ties))
