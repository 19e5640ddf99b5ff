"""The CountPIPNet training-head kernels called directly, at every prototype width the launchers
branch on, against the float64 reference of tests/count_head_ref.py (GumbelSoftmax + spatial sum
+ STE_Round / ClampSTE + oracle.train_ref.loss_terms, gradients by autograd):

  count_gumbel_soft      count_gumbel_kernel<NJ, SOFT=true, NOISE=true|false>      (csrc/head.hip)
  count_head_backward    pool_grad_kernel + head_bwd_kernel<NJ4, SUM=true>         (csrc/backward_ops.hip)
  nonneg_linear_dx, bilinear_bwd_prep, train_loss on count inputs                  (csrc/train_ops.hip)
  and the chain hip_count_train_step composes from them.

Tolerances are those of the sibling tests of the max-pool head: proto rtol 1e-5 / atol 1e-7 and
sums rtol 1e-5 / atol 1e-6 (test_softmax_pool), d logits rtol 2e-4 / atol 1e-6
(test_head_backward_matches_autograd).  The same graph evaluated in torch float32 on the CPU stays
within 0.20 / 0.13 / 0.04 of them over the whole grid.  Every comparison prints its worst
error / tolerance ratio before it asserts (pytest -s)."""
import functools

import pytest
import torch

import count_head_ref as R
from count_pipnet_amd import kernels as K
from oracle import train_ref

pytestmark = pytest.mark.gpu

# (Bh, HW, P, tau): the smallest shape that reaches each branch; N = 2 Bh images
GRID = [
    (1, 1, 4, 1.0),        # one lane, one pixel, three idle waves
    (2, 17, 16, 1.0),      # the fixtures' width; the second workgroup holds one pixel (tail, prefetch guard)
    (1, 15, 100, 0.5),     # partly filled workgroup, lanes >= 25 idle
    (2, 37, 260, 2.0),     # bucket 8 / NJ4 = 2, the second chunk holds one lane
    (1, 16, 768, 1.0),     # bucket 12 / NJ4 = 3
    (3, 33, 1000, 0.5),    # bucket 16 / NJ4 = 4, ragged last chunk, odd half batch
    (1, 17, 2048, 0.5),    # bucket 32 / NJ4 = 8, full LDS
    (2, 64, 2048, 1.0),    # C5's width, 4 workgroups per image adding into sums
]
ROW_16, ROW_1000, ROW_2048, ROW_C5 = GRID[1], GRID[5], GRID[6], GRID[7]
PROTO_TOL = dict(rtol=1e-5, atol=1e-7)
SUMS_TOL = dict(rtol=1e-5, atol=1e-6)
DLOGITS_TOL = dict(rtol=2e-4, atol=1e-6)
W_ALIGN, W_TANH, W_CLASS = 5.0, 2.0, 2.0
MAX_COUNT = 3


def _close(what, got, want, rtol, atol):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got - want).abs()
    ratio = float((err / (atol + rtol * want.abs())).max()) if err.numel() else 0.0
    print(f"{what}: max |err| {float(err.max()):.3e}, worst err / tolerance {ratio:.3f}")
    torch.testing.assert_close(got, want, rtol=rtol, atol=atol, msg=lambda m: f"{what}: {m}")


def _tanh_coeff(bh, hw, p):
    """C with C * (half-batch count) of order 1: the tanh term neither vanishes nor swamps the rest."""
    return 0.5 * p / (bh * hw)


def _nchw(t_nhwc):
    return t_nhwc.permute(0, 3, 1, 2)


@functools.lru_cache(maxsize=None)
def _case(bh, hw, p, tau, seed=None):
    """Seeded inputs and the float64 head of one grid row, computed once: (logits, E, proto, counts)."""
    logits, e = R.draw_inputs(bh, hw, p, bh * 1000 + hw * 7 + p if seed is None else seed)
    proto, counts = R.soft_head(logits, e, tau)
    return logits, e, proto, counts


@functools.lru_cache(maxsize=None)
def _d_counts(bh, p):
    return torch.randn(2 * bh, p, generator=torch.Generator().manual_seed(77 + bh + p)) * 0.1


# ---- 1. soft Gumbel head, injected noise ---------------------------------------------------
@pytest.mark.parametrize("bh,hw,p,tau", GRID)
def test_count_gumbel_soft_injected_noise(gpu, bh, hw, p, tau):
    logits, e, proto, counts = _case(bh, hw, p, tau)
    ln, en = R.nhwc(logits).to(gpu), e.to(gpu)
    pr, sums = K.count_gumbel_soft(ln, tau, en, seed=0)
    assert pr.shape == ln.shape and sums.shape == (2 * bh, p)
    _close("proto", _nchw(pr), proto, **PROTO_TOL)
    _close("sums", sums, counts, **SUMS_TOL)
    _close("sums vs row sums of proto", sums, pr.double().sum(dim=(1, 2)), **SUMS_TOL)
    pr2, sums2 = K.count_gumbel_soft(ln, tau, en, seed=0)
    assert torch.equal(pr2, pr)
    _close("sums, second call", sums2, counts, **SUMS_TOL)          # zeroed per call, never accumulated


# ---- 2. soft Gumbel head, Philox noise -----------------------------------------------------
@pytest.mark.parametrize("bh,hw,p,tau", [ROW_16, ROW_2048, ROW_1000])
def test_count_gumbel_soft_philox_noise(gpu, bh, hw, p, tau):
    """The kernel's documented stream: element i of the NHWC [N, HW, P] map draws word i % 4 of
    Philox block offset + i / 4, so philox_exp1 gives the very E the kernel uses, and images
    [b0:] alone at offset + b0 * HW * P / 4 repeat their bits of the whole batch."""
    n = 2 * bh
    seed, offset = (1 << 40) + 12345, 123457
    logits = _case(bh, hw, p, tau)[0]
    ln = R.nhwc(logits).to(gpu)
    h, w = R.map_hw(hw)
    e = K.philox_exp1(seed, offset, n * hw * p, gpu, log_e=False).view(n, h, w, p)
    proto, counts = R.soft_head(logits, _nchw(e).cpu(), tau)
    pr, sums = K.count_gumbel_soft(ln, tau, None, seed, offset)
    _close("proto", _nchw(pr), proto, **PROTO_TOL)
    _close("sums", sums, counts, **SUMS_TOL)
    b0 = (n + 1) // 3
    assert 0 < b0 < n
    pr_b, sums_b = K.count_gumbel_soft(ln[b0:], tau, None, seed, offset + b0 * hw * p // 4)
    assert torch.equal(pr_b, pr[b0:])
    _close("sums of images [b0:]", sums_b, counts[b0:], **SUMS_TOL)
    pr_o, _ = K.count_gumbel_soft(ln, tau, None, seed, offset + 1)
    assert not torch.equal(pr_o, pr)                                # the offset is not ignored


# ---- 3. head backward ----------------------------------------------------------------------
def _head_backward_case(gpu, row, w_align, w_tanh, with_d_counts):
    bh, hw, p, tau = row
    logits, e, _, _ = _case(*row)
    coeff = _tanh_coeff(bh, hw, p)
    d_counts = _d_counts(bh, p) if with_d_counts else None
    proto, counts, want = R.head_backward(logits, e, tau, w_align, w_tanh, coeff, d_counts)
    assert bool(torch.isfinite(want).all())
    dl = K.count_head_backward(R.nhwc(proto.float()).to(gpu), counts.float().to(gpu),
                               None if d_counts is None else d_counts.to(gpu), w_align, w_tanh, coeff, tau)
    _close("d logits", _nchw(dl), want, **DLOGITS_TOL)


@pytest.mark.parametrize("bh,hw,p,tau", GRID)
def test_count_head_backward_matches_autograd(gpu, bh, hw, p, tau):
    """Inputs: proto and raw counts of the float64 reference cast to float32 (the convention of
    test_head_backward_matches_autograd); align + tanh(C * counts) + <counts, d_counts>, 1/tau."""
    _head_backward_case(gpu, (bh, hw, p, tau), W_ALIGN, W_TANH, True)


@pytest.mark.parametrize("w_align,w_tanh,with_d_counts", [(W_ALIGN, W_TANH, False), (W_ALIGN, 0.0, True),
                                                         (0.0, W_TANH, True)],
                         ids=["no_d_counts", "no_tanh", "no_align"])
@pytest.mark.parametrize("row", [ROW_16, ROW_2048], ids=["p16", "p2048"])
def test_count_head_backward_single_terms(gpu, row, w_align, w_tanh, with_d_counts):
    _head_backward_case(gpu, row, w_align, w_tanh, with_d_counts)


# ---- 4. classifier input gradient ----------------------------------------------------------
@pytest.mark.parametrize("n,d,k", [(1, 4, 1), (6, 37, 3), (5, 257, 10), (8, 6144, 9)])
def test_nonneg_linear_dx(gpu, n, d, k):
    """d_out relu(W) in float64; K <= 10 fused multiply-adds per element leave far less than the
    rtol 1e-5 / atol 1e-7 of test_nonneg_linear_backward."""
    g = torch.Generator().manual_seed(n + d + k)
    d_out = torch.randn(n, k, generator=g) * 1e-2
    w = torch.randn(k, d, generator=g)
    w[w.abs() < 0.3] = 0.0
    w[:, 0] = -w[:, 0].abs()                       # a column with no positive weight
    w[:, d // 2::7] = -w[:, d // 2::7].abs()
    w[:, -1] = w[:, -1].abs() + 0.5                # and one that is all positive
    dead = (w <= 0).all(dim=0)
    assert bool(dead.any()) and not bool(dead.all())
    dx = K.nonneg_linear_dx(d_out.to(gpu), w.to(gpu))
    _close("dx", dx, d_out.double() @ torch.relu(w.double()), rtol=1e-5, atol=1e-7)
    assert torch.all(dx.cpu()[:, dead] == 0)


# ---- 5. bilinear backward front ------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257, 6144 * 8])
def test_bilinear_bwd_prep(gpu, n):
    gen = torch.Generator().manual_seed(n)
    g, u, v = (torch.randn(n, generator=gen) for _ in range(3))
    du, dv = K.bilinear_bwd_prep(g.to(gpu), u.to(gpu), v.to(gpu))
    assert torch.equal(du.cpu(), g * v) and torch.equal(dv.cpu(), g * u)     # one rounded multiply each


# ---- 6. loss kernel on count inputs --------------------------------------------------------
def _classifier(p, k, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(k, p, generator=g)
    w[w.abs() < 0.3] = 0.0
    return w, g


@pytest.mark.parametrize("mode", ["train", "pretrain"])
@pytest.mark.parametrize("bh,hw,p,tau", [ROW_16, ROW_C5])
def test_train_loss_count_inputs(gpu, bh, hw, p, tau, mode):
    """pooled = raw counts (sums over pixels, mostly > 1 at P = 16) with the tanh term on C * counts;
    tolerances of test_loss_kernel_random_shapes."""
    _, _, proto64, counts64 = _case(bh, hw, p, tau)
    proto, counts = proto64.float(), counts64.float()
    k, mult, coeff = 9, 1.5, _tanh_coeff(bh, hw, p)
    w, g = _classifier(p, k, 5 + p)
    out = counts.clamp(0, MAX_COUNT) @ torch.relu(w).t()
    ys = torch.randint(0, k, (bh,), generator=g)
    assert float(counts.max()) > 1.0
    stats, d_out = K.train_loss(R.nhwc(proto).to(gpu), counts.to(gpu), out.to(gpu), ys.to(gpu),
                                torch.tensor([mult]).to(gpu), True, coeff, W_ALIGN, W_TANH, W_CLASS, mode)
    s = stats.cpu().double()
    ref = train_ref.loss_terms(proto.double(), counts.double(), out.double(), ys, mult, True, tanh_coeff=coeff,
                               is_count=True)
    want = W_ALIGN * ref["align"] + W_TANH * ref["tanh"] + (W_CLASS * ref["cls"] if mode == "train" else 0.0)
    for i, (name, val) in enumerate((("align", ref["align"]), ("tanh", ref["tanh"]), ("cls", ref["cls"]),
                                     ("loss", want))):
        print(f"{name}: kernel {float(s[i])!r} reference {float(val)!r}")
    assert float(s[0]) == pytest.approx(float(ref["align"]), rel=2e-5, abs=1e-6)
    assert float(s[1]) == pytest.approx(float(ref["tanh"]), rel=2e-5, abs=1e-6)
    assert float(s[2]) == pytest.approx(float(ref["cls"]), rel=2e-5, abs=1e-6)
    assert float(s[3]) == pytest.approx(float(want), rel=2e-5, abs=1e-6)
    assert float(s[4]) == float(ref["correct"])
    if mode == "pretrain":
        assert d_out is None
    else:
        _close("d_out", d_out, train_ref.d_out(out.double(), ys, mult, True, W_CLASS), rtol=1e-4, atol=1e-9)


# ---- 7. the chain of hip_count_train_step --------------------------------------------------
# Seeds picked on the CPU (smallest that meets the margins asserted below; at P = 16 also one
# count above MAX_COUNT + 0.5, so that both the raw and the rounded gate cut).
CHAIN_ROWS = {"p16": (ROW_16, 2), "p2048": (ROW_2048, 0)}


@pytest.mark.parametrize("use_ste,gated", [(True, True), (True, False), (False, True)],
                         ids=["ste_gated", "ste_identity", "clamp"])
@pytest.mark.parametrize("name", list(CHAIN_ROWS))
def test_count_chain_matches_autograd(gpu, name, use_ste, gated):
    """count_gumbel_soft -> count_finish -> identity intermediate -> nonneg_linear -> train_loss
    ("train") -> nonneg_linear_dx -> count_ste_backward -> count_head_backward against float64
    autograd through GumbelSoftmax -> sum -> STE_Round / ClampSTE (or torch.clamp) -> relu(W) -> loss.

    Rounding and the clamp gate are discontinuous in the raw counts, so the reference's counts
    must keep 1e-3 (some 1e4 float32 ulps of a count) from every half-integer and from
    MAX_COUNT.  With STE the gate reads the rounded count, an exact integer in either precision:
    its only edges are half-integers, and the test asserts that the kernel's clamped counts equal
    the reference's exactly.  The lower gate edge, 0, is asserted at P = 16; at P = 2048 no seed
    can keep the counts 1e-3 from it (some 3600 of the 4096 are below 1e-3, down to 1e-10), and
    there it is no discontinuity of this graph: a count is a sum of softmax values, never negative
    in either precision, so ``>= 0`` passes on both sides -- asserted as counts > 0."""
    (bh, hw, p, tau), seed = CHAIN_ROWS[name]
    k, mult, coeff = 9, 2.0, _tanh_coeff(bh, hw, p)
    logits, e, _, counts = _case(bh, hw, p, tau, seed)
    margins = R.count_margins(counts, MAX_COUNT)
    print("count margins", margins, "max count", float(counts.max()))
    assert margins["half"] >= 1e-3 and margins["top"] >= 1e-3
    assert margins["zero"] >= (1e-3 if p == 16 else 1e-12)
    assert torch.equal(counts.float().round().double(), counts.round()) and float(counts.float().min()) > 0
    if p == 16:
        assert float(counts.max()) > MAX_COUNT + 0.5            # the gate really cuts
    w, g = _classifier(p, k, 9 + p)
    ys = torch.randint(0, k, (bh,), generator=g)
    ref = R.chain(logits, e, tau, w, ys, mult, MAX_COUNT, use_ste, gated, (W_ALIGN, W_TANH, W_CLASS), coeff)

    ln, wd = R.nhwc(logits).to(gpu), w.to(gpu)
    proto, sums = K.count_gumbel_soft(ln, tau, e.to(gpu), seed=0)
    raw, clamped = K.count_finish(None, sums, MAX_COUNT, use_ste)
    _, out = K.nonneg_linear(clamped, wd, None, None)                       # identity intermediate
    stats, d_out = K.train_loss(proto, raw, out, ys.to(gpu), torch.tensor([mult]).to(gpu), True, coeff,
                                W_ALIGN, W_TANH, W_CLASS, "train")
    d_inter = K.nonneg_linear_dx(d_out, wd)
    d_counts = K.count_ste_backward(raw, d_inter, MAX_COUNT, use_ste, gated)
    d_logits = K.count_head_backward(proto, raw, d_counts, W_ALIGN, W_TANH, coeff, tau)

    _close("raw counts", raw, ref["counts"], **SUMS_TOL)
    if use_ste:
        assert torch.equal(clamped.cpu().double(), ref["clamped"])
    else:
        _close("clamped counts", clamped, ref["clamped"], **SUMS_TOL)
    cut = (ref["counts"].round() if use_ste else ref["counts"]) > MAX_COUNT
    if gated:
        assert torch.all(d_counts.cpu()[cut] == 0)
    s = stats.cpu().double()
    for i, term in enumerate(("align", "tanh", "cls")):
        assert float(s[i]) == pytest.approx(float(ref[term]), rel=2e-5, abs=1e-6), term
    _close("d logits", _nchw(d_logits), ref["d_logits"], **DLOGITS_TOL)


# ---- 8. rejected arguments -----------------------------------------------------------------
def test_rejected_arguments(gpu):
    """Widths the launchers have no instantiation for, an odd batch and mismatched counts raise from
    the argument checks; the stream stays usable."""
    def z(*shape):
        return torch.zeros(*shape, device=gpu)

    for p in (30, 2052):
        with pytest.raises(RuntimeError):
            K.count_gumbel_soft(z(2, 1, 1, p), 1.0, None, seed=1)
    with pytest.raises(RuntimeError):
        K.count_head_backward(z(3, 1, 1, 16), z(3, 16), None, 1.0, 1.0, 1.0, 1.0)            # odd batch
    with pytest.raises(RuntimeError):
        K.count_head_backward(z(2, 1, 1, 16), z(2, 20), None, 1.0, 1.0, 1.0, 1.0)            # counts of another width
    with pytest.raises(RuntimeError):
        K.count_head_backward(z(2, 1, 1, 2052), z(2, 2052), None, 1.0, 1.0, 1.0, 1.0)
    with pytest.raises(RuntimeError):                       # the max-pool head shares head_bwd_kernel's widths
        K.head_backward(z(2, 1, 1, 2052), z(2, 2052), None, None, 1.0, 1.0)
    torch.cuda.synchronize()
    _, sums = K.count_gumbel_soft(z(2, 1, 1, 16), 1.0, z(2, 16, 1, 1) + 1.0, seed=1)       # log E = 0: uniform
    assert torch.equal(sums.cpu(), torch.full((2, 16), 1.0 / 16))
