"""tests/head_ref.py against the module paths it restates (CPU), one small case each, and the
conditions the GPU grids rely on, checked on the grids' own seeded inputs (the case builders of
head_ref.py that tests/test_gpu_head_matrix.py and tests/test_gpu_eval_matrix.py import): the
share of hard-head pixels with a single candidate, the planted ties, and how far the float32
eval reference is from a float64 evaluation of the same formula."""
import pytest
import torch
import torch.nn as nn

import head_ref as R
from count_pipnet_amd.count_pipnet_utils import (ClampSTE, GumbelSoftmax, LinearIntermediate, STE_Round,
                                                 create_modified_encoding)
from count_pipnet_amd.pipnet import PRESENCE_THRESHOLD, NonNegLinear
from oracle import ref_cpu


# ---- the helpers are the module paths ------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_softmax_pool_is_softmax_and_pool(mode):
    x = torch.randn(2, 3, 5, 37, generator=torch.Generator().manual_seed(1)) * 4
    nchw = x.double().permute(0, 3, 1, 2)
    proto = nn.Softmax(dim=1)(nchw)
    pooled = nn.AdaptiveMaxPool2d((1, 1))(proto).flatten(1) if mode == 0 else proto.sum(dim=(2, 3))
    got_proto, got_pooled = R.softmax_pool(x, mode)
    assert got_proto.dtype == got_pooled.dtype == torch.float64
    torch.testing.assert_close(got_proto.permute(0, 3, 1, 2), proto, rtol=1e-14, atol=0)     # another summation order
    torch.testing.assert_close(got_pooled, pooled, rtol=1e-14, atol=0)
    xb = x.to(torch.bfloat16)                       # bf16 logits: the softmax of their exact values
    assert torch.equal(R.softmax_pool(xb, mode)[0], torch.softmax(xb.float().double(), dim=-1))


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("thresh", [None, PRESENCE_THRESHOLD])
def test_nonneg_linear_is_the_module(bias, thresh):
    x, w, b = R.linear_case(3, 37, 5)
    assert PRESENCE_THRESHOLD == R.THRESH
    assert bool((x == R.AT_THRESH).any()) and bool((x == R.BELOW_THRESH).any())
    lin = NonNegLinear(37, 5, bias=bias)
    with torch.no_grad():
        lin.weight.copy_(w)
        if bias:
            lin.bias.copy_(b)
    clamped = x if thresh is None else torch.where(x < thresh, 0.0, x)      # PIPNet.forward(inference=True), float32
    got_x, got_out, abs_sum = R.nonneg_linear(x, w, b if bias else None, thresh)
    assert torch.equal(got_x, clamped.double())
    if thresh is not None:
        assert bool((got_x[x == R.AT_THRESH] == float(R.AT_THRESH)).all())   # x < thresh is false: survives
        assert bool((got_x[x == R.BELOW_THRESH] == 0).all())
    torch.testing.assert_close(got_out, lin.double()(clamped.double()), rtol=1e-13, atol=1e-15)
    assert bool((abs_sum >= (got_out - (b.double() if bias else 0.0)).abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("tau", [1.0, 0.5])
def test_hard_head_is_gumbel_softmax_eval(tau):
    c = R.gumbel_case(2, 17, 16, tau)
    gs = GumbelSoftmax(dim=1, tau=tau).eval()
    gs.exp_noise = c["e"].double()
    y = gs(c["x"].double().permute(0, 3, 1, 2))                              # NCHW one-hot (straight-through value)
    assert torch.equal(y.argmax(dim=1), c["top"])
    assert bool(((y - 1).abs() < 1e-12).sum(dim=1).eq(1).all()) and bool((y.abs() < 1e-12).sum(dim=1).eq(15).all())
    z = (c["x"].double() - c["e"].double().log().permute(0, 2, 3, 1)) / tau
    assert torch.equal(c["z"], z)
    assert bool((c["tol"] >= 1e-6 / tau).all())


def test_first_argmax_takes_the_lowest_index():
    z = torch.tensor([[1.0, 3.0, 3.0, 2.0], [5.0, 5.0, 5.0, 5.0], [0.0, 1.0, 0.0, 1.0]], dtype=torch.float64)
    assert R.first_argmax(z).tolist() == [1, 0, 1]


def _edge_counts():
    return R.finish_values(3, 42)


def test_round_half_even_is_torch_round():
    c = _edge_counts()
    assert torch.equal(R.round_half_even(c.double()), torch.round(c.double()))
    assert torch.equal(R.round_half_even(c.double()).float(), STE_Round.apply(c))
    assert R.round_half_even(torch.tensor([0.5, 1.5, 2.5, -0.5], dtype=torch.float64)).tolist() == [0, 2, 2, 0]


@pytest.mark.parametrize("max_count", [0, 3, 7])
@pytest.mark.parametrize("do_round", [True, False])
def test_count_finish_is_ste_round_and_clamp(max_count, do_round):
    c = _edge_counts()
    want = ClampSTE.apply(STE_Round.apply(c) if do_round else c, 0.0, float(max_count), True)
    raw, clamped = R.count_finish(c, max_count, do_round)
    assert torch.equal(raw, c.double()) and torch.equal(clamped, want.double())
    hist = torch.tensor([[0, 1, 2, 9]], dtype=torch.int32)
    assert torch.equal(R.count_finish(hist, max_count, do_round)[1], hist.double().clamp(0, max_count))


@pytest.mark.parametrize("c", [1, 3, 5])
def test_count_encode_is_the_modules(c):
    x = R.encode_counts(c, 4, 6)
    want = create_modified_encoding(x, c).view(4, -1)
    assert torch.equal(R.count_encode(x, c, 0, False), want.double())
    assert torch.equal(R.count_encode(x, c, 0, True), create_modified_encoding(x.round(), c).view(4, -1).double())
    lin = LinearIntermediate(6, c)
    w = lin.linear.weight.detach()[:, 0].contiguous()
    assert torch.equal(R.count_encode(x, c, 1, False, w).float(), lin(x).detach())


# ---- conditions of the GPU grids, on their own inputs ---------------------------------------
def test_hard_head_grid_is_decisive():
    """The candidate rule must leave a single candidate at >= 90 % of every row's pixels and >= 99 %
    of the grid's: a test that accepted any candidate would otherwise assert little."""
    single = total = 0
    for row in R.GUMBEL_GRID:
        s = R.gumbel_case(*row)["single"]
        print(row, f"single-candidate pixels {int(s.sum())} / {s.numel()}")
        assert int(s.sum()) >= 0.9 * s.numel(), row
        single, total = single + int(s.sum()), total + s.numel()
    print(f"grid: {single} / {total}")
    assert total == 466 and single >= 0.99 * total
    for row in R.GUMBEL_EXTRA:
        s = R.gumbel_case(*row)["single"]
        assert int(s.sum()) >= 0.9 * s.numel(), row


@pytest.mark.parametrize("p,tau", R.TIE_ROWS)
def test_tie_case_plants_exact_ties(p, tau):
    x, first = R.tie_case(p, tau)
    assert x.shape[1] > 16 or p == 8                                   # more than one workgroup of 16 pixels
    assert torch.equal(x, x.round()) and float(x.min()) >= 0 and float(x.max()) == 2
    z, top, _ = R.hard_head(x, torch.zeros(x.shape, dtype=torch.float64), tau)
    assert torch.equal(top, first)
    assert bool(((z == z.amax(-1, keepdim=True)).sum(-1) >= 2).all())   # a tie at every pixel
    assert torch.equal(z.float().double(), z)                            # exact in float32
    lanes = torch.where(x == 2, torch.arange(p) // 4 % 64, -1)
    assert bool((lanes.amax(-1) != torch.where(x == 2, lanes, 64).amin(-1)).any())    # ties across lanes ...
    assert bool((x == 2).all(-1).any())                                             # ... and in every channel


@pytest.mark.parametrize("b,p,k", R.EVAL_GRID)
@pytest.mark.parametrize("mult", [None, 2.0])
def test_eval_case_conditions(b, p, k, mult):
    """out stays within the goldens' range; the planted rows are what they claim in the reference;
    and the float32 confidence of the reference is within half the GPU test's rtol 1e-6 / atol 1e-7
    of the same formula in float64, so that bound is a bound on the kernel."""
    case = R.eval_case(b, p, k)
    m = 1.0 if mult is None else mult
    worst = 0.0
    for i, (pooled, out, w, ys) in enumerate(case["batches"]):
        assert float(out.max()) <= 30.0 and float(out.min()) >= 0.0
        assert 0.6 <= float((pooled == 0).float().mean()) <= 0.85 or p < 100      # ~70 %, more with the all-zero image
        r = ref_cpu.eval_batch_metrics(pooled, out, w, ys, m)
        r64 = ref_cpu.eval_batch_metrics(pooled.double(), out.double(), w.double(), ys, m)
        err = (r["conf"].double() - r64["conf"]).abs()
        worst = max(worst, float((err / (1e-7 + 1e-6 * r64["conf"].abs())).max()))
        assert torch.equal(r["ys_pred"], r64["ys_pred"])
        for bi, img, first in case["planted"]["ties"]:
            if bi == i:
                assert int((out[img] == out[img].max()).sum()) == 2 and int(r["ys_pred"][img]) == first
        if i == 1:
            assert float(out[0].abs().max()) == 0.0 and int(r["ys_pred"][0]) == 0 and r["abstained"] >= 1
        prod = pooled[:, 0] * w[0, 0]
        assert bool((prod[prod > 0] >= R.THR_F32).all())
        if not (b == 1 and i == 1):                                 # (that batch is the all-zero image alone)
            assert int((pooled[:, 1] * w[k - 1, 1] > R.EVAL_THR).sum()) == 1 and float(pooled[b - 1, 1]) > 0
    above = sum(int((pl[:, 0] == R.ABOVE_THR).sum()) for pl, _, _, _ in case["batches"])
    at = sum(int((pl[:, 0] == R.THR_F32).sum()) for pl, _, _, _ in case["batches"])
    assert above >= 1 and at >= 1
    print(f"float32 reference confidence vs float64: worst err / tolerance {worst:.3f}")
    assert worst <= 0.5
    labels = torch.cat([ys for _, _, _, ys in case["batches"]])
    assert len(set(labels.tolist())) == min(k, R.EVAL_BATCHES * b)
