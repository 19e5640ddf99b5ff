"""tests/count_head_ref.py against the module path it wraps (CPU, float64): the helper the GPU
tests of the CountPIPNet training head compare with must itself be GumbelSoftmax + spatial sum
+ autograd."""
import pytest
import torch

import count_head_ref as R
from count_pipnet_amd.count_pipnet_utils import GumbelSoftmax


@pytest.mark.parametrize("tau", [1.0, 0.5])
def test_helper_equals_module_path(tau):
    bh, hw, p = 2, 9, 16
    logits, e = R.draw_inputs(bh, hw, p, seed=11)
    d_counts = torch.randn(2 * bh, p, generator=torch.Generator().manual_seed(12), dtype=torch.float64) * 0.1

    gs = GumbelSoftmax(dim=1, tau=tau).train()
    gs.exp_noise = e.double()
    ld = logits.double().requires_grad_(True)
    proto = gs(ld)
    counts = proto.sum((2, 3))
    (grad,) = torch.autograd.grad((counts * d_counts).sum(), ld)

    h_proto, h_counts, h_grad = R.head_backward(logits, e, tau, 0.0, 0.0, 1.0, d_counts)
    assert h_proto.dtype == h_counts.dtype == h_grad.dtype == torch.float64
    assert torch.equal(h_proto, proto.detach()) and torch.equal(h_counts, counts.detach())
    torch.testing.assert_close(h_grad, grad, rtol=1e-12, atol=1e-15)
    s_proto, s_counts = R.soft_head(logits, e, tau)
    assert torch.equal(s_proto, h_proto) and torch.equal(s_counts, h_counts)

    # the same numbers from the definition: y = softmax((x - log E) / tau) over the channels, and
    # for L = <counts, d> the softmax backward y (d - <y, d>) / tau at every pixel -- 1/tau once
    y = torch.softmax((logits.double() - e.double().log()) / tau, dim=1)
    torch.testing.assert_close(h_proto, y, rtol=1e-13, atol=0)
    d = d_counts[:, :, None, None]
    torch.testing.assert_close(h_grad, y * (d - (y * d).sum(1, keepdim=True)) / tau, rtol=1e-9, atol=1e-15)
    assert float(h_counts.sum()) == pytest.approx(2 * bh * hw, rel=1e-12)      # one unit per pixel
