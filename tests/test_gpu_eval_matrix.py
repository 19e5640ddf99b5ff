"""pipnet_eval_batch_f32 and pipnet_weight_sparsify_f32 (csrc/eval_metrics.hip) on synthetic batches
(head_ref.eval_case) against oracle.ref_cpu.eval_batch_metrics / eval_loop, the restatement of
eval_pipnet's per-batch body that tests/test_eval_golden.py pins to the recorded goldens.  What the
golden batches do not guarantee, and the row that plants it:

  block_argmax's first-index rule      ties inside one wave (1, 2), across waves (3 | 70, 70 | 199: neither
                                       the thread loop's second pass nor wave 0 decides) and at 3 | K - 1
  the abstain flag                     an all-zero image in the second batch of every row: prediction 0,
                                       counted, confusion-matrix cell [y, 0]
  K < 64 / K > 256 / B > 256           (1, 4, 2), (5, 100, 3), (3, 6144, 9) / (300, 260, 257): a second pass of the
                                       class loops and of eval_reduce_kernel's strided image loop
  P not a multiple of 256              P = 4, 100, 260
  multiplier = None                    every row, next to multiplier = 2
  products on the 1e-3 threshold       pooled = float32(1e-3) with w = 1 (not counted) and the next float above
  eval_class_kernel's early exit       a prototype over the threshold in the last image of the batch only
  sparsify_kernel's grid-stride loop   4096 x 256 + 77 elements

ys_pred, the confusion matrix, the abstain count and the five accumulated means are exact, as in
test_eval_batch_kernel_matches_reference; the confidence keeps that test's rtol 1e-6 / atol 1e-7,
and tests/test_head_ref_cpu.py shows the float32 reference within 0.13 of that bound of a float64
evaluation on these very batches (out stays below 30, the goldens' range)."""
import numpy as np
import pytest
import torch

import head_ref as R
from count_pipnet_amd import kernels as K
from oracle import ref_cpu

pytestmark = pytest.mark.gpu


def _close(what, got, want, rtol, atol):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got - want).abs()
    ratio = float((err / (atol + rtol * want.abs())).max()) if err.numel() else 0.0
    print(f"{what}: max |err| {float(err.max()):.3e}, worst err / tolerance {ratio:.3f}")
    torch.testing.assert_close(got, want, rtol=rtol, atol=atol, msg=lambda m: f"{what}: {m}")


@pytest.mark.parametrize("mult", [None, 2.0], ids=["nomult", "mult2"])
@pytest.mark.parametrize("b,p,k", R.EVAL_GRID)
def test_eval_batch_matrix(gpu, b, p, k, mult):
    case = R.eval_case(b, p, k)
    m = 1.0 if mult is None else mult
    cm = torch.zeros((k, k), dtype=torch.int64, device=gpu)
    acc = torch.zeros(5, dtype=torch.float64, device=gpu)
    abst = torch.zeros(1, dtype=torch.int64, device=gpu)
    mult_dev = None if mult is None else torch.tensor([mult], device=gpu)
    wd = case["w"].to(gpu)
    for i, (pooled, out, w, ys) in enumerate(case["batches"]):
        ys_pred, conf = K.eval_batch(pooled.to(gpu), out.to(gpu), wd, ys.to(gpu), mult_dev, R.EVAL_THR, cm, acc, abst)
        r = ref_cpu.eval_batch_metrics(pooled, out, w, ys, m)
        assert torch.equal(ys_pred.cpu().long(), r["ys_pred"]), f"batch {i}"
        for bi, img, first in case["planted"]["ties"]:
            if bi == i:
                assert int(ys_pred[img]) == first                            # the first of the tied maxima
        _close(f"batch {i} confidence", conf, r["conf"], rtol=1e-6, atol=1e-7)
    want = ref_cpu.eval_loop(case["batches"], k, m, R.EVAL_THR)
    nb = len(case["batches"])
    a = acc.cpu().tolist()
    assert np.array_equal(cm.cpu().numpy(), want["confusion_matrix"])
    assert int(cm.sum()) == nb * b
    y_abstain = int(case["batches"][1][3][0])
    assert int(cm[y_abstain, 0]) >= 1                                        # the all-zero image: cell [y, 0]
    assert int(abst.item()) == want["abstained"] >= 1
    assert a[0] / nb == want["local_size_for_true_class"]
    assert a[1] / nb == want["local_size_for_all_classes"]
    assert a[2] / nb == want["prototypes_per_class"]
    assert a[3] / nb == want["almost_nonzeros"]
    assert a[4] / nb == want["top1_accuracy"]


def test_weight_sparsify_past_the_grid_cap(gpu):
    n, delta = 4096 * 256 + 77, 1e-3
    g = torch.Generator().manual_seed(9)
    w = torch.randn(n, generator=g) * 2e-3                       # straddles delta: about a third above it
    d32 = torch.tensor(delta, dtype=torch.float32)
    w[::5] = d32                                                 # exactly delta -> 0
    w[1::5] = torch.nextafter(d32, torch.tensor(1.0))            # the float above -> the smallest difference
    w[-77:] = torch.linspace(-1e-3, 3e-3, 77)                    # the tail past the capped grid
    wd = w.to(gpu)
    assert K.weight_sparsify_(wd, delta) is wd
    want = torch.clamp(w - delta, min=0)
    assert 0.2 < float((want > 0).float().mean()) < 0.8
    assert torch.equal(wd.cpu(), want)
