"""The HIP training steps ask the library for what the recorded parent asked, and leave the same bits.

tests/golden/train_call_trace.json (tests/golden/gen_train_call_trace.py) holds, per train_* fixture, every
``_lib.call`` of one iteration -- kernel name, null-ness of each pointer, every other argument by value -- and,
where two runs of the parent gave the same bits, a sha256 over parameters, AdamW state and BatchNorm buffers
after two iterations.  The cases without a digest (CountPIPNets whose raw counts are summed with float atomics)
are held by the trace and by the tolerance tests of tests/test_gpu_train.py.

The clamp rule: after a step that is not a pretrain step, a classifier weight or bias that no AdamW step
clamped is clamped on its own (the reference clamps unconditionally after the optimizer step).
"""
import json
import os

import pytest
import torch

import train_trace_cases as C
from count_pipnet_amd import kernels as K
from count_pipnet_amd import train as T
from golden_util import GOLDEN_DIR

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN_DIR, "train_call_trace.json")) as _f:
    RECORDED = json.load(_f)


def test_every_fixture_is_recorded():
    assert sorted(RECORDED["cases"]) == C.CASES
    assert [tuple(m) for m in RECORDED["masked"]] == list(C.MASKED)
    assert sum(c["digest"] is not None for c in RECORDED["cases"].values()) >= 12      # not vacuous


@pytest.mark.parametrize("name", C.CASES)
def test_step_calls_and_bits_match_parent(gpu, name):
    want = RECORDED["cases"][name]
    trace, digest = C.trace_and_digest(name, gpu)
    expected = [RECORDED["calls"][k] for k in want["trace"]]
    for n, (got, exp) in enumerate(zip(trace, expected)):
        assert got == exp, f"call {n} of {len(expected)}"
    assert len(trace) == len(expected)
    if want["digest"] is not None:
        assert digest == want["digest"]


def test_unstepped_classifier_weight_is_still_clamped(gpu):
    """A joint step with ``_classification.weight`` in no group of optimizer_classifier while it requires grad:
    the weight comes out as ``weight_sparsify_`` of what it was, and the multiplier is >= 1."""
    name = "train_joint_mid_addon"
    meta, rec, fwd_meta = C.load_train_golden(name)
    net = C.build_model(fwd_meta).to(gpu).train()
    opt_net, opt_cls, _, _ = C._optimizers_like_reference(net, meta, fwd_meta)
    cls = net._classification
    opt_cls.param_groups[:] = [g for g in opt_cls.param_groups if all(p is not cls.weight for p in g["params"])]
    assert cls.weight.requires_grad and T._group_of(opt_cls, cls.weight) is None
    c = fwd_meta["case"]
    xs1, xs2, ys = C.train_loader_batches(c["size"], c["num_classes"], 1, meta["batch_per_view"], meta["seed"])[0]
    before = cls.weight.detach().clone()
    want = K.weight_sparsify_(before.clone(), T.SPARSITY_DELTA)
    assert not torch.equal(want, before)
    T.hip_train_step(net, xs1.to(gpu), xs2.to(gpu), ys.to(gpu), opt_net, opt_cls, False, 1, 1, True,
                     sd_keep=C._sd_keep(net, rec["s0_masks"]))
    assert torch.equal(cls.weight.detach(), want)
    assert float(cls.normalization_multiplier.min()) >= 1.0
