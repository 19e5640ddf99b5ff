"""The sharded training step asks the library for what the recorded parent asked, and leaves the same bits.

tests/golden/dist_train_call_trace.json (tests/golden/gen_train_call_trace.py --sharded) holds, per fixture of
``train_trace_cases.SHARDED_CASES``, every ``_lib.call`` of one iteration through
``dist_train.ShardedTraining(net, seed=5, force_exchange=True).step`` at world 1 -- the exchange path with one shard
that is the whole batch: packed rows, the two-call loss, the rows form of the head backward, the gradient arena --
and the sha256 over parameters, AdamW state and BatchNorm buffers after two iterations, in the format of
tests/golden/train_call_trace.json (tests/test_gpu_train_trace.py).  It was recorded at the commit in its "parent"
field, when the sharded step was a second copy of ``train._train_step``; the tree runs both through one function.
"""
import json
import os

import pytest

import train_trace_cases as C
from golden_util import GOLDEN_DIR

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN_DIR, "dist_train_call_trace.json")) as _f:
    RECORDED = json.load(_f)


def test_every_sharded_case_is_recorded():
    cases = RECORDED["cases"]
    assert sorted(cases) == sorted(C.SHARDED_CASES) and set(C.SHARDED_CASES) <= set(C.CASES)
    assert [tuple(m) for m in RECORDED["masked"]] == list(C.MASKED)
    assert sum(c["digest"] is not None for c in cases.values()) >= 5                   # not vacuous
    for name in ("train_joint_mid_addon", "train_pretrain_mid_addon", "train_count_joint_bilinear",
                 "train_count_finetune_bilinear"):
        assert cases[name]["digest"] is not None, name


@pytest.mark.parametrize("name", C.SHARDED_CASES)
def test_sharded_step_calls_and_bits_match_parent(gpu, name):
    want = RECORDED["cases"][name]
    trace, digest = C.trace_and_digest(name, gpu, sharded=True)
    expected = [RECORDED["calls"][k] for k in want["trace"]]
    for n, (got, exp) in enumerate(zip(trace, expected)):
        assert got == exp, f"call {n} of {len(expected)}"
    assert len(trace) == len(expected)
    assert "pipnet_pack_tensors_f32" in [c[0] for c in trace]         # the exchange path, not the plain step's
    if want["digest"] is not None:
        assert digest == want["digest"]
