"""The explanation passes ask the library for what the recorded parent asked, and return the same bits.

tests/golden/explain_call_trace.json (tests/golden/gen_explain_call_trace.py) holds, per case of
tests/explain_trace_cases.py, every ``_lib.call`` of the pass and the sha256 of its result, in the format of
tests/golden/train_call_trace.json (tests/test_gpu_train_trace.py).  It was recorded at the commit in its "parent"
field, when the batch-invariant forward with patch locations was written out in ``topk`` and ``local`` and the
small-map rule in four places; the tree takes both from ``explain_forward``.
"""
import json
import os

import pytest

import explain_trace_cases as C
from count_pipnet_amd import _lib
from golden_util import GOLDEN_DIR

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN_DIR, "explain_call_trace.json")) as _f:
    RECORDED = json.load(_f)


def _side_stream(case):
    """Per launch of the recorded case: whether it went to a side stream (the stream is the last argument)."""
    calls = [RECORDED["calls"][k] for k in RECORDED["cases"][case]["trace"]]
    return [args[-1] == 1 for name, args in calls if _lib.SIGNATURES[name][-1] is _lib.P]


def test_every_case_is_recorded():
    cases = RECORDED["cases"]
    assert list(cases) == list(C.CASES)
    assert [tuple(m) for m in RECORDED["masked"]] == list(C.MASKED)
    for name in ("topk_pipnet_bs5", "topk_pipnet_bs12", "local_pipnet", "purity_all", "purity_topk", "large_topk",
                 "large_purity_topk"):                                                  # not vacuous
        assert cases[name]["digest"] is not None, name
    # the large-map branch: the first batch of 34 (map size unknown) on the current stream, the second as two halves
    # on side streams -- twice the forward's launches; nothing else leaves the current stream
    for name in ("large_topk", "large_purity_topk"):
        side = _side_stream(name)
        first = side.index(True)
        assert 0 < first and sum(side) == 2 * (first - 1) and all(side[first:first + sum(side)]), (name, first, sum(side))
        assert not any(_side_stream(name + "_bs1"))
    assert not any(_side_stream("topk_pipnet_bs12"))


def test_large_map_results_do_not_depend_on_the_batching():
    """On a map of more than K.SPLITK_MAX_M pixels the parent gave the same bits in batches of 34 (the second one as
    two concurrent halves) and one image at a time; the cases below hold each digest to its record."""
    for batched, single in C.BATCH_INVARIANT:
        assert RECORDED["cases"][batched]["digest"] == RECORDED["cases"][single]["digest"] is not None


@pytest.mark.parametrize("name", list(C.CASES))
def test_pass_calls_and_bits_match_parent(gpu, name):
    want = RECORDED["cases"][name]
    trace, digest = C.CASES[name](gpu)
    expected = [RECORDED["calls"][k] for k in want["trace"]]
    for n, (got, exp) in enumerate(zip(trace, expected)):
        assert got == exp, f"call {n} of {len(expected)}"
    assert len(trace) == len(expected)
    if want["digest"] is not None:
        assert digest == want["digest"]
