"""The ConvNeXt executor asks the library for what the recorded parent asked in every precision, and returns the same
bits.

tests/golden/precision_call_trace.json (tests/golden/gen_precision_call_trace.py) holds, per case of
tests/precision_trace_cases.py, every ``_lib.call`` of the forward, the launch hook's (kernel name, flops) rows between
them, and the sha256 of the features, in the format of tests/golden/train_call_trace.json
(tests/test_gpu_train_trace.py).  It was recorded at the commit in its "parent" field, when "bf16x3" and "bf16" were
parallel copies of the fp32 CNBlock, conv wrapper and shape function; the tree writes each once over the operand-format
table ``kernels.LOWP_FORMATS``.
"""
import collections
import json
import os

import pytest

import precision_trace_cases as C
from count_pipnet_amd import _lib
from count_pipnet_amd import kernels as K
from count_pipnet_amd.convnext_features import PRECISIONS
from golden_util import GOLDEN_DIR

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN_DIR, "precision_call_trace.json")) as _f:
    RECORDED = json.load(_f)
# the cases two runs of the parent gave the same bits for: all twelve (no float atomics in these forwards)
REPRODUCIBLE = list(C.CASES)


def _names(case):
    return [row[0] for row in (RECORDED["calls"][k] for k in RECORDED["cases"][case]["trace"])]


def test_every_case_is_recorded():
    cases = RECORDED["cases"]
    assert list(cases) == list(C.CASES) and len(cases) == 12
    assert [tuple(m) for m in RECORDED["masked"]] == list(C.MASKED)
    assert [n for n, c in cases.items() if c["digest"] is not None] == REPRODUCIBLE
    assert len(REPRODUCIBLE) >= 10
    for precision in PRECISIONS:                     # an eval and a train digest of every precision
        for mode in ("eval", "train"):
            assert any(n.endswith(f"_{precision}_{mode}") for n in REPRODUCIBLE), (precision, mode)
    # not vacuous: every train case runs its rowscale entry and, for block 0 (p = 0), the plain Linear2 as well; the
    # fused MLP runs in the fp32 C2 eval forward only; every launch the hook wraps is in the trace with its label
    rowscale = {"fp32": "pipnet_linear_rowscale_f32", "bf16x3": "pipnet_linear_s3_rowscale",
                "bf16": "pipnet_linear_bf16_mix_rowscale"}
    conv = {"bf16x3": "pipnet_conv2d_nhwc_s3", "bf16": "pipnet_conv2d_nhwc_bf16_mix"}
    for model in C.MODELS:
        for precision in PRECISIONS:
            ev, tr = _names(f"{model}_{precision}_eval"), _names(f"{model}_{precision}_train")
            assert rowscale[precision] in tr and not any(r in ev for r in rowscale.values())
            low = [n for n in ev if n in conv.values()]
            assert (set(low) == {conv[precision]}) if precision != "fp32" else not low
            fused = "pipnet_cnblock_mlp_hw_f32" in ev
            assert fused == (precision == "fp32" and model == "c2_pipnet_convnext26")
            hooked = [n for n in ev if n not in _lib.SIGNATURES]          # the launch hook's rows: kernel labels
            assert hooked and all("_kernel" in n for n in hooked), hooked
            assert any(n.startswith("pipnet_bf16::") for n in hooked) == (precision != "fp32")


@pytest.mark.parametrize("name", list(C.CASES))
def test_forward_calls_and_bits_match_parent(gpu, name):
    want = RECORDED["cases"][name]
    trace, digest = C.CASES[name](gpu)
    expected = [RECORDED["calls"][k] for k in want["trace"]]
    for n, (got, exp) in enumerate(zip(trace, expected)):
        assert got == exp, f"call {n} of {len(expected)}"
    assert len(trace) == len(expected)
    if want["digest"] is not None:
        assert digest == want["digest"]


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_the_executor_goes_through_the_public_wrappers(gpu, monkeypatch, precision):
    """tools/ab/ab_s3_rule.py swaps a tile rule in by assigning ``K.conv_s3``: the executor looks the format's four
    wrappers up on the module at call time, once per library call, and the bits stay the recorded ones."""
    fmt, seen = K.LOWP_FORMATS[precision], collections.Counter()
    wrappers = {fmt.conv_fn: fmt.conv, fmt.rowscale_fn: fmt.rowscale, fmt.dwconv7_ln_fn: fmt.dwconv7_ln,
                fmt.layernorm_fn: fmt.layernorm}
    for name in wrappers:
        monkeypatch.setattr(K, name, lambda *a, _name=name, _real=getattr(K, name), **k:
                            (seen.update([_name]), _real(*a, **k))[1])
    case = f"pipnet_mid_addon_{precision}_train"
    trace, digest = C.CASES[case](gpu)
    assert digest == RECORDED["cases"][case]["digest"]
    names = [row[0] for row in trace]
    for name, entry in wrappers.items():
        assert seen[name] == names.count(entry) > 0, (name, seen)
