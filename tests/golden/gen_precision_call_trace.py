"""Re-record tests/golden/precision_call_trace.json: what the forward-only ConvNeXt executor asks of the library in
each precision (the cases of tests/precision_trace_cases.py), the labels and flop counts it hands the launch hook, and
the sha256 of the features where those are reproducible.

The committed file was recorded on an MI355X at the commit named in its "parent" field, while the bf16x3 and bf16
builds were parallel copies of the fp32 executor in ``convnext_features``, ``kernels`` and the library's host code;
tests/test_gpu_precision_trace.py holds the tree to it.  Run this only when a launch is MEANT to change, twice, as
tests/golden/gen_train_call_trace.py (whose ``record`` and file format this uses):

    python tests/golden/gen_precision_call_trace.py            # records traces and digests
    python tests/golden/gen_precision_call_trace.py --merge    # a second run: keeps what both runs agree on
"""
import argparse
import os

import gen_train_call_trace as G                                 # puts the repository and tests/ on sys.path

import torch                                                     # noqa: E402

import precision_trace_cases as C                                # noqa: E402
from count_pipnet_amd import _lib, build                         # noqa: E402

PATH = os.path.join(G.HERE, "precision_call_trace.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge", action="store_true")
    ap.add_argument("--out", default=PATH)
    ap.add_argument("--parent", default=None)
    a = ap.parse_args()
    build.build()
    _lib.load()
    gpu = torch.device("cuda:0")
    G.record(list(C.CASES), lambda name: C.CASES[name](gpu), a.out, a.merge, a.parent,
             "per case: the library calls of the forward as indices into 'calls' ([name, args]; a pointer argument is "
             "0 for null and 1 otherwise, a float is float.hex) interleaved with the launch hook's rows ([kernel name, "
             "flops as float.hex], each just before the call it wraps), and the sha256 of dtype, shape and bytes of "
             "the returned features (null where two runs of the parent gave different bits)", C.MASKED)


if __name__ == "__main__":
    main()
