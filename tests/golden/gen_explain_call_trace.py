"""Re-record tests/golden/explain_call_trace.json: what the explanation passes of tests/explain_trace_cases.py ask of
the library, and the sha256 of their results where those are reproducible.

The committed file was recorded on an MI355X at the commit named in its "parent" field, before ``topk``, ``local``,
``purity``, ``stats`` and ``attribution`` took their located forward, the small-map rule and the patch geometry from
``explain_forward``; tests/test_gpu_explain_trace.py holds the tree to it.  Run this only when a launch is MEANT to
change, twice, as tests/golden/gen_train_call_trace.py (whose ``record`` and file format this uses):

    python tests/golden/gen_explain_call_trace.py            # records traces and digests
    python tests/golden/gen_explain_call_trace.py --merge    # a second run: keeps what both runs agree on
"""
import argparse
import os

import gen_train_call_trace as G                                 # puts the repository and tests/ on sys.path

import torch                                                     # noqa: E402

import explain_trace_cases as C                                  # noqa: E402
from count_pipnet_amd import _lib, build                         # noqa: E402

PATH = os.path.join(G.HERE, "explain_call_trace.json")


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
             "per case: the library calls of the pass as indices into 'calls' ([name, args]; a pointer argument is 0 "
             "for null and 1 otherwise -- the stream, last, is 1 on a side stream --, a float is float.hex), and the "
             "sha256 of the .cpu() result's fields (null where two runs of the parent gave different bits)", C.MASKED)


if __name__ == "__main__":
    main()
