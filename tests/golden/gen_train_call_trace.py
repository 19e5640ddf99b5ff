"""Re-record tests/golden/train_call_trace.json: what one training iteration of every train_* fixture asks of
the library, and the bits it leaves behind where those are reproducible.

The committed file was recorded on an MI355X at the commit named in its "parent" field, before the four HIP
training steps were folded into one; tests/test_gpu_train_trace.py holds the tree to it.  Run this only when a
launch is MEANT to change, twice:

    python tests/golden/gen_train_call_trace.py            # records traces and digests
    python tests/golden/gen_train_call_trace.py --merge    # a second run: keeps what both runs agree on

(``--out FILE`` writes elsewhere, and ``--merge`` then merges with that file; ``--parent HASH`` names the commit where git cannot.)

``--sharded`` records tests/golden/dist_train_call_trace.json instead: ``train_trace_cases.SHARDED_CASES`` through
``dist_train.ShardedTraining.step`` at world 1 with the exchange path forced.  That file was recorded at the
commit in its own "parent" field, while the sharded step was still a second copy of the plain one;
tests/test_gpu_dist_train_trace.py holds the tree to it.

Every case runs twice in each invocation as well.  Traces must agree in every run (an argument position that
does not goes into ``train_trace_cases.MASKED`` and is listed in the header); a state digest is kept only for
the cases where every run gave the same one (float atomics make the others order-dependent).
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import torch                                                     # noqa: E402

import train_trace_cases as C                                    # noqa: E402
from count_pipnet_amd import _lib, build                         # noqa: E402

PATH = os.path.join(HERE, "train_call_trace.json")
SHARDED_PATH = os.path.join(HERE, "dist_train_call_trace.json")


def load(path=PATH):
    """The file -> (header, {case: [[name, args], ...]}, {case: digest or None})."""
    with open(path) as f:
        doc = json.load(f)
    calls = doc["calls"]
    return doc, {n: [calls[k] for k in c["trace"]] for n, c in doc["cases"].items()}, \
        {n: c["digest"] for n, c in doc["cases"].items()}


def record(names, run_case, out, merge, parent, note, masked):
    """Run every case twice (``run_case(name) -> (trace, digest)``), merge with ``out`` if asked, and write ``out``."""
    traces, digests = {}, {}
    if merge:
        _, traces, digests = load(out)
    for name in names:
        for _ in range(2):
            trace, digest = run_case(name)
            if name not in traces:
                traces[name], digests[name] = trace, digest
                continue
            diff = [(x, y) for x, y in zip(traces[name], trace) if x != y]
            if diff or len(trace) != len(traces[name]):
                raise SystemExit(f"{name}: the trace differs between two runs ({len(traces[name])} / {len(trace)} "
                                 f"calls); first difference {diff[:1]}: mask the position in the cases' MASKED")
            if digests[name] != digest:
                digests[name] = None
        print(f"{name}: {len(traces[name])} calls, digest {'kept' if digests[name] else 'not reproducible'}",
              flush=True)
    table, cases = {}, {}
    for name in names:                   # the same launch recurs in many cases: store each distinct one once
        idx = [table.setdefault(json.dumps(c), len(table)) for c in traces[name]]
        cases[name] = {"digest": digests[name], "trace": idx}
    head = {"parent": parent or subprocess.run(["git", "rev-parse", "HEAD"], cwd=HERE, capture_output=True,
                                               text=True, check=True).stdout.strip(),
            "note": note, "masked": [list(m) for m in masked]}
    with open(out, "w") as f:
        f.write("{\n" + "".join(f" {json.dumps(k)}: {json.dumps(v)},\n" for k, v in head.items()))
        f.write(' "cases": {\n' + ",\n".join(f"  {json.dumps(n)}: {json.dumps(c)}" for n, c in cases.items()))
        f.write('\n },\n "calls": [\n' + ",\n".join("  " + c for c in table) + "\n ]\n}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge", action="store_true")
    ap.add_argument("--sharded", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None)
    a = ap.parse_args()
    build.build()
    _lib.load()
    gpu = torch.device("cuda:0")
    record(C.SHARDED_CASES if a.sharded else C.CASES, lambda name: C.trace_and_digest(name, gpu, a.sharded),
           a.out or (SHARDED_PATH if a.sharded else PATH), a.merge, a.parent,
           "per case: the library calls of iteration 0 as indices into 'calls' ([name, args]; a pointer "
           "argument is 0 for null and 1 otherwise, a float is float.hex), and the sha256 of parameters, "
           "AdamW state and BatchNorm buffers after 2 iterations (null where two runs of the parent gave "
           "different bits)", C.MASKED)


if __name__ == "__main__":
    main()
