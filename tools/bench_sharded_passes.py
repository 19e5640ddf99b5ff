"""Cost of the state merges of the sharded dataset passes on one GPU, at W = 8 ranks and the C2 / CUB dimensions
(P = 768 prototypes, K = 200 classes, 50 histogram bins, k = 10, M = 12 merged parts), beside one 64-image C2
forward in the same process.  Each merge is event-timed on a gathered buffer of 8 packed states (what
``dist.ShardedPass.gather_state`` hands to ``kernels.*_merge``) and reported as a share of that forward; a pass
runs one merge, after thousands of forwards.  Scaling over several GPUs cannot be measured on one GPU.

    python tools/bench_sharded_passes.py [--out profiles/sharded_passes/merge.txt]
Prints one JSON line per measurement and writes them to ``--out``."""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import torch  # noqa: E402

from bench_configs import CONFIGS, make  # noqa: E402
from bench_proto_stats import event_ms  # noqa: E402
from count_pipnet_amd import build  # noqa: E402
from count_pipnet_amd import kernels as K  # noqa: E402
from count_pipnet_amd.stats import pipnet_edges  # noqa: E402
from count_pipnet_amd.synthetic import synth_images  # noqa: E402

WORLD, PN, KC, BINS, TOPK, PARTS = 8, 768, 200, 50, 10, 12


def gathered(states):
    """The states as views into one [W, bytes] buffer, as after the all-gather."""
    buf = torch.stack([s.pack() for s in states])
    return [states[0].unpack(row) for row in buf], buf.stride(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sharded_passes", "merge.txt"))
    a = ap.parse_args()
    build.build()
    dev = torch.device("cuda:0")
    cfg = CONFIGS["c2"]
    base = dict(config="c2", world=WORLD, prototypes=PN, classes=KC, bins=BINS, k=TOPK, merged_parts=PARTS)
    lines = []

    def report(**kw):
        lines.append(json.dumps(dict(base, **kw)))
        print(lines[-1], flush=True)

    net = make(cfg, dev)
    assert net._num_prototypes == PN
    xs = synth_images(cfg["batch"], cfg["size"], seed=50).to(dev)

    def forward():
        with torch.no_grad():
            net(xs, inference=True)

    fwd_ms, fwd_lo, fwd_hi = event_ms(forward, 20, 3)
    report(what="forward", batch=cfg["batch"], ms_median=fwd_ms, ms_min=fwd_lo, ms_max=fwd_hi)

    g = torch.Generator().manual_seed(1)
    tops = []
    for r in range(WORLD):              # every rank's list full and sorted, as a pass leaves it
        st = K.TopkState(1, PN, TOPK, dev)
        K.topk_update(st, torch.rand((64, PN), generator=g).to(dev),
                      torch.randint(0, 676, (64, PN), generator=g, dtype=torch.int32).to(dev), 64 * r)
        tops.append(st)
    stats = []
    for r in range(WORLD):
        st = K.ProtoStatsState(KC, PN, 0.01, pipnet_edges(), dev)
        K.proto_stats_update(st, torch.rand((64, PN), generator=g).to(dev),
                             torch.randint(0, KC, (64,), generator=g).to(dev))
        stats.append(st)
    purities = []
    for r in range(WORLD):
        st = K.PartPurityState(PN, PARTS, dev)
        st.n.copy_(torch.randint(0, 99, (PN, PARTS), generator=g))
        st.first_key.copy_(torch.randint(0, 1 << 40, (PN, PARTS), generator=g))
        purities.append(st)
    for what, states, merge in (("topk_merge", tops, K.topk_merge), ("proto_stats_merge", stats, K.proto_stats_merge),
                                ("part_purity_merge", purities, K.part_purity_merge)):
        views, stride = gathered(states)
        med, lo, hi = event_ms(lambda: merge(views), 100, 10)
        report(what=what, state_bytes_per_rank=stride, gathered_bytes=stride * WORLD, ms_median=med, ms_min=lo,
               ms_max=hi, pct_of_forward=100.0 * med / fwd_ms)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# tools/bench_sharded_passes.py on one MI355X: each state merge at W = 8 (device events, median of 100;\n"
                "# the output state's allocation included) beside one 64-image C2 forward in the same process.\n"
                "# One merge runs per pass.  Scaling over several GPUs is not measured.\n")
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
