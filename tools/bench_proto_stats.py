"""Cost of the class-conditional prototype statistics on one GPU, at C2 (PIP-Net ConvNeXt-tiny-26,
224x224, batch 64, K = 200, P = 768, 50 bins) and C5 (CountPIPNet bilinear, 128x128, batch 64,
K = 9, P = 2048, count edges).

(1) the update kernel alone: event-timed ms per batch of ``pipnet_proto_stats_update_f32`` on
    [64, P] activations, for random labels, one class for the whole batch (the longest chain on
    one state entry) and sorted labels; and ``pipnet_colsum_accum_f64`` at the classifier's input
    width.
(2) a ``class_prototype_stats`` pass over N device-resident batches against a loop of plain
    forwards over the same batches (the forward is the baseline: the pass adds the kernel and the
    label copy to it); host clock around work that ends in a device synchronise, the two arms
    alternated, median of the repeats.
(3) the reference-style collection over the same batches: forward, ``pooled.cpu()`` per batch,
    concatenation, then the numpy restatement of the reference's prototype x class loops
    (tests/proto_stats_ref.py ``reference_analysis``).

(4) optional, ``--ab-lib NAME=PATH`` (repeatable): the update kernel of another build of
    csrc/proto_stats.hip, loaded beside the library and timed in the same process on the same
    inputs as (1), e.g. a build without class partitions
      hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -DPS_MAX_PARTS_DEF=1 -I include \
            count_pipnet_amd/csrc/proto_stats.hip -o libps_parts1.so

    python tools/bench_proto_stats.py [--batches 6] [--repeats 5] [--only c2] [--kernels-only]
Prints one JSON line per measurement."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_configs import CONFIGS, make  # noqa: E402
from count_pipnet_amd import _lib, build  # noqa: E402
from count_pipnet_amd import kernels as K  # noqa: E402
from count_pipnet_amd.stats import class_prototype_stats, count_edges, pipnet_edges  # noqa: E402
from count_pipnet_amd.synthetic import synth_images  # noqa: E402
from proto_stats_ref import reference_analysis  # noqa: E402


def event_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def raw_update(lib, st, act, lab):
    """pipnet_proto_stats_update_f32 of ``lib`` on the state ``st`` (the arguments K.proto_stats_update passes)."""
    rc = lib.pipnet_proto_stats_update_f32(act.data_ptr(), act.stride(0), lab.data_ptr(), act.shape[0], act.shape[1],
                                           st.classes, st.threshold, st.edges.data_ptr(), st.bins,
                                           *[t.data_ptr() for t in st.tensors()],
                                           torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab-lib", action="append", default=[], metavar="NAME=PATH")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    build.build()
    dev = torch.device("cuda:0")
    arms = {}
    for spec in a.ab_lib:
        arm, path = spec.split("=", 1)
        arms[arm] = ctypes.CDLL(os.path.abspath(path))
        arms[arm].pipnet_proto_stats_update_f32.argtypes = _lib.SIGNATURES["pipnet_proto_stats_update_f32"]
    for name in ("c2", "c5"):
        if a.only and name not in a.only.split(","):
            continue
        cfg = CONFIGS[name]
        net = make(cfg, dev)
        count = cfg["model"] == "count"
        b, kc, pn = cfg["batch"], cfg["classes"], net._num_prototypes
        edges = count_edges(net._max_count) if count else pipnet_edges()
        base = dict(config=name, batch=b, classes=kc, prototypes=pn, bins=edges.numel() - 1)

        # (1) the kernels alone
        g = torch.Generator().manual_seed(1)
        act = (torch.rand(b, pn, generator=g) * (4.0 if count else 1.0)).to(dev)
        act = act.round() if count else act
        rnd = torch.randint(0, kc, (b,), generator=g)
        for pattern, labels in (("random", rnd), ("equal", torch.full((b,), kc - 1)), ("sorted", rnd.sort().values)):
            st = K.ProtoStatsState(kc, pn, 0.01, edges, dev)
            lab = labels.to(dev)
            med, lo, hi = event_ms(lambda: K.proto_stats_update(st, act, lab), 200, 20)
            print(json.dumps(dict(base, what="update_kernel", labels=pattern, ms_median=med, ms_min=lo, ms_max=hi)),
                  flush=True)
            for arm, lib in arms.items():
                other = K.ProtoStatsState(kc, pn, 0.01, edges, dev)
                med, lo, hi = event_ms(lambda: raw_update(lib, other, act, lab), 200, 20)
                same = all(torch.equal(x, y) for x, y in zip(st.tensors(), other.tensors()))
                print(json.dumps(dict(base, what="update_kernel", build=arm, labels=pattern, ms_median=med, ms_min=lo,
                                      ms_max=hi, same_state=same)), flush=True)
        d = net._classification.weight.shape[1]
        x = torch.rand(b, d, generator=g).to(dev)
        acc = torch.zeros(d, device=dev, dtype=torch.float64)
        med, lo, hi = event_ms(lambda: K.colsum_accum_f64(acc, x), 200, 20)
        print(json.dumps(dict(base, what="colsum_accum_f64", width=d, ms_median=med, ms_min=lo, ms_max=hi)), flush=True)

        if a.kernels_only:
            continue
        # (2) the pass against plain forwards, (3) the reference-style collection
        batches = [(synth_images(b, cfg["size"], seed=50 + i).to(dev), torch.randint(0, kc, (b,), generator=g))
                   for i in range(a.batches)]

        def forwards():
            with torch.no_grad():
                for xs, _ in batches:
                    net(xs, inference=True)

        def stats_pass():
            class_prototype_stats(net, batches, max_images=None)

        def reference_style():
            acts, labels = [], []
            with torch.no_grad():
                for xs, ys in batches:
                    acts.append(net(xs, inference=True)[1].cpu())
                    labels.append(ys)
            reference_analysis(torch.cat(acts).numpy(), torch.cat(labels).numpy(), 0.01, count=count)

        forwards()
        stats_pass()
        t_fwd, t_pass = [], []
        for _ in range(a.repeats):
            t_fwd.append(wall_ms(forwards))
            t_pass.append(wall_ms(stats_pass))
        t_ref = [wall_ms(reference_style) for _ in range(2)]
        fwd, pas = statistics.median(t_fwd), statistics.median(t_pass)
        print(json.dumps(dict(base, what="pass_vs_forwards", batches=a.batches, forwards_ms=fwd, stats_pass_ms=pas,
                              overhead_pct=100.0 * (pas - fwd) / fwd, forwards_all_ms=t_fwd, stats_pass_all_ms=t_pass,
                              reference_style_ms=min(t_ref), reference_style_all_ms=t_ref)), flush=True)
        del net, batches
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
