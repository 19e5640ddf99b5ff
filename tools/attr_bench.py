"""Time count_pipnet_amd.attribute: the HIP path against the same call under torch_backend().

Setups (the issue's): the C2 model (ConvNeXt-tiny-26 PIP-Net, 224^2) and the C5-shaped CountPIPNet
(2048 prototypes, bilinear intermediate, 128^2), method ig, steps 192, batch size 16, 3 prototype
targets.  Both arms are warmed up and alternated in one process, each repeat bracketed by device
events that end in a synchronise; the result is ms per map and the ratio torch / HIP.  Prints one
JSON line per setup.  For the per-kernel split run this script with --arm hip under
``rocprofv3 --kernel-trace --stats`` (a run of its own).

Usage:  python tools/attr_bench.py [--setup c2|c5|all] [--repeats 3] [--steps 192] [--batch-size 16]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import bench  # noqa: E402
from count_pipnet_amd.attribution import attribute  # noqa: E402
from count_pipnet_amd.backend import torch_backend  # noqa: E402
from count_pipnet_amd.synthetic import synth_images  # noqa: E402


def make(setup: str, dev):
    if setup == "c2":
        net, _ = bench.make_net(dev)
        return net, synth_images(1, 224, seed=21)[0].to(dev)
    net = bench.make_extra(bench.EXTRA["c5"], dev)
    return net, synth_images(1, 128, seed=16)[0].to(dev)


def timed(fn) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--setup", default="all", choices=("c2", "c5", "all"))
    ap.add_argument("--arm", default="both", choices=("both", "hip", "torch"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=192)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--method", default="ig")
    ap.add_argument("--targets", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for setup in (("c2", "c5") if a.setup == "all" else (a.setup,)):
        net, x = make(setup, dev)
        with torch.no_grad():
            pooled = net(x.unsqueeze(0), inference=True)[1][0]
        targets = torch.argsort(pooled, descending=True, stable=True)[:a.targets].tolist()   # the most active prototypes
        kw = dict(kind="prototype", method=a.method, steps=a.steps, batch_size=a.batch_size, seed=1)

        def hip():
            return attribute(net, x, targets, **kw)

        def torch_arm():
            with torch_backend():
                return attribute(net, x, targets, **kw)

        arms = {"hip": hip, "torch": torch_arm}
        if a.arm != "both":
            arms = {a.arm: arms[a.arm]}
        times = {k: [] for k in arms}
        for fn in arms.values():          # warm-up: weight caches, the allocator's pools
            fn()
        torch.cuda.synchronize()
        for _ in range(a.repeats):        # alternated
            for k, fn in arms.items():
                times[k].append(timed(fn))
        res = dict(setup=setup, method=a.method, steps=a.steps, batch_size=a.batch_size, targets=len(targets),
                   image=list(x.shape), device=torch.cuda.get_device_name(0))
        for k, v in times.items():
            res[f"{k}_ms_per_map"] = round(min(v) / len(targets), 2)
            res[f"{k}_ms_per_map_all"] = [round(t / len(targets), 2) for t in v]
        if len(arms) == 2:
            res["torch_over_hip"] = round(min(times["torch"]) / min(times["hip"]), 3)
            if not hasattr(net, "_max_count"):      # (the two arms of a Gumbel net draw different noise)
                h, t = hip(), torch_arm()
                res["maps_max_rel_diff"] = float((h.maps - t.maps).abs().max() / t.maps.abs().max())
        res["peak_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
        print(json.dumps(res), flush=True)
        del net


if __name__ == "__main__":
    main()
