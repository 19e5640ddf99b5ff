#!/usr/bin/env python
"""Time the three ConvNeXt builds -- fp32, bf16x3 (split bf16) and bf16 -- on the same net and the same
inputs in one process:  python tools/bench_convnext_precisions.py [--repeats 3] [--arms bf16] [--out FILE]

Shapes: BASELINE C2 (PIP-Net ConvNeXt-tiny-26, batch 64, 224^2, 200 classes) and a C5 shard (CountPIPNet
bilinear, 2048 prototypes, batch 64, 128^2) -- bench.py's make_net / EXTRA["c5"] definitions.
Each arm is warmed up, then the arms alternate (fp32, bf16x3, bf16, fp32, ...) ``--repeats`` times; one
repeat of an arm is at least a second of forwards between two device events, ended by a synchronise.
Prints img/s and ms per step per arm with the spread over the repeats.  ``--arms`` picks the arms (one
arm alone: a per-kernel rocprofv3 run of that build).  There is no CPU path: without a GPU it fails.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

ARMS = ("fp32", "bf16x3", "bf16")


def make(shape, dev):
    import bench
    from count_pipnet_amd.synthetic import synth_images
    if shape == "c2":
        net, _ = bench.make_net(dev)
        return net, synth_images(64, 224, seed=7).to(dev)
    cfg = bench.EXTRA["c5"]
    return bench.make_extra(cfg, dev), synth_images(cfg["batch"], cfg["size"], seed=7).to(dev)


def timed(net, xs, steps):
    """ms per forward over ``steps`` forwards between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        net(xs, inference=True)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=3, help="alternations of the arms (>= 3 for a spread)")
    ap.add_argument("--seconds", type=float, default=1.0, help="least device time of one repeat of one arm")
    ap.add_argument("--shapes", default="c2,c5")
    ap.add_argument("--arms", default=",".join(ARMS), help="comma list out of " + ", ".join(ARMS))
    ap.add_argument("--out", help="also write the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_convnext_precisions: no ROCm GPU visible (there is no CPU path to time)")
    from count_pipnet_amd import build
    from count_pipnet_amd.pipnet import set_hip_dtype
    build.build()
    dev = torch.device("cuda:0")
    arms = tuple(a.arms.split(","))
    if not arms or any(arm not in ARMS for arm in arms):
        raise SystemExit(f"bench_convnext_precisions: --arms takes a comma list out of {ARMS}")
    lines = [f"# {torch.cuda.get_device_name(0)}; arms alternated {a.repeats}x, >= {a.seconds:g} s of forwards per "
             f"repeat, device events + synchronise; spread = min..max over the repeats",
             f"{'shape':5} {'arm':7} {'ms/step':>9} {'img/s':>9} {'spread ms':>19} {'steps':>6}  vs bf16x3"]
    with torch.no_grad():
        for shape in a.shapes.split(","):
            net, xs = make(shape, dev)
            steps, ms = {}, {arm: [] for arm in arms}
            for arm in arms:                                  # warm-up: weight caches, then the step count
                set_hip_dtype(net, arm)
                for _ in range(3):
                    net(xs, inference=True)
                torch.cuda.synchronize()
                steps[arm] = max(3, int(a.seconds * 1e3 / timed(net, xs, 5)) + 1)
            for _ in range(a.repeats):
                for arm in arms:
                    set_hip_dtype(net, arm)
                    ms[arm].append(timed(net, xs, steps[arm]))
            med = {arm: sorted(v)[len(v) // 2] for arm, v in ms.items()}
            for arm in arms:
                ratio = f"{med['bf16x3'] / med[arm]:.2f}x" if "bf16x3" in med else "-"
                lines.append(f"{shape:5} {arm:7} {med[arm]:9.3f} {xs.shape[0] / med[arm] * 1e3:9.0f} "
                             f"{min(ms[arm]):9.3f}..{max(ms[arm]):<8.3f} {steps[arm]:6d}  {ratio}")
            del net, xs
    report = "\n".join(lines)
    print(report, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
