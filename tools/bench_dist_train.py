"""What the data-parallel step's device work costs on ONE GPU (count_pipnet_amd.dist_train).

C2's model (PIP-Net ConvNeXt-tiny-26, 224x224, K = 200, P = 768), 64 images per view, the joint phase with the
reference's trainable set (features[6:] and the classifier):

  arm A  ``train.hip_train_step``: the plain single-device step;
  arm B  ``ShardedTraining(net, force_exchange=True).step`` at world 1: the sharded step's device work -- the packed
         ``[pooled | out | label]`` rows and their split copies, the loss on the "gathered" arrays, the row-sharded
         head backward (tanh coefficients computed once), the gradient arena's pack and the .grad views -- with the
         collectives themselves left out (there is one GPU).

The two arms alternate in one process, each on its own copy of the net and its own AdamW optimizers; every step is
timed with device events and ends in a synchronise; the figure is the median of ``--repeats`` steps per arm.

This says what sharding adds to a rank's own step.  It says NOTHING about scaling over several GPUs: no collective
runs here, and no multi-GPU node was available to measure one.

    python tools/bench_dist_train.py [--batch 64] [--repeats 5] [--warmup 2] [--out FILE]
Prints one JSON line (and writes it to FILE)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import torch  # noqa: E402

from bench_configs import CONFIGS, make  # noqa: E402
from count_pipnet_amd import build  # noqa: E402
from count_pipnet_amd import train as T  # noqa: E402
from count_pipnet_amd.dist_train import ShardedTraining  # noqa: E402
from count_pipnet_amd.synthetic import synth_images  # noqa: E402


def joint_setup(dev):
    """C2's net in the joint phase (main.py:377-390): features.6 / features.7 and the classifier train; the AdamW
    groups of util/args.py:get_optimizer_nn."""
    net = make(CONFIGS["c2"], dev).train()
    train, freeze, backbone = [], [], []
    for name, prm in net._net.named_parameters():
        (train if "features.7.2" in name else freeze if ("features.7" in name or "features.6" in name)
         else backbone).append(prm)
    for prm in net.parameters():
        prm.requires_grad = False
    cls = net._classification
    heads = list(net._add_on.parameters()) + [cls.weight] + ([] if cls.bias is None else [cls.bias])
    for prm in train + freeze + heads:
        prm.requires_grad = True
    opt_net = torch.optim.AdamW([{"params": backbone, "lr": 5e-4, "weight_decay": 0.0},
                                 {"params": freeze, "lr": 5e-4, "weight_decay": 0.0},
                                 {"params": train, "lr": 5e-4, "weight_decay": 0.0},
                                 {"params": list(net._add_on.parameters()), "lr": 5e-3, "weight_decay": 0.0}],
                                lr=5e-4, weight_decay=0.0)
    groups = [{"params": [cls.weight], "lr": 0.05, "weight_decay": 0.0}]
    if cls.bias is not None:
        groups.append({"params": [cls.bias], "lr": 0.05, "weight_decay": 0.0})
    return net, opt_net, torch.optim.AdamW(groups, lr=0.05, weight_decay=0.0)


def timed(fn) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64, help="images per view")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dist_train: no ROCm GPU visible (a CPU run says nothing about step time)")
    build.build()
    dev = torch.device("cuda", 0)
    size, classes = CONFIGS["c2"]["size"], CONFIGS["c2"]["classes"]
    xs1, xs2 = synth_images(a.batch, size, seed=1).to(dev), synth_images(a.batch, size, seed=2).to(dev)
    ys = torch.randint(0, classes, (a.batch,), generator=torch.Generator().manual_seed(3)).to(dev)
    net_a, on_a, oc_a = joint_setup(dev)
    net_b, on_b, oc_b = joint_setup(dev)
    gen_a = torch.Generator().manual_seed(5)
    sharded = ShardedTraining(net_b, seed=5, force_exchange=True)

    def arm_a():
        for o in (on_a, oc_a):
            o.zero_grad(set_to_none=True)
        T.hip_train_step(net_a, xs1, xs2, ys, on_a, oc_a, False, 1, 1, True, generator=gen_a)

    def arm_b():
        for o in (on_b, oc_b):
            o.zero_grad(set_to_none=True)
        sharded.step(xs1, xs2, ys, on_b, oc_b, phase="train", epoch=1, nr_epochs=1)

    for _ in range(a.warmup):
        arm_a()
        arm_b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(a.repeats):
        ta.append(timed(arm_a))
        tb.append(timed(arm_b))
    arena = sharded._arena
    res = dict(tool="bench_dist_train", config="c2 joint", batch_per_view=a.batch, repeats=a.repeats,
               device=torch.cuda.get_device_name(0),
               plain_step_ms=round(statistics.median(ta), 3), plain_step_ms_all=[round(t, 3) for t in ta],
               sharded_world1_step_ms=round(statistics.median(tb), 3), sharded_step_ms_all=[round(t, 3) for t in tb],
               arena_tensors=len(arena.params), arena_floats=arena.numel, arena_mib=round(arena.numel * 4 / 2 ** 20, 2),
               collectives="none run (one GPU): multi-GPU scaling is not measured")
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
