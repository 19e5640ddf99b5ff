"""Cost of the part-purity evaluation on one GPU at C2's shape (PIP-Net ConvNeXt-tiny-26, 224x224,
batch 64, P = 768 prototypes on a 26 x 26 map) with CUB-sized synthetic annotations (N = 11,788
images, Q = 15 part ids, 3 left/right pairs), threshold 0.5.

(1) the update kernel alone: event-timed per batch of ``pipnet_part_purity_update`` on [64, 768]
    scores of which a given share fires (0: the floor of loads and the vote; 2 % is what a trained
    PIP-Net's sparse scores give; 100 %: every row read-modify-writes its state), and its share of
    one C2 forward at the same batch.
(2) ``pipnet_part_purity_rows`` at k = 10 and ``pipnet_part_purity_finish``.
(3) the host restatement (tests/part_purity_ref.py) on the rows of (2), for scale.
(4) a ``part_purity`` pass over device-resident batches against a loop of plain forwards over the
    same batches; host clock around work that ends in a device synchronise, the arms alternated,
    median of the repeats.

    python tools/bench_part_purity.py [--batches 6] [--repeats 5] [--kernels-only]
Prints one JSON line per measurement."""
from __future__ import annotations

import argparse
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
from bench_proto_stats import event_ms, wall_ms  # noqa: E402
from count_pipnet_amd import build  # noqa: E402
from count_pipnet_amd import kernels as K  # noqa: E402
from count_pipnet_amd.purity import PartAnnotations, part_purity  # noqa: E402
from count_pipnet_amd.synthetic import synth_images  # noqa: E402
from part_purity_util import geometry, make_table, restate_rows, rows_topk  # noqa: E402

CUB_PARTS = ["back", "beak", "belly", "breast", "crown", "forehead", "left eye", "left leg", "left wing", "nape",
             "right eye", "right leg", "right wing", "tail", "throat"]


def synthetic_table(n, seed=0):
    """CUB-shaped annotations: image sizes around 500 x 375, about 80 % of the parts visible."""
    rng = np.random.default_rng(seed)
    size = np.stack([rng.integers(300, 501, n), rng.integers(250, 501, n)], axis=1)
    xy = rng.random((n, len(CUB_PARTS), 2)) * size[:, None, :]
    return make_table(np.round(xy, 1), rng.random((n, len(CUB_PARTS))) < 0.8, size, CUB_PARTS)


def annotations_of(table):
    t = {k: torch.from_numpy(table[k]) for k in ("xy", "vis", "size", "merged", "is_left", "pair_index")}
    names = table["names"]
    return PartAnnotations(part_ids=table["ids"], part_names=names, merged_ids=[table["ids"][q] for q in table["keep"]],
                           merged_names=[names[q] for q in table["keep"]],
                           image_keys=[f"c/{i}.jpg" for i in range(table["vis"].shape[0])], **t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    build.build()
    dev = torch.device("cuda:0")
    cfg = CONFIGS["c2"]
    b, pn, hw, n_img, k = cfg["batch"], 768, 26, 11788, 10
    geo = geometry(hw, hw, cfg["size"])
    table = synthetic_table(n_img)
    ann = annotations_of(table).to(dev)
    m = len(table["keep"])
    base = dict(config="c2", batch=b, prototypes=pn, map=hw, parts=len(CUB_PARTS), merged=m, images=n_img)
    g = torch.Generator().manual_seed(1)
    relevant = torch.ones(pn, dtype=torch.uint8, device=dev)

    net = make(cfg, dev)
    assert net._num_prototypes == pn
    xs = synth_images(b, cfg["size"], seed=50).to(dev)

    def forward():
        with torch.no_grad():
            net(xs, inference=True)

    fwd_ms, fwd_lo, fwd_hi = event_ms(forward, 20, 3)
    print(json.dumps(dict(base, what="forward", ms_median=fwd_ms, ms_min=fwd_lo, ms_max=fwd_hi)), flush=True)

    # (1) the update kernel alone
    loc = torch.randint(0, hw * hw, (b, pn), generator=g, dtype=torch.int32).to(dev)
    for share in (0.0, 0.02, 0.2, 1.0):
        u = torch.rand(b, pn, generator=g)
        pooled = torch.where(torch.rand(b, pn, generator=g) < share, 0.5 + 0.5 * u, 0.5 * u).to(dev)
        st = K.PartPurityState(pn, m, dev)
        step = [0]

        def update():
            K.part_purity_update(st, pooled, loc, relevant, (step[0] * b) % (n_img - b), 0.5, geo, ann.table())
            step[0] += 1

        med, lo, hi = event_ms(update, 200, 20)
        print(json.dumps(dict(base, what="update_kernel", firing_share=share, rows_per_batch=int((pooled > 0.5).sum()),
                              ms_median=med, ms_min=lo, ms_max=hi, pct_of_forward=100.0 * med / fwd_ms)), flush=True)

    # (2) rows at k = 10 and finish, (3) the host restatement on the same rows
    index = torch.randint(0, n_img, (pn, k), generator=g).to(dev)
    kloc = torch.randint(0, hw * hw, (pn, k), generator=g, dtype=torch.int32).to(dev)
    st = K.PartPurityState(pn, m, dev)
    med, lo, hi = event_ms(lambda: K.part_purity_rows(st, index, kloc, relevant, geo, ann.table()), 200, 20)
    print(json.dumps(dict(base, what="rows_kernel", k=k, rows=pn * k, ms_median=med, ms_min=lo, ms_max=hi)), flush=True)
    med, lo, hi = event_ms(lambda: K.part_purity_finish(st), 200, 20)
    print(json.dumps(dict(base, what="finish_kernel", ms_median=med, ms_min=lo, ms_max=hi)), flush=True)
    rows = rows_topk(index.cpu().numpy(), kloc.cpu().numpy(), np.ones(pn, bool), geo, n_img)
    t0 = time.perf_counter()
    restate_rows(rows, table, cfg["size"])
    print(json.dumps(dict(base, what="host_restatement", rows=len(rows), ms=(time.perf_counter() - t0) * 1e3)),
          flush=True)
    if a.kernels_only:
        return

    # (4) the pass against plain forwards
    batches = [(synth_images(b, cfg["size"], seed=50 + i).to(dev), torch.zeros(b, dtype=torch.int64))
               for i in range(a.batches)]
    small = annotations_of(synthetic_table(b * a.batches, seed=1))

    def forwards():
        with torch.no_grad():
            for x, _ in batches:
                net(x, inference=True)

    for mode in ("all", "topk"):
        def purity_pass():
            part_purity(net, batches, small, image_size=cfg["size"], mode=mode, k=k)

        forwards()
        purity_pass()
        t_fwd, t_pass = [], []
        for _ in range(a.repeats):
            t_fwd.append(wall_ms(forwards))
            t_pass.append(wall_ms(purity_pass))
        fwd, pas = statistics.median(t_fwd), statistics.median(t_pass)
        print(json.dumps(dict(base, what="pass_vs_forwards", mode=mode, batches=a.batches, images=b * a.batches,
                              forwards_ms=fwd, purity_pass_ms=pas, overhead_pct=100.0 * (pas - fwd) / fwd,
                              forwards_all_ms=t_fwd, purity_pass_all_ms=t_pass)), flush=True)


if __name__ == "__main__":
    main()
