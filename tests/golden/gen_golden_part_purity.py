"""Golden fixtures for the prototype part-purity evaluation (count_pipnet_amd/purity.py), recorded
by running the REFERENCE's own, unchanged ``util/eval_cub_csv.py`` on CPU:
``get_proto_patches_cub`` ("all"), ``get_topk_cub`` ("topk", batch-1 loader as it assumes) and
``eval_prototypes_cub_parts_csv`` on both CSVs.

For each case the reference model of a forward golden case (gen_golden.CASES, same synthetic
weights) gets a copy of its classification weight in which a few columns are zeroed (irrelevant
prototypes).  The dataset is the first ``images`` tensors of ``golden_util.eval_loader_batches``;
tiny image files of distinct, non-square original sizes (larger and smaller than the network's
image size) are written to a temporary directory in CUB-style ``class/file`` folders, with a
synthetic ``images.txt``, CUB's 15 part names and a seeded ``part_locs.txt`` planted with: one
image without visible part (the only image one prototype fires on: an in-csv prototype with an
empty part dict), images with only the left / only the right / both members of a pair, and, for
four rows, one part exactly on each border of the scaled patch plus one a single ulp outside it.

``torchvision.transforms`` is absent here: an empty stand-in module is registered in ``sys.modules``
before ``util.eval_cub_csv`` is imported.  ``print`` in the reference module's namespace is
replaced by a recorder, so the printed per-prototype dicts are kept as objects; ``log`` records the
logged tuple; the network is called through a wrapper that keeps what every forward returned.

Decisiveness: the product's forward agrees with this CPU run to 1e-3; the fixture keeps a
fourfold margin.  Threshold, k and the zeroed columns are searched until
  * no relevant pooled value lies within 4e-3 of the threshold,
  * for every row the two largest values of its prototype's map differ by at least 4e-3,
  * in "topk" mode the k-th and (k+1)-th scores and any adjacent kept scores differ by at least 4e-3,
  * no classification column maximum lies within 1e-6 of 1e-5,
with at least 30 rows per mode and, in mode "all" (in "topk" every relevant prototype has rows), a
relevant prototype without row and an in-csv prototype with an empty part dict.

Usage:  python tests/golden/gen_golden_part_purity.py
"""
from __future__ import annotations

import argparse
import contextlib
import csv
import io
import json
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True            # the reference tree is read-only
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import gen_golden as G  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
from golden_util import eval_loader_batches  # noqa: E402

# name -> (forward golden case, batches, batch size, images, label seed, parts seed)
PURITY_CASES = {
    "pipnet_mid_addon": ("pipnet_mid_addon", 3, 5, 14, 311, 7),
}
OUT = os.path.join(HERE, "part_purity")
MARGIN = 4e-3
RELEVANCE = 1e-5
PATCH = 32
THRESHOLDS = (0.5, 0.45, 0.55, 0.4, 0.6)
KS = (3, 2, 4, 5)
MAX_ZEROED = 8
COORD_SHAPES = [(768, 26, 224), (26, 26, 224), (2048, 7, 224), (768, 13, 224)]     # (P, H = W, image size)
PLANNED_ZERO = 2              # columns zeroed whatever the search finds
CUB_PARTS = ["back", "beak", "belly", "breast", "crown", "forehead", "left eye", "left leg", "left wing", "nape",
             "right eye", "right leg", "right wing", "tail", "throat"]


class _Keep(nn.Module):
    """The ``net.module`` wrapper the reference expects; keeps every forward's (proto map, pooled)."""

    def __init__(self, net):
        super().__init__()
        self.module = net
        self.calls = []

    def forward(self, xs):
        pfs, pooled, out = self.module(xs)
        self.calls.append((pfs.detach().clone(), pooled.detach().clone()))
        return pfs, pooled, out


class _Dataset(torch.utils.data.Dataset):
    def __init__(self, xs, ys, paths):
        self.xs, self.ys = xs, ys
        self.imgs = [(p, int(y)) for p, y in zip(paths, ys)]

    def __len__(self):
        return len(self.imgs)

    def __getitem__(self, i):
        return self.xs[i], self.ys[i]


class _Log:
    def __init__(self):
        self.rows = []

    def log_values(self, name, *values):
        self.rows.append((name, values))


def two_step_loc(pfs):
    """[P] h_idx * W + w_idx by the reference's two torch.max calls (eval_cub_csv.py:209-211)."""
    location_h, location_h_idx = torch.max(pfs, dim=1)
    _, location_w_idx = torch.max(location_h, dim=1)
    h_idx = location_h_idx.gather(1, location_w_idx[:, None])[:, 0]
    return (h_idx * pfs.shape[2] + location_w_idx).numpy().astype(np.int32)


def choose(pooled, top2gap, wmax):
    """(threshold, k, zeroed columns): the first combination under which every decisiveness
    condition holds for the prototypes left relevant."""
    n, pn = pooled.shape
    assert not (np.abs(wmax - RELEVANCE) < 1e-6).any()
    planned = list(np.argsort(pooled.max(axis=0))[-PLANNED_ZERO:])          # two strongly firing prototypes
    order = np.argsort(-pooled, axis=0, kind="stable")
    srt = np.take_along_axis(pooled, order, axis=0)
    for thr in THRESHOLDS:
        for k in KS:
            bad = set(planned)
            for p in range(pn):
                if (np.abs(pooled[:, p] - thr) < MARGIN).any():
                    bad.add(p)
                if (top2gap[pooled[:, p] > thr, p] < MARGIN).any():
                    bad.add(p)
                if (top2gap[order[:k, p], p] < MARGIN).any():
                    bad.add(p)
                if (srt[:k, p] - srt[1:k + 1, p] < MARGIN).any():
                    bad.add(p)
            rel = np.array([p not in bad for p in range(pn)])
            fires = (pooled > thr) & rel[None]
            per = fires.sum(axis=0)
            if len(bad) <= MAX_ZEROED and fires.sum() >= 30 and rel.sum() * k >= 30 and (rel & (per == 0)).any() \
                    and (rel & (per == 1)).any():
                return thr, k, sorted(int(p) for p in bad)
    raise AssertionError("no decisive (threshold, k, zeroed columns) found: change the seeds")


def patch_of(size, shape, skip, loc):
    from util.vis_pipnet import get_img_coordinates
    return get_img_coordinates(size, shape, PATCH, skip, int(loc) // shape[2], int(loc) % shape[2])


def plant_parts(rng, sizes, fires, loc, size, shape, skip):
    """vis [N,15] bool, xy [N,15,2]: seeded annotations with the planted cases; returns them and
    the list of planted (image, part index, what)."""
    n = len(sizes)
    q = len(CUB_PARTS)
    vis = rng.random((n, q)) < 0.6
    xy = np.stack([np.round(rng.random((n, q)) * np.array([w for w, _ in sizes])[:, None], 1),
                   np.round(rng.random((n, q)) * np.array([h for _, h in sizes])[:, None], 1)], axis=-1)
    planted = []
    per = fires.sum(axis=0)
    lonely = int(np.flatnonzero(per == 1)[0])                 # fires on one image only
    empty_img = int(np.flatnonzero(fires[:, lonely])[0])
    vis[empty_img] = False
    planted.append((empty_img, -1, f"no visible part (the only image of prototype {lonely})"))
    free = [i for i in range(n) if i != empty_img]
    le, re = CUB_PARTS.index("left eye"), CUB_PARTS.index("right eye")
    for i, (l, r, what) in zip(free[:3], [(True, False, "left eye only"), (False, True, "right eye only"),
                                          (True, True, "both eyes")]):
        vis[i, le], vis[i, re] = l, r
        planted.append((i, le, what))
    rows = [(i, p) for i in free[3:] for p in np.flatnonzero(fires[i])]
    used = set()
    for b, what in enumerate(("top", "bottom", "left", "right")):
        i, p = next((i, p) for i, p in rows if i not in used)
        used.add(i)
        w, h = sizes[i]
        h0, h1, w0, w1 = patch_of(size, shape, skip, loc[i, p])
        ys = ((h / float(size)) * h0, (h / float(size)) * h1)
        xs = ((w / float(size)) * w0, (w / float(size)) * w1)
        unpaired = [q for q, nm in enumerate(CUB_PARTS) if "left" not in nm and "right" not in nm]
        on, off = unpaired[2 * b], unpaired[2 * b + 1]       # two unpaired ids per border
        mid_x, mid_y = (xs[0] + xs[1]) / 2, (ys[0] + ys[1]) / 2
        if what == "top":
            xy[i, on], xy[i, off] = (mid_x, ys[0]), (mid_x, np.nextafter(ys[0], -np.inf))
        elif what == "bottom":
            xy[i, on], xy[i, off] = (mid_x, ys[1]), (mid_x, np.nextafter(ys[1], np.inf))
        elif what == "left":
            xy[i, on], xy[i, off] = (xs[0], mid_y), (np.nextafter(xs[0], -np.inf), mid_y)
        else:
            xy[i, on], xy[i, off] = (xs[1], mid_y), (np.nextafter(xs[1], np.inf), mid_y)
        vis[i, on] = vis[i, off] = True
        planted.append((i, on, f"on the {what} border of prototype {int(p)}'s patch; id {off + 1} one ulp outside"))
    return vis, xy, planted


def write_dataset(tmp, ys, sizes, vis, xy):
    """Image files and the three annotation files; returns (image paths, the files' texts)."""
    from PIL import Image
    paths, images_txt, locs = [], [], []
    for i, ((w, h), y) in enumerate(zip(sizes, ys)):
        cls = f"{int(y) + 1:03d}.Class_{int(y)}"
        os.makedirs(os.path.join(tmp, "dataset", cls), exist_ok=True)
        fname = f"Bird_{i:04d}.png"
        on_disk = ("normal_" + fname) if i == 1 else fname       # the reference strips this prefix
        path = os.path.join(tmp, "dataset", cls, on_disk)
        Image.new("RGB", (w, h), (i, 2 * i, 3 * i)).save(path)
        paths.append(path)
        images_txt.append(f"{i + 1} {cls}/{fname}")
        for q in range(len(CUB_PARTS)):
            x, yv = (repr(float(xy[i, q, 0])), repr(float(xy[i, q, 1]))) if vis[i, q] else ("0.0", "0.0")
            locs.append(f"{i + 1} {q + 1} {x} {yv} {int(vis[i, q])}")
    texts = dict(images="\n".join(images_txt) + "\n",
                 parts="\n".join(f"{q + 1} {name}" for q, name in enumerate(CUB_PARTS)) + "\n",
                 part_locs="\n".join(locs) + "\n")
    files = {}
    for key, text in texts.items():
        files[key] = os.path.join(tmp, key + ".txt")
        with open(files[key], "w") as f:
            f.write(text)
    return paths, texts, files


def read_csv(path, paths):
    index = {p: i for i, p in enumerate(paths)}
    with open(path, newline="") as f:
        rd = csv.reader(f, delimiter=",")
        header = next(rd)
        rows = [[int(p), index[name], int(a), int(b), int(c), int(d)] for p, name, a, b, c, d in rd]
    return header, np.array(rows, dtype=np.int64).reshape(-1, 6)


def evaluate(E, csvfile, files, args):
    """eval_prototypes_cub_parts_csv with print and log recorded: (printed dicts, logged tuple)."""
    printed = []
    log = _Log()
    E.print = lambda *a, **kw: printed.append(a)
    try:
        E.eval_prototypes_cub_parts_csv(csvfile, files["part_locs"], files["parts"], files["images"], 0, args, log)
    finally:
        del E.print
    by_label = {a[0]: a[1:] for a in printed if a and isinstance(a[0], str)}
    max_part = by_label["Prototypes with highest-purity part (no contraints): "][0]
    most = by_label["Prototype with part that has most often overlap with prototype: "][0]
    n_protos = by_label["Number of prototypes in parts_presences: "][0]
    values = log.rows[1][1]
    assert log.rows[1][0] == "log_epoch_overview" and values[0] == "p_cub_0"
    logged = [float(v) for v in values[1:5]] + [int(values[5]), int(values[6])]
    assert n_protos == logged[4]
    return (dict(max_part={str(k): str(v) for k, v in max_part.items()},
                 most_part={str(k): [str(v[0]), int(v[1])] for k, v in most.items()},
                 order=[str(k) for k in most]), logged)


def run(name):
    fwd_case, nb, bs, n_img, label_seed, parts_seed = PURITY_CASES[name]
    net, case = G.build_reference(fwd_case)
    sys.modules.setdefault("torchvision.transforms", types.ModuleType("torchvision.transforms"))
    import util.eval_cub_csv as E
    size = case["size"]
    batches = eval_loader_batches(size, case["num_classes"], nb, bs, label_seed)
    xs = torch.cat([x for x, _ in batches])[:n_img]
    ys = torch.cat([y for _, y in batches])[:n_img]
    with torch.no_grad():                                    # image by image, as the reference will run it
        singles = [net(xs[i:i + 1])[:2] for i in range(n_img)]
    pfs, pooled_t = torch.cat([s[0] for s in singles]), torch.cat([s[1] for s in singles])
    shape = tuple(pfs.shape[1:])                             # the 3-D shape eval_cub_csv.py hands on
    pooled = pooled_t.numpy()
    top2 = torch.topk(pfs.flatten(2), 2, dim=2).values
    top2gap = (top2[..., 0] - top2[..., 1]).numpy()
    loc = np.stack([two_step_loc(pfs[i]) for i in range(n_img)])
    weight = net._classification.weight.detach().clone()
    thr, k, zeroed = choose(pooled, top2gap, weight.max(dim=0).values.numpy())
    weight[:, zeroed] = 0.0
    with torch.no_grad():
        net._classification.weight.copy_(weight)
    rel = (weight.max(dim=0).values > RELEVANCE).numpy()
    fires = (pooled > thr) & rel[None]

    args = argparse.Namespace(image_size=size, wshape=shape[2], use_mid_layers=case.get("use_mid_layers", False),
                              num_stages=case.get("num_stages", 0))
    _, skip = E.get_patch_size(args)
    rng = np.random.default_rng(parts_seed)
    sizes = [(40 + 9 * i, 120 - 7 * i) for i in range(n_img)]       # (width, height): 40 x 120 ... 157 x 29
    vis, xy, planted = plant_parts(rng, sizes, fires, loc, size, shape, skip)
    rec, modes = {}, {}
    quiet = (contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()))
    with tempfile.TemporaryDirectory() as tmp, quiet[0], quiet[1]:
        paths, texts, files = write_dataset(tmp, ys, sizes, vis, xy)
        args.log_dir = tmp
        ds = _Dataset(xs, ys, paths)
        loader = torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False)
        keep = _Keep(net)
        for mode in ("all", "topk"):
            keep.calls.clear()
            if mode == "all":
                csvfile = E.get_proto_patches_cub(keep, loader, 0, torch.device("cpu"), args, threshold=thr)
            else:
                csvfile = E.get_topk_cub(keep, loader, k, 0, torch.device("cpu"), args)
            seen = keep.calls[:n_img]                       # the pass over the dataset, in order
            m_pooled = torch.cat([c[1] for c in seen]).numpy()
            m_loc = np.stack([two_step_loc(c[0][0]) for c in seen])
            assert np.array_equal(m_pooled, pooled) and np.array_equal(m_loc, loc)
            header, rows = read_csv(csvfile, paths)
            dicts, logged = evaluate(E, csvfile, files, args)
            rec[f"{mode}_rows"], rec[f"{mode}_pooled"], rec[f"{mode}_loc"] = rows, m_pooled, m_loc
            modes[mode] = dict(header=header, logged=logged, **dicts)
    # what was asked of the fixture
    for mode in ("all", "topk"):
        rows = rec[f"{mode}_rows"]
        assert len(rows) >= 30, (mode, len(rows))
        assert (top2gap[rows[:, 1], rows[:, 0]] >= MARGIN).all()
        assert rel[rows[:, 0]].all()
    assert not (np.abs(pooled[:, rel] - thr) < MARGIN).any()
    srt = -np.sort(-pooled[:, rel], axis=0)
    assert (srt[:k] - srt[1:k + 1] >= MARGIN).all()
    in_csv = set(int(p) for p in rec["all_rows"][:, 0])
    assert any(p not in in_csv for p in np.flatnonzero(rel)), "no relevant prototype without row"
    empty = [p for p in modes["all"]["order"] if p not in modes["all"]["max_part"]]
    assert empty, "no in-csv prototype with an empty part dict"
    assert len(rec["all_rows"]) == int(fires.sum()) and len(rec["topk_rows"]) == int(rel.sum()) * k

    # the patch of every latent location under the 3-D map shape eval_cub_csv.py hands on, for the
    # fixture's map and for the maps of the full backbones (26 x 26: the small-stride rule)
    for pn, hw, image_size in [(shape[0], shape[1], size)] + COORD_SHAPES:
        a = argparse.Namespace(image_size=image_size, wshape=hw, use_mid_layers=False, num_stages=0)
        rec[f"coords_{pn}_{hw}_{image_size}"] = np.array(
            [patch_of(image_size, (pn, hw, hw), E.get_patch_size(a)[1], l) for l in range(hw * hw)], dtype=np.int32)
    rec["weight"] = weight.numpy()
    rec["sizes"] = np.array(sizes, dtype=np.int32)
    meta = dict(name=name, forward_case=fwd_case, batches=nb, batch_size=bs, images=n_img, label_seed=label_seed,
                parts_seed=parts_seed, threshold=thr, k=k, zeroed=zeroed, relevance=RELEVANCE, skip=int(skip),
                map_shape=list(shape), image_paths=[os.path.relpath(p, os.path.join(os.path.dirname(p), "..", ".."))
                                                    for p in paths],
                files=texts, planted=[[int(i), int(q), what] for i, q, what in planted], empty_dict=empty,
                modes=modes)
    rec["meta"] = np.array(json.dumps(meta))
    return rec


def main():
    torch.set_num_threads(os.cpu_count() or 8)
    for name in PURITY_CASES:
        rec = run(name)
        os.makedirs(OUT, exist_ok=True)
        path = os.path.join(OUT, f"{name}.npz")
        np.savez_compressed(path, **rec)
        meta = json.loads(str(rec["meta"]))
        print(f"wrote {path} ({os.path.getsize(path) / 1e3:.1f} kB): threshold {meta['threshold']}, k {meta['k']}, "
              f"zeroed {meta['zeroed']}, rows {len(rec['all_rows'])} / {len(rec['topk_rows'])}, "
              f"logged {meta['modes']['all']['logged']} / {meta['modes']['topk']['logged']}", flush=True)


if __name__ == "__main__":
    main()
