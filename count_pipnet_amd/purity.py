"""Prototype part purity on CUB-style part annotations, on the device -- ``util/eval_cub_csv.py``.

The reference writes a CSV of image patches from batch-1 forwards (``get_proto_patches_cub``: every
(image, relevant prototype) with a pooled score above a threshold; ``get_topk_cub``: the k best
images of every relevant prototype), then ``eval_prototypes_cub_parts_csv`` re-reads it, opens every
image for its size and loops over nested dicts.  ``part_purity`` computes the same numbers in one
pass at any batch size with no host synchronisation inside the loop:

  batch-invariant forward with patch locations (explain_forward.located_forward)
    "all"   -> pipnet_part_purity_update per batch
    "topk"  -> pipnet_topk_update per batch, one pipnet_part_purity_rows at the end
  -> pipnet_part_purity_finish

Everything the reference reports reduces, per (prototype, merged part), to three integers (rows in
which the part is visible, rows in which it lies in the patch, and the key of its first
appearance, which fixes the dict order the tie rules depend on), each accumulated by one owner
thread in dataset order: the result is bitwise independent of the batch size.

``write_patch_csv`` / ``eval_patch_csv`` keep the CSV route open for other part-prototype methods.
"""
from __future__ import annotations

import csv
from dataclasses import dataclass, fields
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import kernels as K
from .dist import ShardedPass
from .explain_forward import (PATCH_SIZE, HostCopy, check_first_index, img_coordinates, is_count, located_forward,
                              patch_skip, small_map, unwrap_sharded)

CSV_HEADER = ["prototype", "img name", "h_min_224", "h_max_224", "w_min_224", "w_max_224"]


def image_key(path: str) -> str:
    """``class/file`` of an image path as eval_cub_csv.py:68-72 forms it: the last two components,
    a ``normal_`` prefix of the file name dropped."""
    cls, fname = path.replace("\\", "/").split("/")[-2:]
    if "normal_" in fname:
        fname = fname.split("normal_")[-1]
    return cls + "/" + fname


@dataclass
class PartAnnotations:
    """The part annotations of a whole dataset, image n = the n-th image of the loader.
    N images, Q part ids (in the order of the part-name file), M merged parts (every id whose name
    contains ``left`` is folded into the id named with ``right`` in its place)."""
    xy: Tensor            # [N, Q, 2] float64 (x, y)
    vis: Tensor           # [N, Q] uint8
    size: Tensor          # [N, 2] int32 (width, height) of the original image
    merged: Tensor        # [Q] int32 merged part of each id
    is_left: Tensor       # [Q] uint8
    pair_index: Tensor    # [Q] int32 index of a left id's pair, in pair order (0 elsewhere)
    part_ids: List[str]   # [Q] the ids as written in the files
    part_names: List[str]         # [Q]
    merged_ids: List[str]         # [M] the id that stands for each merged part
    merged_names: List[str]       # [M]
    image_keys: List[str]         # [N] class/file

    @property
    def images(self) -> int:
        return self.vis.shape[0]

    def to(self, device) -> "PartAnnotations":
        return PartAnnotations(**{f.name: (getattr(self, f.name).to(device) if torch.is_tensor(getattr(self, f.name))
                                           else getattr(self, f.name)) for f in fields(self)})

    def table(self):
        return (self.xy, self.vis, self.size, self.merged, self.is_left, self.pair_index)

    def visible_parts(self, n: int) -> Dict[str, Tuple[float, float]]:
        """{part id: (x, y)} of image n's visible parts, in file order (the reference's dict)."""
        vis, xy = self.vis[n].tolist(), self.xy[n].tolist()
        return {self.part_ids[q]: (xy[q][0], xy[q][1]) for q in range(len(vis)) if vis[q]}

    @staticmethod
    def from_cub(parts_loc_path: str, parts_name_path: str, imgs_id_path: str, image_paths: Sequence[str],
                 image_sizes: Optional[Sequence[Tuple[int, int]]] = None) -> "PartAnnotations":
        """Parse CUB's ``parts/part_locs.txt``, ``parts/parts.txt`` and ``images.txt`` as
        eval_cub_csv.py:19-55 does.  ``image_paths``: the dataset's image files in loader order
        (``dataset.imgs[n][0]``), matched by their last two path components.  ``image_sizes``:
        (width, height) per image; None reads each file's header with Pillow (no decode)."""
        path_to_id = {}
        with open(imgs_id_path) as f:
            for line in f:
                img_id, path = line.split("\n")[0].split(" ")
                path_to_id[path] = img_id
        part_ids, part_names = [], []
        with open(parts_name_path) as f:
            for line in f:
                pid, name = line.split("\n")[0].split(" ", 1)
                part_ids.append(pid)
                part_names.append(name)
        q_of = {pid: q for q, pid in enumerate(part_ids)}
        name_to_q = {name: q for q, name in enumerate(part_names)}
        nq = len(part_ids)
        if not 1 <= nq <= K.PART_PURITY_MAX_PARTS:
            raise ValueError(f"part annotations: {nq} part ids, supported 1..{K.PART_PURITY_MAX_PARTS}")
        pairs = []                                   # (left q, right q) in file order
        for q, name in enumerate(part_names):
            if "left" in name:
                partner = name.replace("left", "right")
                if partner not in name_to_q:
                    raise ValueError(f"part annotations: part {part_ids[q]} '{name}' has no partner '{partner}'")
                pairs.append((q, name_to_q[partner]))
        left = {lq: i for i, (lq, _) in enumerate(pairs)}
        right_of = dict(pairs)
        keep = [q for q in range(nq) if q not in left]
        m_of = {q: m for m, q in enumerate(keep)}
        merged = [m_of[right_of[q]] if q in left else m_of[q] for q in range(nq)]

        per_image: Dict[str, list] = {}
        with open(parts_loc_path) as f:
            for line in f:
                img, pid, x, y, vis = line.split("\n")[0].split(" ")
                rows = per_image.setdefault(img, [])
                if pid not in q_of:
                    raise ValueError(f"part annotations: image {img} names the unknown part id {pid}")
                q = q_of[pid]
                if rows and q <= rows[-1][0]:
                    raise ValueError(f"part annotations: the parts of image {img} are not in ascending part id "
                                     f"({part_ids[rows[-1][0]]} before {pid})")
                rows.append((q, float(x), float(y), vis == "1"))

        n = len(image_paths)
        if image_sizes is not None and len(image_sizes) != n:
            raise ValueError(f"part annotations: {len(image_sizes)} image sizes for {n} images")
        xy = torch.zeros((n, nq, 2), dtype=torch.float64)
        vis_t = torch.zeros((n, nq), dtype=torch.uint8)
        size = torch.zeros((n, 2), dtype=torch.int32)
        keys = []
        for i, path in enumerate(image_paths):
            key = image_key(path)
            if key not in path_to_id:
                raise ValueError(f"part annotations: image '{key}' ({path}) is not in {imgs_id_path}")
            img_id = path_to_id[key]
            if img_id not in per_image:
                raise ValueError(f"part annotations: image {img_id} '{key}' has no line in {parts_loc_path}")
            for q, x, y, v in per_image[img_id]:
                if v:
                    xy[i, q, 0], xy[i, q, 1], vis_t[i, q] = x, y, 1
            if image_sizes is not None:
                w, h = image_sizes[i]
            else:
                from PIL import Image
                with Image.open(path) as im:         # the header only: no pixel is decoded
                    w, h = im.size
            size[i, 0], size[i, 1] = int(w), int(h)
            keys.append(key)
        pair_index = [left.get(q, 0) for q in range(nq)]
        return PartAnnotations(
            xy=xy, vis=vis_t, size=size, merged=torch.tensor(merged, dtype=torch.int32),
            is_left=torch.tensor([int(q in left) for q in range(nq)], dtype=torch.uint8),
            pair_index=torch.tensor(pair_index, dtype=torch.int32), part_ids=part_ids, part_names=part_names,
            merged_ids=[part_ids[q] for q in keep], merged_names=[part_names[q] for q in keep], image_keys=keys)


def _summary(max_purity, most_purity) -> Tuple[float, float, float, float, int, int]:
    """The tuple eval_cub_csv.py:175 logs, from the per-prototype values in the dict's order."""
    mx = np.asarray(max_purity, dtype=np.float64)
    mo = np.asarray(most_purity, dtype=np.float64)
    if mx.size == 0:
        nan = float("nan")
        return nan, nan, nan, nan, 0, 0
    return (float(np.mean(mx)), float(np.std(mx)), float(np.mean(mo)), float(np.std(mo)), int(mx.size),
            int((mx > 0.5).sum()))


@dataclass
class PartPurity(HostCopy):
    """Result of ``part_purity``; tensors stay on the device until ``.cpu()`` is asked for.
    P = prototypes, M = merged parts (``merged_names``)."""
    mode: str
    n: Tensor             # [P, M] int64 rows in which a member of the part is visible
    hits: Tensor          # [P, M] int64 those rows in which a visible member lies in the patch
    first_key: Tensor     # [P, M] int64 holding the uint64 key (row ordinal << 6 | slot; all ones: never present)
    rows: Tensor          # [P] int64 rows of the prototype
    in_csv: Tensor        # [P] bool: the prototype has a row
    max_purity: Tensor    # [P] float64 purity of the purest part (0 without a part)
    max_part: Tensor      # [P] int32 its merged part, -1 without a part
    max_sum: Tensor       # [P] int64 its hits
    most_part: Tensor     # [P] int32 the part most often in the patch, -1 for none
    most_sum: Tensor      # [P] int64 its hits
    most_purity: Tensor   # [P] float64 its purity
    purity: Tensor        # [P, M] float64 hits / n, NaN where n == 0
    relevant: Tensor      # [P] bool: max_k weight[k, p] above the relevance threshold
    row_loc: Tensor       # "all": [N, P] int32 loc of the row of (image, prototype), -1 for no row;
    #                       "topk": [P, k] int32 loc of slot j (the top-k state)
    row_index: Optional[Tensor]   # "topk": [P, k] int64 image of slot j, -1 for an empty slot; "all": None
    merged_names: List[str]
    images: int
    geometry: Tuple[int, int, int, int, bool]     # (H, W, image_size, skip, small-stride rule)

    def csv_order(self) -> np.ndarray:
        """The in-csv prototypes in the order of the reference's dict: first appearance in the CSV
        ("all": image-major, prototype-minor) or ascending prototype ("topk")."""
        inc = self.in_csv.cpu().numpy().astype(bool)
        protos = np.flatnonzero(inc)
        if self.mode == "topk" or protos.size == 0:
            return protos
        has = (self.row_loc.cpu().numpy() >= 0)[:, protos]
        return protos[np.argsort(has.argmax(axis=0), kind="stable")]

    def summary(self) -> Tuple[float, float, float, float, int, int]:
        """(mean, std of max_purity, mean, std of most_purity, prototypes in csv, prototypes with
        max_purity > 0.5) in numpy fp64 over the in-csv prototypes, as the reference logs them."""
        order = self.csv_order()
        return _summary(self.max_purity.cpu().numpy()[order], self.most_purity.cpu().numpy()[order])

    def patch_rows(self) -> List[Tuple[int, int, int, int, int, int]]:
        """(prototype, image, h_min, h_max, w_min, w_max) of every row, in the reference's CSV order."""
        h, w, image_size, skip, _ = self.geometry
        pn = self.rows.shape[0]
        if self.mode == "all":
            loc = self.row_loc.cpu().numpy()
            img, proto = np.nonzero(loc >= 0)
            l = loc[img, proto]
        else:
            index = self.row_index.cpu().numpy()
            rel = self.relevant.cpu().numpy().astype(bool)
            proto, slot = np.nonzero((index >= 0) & rel[:, None])
            img, l = index[proto, slot], self.row_loc.cpu().numpy()[proto, slot]
        l = torch.from_numpy(np.asarray(l, dtype=np.int64))
        c = img_coordinates(image_size, (pn, h, w), PATCH_SIZE, skip, l // w, l % w)
        return [(int(p), int(i), int(a), int(b), int(cc), int(d))
                for p, i, a, b, cc, d in zip(proto, img, *[t.tolist() for t in c])]


def _geometry(h: int, w: int, image_size: int):
    skip = patch_skip(image_size, w) if w > 1 else 0
    return (h, w, image_size, skip, h == 26 and w == 26)


def part_purity(net, loader, annotations: PartAnnotations, *, image_size: int, mode: str = "all",
                threshold: float = 0.5, k: int = 10, relevance_threshold: float = 1e-5, first_index: int = 0,
                process_group=None) -> PartPurity:
    """One pass over ``loader`` ((images, labels) batches of any size, in dataset order; image n of
    the pass is image n of ``annotations``): the part purity of every relevant prototype as
    util/eval_cub_csv.py evaluates it -- mode "all" over the rows of ``get_proto_patches_cub`` (raw
    pooled score above ``threshold``), mode "topk" over those of ``get_topk_cub`` (the ``k`` images
    of largest raw pooled score, earlier image first among equals).

    ``net``: a PIPNet on a ROCm device (fp32 or bf16 build), bare, under a ``.module`` wrapper, or
    in a ShardedInference; it is put in eval mode.  A CountPIPNet raises NotImplementedError.  Every
    image gets the bits of its batch-1 forward, so the result does not depend on the batch size.
    Nothing inside the batch loop waits for the device.

    ``first_index``: the dataset index of the first image this loader yields (image n of the pass is
    image ``first_index + n`` of ``annotations``, which always cover the whole dataset).  In a
    ShardedInference of more than one rank (or with ``process_group`` naming such a group around a bare
    net) the pass is sharded: every rank passes the loader of its own contiguous block
    (``dist.dataset_shard``, a block may be empty) and that block's ``first_index``.  Mode "topk"
    merges the ranks' top-k lists (``kernels.topk_merge``) and evaluates their rows on every rank; mode
    "all" merges the integer purity states (``kernels.part_purity_merge``) and gathers the kept rows in
    rank order.  Every rank returns the result of one process over the whole dataset, bit for bit;
    ``images`` is the total, which must equal ``annotations.images``."""
    if mode not in ("all", "topk"):
        raise ValueError(f"part_purity: mode must be 'all' or 'topk', got {mode!r}")
    net, pgroup, world, rank = unwrap_sharded(net, process_group, "part_purity")
    first_index = check_first_index(first_index, "part_purity")
    if is_count(net):
        raise NotImplementedError("part_purity: CountPIPNet is not supported (the reference's evaluation reads "
                                  "PIP-Net's pooled softmax scores); pass a PIPNet")
    if image_size < PATCH_SIZE:
        raise ValueError(f"part_purity: image_size {image_size} is smaller than the {PATCH_SIZE}-pixel patch")
    net.eval()
    n_img = annotations.images
    dev = next(net.parameters()).device
    ex = ShardedPass("part_purity", pgroup, world, rank, dev)
    ds = getattr(loader, "dataset", None)
    if not ex.sharded and first_index == 0 and ds is not None and hasattr(ds, "__len__") and len(ds) != n_img:
        raise ValueError(f"part_purity: the loader's dataset has {len(ds)} images, the annotations {n_img}")
    pn = net._num_prototypes
    ann = annotations.to(dev)
    state = K.PartPurityState(pn, len(annotations.merged_names), dev)
    tstate = K.TopkState(1, pn, k, dev) if mode == "topk" else None
    kept = []
    with torch.no_grad():
        relevant_b = net._classification.weight.max(dim=0).values > relevance_threshold
        relevant = relevant_b.to(torch.uint8).contiguous()
        seen, hw, geo = 0, None, None
        with ex.guard():
            for xs, _ in loader:
                xs = xs.to(dev, non_blocking=True)
                K.require_device(xs, "input images")
                _, loc, _, hw, raw = located_forward(net, xs, small_map(hw), with_raw=True)
                if geo is None:
                    geo = _geometry(hw[0], hw[1], image_size)
                if mode == "all":
                    K.part_purity_update(state, raw, loc, relevant, first_index + seen, threshold, geo, ann.table())
                    kept.append(torch.where((raw.double() > threshold) & relevant_b, loc, torch.full_like(loc, -1)))
                else:
                    K.topk_update(tstate, raw, loc, first_index + seen)
                seen += xs.shape[0]
        if ex.sharded:          # one header exchange, one state exchange ("all": and the kept rows)
            ex.header(first_index, seen, hw, (pn, state.merged_parts, k if mode == "topk" else 0, int(mode == "topk")))
            hw = ex.hw
            if hw is not None:
                geo = _geometry(hw[0], hw[1], image_size)           # an empty rank learns the map size here
                if mode == "topk":
                    tstate = K.topk_merge(ex.gather_state(tstate))
                else:
                    state = K.part_purity_merge(ex.gather_state(state))
                    kept = [ex.gather_rows(torch.cat(kept) if kept else
                                           torch.empty((0, pn), device=dev, dtype=torch.int32))]
                seen = ex.total
        if hw is None:
            raise ValueError("part_purity: the loader yielded no batch")
        if mode == "topk":
            row_index, row_loc = tstate.index[0].contiguous(), tstate.loc[0].contiguous()
            K.part_purity_rows(state, row_index, row_loc, relevant, geo, ann.table())
        else:
            row_index, row_loc = None, torch.cat(kept)
        res = K.part_purity_finish(state)
    first = ex.first[0] if ex.sharded else first_index      # the pass must end where the annotations end
    if first + seen != n_img or int(state.bad) != 0:
        raise ValueError(f"part_purity: the pass saw {seen} images from index {first}, the annotations hold {n_img}")
    in_csv, max_purity, max_part, max_sum, most_part, most_sum, most_purity, purity = res
    return PartPurity(mode=mode, n=state.n, hits=state.hits, first_key=state.first_key, rows=state.rows, in_csv=in_csv,
                      max_purity=max_purity, max_part=max_part, max_sum=max_sum, most_part=most_part,
                      most_sum=most_sum, most_purity=most_purity, purity=purity, relevant=relevant_b,
                      row_index=row_index, row_loc=row_loc, merged_names=list(annotations.merged_names),
                      images=seen, geometry=geo)


def write_patch_csv(result_or_rows, image_paths: Sequence[str], path: str) -> str:
    """Write the reference's patch CSV (eval_cub_csv.py:189-214 / :256-282: same header, same column
    order) from a ``PartPurity`` or from (prototype, image index, h_min, h_max, w_min, w_max) rows."""
    rows = result_or_rows.patch_rows() if isinstance(result_or_rows, PartPurity) else result_or_rows
    with open(path, "w", newline="") as f:
        writer = csv.writer(f, delimiter=",")
        writer.writerow(CSV_HEADER)
        writer.writerows([[p, image_paths[i], h0, h1, w0, w1] for p, i, h0, h1, w0, w1 in rows])
    return path


@dataclass
class CsvPartPurity:
    """What eval_prototypes_cub_parts_csv computes from a CSV, keyed by the CSV's prototype strings
    in its dict order."""
    presences: Dict[str, Dict[str, List[int]]]        # prototype -> part id -> 0/1 per row
    max_purity: Dict[str, float]
    max_part: Dict[str, str]                          # part name; no entry for an empty part dict
    max_sum: Dict[str, int]
    most_part: Dict[str, Tuple[str, int]]             # (part id, hits); ('0', 0) for none
    most_purity: Dict[str, float]

    def summary(self):
        return _summary(list(self.max_purity.values()), list(self.most_purity.values()))


def eval_patch_csv(csvfile: str, annotations: PartAnnotations, image_size: int) -> CsvPartPurity:
    """eval_prototypes_cub_parts_csv (eval_cub_csv.py:57-175) on the host, for a patch CSV of any
    part-prototype method: coordinates in the ``image_size`` resized image, patches larger than 32
    pixels cut to their centre.  Images are matched by their last two path components; sizes and
    parts come from ``annotations`` (no image is opened)."""
    index_of = {key: i for i, key in enumerate(annotations.image_keys)}
    ids, names = annotations.part_ids, annotations.part_names
    id_to_name = dict(zip(ids, names))
    name_to_id = dict(zip(names, ids))
    pairs = [(pid, name_to_id[name.replace("left", "right")]) for pid, name in zip(ids, names) if "left" in name]
    size = annotations.size.tolist()
    imgresize = float(image_size)
    presences: Dict[str, Dict[str, List[int]]] = {}
    parts_cache: Dict[int, Dict[str, Tuple[float, float]]] = {}
    with open(csvfile, newline="") as f:
        reader = csv.reader(f, delimiter=",")
        next(reader)
        for proto, imgname, h_min, h_max, w_min, w_max in reader:
            pres = presences.setdefault(proto, {})
            key = image_key(imgname)
            if key not in index_of:
                raise ValueError(f"eval_patch_csv: image '{key}' is not in the annotations")
            i = index_of[key]
            width, height = size[i]
            h_min, h_max, w_min, w_max = float(h_min), float(h_max), float(w_min), float(w_max)
            diffh, diffw = h_max - h_min, w_max - w_min
            if diffh > PATCH_SIZE:                    # too large a patch: its centre, or size buys purity
                c = diffh - PATCH_SIZE
                h_min, h_max = h_min + c // 2., h_max - c // 2.
            if diffw > PATCH_SIZE:
                c = diffw - PATCH_SIZE
                w_min, w_max = w_min + c // 2., w_max - c // 2.
            oh_min, oh_max = (height / imgresize) * h_min, (height / imgresize) * h_max
            ow_min, ow_max = (width / imgresize) * w_min, (width / imgresize) * w_max
            if i not in parts_cache:
                parts_cache[i] = annotations.visible_parts(i)
            parts = parts_cache[i]
            for part, (x, y) in parts.items():
                inside = int(oh_min <= y <= oh_max and ow_min <= x <= ow_max)
                pres.setdefault(part, []).append(inside)
            for lid, rid in pairs:
                if lid in parts:
                    if rid in parts:
                        if pres[lid][-1] > pres[rid][-1]:
                            pres[rid][-1] = pres[lid][-1]
                    else:
                        pres.setdefault(rid, []).append(pres[lid][-1])
                    del pres[lid]
    out = CsvPartPurity(presences, {}, {}, {}, {}, {})
    for proto, pres in presences.items():
        out.max_purity[proto], out.most_part[proto], out.most_purity[proto] = 0., ("0", 0), 0.
        for part, seq in pres.items():
            purity, total = float(np.mean(seq)), int(np.sum(seq))
            better = purity > out.max_purity[proto]
            if not better and purity == out.max_purity[proto]:
                better = purity == 0. or total > out.max_sum[proto]
            if better:
                out.max_purity[proto], out.max_part[proto], out.max_sum[proto] = purity, id_to_name[part], total
            if total > out.most_part[proto][1]:
                out.most_part[proto], out.most_purity[proto] = (part, total), purity
    return out
