"""Shared helpers of the part-purity tests: the recorded fixture
(tests/golden/gen_golden_part_purity.py), seeded random annotation tables, a numpy version of the
kernels' row function / finish (the n, hits, first_key reduction of csrc/part_purity_row.hpp), and
the comparison of that reduction with the dict restatement (tests/part_purity_ref.py)."""
from __future__ import annotations

import json
import os

import numpy as np

from golden_util import GOLDEN_DIR, load_golden
from part_purity_ref import restate

PATCH = 32
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
FIXTURES = ("pipnet_mid_addon",)
STATE_KEYS = ("n", "hits", "first_key", "rows")


# ---- geometry ------------------------------------------------------------------------------------

def geometry(h, w, image_size, small=None):
    """(H, W, image_size, skip, small-stride rule): skip by Python's round, as util/func.py."""
    skip = round((image_size - PATCH) / (w - 1)) if w > 1 else 0
    return (h, w, image_size, skip, (h == 26 and w == 26) if small is None else bool(small))


def np_axis(geo, i, n):
    h, w, size, skip, small = geo
    if small:
        lo = max(0, (i - 1) * skip + 4)
        if not i < w - 1:
            lo -= 4
        hi = lo + PATCH
    else:
        lo, hi = i * skip, min(size, i * skip + PATCH)
    if i == n - 1:
        hi = size
    if hi == size:
        lo = size - PATCH
    return lo, hi


def np_patch(geo, loc):
    h, w = geo[0], geo[1]
    return np_axis(geo, int(loc) // w, h) + np_axis(geo, int(loc) % w, w)


# ---- annotation tables ---------------------------------------------------------------------------

def fold_table(names):
    """(merged [Q] int32, is_left [Q] uint8, pair_index [Q] int32, merged q list) from part names."""
    q_of = {n: q for q, n in enumerate(names)}
    pairs = [(q, q_of[n.replace("left", "right")]) for q, n in enumerate(names) if "left" in n]
    left = {lq: i for i, (lq, _) in enumerate(pairs)}
    right_of = dict(pairs)
    keep = [q for q in range(len(names)) if q not in left]
    m_of = {q: m for m, q in enumerate(keep)}
    merged = np.array([m_of[right_of[q]] if q in left else m_of[q] for q in range(len(names))], dtype=np.int32)
    return (merged, np.array([int(q in left) for q in range(len(names))], dtype=np.uint8),
            np.array([left.get(q, 0) for q in range(len(names))], dtype=np.int32), keep)


def make_table(xy, vis, size, names):
    merged, is_left, pair_index, keep = fold_table(names)
    ids = [str(q + 1) for q in range(len(names))]
    return dict(xy=np.ascontiguousarray(xy, dtype=np.float64), vis=np.ascontiguousarray(vis, dtype=np.uint8),
                size=np.ascontiguousarray(size, dtype=np.int32), merged=merged, is_left=is_left,
                pair_index=pair_index, ids=ids, names=list(names), keep=keep)


def part_names(q, pairs):
    """q part names with ``pairs`` left/right pairs; lefts first among the paired ones, as in CUB."""
    assert 2 * pairs <= q
    names = [f"left {chr(97 + i)}" for i in range(pairs)] + [f"part {i}" for i in range(q - 2 * pairs)] + \
            [f"right {chr(97 + i)}" for i in range(pairs)]
    return names


def random_table(rng, n, q, pairs, image_size=64):
    """A seeded table of n images whose parts fall on a coarse grid (so patches share hits and
    purities tie), with copies of a part's column (ties in purity and in hit count), a part that
    never lies in a patch (purity 0, twice: the last one wins) and an image without visible part."""
    names = part_names(q, pairs)
    if rng.random() < 0.5:
        names = names[::-1]                                     # the right members before the left ones
    size = np.stack([rng.integers(20, 200, n), rng.integers(20, 200, n)], axis=1)
    grid = rng.integers(0, 5, (n, q, 2)) / 4.0
    xy = grid * size[:, None, :]
    vis = rng.random((n, q)) < 0.7
    unpaired = [i for i, nm in enumerate(names) if nm.startswith("part")]
    if len(unpaired) >= 2:
        a, b = unpaired[0], unpaired[-1]
        xy[:, b], vis[:, b] = xy[:, a], vis[:, a]               # equal purity and equal hits
    if len(unpaired) >= 4:
        xy[:, unpaired[1]] = -5.0                               # purity 0 ...
        xy[:, unpaired[2]] = -7.0                               # ... twice
    if n > 2:
        vis[rng.integers(0, n)] = False
    return make_table(xy, vis, size, names)


def parts_of_image(table, i):
    return {table["ids"][q]: (float(table["xy"][i, q, 0]), float(table["xy"][i, q, 1]))
            for q in range(len(table["ids"])) if table["vis"][i, q]}


# ---- the reduction -------------------------------------------------------------------------------

def new_state(p, m):
    return dict(n=np.zeros((p, m), np.int64), hits=np.zeros((p, m), np.int64),
                first_key=np.full((p, m), NO_KEY, np.uint64), rows=np.zeros(p, np.int64), bad=0)


def np_row(state, p, ordinal, patch, i, table):
    """csrc/part_purity_row.hpp pp_row on numpy state."""
    h0, h1, w0, w1 = patch
    size = float(table["_image_size"])
    width, height = int(table["size"][i, 0]), int(table["size"][i, 1])
    top, bottom = (height / size) * h0, (height / size) * h1
    left, right = (width / size) * w0, (width / size) * w1
    nq = len(table["ids"])
    seen, hit = set(), set()
    for q in range(nq):
        if not table["vis"][i, q]:
            continue
        m = int(table["merged"][q])
        x, y = float(table["xy"][i, q, 0]), float(table["xy"][i, q, 1])
        inside = y >= top and y <= bottom and x >= left and x <= right
        slot = nq + int(table["pair_index"][q]) if table["is_left"][q] else q
        key = np.uint64((int(ordinal) << 6) | slot)
        if m not in seen:
            seen.add(m)
            state["n"][p, m] += 1
        if key < state["first_key"][p, m]:
            state["first_key"][p, m] = key
        if inside and m not in hit:
            hit.add(m)
            state["hits"][p, m] += 1
    state["rows"][p] += 1


def np_update(state, pooled, loc, relevant, i0, thr, geo, table):
    table = dict(table, _image_size=geo[2])
    n_img = table["vis"].shape[0]
    for b in range(pooled.shape[0]):
        i = i0 + b
        if not 0 <= i < n_img:
            state["bad"] += 1
            continue
        for p in np.flatnonzero(relevant):
            if float(pooled[b, p]) > thr:
                np_row(state, p, i, np_patch(geo, loc[b, p]), i, table)
    return state


def np_rows(state, index, loc, relevant, geo, table):
    table = dict(table, _image_size=geo[2])
    n_img = table["vis"].shape[0]
    for p in np.flatnonzero(relevant):
        for j in range(index.shape[1]):
            i = int(index[p, j])
            if i < 0:
                continue
            if i >= n_img:
                state["bad"] += 1
                continue
            np_row(state, p, j, np_patch(geo, loc[p, j]), i, table)
    return state


def np_finish(state):
    """csrc/part_purity.hip part_purity_finish_kernel on numpy state."""
    pn, mn = state["n"].shape
    out = dict(in_csv=state["rows"] > 0, max_purity=np.zeros(pn), max_part=np.full(pn, -1, np.int32),
               max_sum=np.zeros(pn, np.int64), most_part=np.full(pn, -1, np.int32), most_sum=np.zeros(pn, np.int64),
               most_purity=np.zeros(pn), purity=np.full((pn, mn), np.nan))
    for p in range(pn):
        present = [m for m in range(mn) if state["n"][p, m] > 0]
        for m in sorted(present, key=lambda m: int(state["first_key"][p, m])):
            s, n = int(state["hits"][p, m]), int(state["n"][p, m])
            pur = s / n
            out["purity"][p, m] = pur
            if pur > out["max_purity"][p] or (pur == out["max_purity"][p] and (pur == 0.0 or s > out["max_sum"][p])):
                out["max_purity"][p], out["max_part"][p], out["max_sum"][p] = pur, m, s
            if s > out["most_sum"][p]:
                out["most_part"][p], out["most_sum"][p], out["most_purity"][p] = m, s, pur
    return out


# ---- rows for the restatement ----------------------------------------------------------------------

def rows_all(pooled, loc, relevant, i0, thr, geo, n_img):
    """CSV rows of mode "all": image-major, prototype-minor."""
    return [(str(p), i0 + b) + np_patch(geo, loc[b, p]) for b in range(pooled.shape[0]) if 0 <= i0 + b < n_img
            for p in np.flatnonzero(relevant) if float(pooled[b, p]) > thr]


def rows_topk(index, loc, relevant, geo, n_img):
    return [(str(p), int(index[p, j])) + np_patch(geo, loc[p, j]) for p in np.flatnonzero(relevant)
            for j in range(index.shape[1]) if 0 <= index[p, j] < n_img]


def restate_rows(rows, table, image_size):
    n_img = table["vis"].shape[0]
    parts = [parts_of_image(table, i) for i in range(n_img)]
    sizes = [(int(w), int(h)) for w, h in table["size"]]
    return restate(rows, parts, sizes, table["ids"], table["names"], image_size)


def assert_finish_matches(fin, ref, table, what=""):
    """Per-prototype results of a finish (dict of numpy arrays) == the restatement's dicts, exactly."""
    keep = table["keep"]
    ids, names = table["ids"], table["names"]
    in_csv = np.flatnonzero(np.asarray(fin["in_csv"]).astype(bool))
    assert sorted(int(k) for k in ref["order"]) == in_csv.tolist(), (what, ref["order"], in_csv)
    for key in ref["order"]:
        p = int(key)
        assert float(fin["max_purity"][p]) == ref["max_purity"][key], (what, p)
        assert float(fin["most_purity"][p]) == ref["most_purity"][key], (what, p)
        mp = int(fin["max_part"][p])
        if key in ref["max_part"]:
            assert mp >= 0 and names[keep[mp]] == ref["max_part"][key], (what, p, mp, ref["max_part"][key])
            assert int(fin["max_sum"][p]) == ref["max_sum"][key], (what, p)
        else:
            assert mp == -1 and not ref["presences"][key], (what, p)
        mo = int(fin["most_part"][p])
        want = ref["most_part"][key]
        got = ("0", 0) if mo < 0 else (ids[keep[mo]], int(fin["most_sum"][p]))
        assert got == want, (what, p, got, want)
        for m, q in enumerate(keep):
            seq = ref["presences"][key].get(ids[q])
            pur = float(fin["purity"][p, m])
            assert (np.isnan(pur) and seq is None) or (seq is not None and pur == float(np.mean(seq))), (what, p, m)
    out = ~np.asarray(fin["in_csv"]).astype(bool)
    assert (np.asarray(fin["max_part"])[out] == -1).all() and (np.asarray(fin["max_purity"])[out] == 0).all()


def assert_state_equal(got, want, what=""):
    for k in STATE_KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if k == "first_key":
            g, w = g.view(np.uint64), w.view(np.uint64)
        assert g.shape == w.shape and np.array_equal(g, w), (what, k, np.argwhere(g != w)[:5])


def summary_of(fin, order):
    """The logged tuple from a finish and the in-csv prototypes in dict order."""
    mx, mo = np.asarray(fin["max_purity"], np.float64)[order], np.asarray(fin["most_purity"], np.float64)[order]
    return (float(np.mean(mx)), float(np.std(mx)), float(np.mean(mo)), float(np.std(mo)), len(order),
            int((mx > 0.5).sum()))


# ---- the recorded fixture ------------------------------------------------------------------------

def load_purity_fixture(name):
    """(meta, arrays, forward-case meta) of tests/golden/part_purity/<name>.npz."""
    z = np.load(os.path.join(GOLDEN_DIR, "part_purity", name + ".npz"), allow_pickle=False)
    rec = {k: z[k] for k in z.files}
    meta = json.loads(str(rec.pop("meta")))
    fwd_meta, _ = load_golden(meta["forward_case"])
    return meta, rec, fwd_meta


def write_annotation_files(meta, folder):
    """The recorded images.txt / parts.txt / part_locs.txt written under ``folder``; their paths."""
    paths = {}
    for key, text in meta["files"].items():
        paths[key] = os.path.join(str(folder), key + ".txt")
        with open(paths[key], "w") as f:
            f.write(text)
    return paths


def fixture_annotations(meta, rec, folder):
    from count_pipnet_amd.purity import PartAnnotations
    files = write_annotation_files(meta, folder)
    return PartAnnotations.from_cub(files["part_locs"], files["parts"], files["images"],
                                    ["/data/" + p for p in meta["image_paths"]],
                                    image_sizes=[tuple(int(v) for v in s) for s in rec["sizes"]])


def annotations_table(ann):
    """A PartAnnotations as the numpy table of this module."""
    t = make_table(ann.xy.cpu().numpy(), ann.vis.cpu().numpy(), ann.size.cpu().numpy(), ann.part_names)
    assert np.array_equal(t["merged"], ann.merged.cpu().numpy()) and t["ids"] == ann.part_ids
    assert np.array_equal(t["is_left"], ann.is_left.cpu().numpy())
    assert np.array_equal(t["pair_index"], ann.pair_index.cpu().numpy())
    return t


def recorded_rows(rec, mode):
    return [(str(int(r[0])), int(r[1]), int(r[2]), int(r[3]), int(r[4]), int(r[5])) for r in rec[f"{mode}_rows"]]


def assert_matches_recording(ref, meta, mode, ulps=0):
    """A restatement-shaped result against the recorded printed dicts and logged tuple."""
    want = meta["modes"][mode]
    assert ref["order"] == want["order"]
    assert {k: v for k, v in ref["max_part"].items()} == want["max_part"]
    assert {k: [v[0], v[1]] for k, v in ref["most_part"].items()} == want["most_part"]
    got, logged = ref["logged"], want["logged"]
    assert list(got[4:]) == logged[4:]
    tol = ulps * 2.0 ** -52
    for g, w in zip(got[:4], logged[:4]):
        assert abs(g - w) <= tol, (mode, g, w)


def result_from_finish(fin, order, table):
    """A finish (dict of arrays) as the restatement-shaped dicts the recording is compared with."""
    keep, ids, names = table["keep"], table["ids"], table["names"]
    out = dict(order=[str(int(p)) for p in order], max_part={}, most_part={})
    for p in order:
        key = str(int(p))
        if int(fin["max_part"][p]) >= 0:
            out["max_part"][key] = names[keep[int(fin["max_part"][p])]]
        mo = int(fin["most_part"][p])
        out["most_part"][key] = ("0", 0) if mo < 0 else (ids[keep[mo]], int(fin["most_sum"][p]))
    out["logged"] = summary_of(fin, np.asarray(order, dtype=np.int64))
    return out


def first_appearance(rows):
    """Prototypes in the order of their first CSV row."""
    return list(dict.fromkeys(int(r[0]) for r in rows))
