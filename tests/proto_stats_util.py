"""Shared helpers of the prototype-statistics tests: the recorded fixtures
(tests/golden/gen_golden_proto_stats.py), their loaders, and the comparison of an accumulated
state with what the reference reported."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from count_pipnet_amd.synthetic import synth_exponential
from golden_util import GOLDEN_DIR, eval_loader_batches, load_golden
from proto_stats_ref import stats_state

FIXTURES = ("pipnet_mid_addon", "count_onehot")
STATE_KEYS = ("n_class", "n_ge", "n_gt", "total", "total_gt", "vmax", "hist")
PIPNET_EDGES = np.linspace(0.01, 1.01, 51, dtype=np.float32)


def load_stats_fixture(name):
    """(meta, arrays, forward-case meta) of tests/golden/proto_stats/<name>.npz."""
    z = np.load(os.path.join(GOLDEN_DIR, "proto_stats", name + ".npz"), allow_pickle=False)
    rec = {k: z[k] for k in z.files}
    meta = json.loads(str(rec.pop("meta")))
    fwd_meta, _ = load_golden(meta["forward_case"])
    return meta, rec, fwd_meta


def runs_of(meta):
    """[(tag, continuous)] of the analysis runs a fixture holds."""
    return [(tag, meta["runs"][tag]["continuous"]) for tag in ("d", "c") if tag in meta["runs"]]


def count_edges_np(max_count):
    return np.arange(max_count + 1, dtype=np.float32) + 0.5


def fixture_loader(meta, fwd_meta, net, noise_seed, max_images=None, device=None):
    """The fixture's batches, in order; before each one the Gumbel head of a CountPIPNet gets the
    Exp(1) draw the recording injected for it (shape of the batch as cut at ``max_images``)."""
    case = fwd_meta["case"]
    batches = eval_loader_batches(case["size"], case["num_classes"], meta["batches"], meta["batch_size"],
                                  meta["label_seed"])
    head = net._add_on[-1] if hasattr(net, "_max_count") else None
    hw = case["size"] // 8

    def gen():
        seen = 0
        for k, (xs, ys) in enumerate(batches):
            if max_images is not None and seen >= max_images:
                return
            b = xs.shape[0] if max_images is None else min(xs.shape[0], max_images - seen)
            if head is not None:
                e = synth_exponential((b, net._num_prototypes, hw, hw), noise_seed + k)
                head.exp_noise = e if device is None else e.to(device)
            yield xs, ys
            seen += b

    return gen()


def state_np(st):
    """A PrototypeClassStats / ProtoStatsState as the dict of numpy arrays ``stats_state`` returns."""
    out = {k: getattr(st, k).detach().cpu().numpy() for k in STATE_KEYS}
    out["hist"] = out["hist"].astype(np.int64)
    return out


def assert_state_equal(got, want, what=""):
    """Integer state exact, vmax and both fp64 sums bitwise."""
    for k in STATE_KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        if g.dtype.kind == "f":
            assert g.dtype == w.dtype and np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes(), \
                (what, k, np.argwhere(g != w)[:5])
        else:
            assert np.array_equal(g, w), (what, k, np.argwhere(g != w)[:5])


def check_against_fixture(st, rec, tag, *, count, continuous, mean_rtol=None, mean_atol=None, pairs=None):
    """Every quantity the reference reported in run ``tag``, derived from the state ``st`` (dict of
    numpy arrays).  ``pairs`` [K,P] bool restricts the exact comparisons to decisive pairs (the
    end-to-end runs); None: all pairs, plus the report and the plotting order.  Returns the number
    of bar traces compared bin by bin."""
    classes = rec[f"{tag}_classes"]
    labels = rec[f"{tag}_labels"]
    n = len(labels)
    kc, pn = st["n_ge"].shape
    assert np.array_equal(np.flatnonzero(st["n_class"]), classes)
    assert np.array_equal(st["n_class"], np.bincount(labels, minlength=kc))
    exact = pairs is None
    ok = np.ones((kc, pn), bool) if exact else pairs
    nonzero = st["n_ge"][classes].T                                  # [P, classes present]
    assert np.array_equal(nonzero[ok[classes].T], rec[f"{tag}_nonzero"][ok[classes].T])
    mean = (st["total"][classes] / st["n_class"][classes, None]).T
    np.testing.assert_allclose(mean, rec[f"{tag}_mean"], rtol=mean_rtol or 0, atol=mean_atol or 0)
    if exact:
        zero = n - st["n_ge"].sum(0)
        assert np.array_equal(zero, rec[f"{tag}_zero"][:, 0]) and (rec[f"{tag}_zero"][:, 1] == n).all()
        assert [f"{z / n * 100.0:.2f}" for z in zero] == rec[f"{tag}_zero_pct"].tolist()
    tp, tc, off = rec[f"{tag}_trace_proto"], rec[f"{tag}_trace_class"], rec[f"{tag}_trace_off"]
    compared = 0
    std_centers = (PIPNET_EDGES[:-1].astype(np.float64) + PIPNET_EDGES[1:]) / 2.0
    for i, (p, c) in enumerate(zip(tp, tc)):
        x, y = rec[f"{tag}_trace_x"][off[i]:off[i + 1]], rec[f"{tag}_trace_y"][off[i]:off[i + 1]]
        if not ok[c, p]:
            continue
        h = st["hist"][c, p]
        if count and not continuous:            # np.unique on counts: value v sits in bin v - 1
            want = np.zeros_like(h)
            want[x.astype(np.int64) - 1] = y
            assert np.array_equal(x, np.round(x)) and np.array_equal(h, want), (p, c, h, x, y)
        elif len(x) == len(std_centers) and np.allclose(x, std_centers, rtol=0, atol=1e-6):
            assert np.array_equal(h, y), (p, c, h, y)            # the fixed range (thr, 1.01)
        else:
            continue                            # the pair's own range (its maximum exceeds 1): not this pass
        assert st["n_gt"][c, p] == y.sum()
        compared += 1
    if exact:
        # a trace for every pair with an activation above the threshold, most active class first
        # (a stable descending sort of n_gt / n_class over the classes present, histograms.py:663)
        for p in range(pn):
            act = {int(c): st["n_gt"][c, p] / st["n_class"][c] for c in classes}
            order = [c for c, a in sorted(act.items(), key=lambda it: it[1], reverse=True) if st["n_gt"][c, p] > 0]
            assert tc[tp == p].tolist() == order, p
    return compared


def planted_activations(b, p, thr, edges, seed, counts=0):
    """[b, p] float32 in [0, 1.2) (``counts`` > 0: half of them whole numbers 0..counts + 1, the
    rest in [0, counts + 2)) with, scattered over it: the threshold and one ulp on either side,
    every edge and one ulp on either side, a value above the last edge, exact zeros and 1.0."""
    g = np.random.default_rng(seed)
    x = (g.random((b, p), dtype=np.float32) * np.float32(counts + 2 if counts else 1.2)).astype(np.float32)
    if counts:
        x = np.where(g.random((b, p)) < 0.5, np.floor(x), x).astype(np.float32)
    x[g.random((b, p)) < 0.2] = 0.0
    marks = [np.float32(thr)] + ([] if edges is None else [np.float32(e) for e in edges])
    special = [np.float32(0.0), np.float32(1.0)]
    for m in marks:
        if np.isfinite(m):
            special += [m, np.nextafter(m, np.float32(-np.inf)), np.nextafter(m, np.float32(np.inf))]
    if edges is not None and np.isfinite(edges[-1]):
        special.append(np.float32(edges[-1]) * np.float32(1.5) + np.float32(1.0))
    special = np.array(special, dtype=np.float32)
    flat = x.reshape(-1)
    if len(special) <= flat.size:
        pos = g.choice(flat.size, size=len(special), replace=False)
        flat[pos] = special
    else:                                       # a tiny matrix: as many as fit, the threshold marks first
        flat[:] = special[:flat.size]
    return torch.from_numpy(x)


def label_pattern(kind, b, k, seed=0):
    if kind == "equal":
        return torch.full((b,), k - 1, dtype=torch.int64)
    if kind == "sorted":
        return torch.sort(torch.randint(0, k, (b,), generator=torch.Generator().manual_seed(seed))).values
    if kind == "alternating":
        return (torch.arange(b) % min(k, 2)) * (k - 1)
    raise ValueError(kind)


def reference_state(act, labels, k, thr, edges):
    return stats_state(act.numpy(), labels.numpy(), k, thr, None if edges is None else np.asarray(edges, np.float32))


def ragged_loader(meta, fwd_meta, net, noise_seed, sizes, max_images, device):
    """The fixture's images and labels re-cut into batches of ``sizes``; every image keeps the
    Exp(1) draw the recording injected for it (the recording drew one tensor per batch of
    ``batch_size`` images, the last one cut at ``max_images``).  Yields CPU batches; the Gumbel head
    of a CountPIPNet holds the noise of the images that will be used."""
    case = fwd_meta["case"]
    batches = eval_loader_batches(case["size"], case["num_classes"], meta["batches"], meta["batch_size"],
                                  meta["label_seed"])
    xs_all = torch.cat([x for x, _ in batches])
    ys_all = torch.cat([y for _, y in batches])
    assert sum(sizes) == xs_all.shape[0]
    head = net._add_on[-1] if hasattr(net, "_max_count") else None
    noise = None
    if head is not None:
        hw, bs = case["size"] // 8, meta["batch_size"]
        noise = torch.cat([synth_exponential((min(bs, max_images - k * bs), net._num_prototypes, hw, hw), noise_seed + k)
                           for k in range(meta["batches"]) if k * bs < max_images]).to(device)

    def gen():
        seen = 0
        for s in sizes:
            if seen >= max_images:
                return
            b = min(s, max_images - seen)
            if head is not None:
                head.exp_noise = noise[seen:seen + b]
            yield xs_all[seen:seen + s], ys_all[seen:seen + s]
            seen += b

    return gen()
