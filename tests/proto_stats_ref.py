"""Numpy restatement of the reference's class-conditional prototype activation analysis
(util/histograms.py) over an activation matrix [N, P] and labels [N], and of the state the
streaming kernel (pipnet_proto_stats_update_f32) accumulates from the same data.

``reference_analysis`` follows the cited lines literally (same masks, same numpy calls, the
threshold as the Python float the reference passes), for all prototypes
(only_important_prototypes=False, filter_outlier_prototypes=False).  ``stats_state`` is the
kernel's contract: fp32 comparisons against the fp32 threshold, fp64 sums in image order,
np.histogram(values, bins=edges) bins.
"""
from __future__ import annotations

import numpy as np


def reference_analysis(acts, labels, thr=0.01, count=False, continuous=False, bins=50):
    """acts [N,P] float32, labels [N] int.  Returns a dict:
    classes   sorted unique labels (histograms.py:553)
    mean      [P][len(classes)] np.mean per class (:645)
    nonzero   [P] {class: count of act >= thr} (:644)
    activity  [P] {class: share of act > thr} (:660-661)
    overall   [P] mean of act > thr over all images, 0.0 without any (:521-522)
    zero      [P] (num_zero, total, pct) of act < thr (:206-209)
    traces    [P] list of (class, x, counts) in plotting order (:663-715, normalize_frequencies=False)
    """
    acts = np.asarray(acts)
    labels = np.asarray(labels)
    n, pn = acts.shape
    classes = sorted(np.unique(labels).tolist())
    out = dict(classes=classes, mean=[], nonzero=[], activity=[], overall=[], zero=[], traces=[])
    for p in range(pn):
        a = acts[:, p]
        nz = a[a > thr]
        out["overall"].append(float(np.mean(nz)) if len(nz) > 0 else 0.0)
        num_zero = int(np.sum(a < thr))
        out["zero"].append((num_zero, n, num_zero / n * 100.0))
        means, nonzero, activity = [], {}, {}
        for c in classes:
            m = labels == c
            nonzero[c] = int(np.sum(a[m] >= thr))
            means.append(np.mean(a[m]))
            activity[c] = np.sum(a[m] > thr) / int(np.sum(m))
        out["mean"].append(means)
        out["nonzero"].append(nonzero)
        out["activity"].append(activity)
        traces = []
        for c, _ in sorted(activity.items(), key=lambda it: it[1], reverse=True):
            v = a[labels == c]
            v = v[v > thr]
            if len(v) == 0:
                continue
            if count and not continuous:
                x, cnt = np.unique(v, return_counts=True)
            else:
                hmax = max(1.0, np.max(v) if len(v) > 0 else 1.0)
                cnt, e = np.histogram(v, bins=bins, range=(thr, hmax * 1.01))
                x = (e[:-1] + e[1:]) / 2.0
            traces.append((c, np.asarray(x, dtype=np.float64), np.asarray(cnt, dtype=np.int64)))
        out["traces"].append(traces)
    return out


def bin_index(values, edges):
    """np.histogram(values, bins=edges)'s bin of each fp32 value: the largest i < NB with
    edges[i] <= v (v == edges[NB] in the last bin), -1 outside [edges[0], edges[NB]]."""
    v = np.asarray(values, dtype=np.float32)
    e = np.asarray(edges, dtype=np.float32)
    nb = len(e) - 1
    idx = np.searchsorted(e, v, side="right") - 1
    idx = np.where(v == e[nb], nb - 1, idx)
    return np.where((v >= e[0]) & (v <= e[nb]), idx, -1)


def stats_state(acts, labels, num_classes, thr, edges=None):
    """The state after streaming (acts, labels) through pipnet_proto_stats_update_f32 in order."""
    acts = np.asarray(acts, dtype=np.float32)
    labels = np.asarray(labels, dtype=np.int64)
    n, pn = acts.shape
    kc = num_classes
    t = np.float32(thr)
    nb = 0 if edges is None else len(edges) - 1
    st = dict(n_class=np.zeros(kc, np.int64), n_ge=np.zeros((kc, pn), np.int64), n_gt=np.zeros((kc, pn), np.int64),
              total=np.zeros((kc, pn), np.float64), total_gt=np.zeros((kc, pn), np.float64),
              vmax=np.full((kc, pn), -np.inf, np.float32), hist=np.zeros((kc, pn, nb), np.int64),
              bad=int(np.sum((labels < 0) | (labels >= kc))))
    for k in range(kc):
        rows = acts[labels == k]                       # image order
        st["n_class"][k] = len(rows)
        if len(rows) == 0:
            continue
        gt = rows > t
        st["n_ge"][k] = (rows >= t).sum(0)
        st["n_gt"][k] = gt.sum(0)
        st["total"][k] = np.cumsum(rows.astype(np.float64), axis=0)[-1]
        st["total_gt"][k] = np.cumsum(np.where(gt, rows, np.float32(0)).astype(np.float64), axis=0)[-1]
        st["vmax"][k] = rows.max(0)
        if nb:
            b = bin_index(rows, edges)
            rr, pp = np.nonzero(gt & (b >= 0))
            np.add.at(st["hist"][k], (pp, b[rr, pp]), 1)
    return st


def decisive_pairs(acts, labels, num_classes, thr, edges, margin=1e-3):
    """[K, P] bool: no activation of the (class, prototype) pair lies within ``margin`` of the
    threshold or of a histogram edge, so a forward that differs by less than ``margin`` counts
    the same."""
    acts = np.asarray(acts, dtype=np.float64)
    marks = np.concatenate(([float(np.float32(thr))], np.asarray(edges, dtype=np.float64)))
    marks = marks[np.isfinite(marks)]
    near = (np.abs(acts[:, :, None] - marks[None, None, :]) <= margin).any(-1)       # [N, P]
    ok = np.ones((num_classes, acts.shape[1]), bool)
    for k in range(num_classes):
        ok[k] = ~near[np.asarray(labels) == k].any(0)
    return ok
