"""Golden fixtures for the class-conditional prototype activation statistics
(count_pipnet_amd/stats.py), recorded by running the REFERENCE's own, unchanged
``util/histograms.py:plot_prototype_activations_by_class`` (and, for the one-hot CountPIPNet,
``pipnet/count_pipnet.py:estimate_mean_intermediate_features`` / ``calculate_virtual_weights``)
on CPU.

For each case the reference model of a forward golden case (gen_golden.CASES, same synthetic
weights) is wrapped in ``nn.DataParallel`` (CPU: it calls the module directly) and analysed over
``golden_util.eval_loader_batches`` with ``max_images`` falling inside the last batch, all
prototypes, ``return_type='both'``, ``filter_outlier_prototypes=False``,
``normalize_frequencies=False``, into a temporary directory.  While it runs, three names in the
reference module's namespace are replaced by recording stand-ins (the reference file itself is
untouched): ``go`` (every ``go.Figure()`` starts a prototype, every ``go.Bar(x, y, name)`` is one
class trace), ``write_image`` (no static export) and ``_collect_activations`` (the original, its
result kept).

Recorded per run (prefix ``d_`` discrete / default, ``c_`` CountPIPNet with
plot_always_histograms=True): labels, the pooled activations the reference collected, the returned
mean values [P, classes present] and non-zero counts, the per-prototype lines of
zero_activation_summary_report.txt (num_zero, total, the printed percentage) and the bar traces
(prototype, class, offsets into flat x / count arrays, in plotting order).

Usage:  python tests/golden/gen_golden_proto_stats.py
"""
from __future__ import annotations

import contextlib
import io
import json
import os
import re
import sys
import tempfile

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True            # the reference tree is read-only
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import gen_golden as G  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
from golden_util import eval_loader_batches  # noqa: E402
from proto_stats_ref import decisive_pairs  # noqa: E402

# name -> (forward golden case, batches, batch size, max_images, label seed)
STATS_CASES = {
    "pipnet_mid_addon": ("pipnet_mid_addon", 3, 5, 12, 257),
    "count_onehot": ("count_onehot", 5, 5, 23, 213),
}
# a directory of their own, as tests/golden/attr: golden_util.golden_names() takes every top-level
# .npz without a known prefix for a forward case
OUT = os.path.join(HERE, "proto_stats")
THRESHOLD = 0.01
NOISE_BASE = 3000            # noise seed of a run = NOISE_BASE + 100 * run + weight seed; + k for the k-th forward


class _GoRecorder:
    """plotly.graph_objects with Figure / Bar calls noted."""

    def __init__(self, real):
        self._real = real
        self.figures = -1
        self.bars = []

    def __getattr__(self, name):
        return getattr(self._real, name)

    def Figure(self, *a, **kw):
        self.figures += 1
        return self._real.Figure(*a, **kw)

    def Bar(self, **kw):
        self.bars.append((self.figures, int(kw["name"]), np.asarray(kw["x"], dtype=np.float64),
                          np.asarray(kw["y"], dtype=np.int64)))
        return self._real.Bar(**kw)


def analyse(H, dp, batches, max_images, noise_seed, continuous):
    """One run of the reference's plot_prototype_activations_by_class; returns the recorded arrays."""
    go, collect, write_image = H.go, H._collect_activations, H.write_image
    rec_go = _GoRecorder(go)
    kept = {}

    def collect_and_keep(*a, **kw):
        acts, labels = collect(*a, **kw)
        kept["acts"], kept["labels"] = acts.copy(), labels.copy()
        return acts, labels

    H.go, H._collect_activations, H.write_image = rec_go, collect_and_keep, lambda *a, **kw: None
    try:
        with tempfile.TemporaryDirectory() as tmp, G.injected_exponential(seed=noise_seed) as drawn, \
                contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            means, nonzero = H.plot_prototype_activations_by_class(
                dp, batches, torch.device("cpu"), tmp, only_important_prototypes=False, max_images=max_images,
                class_idx_to_name_func=str, near_zero_threshold=THRESHOLD, plot_always_histograms=continuous,
                normalize_frequencies=False, filter_outlier_prototypes=False, return_type="both")
            report = open(os.path.join(tmp, "zero_activation_summary_report.txt")).read()
            draws = len(drawn)
    finally:
        H.go, H._collect_activations, H.write_image = go, collect, write_image
    acts, labels = kept["acts"], kept["labels"]
    pn = acts.shape[1]
    classes = sorted(np.unique(labels).tolist())
    assert sorted(means) == list(range(pn)) and acts.shape[0] == max_images
    zero = np.array([[int(p), int(z), int(t)] for p, _, z, t in
                     re.findall(r"Proto (\d+)\s*:\s*([0-9.]+)% \(\s*(\d+)/(\d+)\s*\)", report)], dtype=np.int64)
    pct = [s for _, s, _, _ in re.findall(r"Proto (\d+)\s*:\s*([0-9.]+)% \(\s*(\d+)/(\d+)\s*\)", report)]
    assert zero.shape == (pn, 3) and (zero[:, 0] == np.arange(pn)).all()
    bars = [b for b in rec_go.bars if b[0] < pn]         # figure p = prototype p (none is filtered out)
    off = np.cumsum([0] + [len(b[2]) for b in bars])
    rec = dict(labels=labels.astype(np.int64), acts=acts, classes=np.array(classes, dtype=np.int64),
               mean=np.array([[float(v) for v in means[p]] for p in range(pn)], dtype=np.float64),
               nonzero=np.array([[nonzero[p][c] for c in classes] for p in range(pn)], dtype=np.int64),
               zero=zero[:, 1:], zero_pct=np.array(pct),
               trace_proto=np.array([b[0] for b in bars], dtype=np.int64),
               trace_class=np.array([b[1] for b in bars], dtype=np.int64), trace_off=off.astype(np.int64),
               trace_x=np.concatenate([b[2] for b in bars]), trace_y=np.concatenate([b[3] for b in bars]))
    return rec, draws


def run(name):
    fwd_case, nb, bs, max_images, label_seed = STATS_CASES[name]
    net, case = G.build_reference(fwd_case)
    sys.path.insert(0, G.REF)
    import util.histograms as H
    batches = eval_loader_batches(case["size"], case["num_classes"], nb, bs, label_seed)
    assert (nb - 1) * bs < max_images < nb * bs, "max_images must fall inside the last batch"
    dp = nn.DataParallel(net)
    count = hasattr(net, "_max_count")
    rec, runs = {}, {}
    for run_i, (tag, continuous) in enumerate([("d", False)] + ([("c", True)] if count else [])):
        seed = NOISE_BASE + 100 * run_i + case["seed"]
        r, draws = analyse(H, dp, batches, max_images, seed, continuous)
        rec.update({f"{tag}_{k}": v for k, v in r.items()})
        runs[tag] = dict(noise_seed=seed, noise_draws=draws, continuous=continuous)
        if not continuous:
            # the GPU forward agrees with this CPU run to 1e-3: most (class, prototype) pairs must
            # be decided by a wider margin for the end-to-end comparison to mean something
            edges = (np.arange(case["max_count"] + 1) + 0.5 if count
                     else np.linspace(THRESHOLD, 1.01, 51, dtype=np.float32))
            ok = decisive_pairs(r["acts"], r["labels"], case["num_classes"], THRESHOLD, edges)
            present = np.isin(np.arange(case["num_classes"]), r["classes"])
            runs[tag]["decisive"] = float(ok[present].mean())
            assert runs[tag]["decisive"] >= 0.9, f"{name}: only {runs[tag]['decisive']:.3f} of the pairs are decisive"
    if count:
        import pipnet.count_pipnet as cp
        dev = torch.device("cpu")
        quiet = (contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()))
        for key, fn in (("mean_intermediate", lambda: cp.estimate_mean_intermediate_features(dp, batches, dev)),
                        ("virtual_scaled", lambda: cp.calculate_virtual_weights(dp, batches, dev, custom_onehot_scale=True)),
                        ("virtual_plain", lambda: cp.calculate_virtual_weights(dp, batches, dev, custom_onehot_scale=False))):
            seed = NOISE_BASE + 100 * (2 + len(runs)) + case["seed"]
            with torch.no_grad(), G.injected_exponential(seed=seed) as drawn, quiet[0], quiet[1]:
                rec[key] = fn().detach().numpy()
            runs[key] = dict(noise_seed=seed, noise_draws=len(drawn))
    meta = dict(name=name, forward_case=fwd_case, batches=nb, batch_size=bs, max_images=max_images,
                label_seed=label_seed, threshold=THRESHOLD, runs=runs)
    rec["meta"] = np.array(json.dumps(meta))
    return rec


def main():
    torch.set_num_threads(os.cpu_count() or 8)
    for name in STATS_CASES:
        rec = run(name)
        os.makedirs(OUT, exist_ok=True)
        path = os.path.join(OUT, f"{name}.npz")
        np.savez_compressed(path, **rec)
        print(f"wrote {path} ({os.path.getsize(path) / 1e3:.1f} kB)", json.loads(str(rec["meta"]))["runs"], flush=True)


if __name__ == "__main__":
    main()
