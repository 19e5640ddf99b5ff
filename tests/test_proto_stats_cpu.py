"""Class-conditional prototype statistics, the parts that need no GPU: the numpy restatement
(tests/proto_stats_ref.py) against what the reference recorded, ``class_prototype_stats`` on the
torch path against the restatement, the explicit-edge bin rule against np.histogram, and the
argument checks of the two C entry points (status before any HIP call)."""
import ctypes

import numpy as np
import pytest
import torch

from count_pipnet_amd import _lib, build
from count_pipnet_amd import kernels as K
from count_pipnet_amd.backend import torch_backend
from count_pipnet_amd.stats import (class_prototype_stats, count_edges, count_range_edges, mean_intermediate_features,
                                    pipnet_edges, virtual_weights)
from model_util import build_model
from proto_stats_ref import bin_index, reference_analysis, stats_state
from proto_stats_util import (FIXTURES, PIPNET_EDGES, assert_state_equal, check_against_fixture, count_edges_np,
                              fixture_loader, load_stats_fixture, runs_of, state_np)


# ---- the restatement against the recording ---------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_the_reference(name):
    """Counts, traces and report numbers exact; means to rtol 1e-5 (np.mean sums a few dozen
    non-negative fp32 values in fp32: within n * 2^-24 of the exact sum)."""
    meta, rec, fwd = load_stats_fixture(name)
    count = fwd["case"]["model"] != "pipnet"
    for tag, continuous in runs_of(meta):
        acts, labels = rec[f"{tag}_acts"], rec[f"{tag}_labels"]
        assert acts.dtype == np.float32 and acts.shape[0] == meta["max_images"] == len(labels)
        r = reference_analysis(acts, labels, meta["threshold"], count=count, continuous=continuous)
        classes = rec[f"{tag}_classes"].tolist()
        assert r["classes"] == classes
        np.testing.assert_allclose(np.array(r["mean"], dtype=np.float64), rec[f"{tag}_mean"], rtol=1e-5, atol=0)
        assert np.array_equal(np.array([[d[c] for c in classes] for d in r["nonzero"]]), rec[f"{tag}_nonzero"])
        assert [(z, t) for z, t, _ in r["zero"]] == [tuple(v) for v in rec[f"{tag}_zero"].tolist()]
        assert [f"{pct:.2f}" for _, _, pct in r["zero"]] == rec[f"{tag}_zero_pct"].tolist()
        flat = [(p, c, x, y) for p, tr in enumerate(r["traces"]) for c, x, y in tr]
        assert [f[0] for f in flat] == rec[f"{tag}_trace_proto"].tolist()
        assert [f[1] for f in flat] == rec[f"{tag}_trace_class"].tolist()            # plotting order too
        off = rec[f"{tag}_trace_off"]
        assert len(flat) > 0
        for i, (_, _, x, y) in enumerate(flat):
            assert np.array_equal(y, rec[f"{tag}_trace_y"][off[i]:off[i + 1]])
            np.testing.assert_allclose(x, rec[f"{tag}_trace_x"][off[i]:off[i + 1]], rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", FIXTURES)
def test_streamed_state_gives_every_recorded_quantity(name):
    """The state the kernel is specified to hold (stats_state) is enough to report what the
    reference reported from the whole activation matrix."""
    meta, rec, fwd = load_stats_fixture(name)
    case = fwd["case"]
    count = case["model"] != "pipnet"
    compared = 0
    for tag, continuous in runs_of(meta):
        edges = count_edges_np(case["max_count"]) if count and not continuous else PIPNET_EDGES
        st = stats_state(rec[f"{tag}_acts"], rec[f"{tag}_labels"], case["num_classes"], meta["threshold"], edges)
        compared += check_against_fixture(st, rec, tag, count=count, continuous=continuous, mean_rtol=1e-5)
    assert compared > 20


# ---- class_prototype_stats on the torch path -------------------------------------------------------
@pytest.mark.parametrize("name,continuous", [("pipnet_mid_addon", False), ("count_onehot", False),
                                             ("count_onehot", True)])
def test_class_prototype_stats_torch_backend_equals_restatement(name, continuous):
    meta, rec, fwd = load_stats_fixture(name)
    case = fwd["case"]
    count = case["model"] != "pipnet"
    net = build_model(fwd)
    tag = "c" if continuous else "d"
    seed = meta["runs"][tag]["noise_seed"]
    mx = meta["max_images"]
    edges = PIPNET_EDGES if continuous else None
    with torch_backend():
        res = class_prototype_stats(net, fixture_loader(meta, fwd, net, seed, mx), max_images=mx,
                                    continuous=continuous, edges=edges)
        with torch.no_grad():       # the same forwards, collected as the reference collects them
            acts = torch.cat([net(xs[:mx - i * meta["batch_size"]], inference=not continuous)[1]
                              for i, (xs, _) in enumerate(fixture_loader(meta, fwd, net, seed, mx))]).numpy()
    labels = rec[f"{tag}_labels"]
    assert res.images == mx and acts.shape[0] == mx
    want_edges = np.asarray(res.edges)
    assert np.array_equal(want_edges, count_edges_np(case["max_count"]) if count and not continuous else PIPNET_EDGES)
    assert_state_equal(state_np(res), stats_state(acts, labels, case["num_classes"], meta["threshold"], want_edges), name)
    np.testing.assert_allclose(acts, rec[f"{tag}_acts"], rtol=0, atol=1e-3)
    # the derived quantities, against the restatement of the cited lines on the same activations
    r = reference_analysis(acts, labels, meta["threshold"], count=count, continuous=continuous)
    cl = r["classes"]
    np.testing.assert_allclose(res.mean_per_class()[:, cl].numpy(), np.array(r["mean"], dtype=np.float64), rtol=1e-5)
    assert np.array_equal(res.nonzero_counts()[:, cl].numpy(), np.array([[d[c] for c in cl] for d in r["nonzero"]]))
    np.testing.assert_allclose(res.class_activity()[:, cl].numpy(),
                               np.array([[d[c] for c in cl] for d in r["activity"]]), rtol=1e-15)
    np.testing.assert_allclose(res.overall_avg_nonzero().numpy(), np.array(r["overall"]), rtol=1e-5)
    zero, pct = res.near_zero()
    assert zero.tolist() == [z for z, _, _ in r["zero"]]
    np.testing.assert_allclose(pct.numpy(), [p for _, _, p in r["zero"]], rtol=1e-15)
    nh = res.normalized_hist()
    assert torch.equal(nh.sum(-1) > 0, res.hist.sum(-1) > 0) and float(nh.sum(-1).max()) <= 1.0 + 1e-12
    absent = [k for k in range(case["num_classes"]) if k not in cl]
    assert (res.mean_per_class()[:, absent] == 0).all() and (res.class_activity()[:, absent] == 0).all()
    imp = torch.linspace(0, 1, res.n_ge.shape[1])
    assert torch.equal(res.selected(imp, 0.5), imp > 0.5) and res.selected(imp, 2.0).all()       # :479-484
    assert torch.equal(res.outliers(0.3), res.overall_avg_nonzero() > 0.3) and not res.outliers().any()


def test_class_prototype_stats_argument_rules():
    meta, rec, fwd = load_stats_fixture("count_onehot")
    net = build_model(fwd)
    seed = meta["runs"]["d"]["noise_seed"]
    with torch_backend():
        with pytest.raises(ValueError, match="explicit edges"):
            class_prototype_stats(net, fixture_loader(meta, fwd, net, seed), continuous=True)
        with pytest.raises(ValueError, match="outside"):                    # 9 classes, told there are 4
            class_prototype_stats(net, fixture_loader(meta, fwd, net, seed), num_classes=4)
        with pytest.raises(ValueError, match="no image"):
            class_prototype_stats(net, [])
        # batching does not matter on the torch path either: one image at a time
        a = class_prototype_stats(net, fixture_loader(meta, fwd, net, seed, 7), max_images=7)
    assert a.images == 7 and int(a.n_class.sum()) == 7
    pm, _, pfwd = load_stats_fixture("pipnet_mid_addon")
    with torch_backend(), pytest.raises(ValueError, match="CountPIPNet"):
        class_prototype_stats(build_model(pfwd), [], continuous=True)
    with pytest.raises(ValueError):
        K.ProtoStatsState(3, 4, 0.01, torch.zeros(K.PROTO_STATS_MAX_BINS + 2), "cpu")
    assert count_edges(3).tolist() == [0.5, 1.5, 2.5, 3.5]
    assert count_range_edges(2).tolist() == [0.0, 0.5, 1.5, 2.5, float("inf")]
    assert np.array_equal(pipnet_edges().numpy(), PIPNET_EDGES)


def test_virtual_weights_and_mean_features_torch_backend():
    """count_pipnet.py:226-321 on the CPU model: the fixture's values (the same arithmetic up to the
    fp64 sum), and the unscaled matrix equal to the stacked per-prototype columns."""
    meta, rec, fwd = load_stats_fixture("count_onehot")
    net = build_model(fwd)
    runs = meta["runs"]
    with torch_backend():
        m = mean_intermediate_features(net, fixture_loader(meta, fwd, net, runs["mean_intermediate"]["noise_seed"]))
        vs = virtual_weights(net, fixture_loader(meta, fwd, net, runs["virtual_scaled"]["noise_seed"]), True)
        vp = virtual_weights(net)
        with pytest.raises(ValueError):
            virtual_weights(net, None, True)
    assert m.dtype == torch.float32
    np.testing.assert_allclose(m.numpy(), rec["mean_intermediate"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(vs.detach().numpy(), rec["virtual_scaled"], rtol=1e-4, atol=1e-6)
    cols = torch.stack([net.get_prototype_importance_per_class(p) for p in range(net._num_prototypes)], dim=1)
    assert torch.equal(vp, cols)
    np.testing.assert_allclose(vp.detach().numpy(), rec["virtual_plain"], rtol=1e-5, atol=1e-7)


# ---- the bin rule ------------------------------------------------------------------------------------
def test_explicit_edges_equal_numpy_histogram_on_planted_values():
    """bin_index over the fp32 edges == np.histogram(values, bins=50, range=(0.01, 1.01)) -- the
    reference's call at histograms.py:701 for activations up to 1 -- and == np.histogram(values,
    bins=edges), with values on, just below and just above every edge."""
    e = PIPNET_EDGES
    for seed in range(20):
        g = np.random.default_rng(seed)
        v = g.random(2000, dtype=np.float32) * np.float32(1.05)
        planted = np.concatenate([e, np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf))])
        v = np.concatenate([v, planted]).astype(np.float32)
        v = v[v > np.float32(0.01)]                      # the reference histograms the values above the threshold
        b = bin_index(v, e)
        mine = np.bincount(b[b >= 0], minlength=50)
        assert np.array_equal(mine, np.histogram(v, bins=50, range=(0.01, 1.0 * 1.01))[0])
        assert np.array_equal(mine, np.histogram(v, bins=e)[0])
        assert (b[v > e[-1]] == -1).all() and (b[v == e[-1]] == 49).all()
    # discrete counts: the count edges reproduce np.unique(..., return_counts=True)
    c = np.random.default_rng(3).integers(0, 4, 500).astype(np.float32)
    nz = c[c > np.float32(0.01)]
    values, counts = np.unique(nz, return_counts=True)
    b = bin_index(nz, count_edges_np(3))
    assert np.array_equal(np.bincount(b, minlength=3)[values.astype(int) - 1], counts)
    # the count ranges of histograms.py:1058-1065 with a -inf threshold
    raw = (np.random.default_rng(4).random(500, dtype=np.float32) * 5).astype(np.float32)
    b = bin_index(raw, count_range_edges(3).numpy())
    want = [np.sum((raw >= 0) & (raw < 0.5))] + [np.sum((raw >= k - 0.5) & (raw < k + 0.5)) for k in (1, 2, 3)] \
        + [np.sum(raw >= 3.5)]
    assert np.bincount(b, minlength=5).tolist() == want


# ---- argument validation of the two entries, without a GPU -------------------------------------------
def test_entry_points_reject_bad_arguments_before_any_hip_call():
    build.build()
    lib = _lib.load()
    p = ctypes.c_void_p(16)

    def update(act=p, lda=768, labels=p, b=64, pn=768, k=200, edges=p, nb=50, n_class=p, n_ge=p, n_gt=p, total=p,
               total_gt=p, vmax=p, hist=p, bad=p):
        return lib.pipnet_proto_stats_update_f32(act, lda, labels, b, pn, k, 0.01, edges, nb, n_class, n_ge, n_gt,
                                                 total, total_gt, vmax, hist, bad, None)

    bad = [dict(b=0), dict(b=-1), dict(pn=0), dict(k=0), dict(lda=767), dict(nb=K.PROTO_STATS_MAX_BINS + 1),
           dict(nb=-1), dict(edges=None), dict(hist=None)]
    bad += [{name: None} for name in ("act", "labels", "n_class", "n_ge", "n_gt", "total", "total_gt", "vmax", "bad")]
    for kw in bad:
        assert update(**kw) == 1, kw
    assert lib.pipnet_colsum_accum_f64(None, 48, 4, 48, p, None) == 1
    assert lib.pipnet_colsum_accum_f64(p, 48, 4, 48, None, None) == 1
    assert lib.pipnet_colsum_accum_f64(p, 48, 0, 48, p, None) == 1
    assert lib.pipnet_colsum_accum_f64(p, 48, 4, 0, p, None) == 1
    assert lib.pipnet_colsum_accum_f64(p, 47, 4, 48, p, None) == 1
    # the wrappers refuse host tensors: there is no CPU fallback behind the kernel entry
    st = K.ProtoStatsState(3, 4, 0.01, None, "cpu")
    with pytest.raises(RuntimeError):
        K.proto_stats_update(st, torch.zeros(2, 4), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError):
        K.colsum_accum_f64(torch.zeros(4, dtype=torch.float64), torch.zeros(2, 4))
