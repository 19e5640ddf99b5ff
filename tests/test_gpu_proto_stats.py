"""Class-conditional prototype statistics on the device (csrc/proto_stats.hip,
count_pipnet_amd/stats.py): the update kernel against the numpy restatement on planted values,
batch-split invariance of every state tensor (fp64 sums bitwise), the recorded reference
activations through the kernel, the end-to-end passes over the fixture models, and the mean
intermediate features / virtual weights."""
import numpy as np
import pytest
import torch

from count_pipnet_amd import kernels as K
from count_pipnet_amd.stats import (class_prototype_stats, count_range_edges, mean_intermediate_features,
                                    virtual_weights)
from model_util import build_model
from proto_stats_ref import decisive_pairs, stats_state
from proto_stats_util import (FIXTURES, PIPNET_EDGES, assert_state_equal, check_against_fixture, count_edges_np,
                              label_pattern, load_stats_fixture, planted_activations, ragged_loader, reference_state,
                              runs_of, state_np)

pytestmark = pytest.mark.gpu

THR = 0.01
# (B, P, K, NB): one thread / one class; odd sizes; C2 (12 column blocks, 16 class partitions);
# C5's width with the count edges
KERNEL_CASES = [(1, 16, 1, 1), (7, 100, 3, 50), (64, 768, 200, 50), (5, 2048, 9, 4)]


def _edges(nb):
    if nb == 50:
        return PIPNET_EDGES
    if nb == 4:
        return count_edges_np(4)
    return np.array([THR, 1.01], dtype=np.float32)


def _run(gpu, act, labels, k, thr, edges, splits=None):
    """Stream (act, labels) through the kernel in batches of ``splits`` (None: one batch)."""
    st = K.ProtoStatsState(k, act.shape[1], thr, None if edges is None else torch.from_numpy(np.asarray(edges)), gpu)
    a, l = act.to(gpu), labels.to(gpu)
    i = 0
    for s in splits or [act.shape[0]]:
        K.proto_stats_update(st, a[i:i + s], l[i:i + s].contiguous())
        i += s
    assert i == act.shape[0]
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("pattern", ["equal", "sorted", "alternating"])
@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_update_kernel_matches_restatement(gpu, case, pattern):
    b, p, k, nb = case
    edges = _edges(nb)
    act = planted_activations(b, p, THR, edges, seed=sum(case), counts=4 if nb == 4 else 0)
    labels = label_pattern(pattern, b, k, seed=b + k)
    st = _run(gpu, act, labels, k, THR, edges)
    want = reference_state(act, labels, k, THR, edges)
    assert_state_equal(state_np(st), want, (case, pattern))
    assert int(st.bad) == 0 and int(st.n_class.sum()) == b
    if b * p >= 3 * (nb + 2) + 3:            # every planted value went in: the edge bins are populated
        assert want["hist"].sum() > 0 and want["n_ge"].sum() > want["n_gt"].sum()


def test_update_kernel_strided_view_bad_labels_and_infinite_edges(gpu):
    b, p, k = 23, 100, 5
    # a sliced view: row stride 137 > P, storage offset 5
    wide = planted_activations(b, 137, THR, PIPNET_EDGES, seed=9)
    act = wide[:, 5:5 + p]
    labels = torch.randint(0, k, (b,), generator=torch.Generator().manual_seed(2))
    st = K.ProtoStatsState(k, p, THR, torch.from_numpy(PIPNET_EDGES), gpu)
    K.proto_stats_update(st, wide.to(gpu)[:, 5:5 + p], labels.to(gpu))
    assert_state_equal(state_np(st), reference_state(act.contiguous(), labels, k, THR, PIPNET_EDGES), "lda > P")
    # labels -1 and K only raise ``bad``
    lb = labels.clone()
    lb[3], lb[11], lb[12] = -1, k, k + 40
    st = _run(gpu, act.contiguous(), lb, k, THR, PIPNET_EDGES)
    keep = (lb >= 0) & (lb < k)
    assert int(st.bad) == 3
    assert_state_equal(state_np(st), reference_state(act[keep].contiguous(), lb[keep], k, THR, PIPNET_EDGES), "bad labels")
    # threshold -inf, last edge +inf: the count ranges of histograms.py:1058-1065, every value counted
    e = count_range_edges(3).numpy()
    raw = planted_activations(b, p, 0.5, e[:-1], seed=10, counts=3)
    st = _run(gpu, raw, labels, k, float("-inf"), e)
    want = reference_state(raw, labels, k, float("-inf"), e)
    assert_state_equal(state_np(st), want, "-inf threshold")
    assert int(st.hist.sum()) == int((raw >= 0).sum()) and torch.equal(st.n_ge, st.n_gt)
    # no histogram at all
    st = _run(gpu, act.contiguous(), labels, k, THR, None)
    assert_state_equal(state_np(st), reference_state(act.contiguous(), labels, k, THR, None), "NB = 0")


def test_state_is_bitwise_independent_of_the_batch_split(gpu):
    b, p, k = 37, 768, 7
    act = planted_activations(b, p, THR, PIPNET_EDGES, seed=37)
    labels = torch.randint(0, k, (b,), generator=torch.Generator().manual_seed(37))
    runs = [_run(gpu, act, labels, k, THR, PIPNET_EDGES, s) for s in (None, [1] * 37, [5, 32])]
    for other in runs[1:]:
        for x, y in zip(runs[0].tensors(), other.tensors()):
            assert x.dtype == y.dtype and torch.equal(x, y)
    assert_state_equal(state_np(runs[0]), reference_state(act, labels, k, THR, PIPNET_EDGES), "one batch")


@pytest.mark.parametrize("d", [48, 6144])
def test_colsum_accum_f64_in_image_order_and_split_invariant(gpu, d):
    g = torch.Generator().manual_seed(d)
    wide = torch.rand(37, d + 8, generator=g) * 3.0
    x = wide[:, :d].to(gpu)                      # row stride d + 8
    accs = []
    for splits in ([37], [1] * 37, [5, 32]):
        acc = torch.zeros(d, device=gpu, dtype=torch.float64)
        i = 0
        for s in splits:
            K.colsum_accum_f64(acc, x[i:i + s])
            i += s
        accs.append(acc)
    assert torch.equal(accs[0], accs[1]) and torch.equal(accs[0], accs[2])
    want = np.cumsum(wide[:, :d].numpy().astype(np.float64), axis=0)[-1]
    assert accs[0].cpu().numpy().tobytes() == want.tobytes()


@pytest.mark.parametrize("name", FIXTURES)
def test_recorded_activations_through_the_kernel(gpu, name):
    """Every quantity the reference reported, from the state the kernel accumulates over the
    activations the reference collected, cut raggedly: counts, traces and report exact, means to
    rtol 1e-5 (the reference's fp32 np.mean against the fp64 sum)."""
    meta, rec, fwd = load_stats_fixture(name)
    case = fwd["case"]
    count = case["model"] != "pipnet"
    compared = 0
    for tag, continuous in runs_of(meta):
        edges = count_edges_np(case["max_count"]) if count and not continuous else PIPNET_EDGES
        acts, labels = torch.from_numpy(rec[f"{tag}_acts"]), torch.from_numpy(rec[f"{tag}_labels"])
        n = acts.shape[0]
        st = _run(gpu, acts, labels, case["num_classes"], meta["threshold"], edges, [3, 1, n - 4])
        got = state_np(st)
        assert_state_equal(got, stats_state(acts.numpy(), labels.numpy(), case["num_classes"], meta["threshold"], edges),
                           (name, tag))
        compared += check_against_fixture(got, rec, tag, count=count, continuous=continuous, mean_rtol=1e-5)
    assert compared > 20


# (fixture, continuous, ragged batch sizes: max_images falls inside the last one used)
E2E = [("pipnet_mid_addon", False, (4, 1, 6, 4)), ("count_onehot", False, (7, 2, 9, 7)), ("count_onehot", True, (7, 2, 9, 7))]


@pytest.mark.parametrize("name,continuous,sizes", E2E, ids=lambda v: str(v).replace(" ", ""))
def test_class_prototype_stats_end_to_end(gpu, name, continuous, sizes):
    meta, rec, fwd = load_stats_fixture(name)
    case = fwd["case"]
    count = case["model"] != "pipnet"
    net = build_model(fwd).to(gpu)
    tag = "c" if continuous else "d"
    seed, mx, kc = meta["runs"][tag]["noise_seed"], meta["max_images"], case["num_classes"]
    assert sum(sizes[:-1]) < mx < sum(sizes)
    edges = PIPNET_EDGES if continuous else None
    res = class_prototype_stats(net, ragged_loader(meta, fwd, net, seed, sizes, mx, gpu), max_images=mx,
                                continuous=continuous, edges=edges)
    assert res.n_ge.is_cuda and res.images == mx
    # (a) the restatement on the existing forward's own pooled outputs for the same batches
    own, seen = [], 0
    with torch.no_grad():
        for xs, _ in ragged_loader(meta, fwd, net, seed, sizes, mx, gpu):
            xs = xs[:mx - seen]
            own.append(net(xs.to(gpu), inference=not continuous)[1].cpu())
            seen += xs.shape[0]
    own = torch.cat(own).numpy()
    labels = rec[f"{tag}_labels"]
    used = np.asarray(res.edges.cpu())
    assert np.array_equal(used, count_edges_np(case["max_count"]) if count and not continuous else PIPNET_EDGES)
    got = state_np(res)
    assert_state_equal(got, stats_state(own, labels, kc, meta["threshold"], used), (name, tag))
    # (b) the fixture: means within the project's 1e-3, counts and bins exact on every decisive pair
    ref_acts = rec[f"{tag}_acts"]
    print(f"{name}/{tag}: max |pooled - reference| = {np.abs(own - ref_acts).max():.3e}")
    pairs = decisive_pairs(ref_acts, labels, kc, meta["threshold"], used)
    share = pairs[rec[f"{tag}_classes"]].mean()
    print(f"{name}/{tag}: decisive pairs {100 * share:.1f} %")
    assert share >= 0.9
    compared = check_against_fixture(got, rec, tag, count=count, continuous=continuous, mean_atol=1e-3, pairs=pairs)
    print(f"{name}/{tag}: {compared} traces compared bin by bin")
    assert compared > (0 if continuous else 20)
    # the derived views stay on the device and agree with the state
    assert torch.equal(res.nonzero_counts(), res.n_ge.t()) and res.mean_per_class().is_cuda
    zero, pct = res.near_zero()
    assert torch.equal(zero, mx - res.n_ge.sum(0)) and float(pct.max()) <= 100.0
    cpu = res.cpu()
    assert not cpu.hist.is_cuda and torch.equal(cpu.hist, res.hist.cpu())


def test_mean_intermediate_features_and_virtual_weights(gpu):
    meta, rec, fwd = load_stats_fixture("count_onehot")
    net = build_model(fwd).to(gpu)
    runs = meta["runs"]
    total = meta["batches"] * meta["batch_size"]
    sizes = (7, 2, 9, 7)
    seed = runs["mean_intermediate"]["noise_seed"]
    m = mean_intermediate_features(net, ragged_loader(meta, fwd, net, seed, sizes, total, gpu))
    counts = []
    with torch.no_grad():
        for xs, _ in ragged_loader(meta, fwd, net, seed, sizes, total, gpu):
            counts.append(net(xs.to(gpu), inference=True)[1])
        want = net._intermediate(torch.cat(counts)).double().mean(0)
    assert m.dtype == torch.float32 and m.is_cuda and tuple(m.shape) == tuple(want.shape)
    torch.testing.assert_close(m.double(), want, rtol=1e-6, atol=0)
    np.testing.assert_allclose(m.cpu().numpy(), rec["mean_intermediate"], rtol=0, atol=1e-3)
    vp = virtual_weights(net)
    with torch.no_grad():
        cols = torch.stack([net.get_prototype_importance_per_class(p) for p in range(net._num_prototypes)], dim=1)
    assert torch.equal(vp, cols)
    np.testing.assert_allclose(vp.cpu().numpy(), rec["virtual_plain"], rtol=0, atol=1e-3)
    vs = virtual_weights(net, ragged_loader(meta, fwd, net, runs["virtual_scaled"]["noise_seed"], sizes, total, gpu), True)
    np.testing.assert_allclose(vs.cpu().numpy(), rec["virtual_scaled"], rtol=0, atol=1e-3)
    assert not torch.equal(vs, vp)


def test_bad_label_raises_after_the_pass(gpu):
    meta, rec, fwd = load_stats_fixture("pipnet_mid_addon")
    net = build_model(fwd).to(gpu)
    with pytest.raises(ValueError, match="outside"):
        class_prototype_stats(net, ragged_loader(meta, fwd, net, 0, (15,), 15, gpu), num_classes=4)
    with pytest.raises(RuntimeError):          # no CPU fallback behind a device net: images must be device-ready floats
        class_prototype_stats(net, [(torch.zeros(2, 3, 64, 64, dtype=torch.float64), torch.zeros(2, dtype=torch.int64))])
