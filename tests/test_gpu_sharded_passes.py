"""The dataset passes sharded over ranks, on the device (csrc/state_merge.hip, count_pipnet_amd/dist.py
ShardedPass): the three merge kernels against the one-pass state and against the torch merge paths (whose own
oracle is brute force, tests/test_sharded_passes_cpu.py), ``first_index`` in one process, and gloo worlds of 2 and
3 ranks on cuda:0 (RCCL refuses two ranks on one device) running every pass sharded against one process."""
import copy

import numpy as np
import pytest
import torch

from count_pipnet_amd import kernels as K
from count_pipnet_amd.explain_forward import located_forward
from count_pipnet_amd.purity import part_purity
from count_pipnet_amd.topk import prototype_topk
from explain_trace_cases import _purity_fixture
from golden_util import eval_loader_batches
from model_util import build_model
from part_purity_util import annotations_table, assert_state_equal, geometry, new_state, np_update, random_table
from proto_stats_util import planted_activations
from sharded_pass_util import assert_world, case_data, block_loader, chain_sum, cuts, run_world, sum_bound

pytestmark = pytest.mark.gpu

TOPK_N = 40
# W -> block sizes of the 40 images: an empty block, blocks shorter than k = 3 (and all shorter than k = 32)
TOPK_BLOCKS = {1: (40,), 2: (13, 27), 3: (0, 2, 38), 8: (0, 1, 2, 3, 5, 7, 9, 13)}
STATS_BLOCKS = ((5, 32), (12, 12, 13), (0, 37))
PURITY_BLOCKS = ((5, 18), (7, 8, 8), (0, 23))


def _host(state):
    """A state with every tensor on the host (the torch merge path takes it)."""
    out = copy.copy(state)
    for f in state.PACK:
        setattr(out, f, getattr(state, f).cpu())
    if getattr(state, "edges", None) is not None:
        out.edges = state.edges.cpu()
    return out


def _equal_states(a, b):
    return [f for f in a.PACK if not (getattr(a, f).dtype == getattr(b, f).dtype
                                      and torch.equal(getattr(a, f).cpu(), getattr(b, f).cpu()))]


# ---- the top-k merge kernel ----------------------------------------------------------------------------------
@pytest.mark.parametrize("ties", [True, False], ids=["ties", "floats"])
@pytest.mark.parametrize("pn", [1, 63, 64, 65, 768])
def test_topk_merge_kernel_gives_the_one_pass_state(gpu, pn, ties):
    g = torch.Generator().manual_seed(pn + ties)
    if ties:
        score = torch.tensor([0.0, 0.25, 0.5, 1.0])[torch.randint(0, 4, (TOPK_N, pn), generator=g)]
    else:
        score = torch.rand((TOPK_N, pn), generator=g)
    loc = torch.randint(0, 64, (TOPK_N, pn), generator=g, dtype=torch.int32)
    logits = torch.rand((TOPK_N, 5), generator=g) * (torch.rand((TOPK_N, 1), generator=g) < 0.7)   # zero rows abstain
    score, loc, logits = score.to(gpu), loc.to(gpu), logits.to(gpu).contiguous()
    compared = 0
    for groups in (1, 3):
        group = torch.randint(-1, groups, (TOPK_N,), generator=g, dtype=torch.int32).to(gpu)     # -1 skips the image
        for k in (1, 3, 32):
            for min_score in (None, 0.3):
                def fill(lo, hi, step):
                    st = K.TopkState(groups, pn, k, gpu)
                    for i in range(lo, hi, step):
                        j = min(i + step, hi)
                        K.topk_update(st, score[i:j], loc[i:j], i, group[i:j], min_score, logits[i:j])
                    return st
                one = fill(0, TOPK_N, 7)
                assert int(one.abstained) == int((logits.amax(dim=1) == 0).sum()) > 0
                for world, sizes in TOPK_BLOCKS.items():
                    states = [fill(lo, hi, TOPK_N) for lo, hi in cuts(sizes)]
                    merged = K.topk_merge(states)
                    assert _equal_states(merged, one) == [], (groups, k, min_score, world)
                    assert _equal_states(K.topk_merge([_host(s) for s in states]), one) == [], (groups, k, world)
                    compared += 1
    assert compared == 2 * 3 * 2 * 4 and int((one.index < 0).sum()) > 0          # empty slots were compared too


def test_topk_merge_reads_views_of_one_gathered_buffer_where_they_lie(gpu):
    """The passes hand over views into the all-gathered buffer: same result as from separate states, and with an
    odd G * P (fill's bytes are no multiple of 8) every field still sits on its alignment."""
    g = torch.Generator().manual_seed(3)
    pn, k, world = 65, 3, 3
    states = []
    for r in range(world):
        st = K.TopkState(1, pn, k, gpu)
        K.topk_update(st, torch.rand((4, pn), generator=g).to(gpu), torch.randint(0, 64, (4, pn), generator=g,
                                                                                  dtype=torch.int32).to(gpu), 4 * r)
        states.append(st)
    buf = torch.stack([s.pack() for s in states])
    views = [states[0].unpack(row) for row in buf]
    assert all(getattr(v, f).data_ptr() % getattr(v, f).element_size() == 0 for v in views for f in v.PACK)
    assert _equal_states(K.topk_merge(views), K.topk_merge(states)) == []
    assert int(K.topk_merge(states).fill.min()) == k


# ---- the statistics merge kernel -------------------------------------------------------------------------------
@pytest.mark.parametrize("integers", [False, True], ids=["floats", "integers"])
@pytest.mark.parametrize("pn", [1, 65, 768])
def test_proto_stats_merge_kernel(gpu, pn, integers):
    n, kc, nb, thr = 37, 5, 8, 0.01
    edges = np.linspace(0.01, 4.0 if integers else 1.01, nb + 1, dtype=np.float32)
    act = planted_activations(n, pn, thr, edges, seed=pn, counts=3 if integers else 0).numpy()
    if integers:
        act = np.floor(act)
    labels = torch.randint(0, kc - 1, (n,), generator=torch.Generator().manual_seed(pn))      # class 4 is absent
    labels[5] = 0
    ad, ld = torch.from_numpy(act.astype(np.float32)).to(gpu), labels.to(gpu)

    def fill(lo, hi):
        st = K.ProtoStatsState(kc, pn, thr, torch.from_numpy(edges), gpu)
        return K.proto_stats_update(st, ad[lo:hi], ld[lo:hi]) if hi > lo else st

    one = fill(0, n)
    assert int(one.n_class[kc - 1]) == 0 and int(one.n_class.sum()) == n and int(one.hist.sum()) > 0
    for sizes in STATS_BLOCKS:
        states = [fill(lo, hi) for lo, hi in cuts(sizes)]
        merged = K.proto_stats_merge(states)
        for f in ("n_class", "n_ge", "n_gt", "vmax", "hist", "bad"):
            assert torch.equal(getattr(merged, f), getattr(one, f)), (f, sizes)
        assert _equal_states(K.proto_stats_merge([_host(s) for s in states]), merged) == [], sizes
        for f in ("total", "total_gt"):
            got = getattr(merged, f).cpu().numpy()
            assert np.array_equal(got, chain_sum([getattr(s, f).cpu().numpy() for s in states])), (f, sizes)
            want = getattr(one, f).cpu().numpy()
            if integers:
                assert np.array_equal(got, want), (f, sizes)
            else:
                bound = sum_bound(one.n_class.cpu().numpy()[:, None], len(sizes), want)
                assert (np.abs(got - want) <= bound).all(), (f, sizes)
    acc = torch.rand((3, pn), dtype=torch.float64, generator=torch.Generator().manual_seed(1)).to(gpu)
    assert np.array_equal(K.colsum_merge_f64(acc).cpu().numpy(), chain_sum(list(acc.cpu().numpy())))
    wide = torch.zeros((3, pn + 3), dtype=torch.float64, device=gpu)
    wide[:, :pn] = acc
    assert torch.equal(K.colsum_merge_f64(wide[:, :pn]), K.colsum_merge_f64(acc))          # a row stride above D


# ---- the part-purity merge kernel ------------------------------------------------------------------------------
@pytest.mark.parametrize("pn", [1, 65])
def test_part_purity_merge_kernel(gpu, pn):
    n, q, hw, thr = 23, 15, 8, 0.5
    assert q <= K.PART_PURITY_MAX_PARTS
    rng = np.random.default_rng(pn)
    table = random_table(rng, n, q, 3)
    geo = geometry(hw, hw, 64)
    pooled = rng.random((n, pn), dtype=np.float32)
    loc = rng.integers(0, hw * hw, (n, pn)).astype(np.int32)
    relevant = np.ones(pn, dtype=bool) if pn == 1 else rng.random(pn) < 0.9
    dt = tuple(torch.from_numpy(table[k]).to(gpu) for k in ("xy", "vis", "size", "merged", "is_left", "pair_index"))
    pd, ld = torch.from_numpy(pooled).to(gpu), torch.from_numpy(loc).to(gpu)
    rd = torch.from_numpy(relevant.astype(np.uint8)).to(gpu)
    mn = len(table["keep"])

    def fill(lo, hi):
        st = K.PartPurityState(pn, mn, gpu)
        return K.part_purity_update(st, pd[lo:hi], ld[lo:hi], rd, lo, thr, geo, dt) if hi > lo else st

    def as_np(st):
        return dict(n=st.n.cpu().numpy(), hits=st.hits.cpu().numpy(), rows=st.rows.cpu().numpy(),
                    first_key=st.first_key.cpu().numpy().view(np.uint64))

    one = fill(0, n)
    want = np_update(new_state(pn, mn), pooled, loc, relevant, 0, thr, geo, table)
    assert want["rows"].sum() > 0
    fin_one = K.part_purity_finish(one)
    for sizes in PURITY_BLOCKS:
        states = [fill(lo, hi) for lo, hi in cuts(sizes)]
        merged = K.part_purity_merge(states)
        assert_state_equal(as_np(merged), as_np(one), sizes)
        assert_state_equal(as_np(merged), want, sizes)
        assert int(merged.bad) == 0
        assert _equal_states(K.part_purity_merge([_host(s) for s in states]), merged) == [], sizes
        for a, b in zip(K.part_purity_finish(merged), fin_one):
            assert a.dtype == b.dtype and torch.equal(torch.nan_to_num(a.double(), nan=-1.0),
                                                      torch.nan_to_num(b.double(), nan=-1.0)), sizes


# ---- the wrappers' argument checks -----------------------------------------------------------------------------
def test_merge_wrappers_refuse_before_any_launch(gpu):
    a = K.TopkState(1, 4, 3, gpu)
    for states, what in (([a, K.TopkState(1, 4, 2, gpu)], "k"), ([a, K.TopkState(1, 5, 3, gpu)], "prototypes"),
                         ([a, K.TopkState(1, 4, 3, "cpu")], "cpu"), ([], "W = 0")):
        with pytest.raises(RuntimeError, match=what):
            K.topk_merge(states)
    e4, e5 = torch.linspace(0, 1, 4), torch.linspace(0, 1, 5)
    with pytest.raises(RuntimeError, match="bins"):
        K.proto_stats_merge([K.ProtoStatsState(2, 3, 0.01, e4, gpu), K.ProtoStatsState(2, 3, 0.01, e5, gpu)])
    with pytest.raises(RuntimeError, match="cpu"):
        K.proto_stats_merge([K.ProtoStatsState(2, 3, 0.01, e4, gpu), K.ProtoStatsState(2, 3, 0.01, e4, "cpu")])
    with pytest.raises(RuntimeError, match="merged_parts"):
        K.part_purity_merge([K.PartPurityState(3, 2, gpu), K.PartPurityState(3, 4, gpu)])
    with pytest.raises(RuntimeError, match="W = 0"):
        K.part_purity_merge([])
    with pytest.raises(RuntimeError):
        K.colsum_merge_f64(torch.zeros((0, 4), dtype=torch.float64, device=gpu))
    lib = K._lib.load()         # the library's own checks: no rank, too many ranks, a stride that is no multiple of 8
    p = K._lib.P(16)
    assert lib.pipnet_topk_merge(p, p, p, p, p, 8, 0, 1, 4, 3, p, p, p, p, p, None) == 1
    assert lib.pipnet_topk_merge(p, p, p, p, p, 8, K.STATE_MERGE_MAX_RANKS + 1, 1, 4, 3, p, p, p, p, p, None) == 1
    assert lib.pipnet_topk_merge(p, p, p, p, p, 12, 2, 1, 4, 3, p, p, p, p, p, None) == 1
    assert lib.pipnet_part_purity_merge(p, p, p, p, p, 8, 2, 3, K.PART_PURITY_MAX_PARTS + 1, p, p, p, p, p, None) == 1
    assert lib.pipnet_proto_stats_merge(p, p, p, p, p, p, None, p, 8, 2, 2, 3, 4, p, p, p, p, p, p, p, p, None) == 1
    assert lib.pipnet_colsum_merge_f64(p, 8, 2, 0, p, None) == 1


# ---- first_index in one process --------------------------------------------------------------------------------
def test_first_index_shifts_the_topk_indices_and_nothing_else(gpu):
    from sharded_pass_util import same
    net, xs, ys, _ = case_data("pipnet_mid_addon", 12, 700, gpu)
    plain = prototype_topk(net, block_loader(net, xs, ys, None, 0, 12, bs=5), 3, image_size=64).cpu()
    moved = prototype_topk(net, block_loader(net, xs, ys, None, 0, 12, bs=5), 3, image_size=64, first_index=100).cpu()
    assert int((plain.index >= 0).sum()) > 0
    assert torch.equal(moved.index, torch.where(plain.index >= 0, plain.index + 100, plain.index))
    assert same(moved, plain) == ["index"]
    with pytest.raises(ValueError, match="first_index"):
        prototype_topk(net, [], 3, image_size=64, first_index=-1)


def test_first_index_gives_part_purity_of_the_second_half(gpu):
    meta, rec, fwd_meta, ann = _purity_fixture()
    c = fwd_meta["case"]
    net = build_model(fwd_meta).to(gpu)
    with torch.no_grad():
        net._classification.weight.copy_(torch.from_numpy(rec["weight"]))
    batches = eval_loader_batches(c["size"], c["num_classes"], meta["batches"], meta["batch_size"], meta["label_seed"])
    xs = torch.cat([x for x, _ in batches])[:meta["images"]]
    n, half = xs.shape[0], xs.shape[0] // 2
    ys = torch.zeros(n, dtype=torch.int64)
    res = part_purity(net, block_loader(net, xs, ys, None, half, n, bs=5), ann, image_size=c["size"], mode="all",
                      threshold=meta["threshold"], relevance_threshold=meta["relevance"], first_index=half).cpu()
    with torch.no_grad():
        outs = [located_forward(net, xs[i:i + 1].to(gpu), None, with_raw=True) for i in range(half, n)]
    pooled = torch.cat([o.raw for o in outs]).cpu().numpy()
    loc = torch.cat([o.loc for o in outs]).cpu().numpy()
    relevant = rec["weight"].max(axis=0) > np.float32(meta["relevance"])
    table = annotations_table(ann)
    want = np_update(new_state(pooled.shape[1], len(table["keep"])), pooled, loc, relevant, half, meta["threshold"],
                     geometry(outs[0].hw[0], outs[0].hw[1], c["size"]), table)
    got = dict(n=res.n.numpy(), hits=res.hits.numpy(), rows=res.rows.numpy(),
               first_key=res.first_key.numpy().view(np.uint64))
    assert_state_equal(got, want)
    assert want["rows"].sum() > 0 and res.images == n - half and tuple(res.row_loc.shape) == (n - half, pooled.shape[1])
    with pytest.raises(ValueError, match="saw"):           # the pass must end where the annotations end
        part_purity(net, block_loader(net, xs, ys, None, half, n - 1, bs=5), ann, image_size=c["size"],
                    first_index=half)


# ---- gloo worlds on cuda:0 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_passes_over_gloo_on_one_gpu_equal_one_process(gpu, world):
    """One spawn per world: every rank runs each pass sharded on its block (3+2, 2+2+1, 1+1+0; the purity fixture
    in chunks) and in one process over everything, and compares (tests/sharded_pass_util.py stats_scenarios,
    gpu_scenarios)."""
    res = run_world(world, "cuda")
    assert_world(res, world)
    checks = set(res[0]) - {"rank"}
    for name in ("topk_pipnet_mid_addon_5", "topk_count_onehot_5", "topk_count_onehot_5_everywhere",
                 "stats_pipnet_mid_addon_5_exact", "stats_count_onehot_5_total_equal", "mean_count_onehot_5",
                 "process_group_argument") + (("purity_all_2", "topk_pipnet_mid_addon_2") if world == 3 else ()):
        assert name in checks, (name, sorted(checks))
    assert any(c.startswith("purity_all_") and c.endswith("_rows") for c in checks)
    assert any(c.startswith("purity_topk_") and c.endswith("_summary") for c in checks)
