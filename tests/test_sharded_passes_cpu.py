"""The dataset passes sharded over ranks, without a GPU: ``dist.dataset_shard``, the torch paths of the three
state merges (``kernels.topk_merge`` / ``proto_stats_merge`` / ``part_purity_merge``, the oracles of the kernel
tests in tests/test_gpu_sharded_passes.py) against brute force, and ``class_prototype_stats`` /
``mean_intermediate_features`` on CPU nets over gloo worlds of 2 and 3 ranks -- blocks 3+2, 2+2+1 and 1+1+0 --
with the failures that must reach every rank instead of hanging one of them in a collective."""
import time

import numpy as np
import pytest
import torch

from count_pipnet_amd import kernels as K
from count_pipnet_amd.dist import dataset_shard, shard_sizes
from part_purity_util import NO_KEY
from sharded_pass_util import SPAWN_TIMEOUT, assert_world, brute_topk, chain_sum, cuts, run_world


@pytest.mark.parametrize("world", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("n", [0, 1, 5, 13])
def test_dataset_shard_tiles_the_dataset_like_shard_sizes(n, world):
    blocks = [dataset_shard(n, world, r) for r in range(world)]
    assert [hi - lo for lo, hi in blocks] == shard_sizes(n, world)
    assert blocks[0][0] == 0 and blocks[-1][1] == n
    assert all(blocks[r][1] == blocks[r + 1][0] for r in range(world - 1))


def test_dataset_shard_example_and_argument_rule():
    assert [dataset_shard(5, 4, r) for r in range(4)] == [(0, 2), (2, 4), (4, 5), (5, 5)]
    for bad in ((5, 0, 0), (5, 2, 2), (5, 2, -1), (-1, 2, 0)):
        with pytest.raises(ValueError):
            dataset_shard(*bad)


@pytest.mark.parametrize("world,k", [(1, 3), (2, 1), (3, 5), (8, 32)])
def test_torch_topk_merge_is_the_sorted_union(world, k):
    """40 candidates per (group, prototype) with scores from four values, so nearly all tie; cut into ``world``
    blocks (one empty, some shorter than k); every block's list is its own k best."""
    g = np.random.default_rng(world * 100 + k)
    groups, protos, n = 2, 5, 40
    score = g.choice(np.array([0.0, 0.25, 0.5, 1.0], dtype=np.float32), (groups, protos, n))
    loc = g.integers(0, 64, (groups, protos, n)).astype(np.int32)
    sizes = [0] + list(np.diff(np.sort(np.concatenate(([0, n], g.integers(0, n + 1, world - 2))))))  \
        if world > 1 else [n]
    assert len(sizes) == world and sum(sizes) == n
    states, lists = [], {}
    for r, (lo, hi) in enumerate(cuts(sizes)):
        st = K.TopkState(groups, protos, k, "cpu")
        st.abstained += r + 1
        for gi in range(groups):
            for p in range(protos):
                cand = [(float(score[gi, p, i]), i, int(loc[gi, p, i])) for i in range(lo, hi)]
                lists.setdefault((gi, p), []).append(cand)
                best = brute_topk([cand], k)
                st.fill[gi, p] = len(best)
                for j, (s, i, l) in enumerate(best):
                    st.score[gi, p, j], st.index[gi, p, j], st.loc[gi, p, j] = s, i, l
        states.append(st)
    out = K.topk_merge(states)
    assert int(out.abstained) == world * (world + 1) // 2
    for (gi, p), cand in lists.items():
        want = brute_topk(cand, k)
        assert int(out.fill[gi, p]) == len(want) == min(k, n)
        got = list(zip(out.score[gi, p].tolist(), out.index[gi, p].tolist(), out.loc[gi, p].tolist()))
        assert got[:len(want)] == want and all(e == (0.0, -1, -1) for e in got[len(want):]), (gi, p)


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_torch_proto_stats_merge_is_the_rank_ordered_sum(world):
    g = np.random.default_rng(world)
    kc, pn, nb = 4, 6, 5
    edges = torch.linspace(0.0, 1.0, nb + 1)
    states = []
    for r in range(world):
        st = K.ProtoStatsState(kc, pn, 0.01, edges, "cpu")
        st.n_class.copy_(torch.from_numpy(g.integers(0, 9, kc)))
        st.n_ge.copy_(torch.from_numpy(g.integers(0, 9, (kc, pn))))
        st.n_gt.copy_(torch.from_numpy(g.integers(0, 9, (kc, pn))))
        st.total.copy_(torch.from_numpy(g.random((kc, pn)) * 10.0 ** g.integers(-8, 8, (kc, pn))))
        st.total_gt.copy_(torch.from_numpy(g.random((kc, pn))))
        vmax = np.where(g.random((kc, pn)) < 0.3, -np.inf, g.random((kc, pn)))
        st.vmax.copy_(torch.from_numpy(vmax.astype(np.float32)))
        st.hist.copy_(torch.from_numpy(g.integers(0, 9, (kc, pn, nb)).astype(np.int32)))
        st.bad += int(g.integers(0, 3))
        states.append(st)
    out = K.proto_stats_merge(states)
    for f in ("n_class", "n_ge", "n_gt", "hist", "bad"):
        assert np.array_equal(getattr(out, f).numpy(), sum(getattr(s, f).numpy().astype(np.int64) for s in states)), f
    assert np.array_equal(out.vmax.numpy(), np.max([s.vmax.numpy() for s in states], axis=0))
    for f in ("total", "total_gt"):
        want = np.zeros((kc, pn))
        for i in range(kc):
            for j in range(pn):
                acc = 0.0
                for s in states:                        # a Python loop of float64 adds in rank order
                    acc += float(getattr(s, f)[i, j])
                want[i, j] = acc
        assert np.array_equal(getattr(out, f).numpy(), want) and np.array_equal(
            want, chain_sum([getattr(s, f).numpy() for s in states])), f
    assert out.bins == nb and torch.equal(out.edges, states[0].edges) and out.threshold == states[0].threshold
    acc = torch.from_numpy(g.random((world, 7)))
    assert np.array_equal(K.colsum_merge_f64(acc).numpy(), chain_sum(list(acc.numpy())))


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_torch_part_purity_merge_adds_and_takes_the_unsigned_minimum(world):
    g = np.random.default_rng(world + 50)
    pn, mn = 5, 7
    states, keys = [], []
    for r in range(world):
        st = K.PartPurityState(pn, mn, "cpu")
        for f in ("n", "hits", "rows", "bad"):
            t = getattr(st, f)
            t.copy_(torch.from_numpy(g.integers(0, 50, tuple(t.shape))))
        # keys with the top bit set (they are negative as int64) next to small ones and NO_KEY
        key = g.integers(0, 2 ** 63, (pn, mn), dtype=np.uint64) * np.uint64(2)
        key = key + g.integers(0, 2, (pn, mn), dtype=np.uint64)
        key = np.where(g.random((pn, mn)) < 0.3, NO_KEY, np.where(g.random((pn, mn)) < 0.5, key >> np.uint64(40), key))
        st.first_key.copy_(torch.from_numpy(key.astype(np.uint64).view(np.int64)))
        keys.append(key.astype(np.uint64))
        states.append(st)
    out = K.part_purity_merge(states)
    for f in ("n", "hits", "rows", "bad"):
        assert np.array_equal(getattr(out, f).numpy(), sum(getattr(s, f).numpy() for s in states)), f
    want = keys[0]
    for key in keys[1:]:
        want = np.minimum(want, key)
    assert np.array_equal(out.first_key.numpy().view(np.uint64), want)
    assert (want == NO_KEY).any() or world > 2          # never inserted on any rank stays never inserted


def test_merge_wrappers_refuse_states_that_do_not_fit():
    a, b = K.TopkState(1, 4, 3, "cpu"), K.TopkState(1, 4, 2, "cpu")
    with pytest.raises(RuntimeError, match="k"):
        K.topk_merge([a, b])
    with pytest.raises(RuntimeError, match="W = 0"):
        K.topk_merge([])
    with pytest.raises(RuntimeError, match="prototypes"):
        K.part_purity_merge([K.PartPurityState(3, 2, "cpu"), K.PartPurityState(4, 2, "cpu")])
    with pytest.raises(RuntimeError, match="bins"):
        K.proto_stats_merge([K.ProtoStatsState(2, 3, 0.01, torch.linspace(0, 1, 4), "cpu"),
                             K.ProtoStatsState(2, 3, 0.01, torch.linspace(0, 1, 5), "cpu")])
    with pytest.raises(RuntimeError, match="at most"):
        K.topk_merge([a] * (K.STATE_MERGE_MAX_RANKS + 1))
    with pytest.raises(RuntimeError, match="TopkState"):
        K.topk_merge([a, K.PartPurityState(3, 2, "cpu")])


def test_packed_states_round_trip_and_keep_every_field_aligned():
    for st in (K.TopkState(3, 65, 5, "cpu"), K.ProtoStatsState(3, 5, 0.01, torch.linspace(0, 1, 4), "cpu"),
               K.ProtoStatsState(3, 5, 0.01, None, "cpu"), K.PartPurityState(5, 3, "cpu")):
        for n, f in enumerate(st.PACK):
            getattr(st, f).copy_(torch.arange(getattr(st, f).numel()).view(getattr(st, f).shape) + n)
        buf = st.pack()
        assert buf.dtype == torch.uint8 and buf.numel() == st.packed_bytes() and buf.numel() % 8 == 0
        back = st.unpack(buf)
        sizes = [getattr(st, f).element_size() for f in st.PACK]
        assert sizes == sorted(sizes, reverse=True)             # descending element size: every view aligned
        for f in st.PACK:
            assert torch.equal(getattr(back, f), getattr(st, f)) and getattr(back, f).dtype == getattr(st, f).dtype
            assert getattr(back, f).data_ptr() % getattr(st, f).element_size() == 0
        with pytest.raises(RuntimeError):
            st.unpack(buf[:-8])
    # the sizes DESIGN.md quotes for C2 / CUB: P = 768, K = 200, 50 bins, k = 10
    assert K.TopkState(1, 768, 10, "meta").packed_bytes() == 125960
    assert 36.0e6 < K.ProtoStatsState(200, 768, 0.01, torch.zeros(51), "meta").packed_bytes() < 36.5e6


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_stats_over_gloo_equal_one_process(world):
    """One spawn per world: every scenario of tests/sharded_pass_util.py (stats_scenarios, protocol_scenarios) on
    CPU nets; no rank may come near the spawn helper's timeout (a mismatched collective would)."""
    t0 = time.monotonic()
    res = run_world(world, "cpu")
    assert_world(res, world)
    assert time.monotonic() - t0 < SPAWN_TIMEOUT / 2
    checks = set(res[0]) - {"rank"}
    for name in ("stats_pipnet_mid_addon_5_exact", "stats_count_onehot_5_total_equal",
                 "stats_pipnet_mid_addon_5_total_bound", "stats_pipnet_mid_addon_5_total_chain", "mean_count_onehot_5", "stats_count_onehot_max_images",
                 "label_outside_raises_everywhere", "loader_failure", "blocks_out_of_order", "process_group_argument"):
        assert name in checks, name
    if world == 3:
        assert "stats_pipnet_mid_addon_2_exact" in checks and "mean_count_onehot_2" in checks      # 1 + 1 + 0
