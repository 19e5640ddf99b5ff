"""The host side of data-parallel training (count_pipnet_amd.dist_train), without a GPU.

* the packed exchange -- rows ``[pooled 1 | out 1 | pooled 2 | out 2 | label lane]`` through ONE all-gather --
  on gloo CPU worlds of 2 and 3 with uneven shards (3+2, 2+1, 3+3+1): the gathered ``pooled / out / ys`` are
  ``torch.equal`` to ``torch.cat`` of every rank's rows in ``[view 1 of all ranks | view 2 of all ranks]`` order;
* the rank's rows of the global stochastic-depth masks; the shared generator's draws;
* the gradient arena's table: every trainable parameter once, 16-byte aligned slots, optimizer group order;
* the refusals, raised before torch.distributed is touched (a process-group stub that only knows its size and
  rank, with every collective of torch.distributed made to raise).

The device side is tests/test_gpu_dist_train.py.
"""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from count_pipnet_amd import dist_train as DT

P, K = 8, 5
# labels whose int32 bits are a denormal, a NaN pattern and an integer no float32 holds exactly: a value cast
# (instead of the bit cast) of the label lane, or a copy that is not bit-exact, would change them
LABELS = [0, 1, 199, 2 ** 24 + 1, 2 ** 31 - 1, 7, 3]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_rows(sizes, rank):
    """(pooled [2b, P], out [2b, K], ys [b]) of a rank: seeded, so every rank can rebuild every other's."""
    b = sizes[rank]
    g = torch.Generator().manual_seed(100 * len(sizes) + 10 * sum(sizes) + rank)
    start = sum(sizes[:rank])
    return (torch.randn(2 * b, P, generator=g), torch.randn(2 * b, K, generator=g),
            torch.tensor(LABELS[start:start + b], dtype=torch.int64))


def _exchange_worker(rank, world, port, cases, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    res = {"rank": rank}
    try:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        calls = []
        real = dist.all_gather_into_tensor
        dist.all_gather_into_tensor = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
        for sizes in cases:
            parts = [_rank_rows(sizes, r) for r in range(world)]
            pooled, out, ys = DT.exchange_rows(*parts[rank], sizes)
            want = [torch.cat([t[j][:s] for t, s in zip(parts, sizes)] + [t[j][s:] for t, s in zip(parts, sizes)])
                    for j in (0, 1)] + [torch.cat([y for _, _, y in parts])]
            res[str(sizes)] = (torch.equal(pooled, want[0]) and torch.equal(out, want[1]) and torch.equal(ys, want[2])
                               and ys.dtype == torch.int64 and pooled.is_contiguous() and out.is_contiguous())
        res["one_collective_each"] = len(calls) == len(cases)
    except Exception as e:
        res["error"] = repr(e)
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
    q.put(res)


@pytest.mark.parametrize("world,cases", [(2, [[3, 2], [2, 1], [2, 2]]), (3, [[3, 3, 1], [1, 1, 1]])])
def test_packed_exchange_rows_and_label_lane(world, cases):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_exchange_worker, args=(r, world, port, cases, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(world):
            r = q.get(timeout=180)
            res[r["rank"]] = r
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    assert sorted(res) == list(range(world)), res
    for r in res.values():
        assert "error" not in r, r
        assert all(r[str(s)] for s in cases) and r["one_collective_each"], r


def test_exchange_world1_is_the_identity():
    pooled, out, ys = _rank_rows([3], 0)
    got = DT.exchange_rows(pooled, out, ys, [3])
    assert torch.equal(got[0], pooled) and torch.equal(got[1], out) and torch.equal(got[2], ys)


def test_mask_slicing_is_the_global_masks_rows():
    batch = 7
    g = torch.Generator().manual_seed(3)
    masks = {1: torch.rand(2 * batch, generator=g) > 0.3, 4: torch.rand(2 * batch, generator=g) > 0.6}
    sizes = [3, 3, 1]
    for rank, rows in enumerate(sizes):
        start = sum(sizes[:rank])
        got = DT.shard_masks(masks, start, rows, batch)
        assert sorted(got) == [1, 4]
        for bid, mk in masks.items():
            assert torch.equal(got[bid][:rows], mk[start:start + rows])
            assert torch.equal(got[bid][rows:], mk[batch + start:batch + start + rows])
    # all ranks' rows, view by view, are the global mask again
    for bid, mk in masks.items():
        parts = [DT.shard_masks(masks, sum(sizes[:r]), s, batch)[bid] for r, s in enumerate(sizes)]
        assert torch.equal(torch.cat([p[:s] for p, s in zip(parts, sizes)] + [p[s:] for p, s in zip(parts, sizes)]), mk)


def _mid_net(name="train_joint_mid_addon"):
    import train_trace_cases as C
    meta, _, fwd_meta = C.load_train_golden(name)
    net = C.build_model(fwd_meta).train()
    return meta, fwd_meta, net


def test_same_seed_same_masks_and_gumbel_seeds():
    _, _, net = _mid_net()
    a, b, c = DT.ShardedTraining(net, seed=11), DT.ShardedTraining(net, seed=11), DT.ShardedTraining(net, seed=12)
    assert a.module is net and a.world == 1 and a.rank == 0
    drawn = []
    for st in (a, b, c):
        m1, s1, m2, s2 = st.draw_masks(5), st.draw_seed(), st.draw_masks(5), st.draw_seed()
        assert m1 and all(v.shape == (10,) and v.dtype == torch.bool for v in m1.values())
        drawn.append((m1, s1, m2, s2))
    (am1, as1, am2, as2), (bm1, bs1, bm2, bs2), (cm1, cs1, _, _) = drawn
    assert as1 == bs1 and as2 == bs2 and as1 != as2 and 0 <= as1 < 2 ** 62
    assert sorted(am1) == sorted(bm1) and all(torch.equal(am1[k], bm1[k]) and torch.equal(am2[k], bm2[k]) for k in am1)
    assert cs1 != as1 or any(not torch.equal(cm1[k], am1[k]) for k in am1)


def test_arena_table():
    import train_trace_cases as C
    meta, fwd_meta, net = _mid_net()
    opt_net, opt_cls, _, _ = C._optimizers_like_reference(net, meta, fwd_meta)
    params = DT.arena_params(net, "train", opt_cls, opt_net)
    trainable = [p for p in net.parameters() if p.requires_grad]
    assert len(params) == len(trainable) > 10 and {id(p) for p in params} == {id(p) for p in trainable}
    in_order = [p for o in (opt_cls, opt_net) for g in o.param_groups for p in g["params"] if p.requires_grad]
    assert all(a is b for a, b in zip(params, in_order)) and len(params) == len(in_order)
    # pretrain rests the classifier optimizer, finetune the backbone's: their parameters go behind the others
    pre = DT.arena_params(net, "pretrain", opt_cls, opt_net)
    assert pre[0] is [p for g in opt_net.param_groups for p in g["params"] if p.requires_grad][0]
    assert {id(p) for p in pre} == {id(p) for p in trainable}
    for p in params:
        p.grad = torch.zeros_like(p)
    arena = DT.GradArena(params)
    rows = arena.table_rows()
    assert [r[0] for r in rows] == [p.grad.data_ptr() for p in params]
    assert [r[2] for r in rows] == [p.numel() for p in params]
    assert all(r[1] % 4 == 0 for r in rows) and arena.buffer.data_ptr() % 16 == 0           # 16-byte slots
    assert all(rows[i + 1][1] == rows[i][1] + (rows[i][2] + 3) // 4 * 4 for i in range(len(rows) - 1))
    assert arena.numel == rows[-1][1] + (rows[-1][2] + 3) // 4 * 4 == arena.buffer.numel()
    assert any(r[2] % 4 for r in rows) or DT.arena_layout([1, 3, 4, 5]) == ([0, 4, 8, 12], 20)
    arena.scatter()
    assert all(p.grad.shape == p.shape and p.grad.data_ptr() == arena.buffer.data_ptr() + 4 * r[1]
               for p, r in zip(params, rows))
    params[3].grad = None
    with pytest.raises(RuntimeError):
        arena.table_rows()


class _GroupStub:
    """A process group that knows its size and rank and nothing else."""

    def __init__(self, world, rank):
        self._world, self._rank = world, rank

    def size(self):
        return self._world

    def rank(self):
        return self._rank

    def __getattr__(self, name):
        raise AssertionError(f"process group touched: {name}")


@pytest.fixture
def no_collectives(monkeypatch):
    def refuse(name):
        def f(*a, **k):
            raise AssertionError(f"torch.distributed.{name} called before the refusal")
        return f
    for name in ("all_reduce", "all_gather", "all_gather_into_tensor", "broadcast", "gather", "barrier", "get_rank",
                 "get_world_size", "get_global_rank", "reduce_scatter", "all_to_all"):
        monkeypatch.setattr(dist, name, refuse(name))


def test_refusals_come_before_any_collective(no_collectives):
    from count_pipnet_amd import train as T
    from golden_util import load_golden
    from model_util import build_model
    _, _, net = _mid_net()
    st = DT.ShardedTraining(net, _GroupStub(2, 1), seed=5)
    assert (st.world, st.rank) == (2, 1)
    xs, ys = torch.zeros(2, 3, 64, 64), torch.zeros(2, dtype=torch.int64)
    empty = torch.zeros(0, 3, 64, 64)
    with pytest.raises(ValueError):                        # sizes name three ranks in a world of two
        st.step(xs, xs, ys, None, None, phase="train", sizes=[2, 2, 2])
    with pytest.raises(ValueError):                        # a rank with zero rows
        st.step(xs, xs, ys, None, None, phase="train", sizes=[0, 2])
    with pytest.raises(ValueError):
        st.step(empty, empty, ys[:0], None, None, phase="train")
    with pytest.raises(ValueError):                        # sizes disagree with the rows this rank holds
        st.step(xs, xs, ys, None, None, phase="train", sizes=[2, 3])
    # no HIP step for this setup (here: parameters on the CPU): train.train_pipnet's own refusal text
    for phase, finetune in (("train", False), ("pretrain", False), ("finetune", True)):
        with pytest.raises(NotImplementedError) as e:
            st.step(xs, xs, ys, None, None, phase=phase)
        assert str(e.value) == T._STEPS[False, finetune][2]
    meta, _ = load_golden("pipnet_resnet50_small")
    resnet = DT.ShardedTraining(build_model(meta).train(), _GroupStub(2, 0), seed=5)
    with pytest.raises(NotImplementedError, match="BatchNorm") as e:
        resnet.step(xs, xs, ys, None, None, phase="train")
    assert "per-replica" in str(e.value) and "later change" in str(e.value)
    # world 1: a ResNet is not refused for being one (its setup still is, on the CPU)
    with pytest.raises(NotImplementedError) as e:
        DT.ShardedTraining(resnet.module, seed=5).step(xs, xs, ys, None, None, phase="train")
    assert "BatchNorm" not in str(e.value)
