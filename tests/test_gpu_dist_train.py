"""Data-parallel HIP training (count_pipnet_amd.dist_train) on the 1-GPU box.

Kernels, in process:
  1. pipnet_head_bwd_rows_f32 / pipnet_count_head_bwd_rows_f32: every contiguous split of a batch's rows into 1, 2
     and 3 shards gives, shard by shard, the BITS of the full-batch entry point's rows (same arithmetic, same order);
  2. pipnet_pack_tensors_f32 against ``copy_`` into the slots: vector and scalar paths, zeroed padding, nothing
     written behind the arena;
  3. the Gumbel head on a row range with its Philox offset against those rows of the full-batch launch;
  4. world 1: ``ShardedTraining.step`` is the plain step, bit for bit (stats, every .grad, parameters after 2 steps),
     also with the exchange path forced (``force_exchange``: one shard that is the whole batch).

Multi-rank, as tests/test_gpu_dist.py: torch.multiprocessing spawn, gloo, every rank on cuda:0 (RCCL refuses two
ranks on one device), ONE spawn per world size running every scenario of that world:
  5. worlds 2 and 3: gradients of a step against the single-device step on the concatenated batch (below);
  6. world 2: parameters and AdamW moments stay bit-identical across ranks over 3 joint and 2 finetune steps, and
     equal a fresh copy stepped with the rank's reduced gradients; the sparsity clamps; pretrain leaves the classifier;
  7. world 2: ``dist_train.train_pipnet`` over two batches against ``train.train_pipnet`` on the concatenated ones;
  8. world 2: a ResNet-50 PIP-Net is refused on every rank and the run ends.

The gradient gate (test 5).  Per trainable tensor r = max|g_dp - g_1| / max|g_1|, g_1 the single-device
``hip_*_step`` on the concatenated batch with the same masks and noise.  Measured on an MI355X, worst r per scenario
(fixture, global rows per view, shards):

    fixture                    rows  shards   worst r
    train_joint_mid_addon         4  2+2      7.83e-07
    train_joint_mid_addon         3  2+1      8.10e-07
    train_joint_mid_addon         3  1+1+1    8.37e-07
    train_pretrain_mid_addon      4  2+2      9.25e-07    <- the worst of all
    train_pretrain_mid_addon      3  2+1      7.29e-07
    train_pretrain_mid_addon      3  1+1+1    9.14e-07
    train_count_joint_onehot      4  2+2      8.60e-07
    train_count_joint_onehot      3  2+1      6.38e-07
    train_count_joint_onehot      3  1+1+1    6.97e-07

The bound is the smallest power of two that is at least twice the worst ratio, capped at 2^-13 (the rtol = 1e-4 the
suite grants "a float32 forward of the whole net"): 2 * 9.25e-07 = 1.85e-06 <= 2^-19 = 1.91e-06 = BOUND.
``stats[4]`` (correct count) is exactly equal, the other stats within 1e-6 relative.

The inputs are decisive, since a shard's GEMMs run at another M than the full batch's and may sum in another order:
for a PIP-Net the top-two pixel gap of every (row, prototype) softmax map is >= 1e-4 (a max-pool argmax cannot flip);
for the CountPIPNet every raw count is >= 1e-3 away from a rounding boundary (x.5) and from the clamp ends (0,
max_count).  The image seeds in SEEDS were chosen with the CPU torch path (``backend.torch_backend()``) so that these
hold with a factor of two to spare; they are asserted again on the device, and a violated one fails the test.

World 1 (test 4) needs a plain step that repeats its own bits.  The CountPIPNet one did not while the soft Gumbel
head added its workgroups' partial sums into the raw counts with float atomics (four workgroups per image on these
fixtures; tests/golden/train_call_trace.json records no digest for ``train_count_joint_onehot`` for that reason): two
runs came out 7.6e-08 .. 3.3e-07 apart in 30 gradient tensors.  The head now adds the partial sums in workgroup order
(``test_soft_gumbel_sums_repeat_their_bits``).

Gumbel sharding at "an h*w*P that is no multiple of 4": every head kernel requires P % 4 == 0, so no such launch
exists; test 3 asserts the refusal instead.
"""
import functools
import itertools
import os
import socket
import time
import traceback

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
BOUND = 2.0 ** -19
# (fixture, global rows per view) -> seed of the synthetic images / labels / masks / noise (see the docstring)
SEEDS = {("train_joint_mid_addon", 4): 1000, ("train_joint_mid_addon", 3): 1010,         # CPU margins 3.0, 6.2
         ("train_pretrain_mid_addon", 4): 1000, ("train_pretrain_mid_addon", 3): 1010,   # 3.0, 6.2
         ("train_count_joint_onehot", 4): 1000, ("train_count_joint_onehot", 3): 1000}   # 2.9, 2.5
# a world's whole spawn measured 6.5 s (world 3) and 7.9 s (world 2) on an MI355X; the limit leaves room for the
# ranks' first import of torch on a cold machine
SPAWN_TIMEOUT_S = 120


# ------------------------------------------------------------------------------------------
# 1. rows kernels
# ------------------------------------------------------------------------------------------
def _splits(n, parts):
    """Every way to cut range(n) into ``parts`` contiguous non-empty pieces: lists of (start, rows)."""
    out = []
    for cuts in itertools.combinations(range(1, n), parts - 1):
        edges = (0,) + cuts + (n,)
        out.append([(a, b - a) for a, b in zip(edges[:-1], edges[1:])])
    return out


@pytest.mark.parametrize("p", [4, 16, 768, 2048])
@pytest.mark.parametrize("head", ["pipnet", "count"])
def test_rows_kernels_give_the_full_batch_bits(gpu, head, p):
    from count_pipnet_amd import kernels as K
    from count_pipnet_amd.dist_train import shard_rows
    k, shards_checked = 7, 0
    g = torch.Generator().manual_seed(1000 + p)
    w = torch.randn(k, p, generator=g).to(gpu)
    for hw, bh_all in itertools.product([1, 36, 64], [1, 3, 5]):
        n = 2 * bh_all
        proto = torch.softmax(3.0 * torch.randn(n, hw, 1, p, generator=g), dim=3).to(gpu).contiguous()
        rows_all = (proto.amax(dim=(1, 2)) if head == "pipnet" else proto.sum(dim=(1, 2))).contiguous()
        grad_all = (torch.randn(n, k if head == "pipnet" else p, generator=g) * 0.1).to(gpu)
        for with_grad, (w_align, w_tanh) in itertools.product([True, False], [(5.0, 2.0), (0.5, 5.0), (5.0, 0.0)]):
            gr = grad_all if with_grad else None

            def run(proto_r, rows_r, gr_r, all_rows):
                if head == "pipnet":
                    return K.head_backward(proto_r, rows_r, gr_r, w if gr_r is not None else None, w_align, w_tanh, 1.0,
                                           pooled_all=all_rows)
                return K.count_head_backward(proto_r, rows_r, gr_r, w_align, w_tanh, 0.7, 0.5, counts_all=all_rows)

            full = run(proto, rows_all, gr, None)                       # the existing full-batch entry point
            for parts in (1, 2, 3):
                for split in _splits(bh_all, parts):
                    for start, rows in split:
                        got = run(shard_rows(proto, start, rows, bh_all), shard_rows(rows_all, start, rows, bh_all),
                                  None if gr is None else shard_rows(gr, start, rows, bh_all), rows_all)
                        want = shard_rows(full, start, rows, bh_all)
                        assert torch.equal(got, want), (head, p, hw, bh_all, with_grad, w_align, w_tanh, start, rows)
                        shards_checked += 1
    assert shards_checked == 3 * 6 * (1 + (1 + 2 * 2 + 3) + (1 + 2 * 4 + 3 * 6))


def test_rows_kernels_refuse_bad_operands(gpu):
    from count_pipnet_amd import kernels as K
    proto = torch.softmax(torch.randn(4, 3, 3, 8), dim=3).to(gpu)
    pooled = proto.amax(dim=(1, 2)).contiguous()
    with pytest.raises(RuntimeError):                       # fewer gathered rows than the shard holds
        K.head_backward(proto, pooled, None, None, 5.0, 2.0, pooled_all=pooled[:2].contiguous())
    with pytest.raises(RuntimeError):                       # another prototype width
        K.count_head_backward(proto, pooled, None, 5.0, 2.0, 1.0, 1.0, counts_all=torch.zeros(4, 12, device=gpu))
    with pytest.raises(RuntimeError):
        K.head_backward(proto, pooled, None, None, 5.0, 2.0, pooled_all=pooled.cpu())


# ------------------------------------------------------------------------------------------
# 2. pack kernel
# ------------------------------------------------------------------------------------------
COUNTS = [1, 3, 4, 5, 4097, 2 ** 20 + 3]
SENTINEL = 12345.0


def _pack_case(gpu, counts, lead):
    """Sources of ``counts`` elements that start ``lead[i]`` floats behind a 16-byte boundary; returns
    (arena after the launch incl. a guard behind its end, the same filled by copy_)."""
    from count_pipnet_amd import kernels as K
    from count_pipnet_amd.dist_train import arena_layout
    offsets, total = arena_layout(counts)
    g = torch.Generator().manual_seed(len(counts) * 31 + sum(lead))
    srcs = []
    for n, ld in zip(counts, lead):
        base = torch.randn(n + 8, generator=g).to(gpu)
        assert base.data_ptr() % 16 == 0
        srcs.append(base[ld:ld + n])
        assert srcs[-1].data_ptr() % 16 == 4 * ld
    guard = 64
    buf = torch.full((total + guard,), SENTINEL, device=gpu)
    want = buf.clone()
    want[:total] = 0.0
    for s, off, n in zip(srcs, offsets, counts):
        want[off:off + n].copy_(s)
    rows = [[s.data_ptr(), off, n] for s, off, n in zip(srcs, offsets, counts)]
    table = torch.tensor(rows, dtype=torch.int64).to(gpu)
    K.pack_tensors(table, buf[:total])
    return buf, want, total


def test_pack_single_tensors(gpu):
    for n, lead in itertools.product(COUNTS, [0, 1, 2, 3]):
        buf, want, total = _pack_case(gpu, [n], [lead])
        assert total == (n + 3) // 4 * 4
        assert torch.equal(buf, want), (n, lead)
        assert bool((buf[total:] == SENTINEL).all()) and bool((buf[n:total] == 0).all())


def test_pack_two_hundred_tensors(gpu):
    counts = [COUNTS[i % 5] for i in range(200)]
    counts[17] = counts[150] = COUNTS[5]
    lead = [(i // 5) % 4 for i in range(200)]
    assert {(c, l) for c, l in zip(counts, lead)} >= set(itertools.product(COUNTS[:5], range(4)))
    buf, want, total = _pack_case(gpu, counts, lead)
    assert torch.equal(buf, want)
    assert bool((buf[total:] == SENTINEL).all())


def test_pack_refuses_bad_operands(gpu):
    from count_pipnet_amd import kernels as K
    arena = torch.zeros(16, device=gpu)
    with pytest.raises(RuntimeError):
        K.pack_tensors(torch.zeros(2, 3, dtype=torch.int64), arena)                  # table on the host
    with pytest.raises(RuntimeError):
        K.pack_tensors(torch.zeros(2, 2, dtype=torch.int64, device=gpu), arena)      # not [n, 3]
    with pytest.raises(RuntimeError):
        K.pack_tensors(torch.zeros(1, 3, dtype=torch.int64, device=gpu), arena[1:])   # arena off 16 bytes


# ------------------------------------------------------------------------------------------
# 3. Gumbel sharding
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,p", [(3, 3, 16), (8, 8, 32), (5, 7, 4)])
def test_gumbel_row_range_with_offset(gpu, h, w, p):
    from count_pipnet_amd import kernels as K
    b, seed, tau = 5, 0x1234567, 0.8
    logits = torch.randn(b, h, w, p, generator=torch.Generator().manual_seed(h * w * p)).to(gpu)
    per = h * w * p
    assert per % 4 == 0
    proto, sums = K.count_gumbel_soft(logits, tau, None, seed)
    for g0, rows in [(0, 5), (0, 2), (2, 3), (1, 1), (4, 1), (3, 2)]:
        pr, sr = K.count_gumbel_soft(logits[g0:g0 + rows], tau, None, seed, offset=g0 * per // 4)
        assert torch.equal(pr, proto[g0:g0 + rows]), (g0, rows)
        assert torch.equal(sr, sums[g0:g0 + rows]), (g0, rows)   # an image's workgroups are added in their order
    # a row launched at another row's offset draws other noise
    assert not torch.equal(K.count_gumbel_soft(logits[1:2], tau, None, seed, offset=0)[0], proto[1:2])


@pytest.mark.parametrize("b,h,w,p", [(6, 8, 8, 16), (4, 12, 12, 16), (3, 28, 28, 768), (2, 5, 7, 2048), (5, 4, 4, 32)])
def test_soft_gumbel_sums_repeat_their_bits(gpu, b, h, w, p):
    """The raw counts of the soft head: the same bits from launch to launch (1 .. 49 workgroups per image, on
    Philox and on injected noise), and the spatial sums of the map to float32 rounding of <= h*w positive terms."""
    from count_pipnet_amd import kernels as K
    from count_pipnet_amd.synthetic import synth_exponential
    logits = (3 * torch.randn(b, h, w, p, generator=torch.Generator().manual_seed(b + h * w + p))).to(gpu)
    for noise in (None, synth_exponential((b, p, h, w), 11).to(gpu)):
        proto, sums = K.count_gumbel_soft(logits, 0.7, noise, 99)
        for _ in range(4):
            again = K.count_gumbel_soft(logits, 0.7, noise, 99)
            assert torch.equal(again[1], sums) and torch.equal(again[0], proto)
        want = proto.double().sum(dim=(1, 2))
        # h*w - 1 float32 additions of positive terms and the map's own rounding: h*w units of 2^-24, to first order
        assert torch.allclose(sums.double(), want, rtol=(h * w + 1) * 2.0 ** -24, atol=0)


def test_gumbel_width_is_a_multiple_of_4(gpu):
    """h*w*P % 4 != 0 needs P % 4 != 0, which the head refuses: there is no per-row launch to shard."""
    from count_pipnet_amd import kernels as K
    with pytest.raises(RuntimeError):
        K.count_gumbel_soft(torch.randn(2, 3, 3, 6).to(gpu), 1.0, None, 1)


# ------------------------------------------------------------------------------------------
# fixtures' networks and steps
# ------------------------------------------------------------------------------------------
class _Case:
    """A train_* fixture's network with the reference run's optimizers (tests/train_trace_cases.py)."""

    def __init__(self, name, dev):
        import train_trace_cases as C
        self.name, self.dev = name, dev
        self.count, self.finetune = name.startswith("train_count_"), "_finetune_" in name
        if self.finetune:
            meta, rec, fwd, net, opt, _, batches = (C._count_setup if self.count else C._finetune_setup)(name, dev)
            self.opt_net, self.opt_cls, pretrain = None, opt, False
        elif self.count:
            meta, rec, fwd, net, self.opt_net, self.opt_cls, _, _, pretrain, batches = C._count_suffix_setup(name, dev)
        else:
            meta, rec, fwd = C.load_train_golden(name)
            net = C.build_model(fwd).to(dev).train()
            self.opt_net, self.opt_cls, _, _ = C._optimizers_like_reference(net, meta, fwd)
            pretrain = meta["phase"] == "pretrain"
            c = fwd["case"]
            batches = C.train_loader_batches(c["size"], c["num_classes"], meta["iterations"], meta["batch_per_view"],
                                             meta["seed"])
        self.meta, self.rec, self.fwd, self.net, self.batches = meta, rec, fwd, net, batches
        self.phase = "finetune" if self.finetune else "pretrain" if pretrain else "train"
        self.nr_epochs = 2 if pretrain else 1
        self.opts = [o for o in (self.opt_net, self.opt_cls) if o is not None]

    def zero_grad(self):
        for o in self.opts:
            o.zero_grad(set_to_none=True)
        for p in self.net.parameters():
            p.grad = None

    def plain_step(self, xs1, xs2, ys, sd_keep, step_optimizers=True):
        """The parent's single-device step: the public ``hip_*_step`` of the fixture's phase."""
        from count_pipnet_amd import train as T
        if self.finetune:
            assert step_optimizers
            fn = T.hip_count_finetune_step if self.count else T.hip_finetune_step
            return fn(self.net, xs1, xs2, ys, self.opt_cls, True, sd_keep=sd_keep)
        fn = T.hip_count_train_step if self.count else T.hip_train_step
        return fn(self.net, xs1, xs2, ys, self.opt_net, self.opt_cls, self.phase == "pretrain", 1, self.nr_epochs, True,
                  sd_keep=sd_keep, step_optimizers=step_optimizers)

    def sharded_step(self, st, xs1, xs2, ys, sd_keep, **kw):
        return st.step(xs1, xs2, ys, self.opt_net, self.opt_cls, phase=self.phase, epoch=1, nr_epochs=self.nr_epochs,
                       sd_keep=sd_keep, **kw)

    def grads(self):
        return {n: p.grad.detach().clone() for n, p in self.net.named_parameters() if p.grad is not None}


def _same_tensors(a, b):
    return sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)


# ------------------------------------------------------------------------------------------
# 4. world 1
# ------------------------------------------------------------------------------------------
WORLD1 = ["train_joint_mid_addon", "train_pretrain_mid_addon", "train_finetune_mid_addon", "train_count_joint_onehot",
          "train_count_finetune_bilinear"]


@pytest.mark.parametrize("name,force_exchange", [(n, f) for f in (False, True) for n in WORLD1],
                         ids=[n + f for f in ("", "-forced") for n in WORLD1])
def test_world1_is_the_plain_step_bitwise(gpu, name, force_exchange):
    """``force_exchange``: the exchange path on one shard that is the whole batch -- the rows kernels give the
    full-batch bits, ``exchange_rows`` and the arena pack are copies, the GEMMs run at the same M."""
    import train_trace_cases as C
    from count_pipnet_amd.dist_train import ShardedTraining
    plain, dp = _Case(name, gpu), _Case(name, gpu)
    st = ShardedTraining(dp.net, seed=3, force_exchange=force_exchange)
    assert st.world == 1 and st.rank == 0 and st.module is dp.net
    for i in range(2):
        xs1, xs2, ys = (t.to(gpu) for t in plain.batches[i])
        stats = []
        for case in (plain, dp):
            sd_keep = C._sd_keep(case.net, case.rec[f"s{i}_masks"])
            if case.count:
                C._inject_noise(case.net, case.meta, case.rec, i, gpu)
            case.zero_grad()
            stats.append(case.plain_step(xs1, xs2, ys, sd_keep) if case is plain
                         else case.sharded_step(st, xs1, xs2, ys, sd_keep))
        torch.cuda.synchronize()
        g0, g1 = plain.grads(), dp.grads()
        differ = {n: float((g0[n] - g1[n]).abs().max() / g0[n].abs().max()) for n in g0
                  if n in g1 and not torch.equal(g0[n], g1[n])}
        print(f"{name} step {i}: stats {stats[0].tolist()} / {stats[1].tolist()}; tensors that differ "
              f"(max|d| / max|g|): {differ}")
        assert torch.equal(stats[0], stats[1]), (i, stats)
        assert len(g0) >= 2 and _same_tensors(g0, g1), (i, differ)
    assert _same_tensors(dict(plain.net.named_parameters()), dict(dp.net.named_parameters()))
    assert (st._arena is not None) == force_exchange          # no arena, no collective at world 1 unless forced


# ------------------------------------------------------------------------------------------
# multi-rank scenarios (run inside the ranks; each returns a dict of plain Python values)
# ------------------------------------------------------------------------------------------
GRAD_FIXTURES = ["train_joint_mid_addon", "train_pretrain_mid_addon", "train_count_joint_onehot"]
GRAD_SHARDS = {2: [(4, [2, 2]), (3, [2, 1])], 3: [(3, [1, 1, 1])]}


def _grad_inputs(case, batch):
    """Global batch of ``batch`` rows per view for a gradient scenario: images, labels, global masks, Gumbel noise."""
    from count_pipnet_amd import train as T
    from count_pipnet_amd.synthetic import synth_exponential, synth_images
    seed = SEEDS[case.name, batch]
    c = case.fwd["case"]
    xs1, xs2 = synth_images(batch, c["size"], seed=seed), synth_images(batch, c["size"], seed=seed + 1)
    ys = torch.randint(0, c["num_classes"], (batch,), generator=torch.Generator().manual_seed(seed))
    masks = T._sd_masks(case.net, 2 * batch, torch.Generator().manual_seed(seed + 2))
    noise = None
    if case.count:
        noise = synth_exponential((2 * batch,) + tuple(case.rec["s0_proto"].shape[1:]), seed + 3)
    return xs1, xs2, ys, masks, noise


def _decisive_margin(case, proto_nchw, pooled):
    """How far the forward is from a discrete flip, in units of the issue's thresholds (>= 1 passes): PIP-Net:
    min top-two pixel gap of the (row, prototype) softmax maps / 1e-4; CountPIPNet: min distance of a raw count
    from x.5, 0 and max_count / 1e-3."""
    if not case.count:
        top = proto_nchw.flatten(2).topk(2, dim=2).values
        return float((top[..., 0] - top[..., 1]).min()) / 1e-4
    mc = float(case.net._max_count)
    frac = (pooled - torch.floor(pooled) - 0.5).abs().min()
    return float(torch.minimum(frac, torch.minimum(pooled.abs().min(), (pooled - mc).abs().min()))) / 1e-3


def _device_margin(case, xs, masks):
    from count_pipnet_amd import train as T
    with torch.no_grad():
        if case.count:
            proto, counts, _, _, _, _ = T._count_train_forward(case.net, xs, masks)
            return _decisive_margin(case, proto.permute(0, 3, 1, 2), counts)
        proto, pooled, _ = T.train_forward_hip(case.net, xs, masks)
        return _decisive_margin(case, proto.permute(0, 3, 1, 2), pooled)


def _set_noise(case, noise):
    if noise is not None:
        list(case.net._add_on)[-1].exp_noise = noise.to(case.dev)


def _scenario_gradients(rank, world, dev):
    from count_pipnet_amd.dist_train import ShardedTraining
    out = {}
    for name in GRAD_FIXTURES:
        ref, dp = _Case(name, dev), _Case(name, dev)
        st = ShardedTraining(dp.net, seed=9)
        for batch, sizes in GRAD_SHARDS[world]:
            xs1, xs2, ys, masks, noise = _grad_inputs(ref, batch)
            xs1, xs2, ys = xs1.to(dev), xs2.to(dev), ys.to(dev)
            _set_noise(ref, noise)
            _set_noise(dp, noise)
            margin = _device_margin(ref, torch.cat([xs1, xs2]), masks)
            ref.zero_grad()
            s1 = ref.plain_step(xs1, xs2, ys, masks, step_optimizers=False)
            start, rows = sum(sizes[:rank]), sizes[rank]
            dp.zero_grad()
            sd = dp.sharded_step(st, xs1[start:start + rows].contiguous(), xs2[start:start + rows].contiguous(),
                                 ys[start:start + rows].contiguous(), masks, sizes=sizes, step_optimizers=False)
            torch.cuda.synchronize()
            g1, gd = ref.grads(), dp.grads()
            ratios = {}
            for n, g in g1.items():
                scale = float(g.abs().max())
                diff = float((gd[n] - g).abs().max())
                ratios[n] = diff / scale if scale > 0 else (0.0 if diff == 0 else float("inf"))
            out[f"{name}/{batch}/{'+'.join(map(str, sizes))}"] = dict(
                margin=margin, same_names=sorted(g1) == sorted(gd), ratios=ratios, stats_1=s1.cpu().tolist(),
                stats_dp=sd.cpu().tolist(), tensors=len(g1))
    return out


def _flat_state(case):
    """Every parameter and both AdamW moments of every stepped parameter, as one vector."""
    parts = [p.detach().flatten() for p in case.net.parameters()]
    for o in case.opts:
        for g in o.param_groups:
            for p in g["params"]:
                st = o.state.get(p, {})
                if "exp_avg" in st:
                    parts += [st["exp_avg"].flatten(), st["exp_avg_sq"].flatten(),
                              st["step"].to(p.device, torch.float32).flatten()]
    return torch.cat(parts)


def _scenario_optimizers(rank, world, dev):
    import torch.distributed as dist
    from count_pipnet_amd import train as T
    from count_pipnet_amd.dist_train import ShardedTraining
    out = {}
    for name, steps in [("train_joint_mid_addon", 3), ("train_finetune_mid_addon", 2), ("train_pretrain_mid_addon", 1)]:
        dp, twin = _Case(name, dev), _Case(name, dev)
        st = ShardedTraining(dp.net, seed=21)
        cls = dp.net._classification
        cls_before = cls.weight.detach().clone()
        res = dict(across_ranks=[], twin=[], clamps=[], moments=0)
        for i in range(steps):
            batch = 4
            from count_pipnet_amd.synthetic import synth_images
            c = dp.fwd["case"]
            xs1 = synth_images(batch, c["size"], seed=500 + 2 * i).to(dev)
            xs2 = synth_images(batch, c["size"], seed=501 + 2 * i).to(dev)
            ys = torch.randint(0, c["num_classes"], (batch,), generator=torch.Generator().manual_seed(500 + i)).to(dev)
            start, rows = 2 * rank, 2
            dp.zero_grad()
            dp.sharded_step(st, xs1[start:start + rows].contiguous(), xs2[start:start + rows].contiguous(),
                            ys[start:start + rows].contiguous(), None)          # masks from the shared generator
            flat = _flat_state(dp)
            every = [torch.empty_like(flat) for _ in range(world)]
            dist.all_gather(every, flat)
            res["across_ranks"].append(all(torch.equal(every[0], e) for e in every[1:]))
            res["moments"] = int(flat.numel()) - sum(p.numel() for p in dp.net.parameters())
            # a fresh copy, stepped with this rank's reduced gradients by the device AdamW and the clamps
            twin.zero_grad()
            named = dict(dp.net.named_parameters())
            for n, p in twin.net.named_parameters():
                if named[n].grad is not None:
                    p.grad = named[n].grad.detach().clone()
            T._step_optimizers(twin.net, None if dp.phase == "pretrain" else twin.opt_cls,
                               None if dp.phase == "finetune" else twin.opt_net, True)
            res["twin"].append(_same_tensors(named, dict(twin.net.named_parameters()))
                               and torch.equal(_flat_state(dp), _flat_state(twin)))
            res["clamps"].append(float(cls.weight.min()) >= 0.0 and float(cls.normalization_multiplier.min()) >= 1.0)
        res["classifier_moved"] = not torch.equal(cls.weight.detach(), cls_before)
        out[name] = res
    return out


def _epoch_setup(dev):
    case = _Case("train_joint_mid_addon", dev)
    sched_net = torch.optim.lr_scheduler.CosineAnnealingLR(case.opt_net, T_max=10, eta_min=5e-6)
    sched_cls = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(case.opt_cls, T_0=10, eta_min=0.001, T_mult=1)
    return case, sched_net, sched_cls


def _scenario_epoch(rank, world, dev):
    from count_pipnet_amd import dist_train as DT
    from count_pipnet_amd import train as T
    from count_pipnet_amd.synthetic import synth_images
    batches = []
    for i in range(2):
        g = torch.Generator().manual_seed(700 + i)
        batches.append((synth_images(4, 64, seed=700 + 2 * i), synth_images(4, 64, seed=701 + 2 * i),
                        torch.randint(0, 9, (4,), generator=g)))
    one, s_net, s_cls = _epoch_setup(dev)
    assert one.fwd["case"]["size"] == 64 and one.fwd["case"]["num_classes"] >= 9
    info_1 = T.train_pipnet(one.net, batches, one.opt_net, one.opt_cls, s_net, s_cls, None, 1, 1, dev,
                            generator=torch.Generator().manual_seed(77))
    dp, s_net, s_cls = _epoch_setup(dev)
    own = [tuple(t[2 * rank:2 * rank + 2].contiguous() for t in b) for b in batches]
    info_dp = DT.train_pipnet(dp.net, own, dp.opt_net, dp.opt_cls, s_net, s_cls, None, 1, 1, dev,
                              generator=torch.Generator().manual_seed(77))
    return dict(info_1=info_1, info_dp=info_dp)


def _scenario_resnet_refused(rank, world, dev):
    from count_pipnet_amd.dist_train import ShardedTraining
    case = _Case("train_joint_resnet50", dev)
    st = ShardedTraining(case.net, seed=1)
    xs1, xs2, ys = (t.to(dev) for t in case.batches[0])
    try:
        case.sharded_step(st, xs1[:1], xs2[:1], ys[:1], None)
        return dict(raised=None)
    except NotImplementedError as e:
        return dict(raised=str(e), world=st.world)


SCENARIOS = {2: [("gradients", _scenario_gradients), ("optimizers", _scenario_optimizers), ("epoch", _scenario_epoch),
                 ("resnet", _scenario_resnet_refused)],
             3: [("gradients", _scenario_gradients)]}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, q):
    import sys
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0")
    sys.path.insert(0, TESTS)
    sys.path.insert(0, os.path.dirname(TESTS))
    import torch.distributed as dist
    res = {"rank": rank, "seconds": {}}
    try:
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        for name, fn in SCENARIOS[world]:
            t0 = time.time()
            res[name] = fn(rank, world, dev)
            torch.cuda.synchronize()
            res["seconds"][name] = round(time.time() - t0, 1)
    except Exception:          # reported to the parent, which ends the other ranks and fails the tests with it
        res["error"] = traceback.format_exc()
    finally:
        if dist.is_initialized() and "error" not in res:
            dist.destroy_process_group()
    q.put(res)


@functools.lru_cache(maxsize=None)
def _world(world):
    """Every scenario of ``world`` in one spawn; a rank that fails or a run past the time limit ends the others.
    No second attempt: the result (or the failure) is what every test of this world sees."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    t0 = time.time()
    for p in procs:
        p.start()
    res = {}
    try:
        while len(res) < world:
            left = SPAWN_TIMEOUT_S - (time.time() - t0)
            if left <= 0:
                break
            try:
                r = q.get(timeout=left)
            except Exception:
                break
            res[r["rank"]] = r
            if "error" in r:
                break
    finally:
        for p in procs:
            if len(res) == world and not any("error" in r for r in res.values()):
                p.join(timeout=60)
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
                if p.is_alive():
                    p.kill()
    print(f"world {world}: {time.time() - t0:.1f} s; per scenario {[r.get('seconds') for r in res.values()]}")
    return res


def _ranks(world, gpu):
    res = _world(world)
    errors = {k: r["error"] for k, r in res.items() if "error" in r}
    assert not errors, "\n".join(f"rank {k}:\n{e}" for k, e in errors.items())
    assert sorted(res) == list(range(world)), f"ranks {sorted(res)} of {world} answered within {SPAWN_TIMEOUT_S} s"
    return [res[r] for r in range(world)]


# ---- 5 ----
@pytest.mark.parametrize("world", [2, 3])
def test_gradients_match_the_single_device_step(gpu, world):
    ranks = _ranks(world, gpu)
    keys = [f"{n}/{b}/{'+'.join(map(str, s))}" for n in GRAD_FIXTURES for b, s in GRAD_SHARDS[world]]
    assert sorted(ranks[0]["gradients"]) == sorted(keys)
    worst, failures = {}, []
    for key in keys:
        for rank, r in enumerate(ranks):
            sc = r["gradients"][key]
            w = max(sc["ratios"].items(), key=lambda kv: kv[1])
            worst[key] = max(worst.get(key, 0.0), w[1])
            print(f"world {world} rank {rank} {key}: margin {sc['margin']:.2f}, {sc['tensors']} tensors, "
                  f"worst r = {w[1]:.3e} ({w[0]}), stats_1 {sc['stats_1'][:5]}, stats_dp {sc['stats_dp'][:5]}")
            for n, v in sorted(sc["ratios"].items()):
                print(f"    r[{n}] = {v:.3e}")
            if not sc["margin"] >= 1.0:
                failures.append(f"{key} rank {rank}: inputs not decisive (margin {sc['margin']:.3f} of the threshold)")
            if not sc["same_names"] or sc["tensors"] < 2:
                failures.append(f"{key} rank {rank}: the ranks' gradients cover other tensors than the single device's")
            s1, sd = sc["stats_1"], sc["stats_dp"]
            if sd[4] != s1[4]:
                failures.append(f"{key} rank {rank}: correct count {sd[4]} vs {s1[4]}")
            for j in (0, 1, 2, 3, 5, 6, 7):
                if not abs(sd[j] - s1[j]) <= 1e-6 * abs(s1[j]):
                    failures.append(f"{key} rank {rank}: stats[{j}] {sd[j]!r} vs {s1[j]!r}")
            if sd != ranks[0]["gradients"][key]["stats_dp"]:
                failures.append(f"{key} rank {rank}: stats differ from rank 0's")
            failures += [f"{key} rank {rank}: r[{n}] = {v:.3e} > {BOUND:.3e}" for n, v in sc["ratios"].items()
                         if not v <= BOUND]
    print(f"worst ratios, world {world}: " + ", ".join(f"{k}: {v:.3e}" for k, v in worst.items()))
    assert not failures, "\n".join(failures)


# ---- 6 ----
def test_world2_optimizers_keep_the_ranks_identical(gpu):
    ranks = _ranks(2, gpu)
    for r in ranks:
        for name, steps in [("train_joint_mid_addon", 3), ("train_finetune_mid_addon", 2),
                            ("train_pretrain_mid_addon", 1)]:
            res = r["optimizers"][name]
            assert res["across_ranks"] == [True] * steps, (name, res)
            assert res["twin"] == [True] * steps, (name, res)
            assert res["clamps"] == [True] * steps and res["moments"] > 0, (name, res)
            assert res["classifier_moved"] == (name != "train_pretrain_mid_addon"), (name, res)


# ---- 7 ----
def test_world2_train_pipnet_epoch(gpu):
    ranks = _ranks(2, gpu)
    a, b = ranks[0]["epoch"], ranks[1]["epoch"]
    assert a["info_dp"] == b["info_dp"]                                  # the same values on both ranks
    one, dp = a["info_1"], a["info_dp"]
    assert sorted(one) == sorted(dp) and "train_accuracy" in dp and len(dp["lrs_net"]) == 2
    assert dp["lrs_net"] == one["lrs_net"] and dp["lrs_class"] == one["lrs_class"]
    for k, v in one.items():
        if isinstance(v, float):
            print(f"{k}: single device {v!r}, world 2 {dp[k]!r}")
            assert abs(dp[k] - v) <= BOUND * abs(v), (k, v, dp[k])
    assert one["loss"] > 0


# ---- 8 ----
def test_world2_resnet_is_refused_on_every_rank(gpu):
    for r in _ranks(2, gpu):
        msg = r["resnet"]["raised"]
        assert msg is not None and "BatchNorm" in msg and r["resnet"]["world"] == 2, r["resnet"]
