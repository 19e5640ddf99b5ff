"""Data-parallel HIP training: one process per GPU, each rank trains on its own rows of the batch.

Replaces the reference's ``nn.DataParallel(net, device_ids=...)`` (``main.py:117-118``) for the training loop
(``pipnet/train.py:8-150``), as ``dist.ShardedInference`` does for inference.  A ConvNeXt backbone normalises per
pixel (LayerNorm) and drops per row (stochastic depth), so the only terms that couple the rows of a batch are in
the loss; DataParallel training therefore computes what one device computes on the concatenated batch, and that
is the definition here:

    a step on W ranks, rank r holding ``xs1_r, xs2_r, ys_r``, is ``train._train_step`` on one device with
    ``xs1 = cat_r xs1_r``, ``xs2 = cat_r xs2_r``, ``ys = cat_r ys_r``, the same stochastic-depth masks and the same
    Gumbel noise, up to floating-point summation order -- and every rank ends with bit-identical parameters.

What crosses ranks in one step (world > 1):

  1. before the loss, ONE packed all-gather (``exchange_rows``, on ``dist.all_gather_rows``): per row of the
     rank, ``[pooled 1 | out 1 | pooled 2 | out 2 | label]`` -- both views side by side, the int32 label bit-cast
     into a float lane -- so the rank-order concatenation is the global order of each view, and the split copies
     give ``pooled / out`` as ``[view 1 of all ranks | view 2 of all ranks]``; and one small all-reduce of the
     align term's fp64 partial sums.  Every rank then runs the loss kernel on the global arrays (same ``stats``,
     global ``d_out``) and takes its rows of ``d_out``;
  2. after the backward, ONE all-reduce (sum) over a flat fp32 gradient arena (``GradArena``).  The loss's
     normalisations carry the global counts (``pipnet_head_bwd_rows_f32``), so the sum of the ranks' gradients is
     the global gradient.  Each ``p.grad`` becomes a view of the arena and ``train.hip_adamw_step`` reads it
     there: identical gradients and identical AdamW give identical parameters, with no broadcast.

Randomness comes from one host ``torch.Generator`` that is the same on every rank: the global stochastic-depth
masks (each rank keeps its rows of each view) and, for a CountPIPNet, the step's Philox seed -- global row g of
the ``cat([xs1, xs2])`` stream gets the draw ``kernels.count_gumbel_soft(logits, tau, None, seed)`` gives row g.

Every world runs the one ``train._train_step``: it is handed a ``Shard`` and asks it in the five places where a
rank's rows are not the whole batch -- the masks' rows, the Gumbel draw, the loss on the gathered rows, the gathered
pooled rows of the head backward, the gradient all-reduce.  World 1 (no group, or a group of one) hands it none: the
single-device step itself, no arena, no collective.
A ResNet backbone at world > 1 is refused: see ``_RESNET_REFUSAL``.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist
import torch.nn as nn
from torch import Tensor

from . import kernels as K
from . import train as T
from .dist import all_gather_rows
from .resnet_features import ResNet_features

PHASES = ("pretrain", "train", "finetune")
_RESNET_REFUSAL = ("count_pipnet_amd.dist_train: a ResNet backbone trains with train-mode BatchNorm, which couples "
                   "the rows of a batch: the reference's DataParallel replicas normalise with per-replica batch "
                   "statistics and keep replica 0's running statistics.  That semantic is not implemented for "
                   "world > 1 yet (left for a later change); train a ResNet on one device (train.train_pipnet)")


# ------------------------------------------------------------------------------------------
# rows of the global batch
# ------------------------------------------------------------------------------------------
def shard_rows(x: Tensor, start: int, rows: int, batch: int) -> Tensor:
    """A rank's rows of a global ``cat([view 1, view 2])`` array [2 * batch, ...]: rows
    [start, start + rows) of each view, as ``[view 1 | view 2]``."""
    return torch.cat([x[start:start + rows], x[batch + start:batch + start + rows]])


def shard_masks(masks: Dict[int, Tensor], start: int, rows: int, batch: int) -> Dict[int, Tensor]:
    """The rank's rows of the global stochastic-depth masks (``train._sd_masks`` for 2 * batch rows)."""
    return {bid: shard_rows(mk, start, rows, batch) for bid, mk in masks.items()}


def exchange_rows(pooled: Tensor, out: Tensor, ys: Tensor, sizes: Sequence[int],
                  group=None) -> Tuple[Tensor, Tensor, Tensor]:
    """All-gather a rank's ``pooled`` [2b, P], ``out`` [2b, K] (rows ``[view 1 | view 2]``) and labels ``ys`` [b]
    in ONE collective -> (pooled [2B, P], out [2B, K], ys [B]) of the global batch, the views' rows in rank order.
    Row i of the rank travels as ``[pooled 1 | out 1 | pooled 2 | out 2 | label]``, the label as the bits of an
    int32 in a lane of the rows' dtype; ``dist.all_gather_rows`` pads and compacts uneven shards."""
    b, p, k = ys.shape[0], pooled.shape[1], out.shape[1]
    if pooled.shape[0] != 2 * b or out.shape[0] != 2 * b or pooled.dtype != torch.float32 or out.dtype != torch.float32:
        raise RuntimeError(f"exchange_rows: pooled {tuple(pooled.shape)} / out {tuple(out.shape)} must be float32 "
                           f"rows of both views of {b} labels")
    lane = ys.to(torch.int32).view(torch.float32).unsqueeze(1)
    g = all_gather_rows(torch.cat([pooled[:b], out[:b], pooled[b:], out[b:], lane], dim=1), list(sizes), group)
    w = p + k
    return (torch.cat([g[:, :p], g[:, w:w + p]]), torch.cat([g[:, p:w], g[:, w + p:2 * w]]),
            g[:, 2 * w].contiguous().view(torch.int32).to(torch.int64))


# ------------------------------------------------------------------------------------------
# the gradient arena
# ------------------------------------------------------------------------------------------
def arena_params(m: nn.Module, phase: str, optimizer_classifier, optimizer_net) -> List[Tensor]:
    """Every trainable parameter exactly once, in the order ``train._step_optimizers`` walks them: the groups of
    the classifier optimizer (it rests in pretrain), then the backbone optimizer's (it rests in finetune), then
    whatever trains outside both."""
    opts = [None if phase == "pretrain" else optimizer_classifier, None if phase == "finetune" else optimizer_net]
    params, seen = [], set()
    for src in [p for o in opts if o is not None for g in o.param_groups for p in g["params"]] + list(m.parameters()):
        if src.requires_grad and id(src) not in seen:
            seen.add(id(src))
            params.append(src)
    return params


def arena_layout(counts: Sequence[int]) -> Tuple[List[int], int]:
    """(slot offsets, arena size) in floats: a slot is its tensor's element count rounded up to a multiple of 4,
    so every slot starts on a 16-byte boundary of a 16-byte aligned arena."""
    offsets, total = [], 0
    for n in counts:
        offsets.append(total)
        total += (int(n) + 3) // 4 * 4
    return offsets, total


class GradArena:
    """The flat fp32 buffer one all-reduce covers, for a fixed list of parameters: ``pack()`` gathers their
    ``.grad`` tensors into it in one launch (``kernels.pack_tensors``), ``scatter()`` makes each ``.grad`` a view
    of its slot.  The layout is fixed; the device table is rewritten only when a gradient's address moved."""

    def __init__(self, params: Sequence[Tensor]):
        self.params = list(params)
        self.key = tuple(id(p) for p in self.params)
        self.counts = [p.numel() for p in self.params]
        self.offsets, self.numel = arena_layout(self.counts)
        self.buffer = torch.empty(self.numel, device=self.params[0].device, dtype=torch.float32)
        self._rows: Optional[List[List[int]]] = None
        self._table: Optional[Tensor] = None

    def table_rows(self) -> List[List[int]]:
        """[source address, arena offset, element count] per parameter, from the live ``.grad`` tensors."""
        rows = []
        for p, off, n in zip(self.params, self.offsets, self.counts):
            g = p.grad
            if g is None or g.dtype != torch.float32 or g.device != self.buffer.device or not g.is_contiguous() \
                    or g.numel() != n:
                raise RuntimeError("GradArena: every parameter of the arena needs a contiguous float32 .grad of its "
                                   "own size on the arena's device")
            rows.append([g.data_ptr(), off, n])
        return rows

    def pack(self) -> Tensor:
        rows = self.table_rows()
        if rows != self._rows:         # the caching allocator hands a steady-state step the same blocks again
            self._table = torch.tensor(rows, dtype=torch.int64).pin_memory().to(self.buffer.device, non_blocking=True)
            self._rows = rows
        K.pack_tensors(self._table, self.buffer)
        return self.buffer

    def scatter(self) -> None:
        for p, off, n in zip(self.params, self.offsets, self.counts):
            p.grad = self.buffer[off:off + n].view(p.shape)


# ------------------------------------------------------------------------------------------
# the wrapper
# ------------------------------------------------------------------------------------------
def _group_size_rank(group) -> Tuple[int, int]:
    if group is not None:
        return int(group.size()), int(group.rank())
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(), dist.get_rank()
    return 1, 0


class ShardedTraining(nn.Module):
    """Data-parallel training wrapper (DataParallel semantics, one process per GPU).  Keeps DataParallel's
    ``.module``; ``.world`` / ``.rank`` as ``dist.ShardedInference``.  ``seed``: of the host generator every rank
    shares (masks, Gumbel seeds); None takes rank 0's fresh seed, broadcast once here."""

    def __init__(self, net: nn.Module, process_group=None, seed: Optional[int] = None, force_exchange: bool = False):
        super().__init__()
        self.module = T._inner(net)
        self.process_group = process_group
        # world 1 gets a Shard too, of one shard that is the whole batch -- packed rows, rows kernels, loss on the
        # "gathered" arrays, arena pack, no collective: how one GPU measures and tests the step of world > 1
        self.force_exchange = force_exchange
        self.world, self.rank = _group_size_rank(process_group)
        if seed is None:
            from .count_pipnet import _fresh_seed
            seed = _fresh_seed()
            if self.world > 1:
                dev = next(self.module.parameters()).device
                box = torch.tensor([seed], dtype=torch.int64, device=dev)
                src = dist.get_global_rank(process_group, 0) if process_group is not None else 0
                dist.broadcast(box, src=src, group=process_group)
                seed = int(box.item())
        self.generator = torch.Generator().manual_seed(int(seed))
        self._arena: Optional[GradArena] = None

    def forward(self, *args, **kwargs):
        return self.module(*args, **kwargs)

    # ---- the shared draws: every rank calls these in the same order ----
    def draw_masks(self, batch: int) -> Dict[int, Tensor]:
        """Global stochastic-depth masks for the 2 * ``batch`` rows of ``cat([xs1, xs2])``."""
        return T._sd_masks(self.module, 2 * batch, self.generator)

    def draw_seed(self) -> int:
        """A step's Philox key for the Gumbel head."""
        return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, generator=self.generator).item())

    # ---- refusals: from what every rank knows, before any collective ----
    def check(self, phase: str, rows: int, sizes: Optional[Sequence[int]]) -> List[int]:
        """Every rank's row count for a step of ``phase`` with ``rows`` rows here, or the refusal."""
        if phase not in PHASES:
            raise ValueError(f"dist_train: phase must be one of {PHASES}, got {phase!r}")
        sizes = [rows] * self.world if sizes is None else [int(s) for s in sizes]
        if len(sizes) != self.world:
            raise ValueError(f"dist_train: sizes {sizes} names {len(sizes)} ranks, the group has {self.world}")
        if min(sizes) <= 0 or sizes[self.rank] != rows:
            raise ValueError(f"dist_train: every rank needs at least one row and rank {self.rank} holds {rows} "
                             f"(sizes {sizes})")
        m = self.module
        if self.world > 1 and isinstance(getattr(m, "_net", None), ResNet_features):
            raise NotImplementedError(_RESNET_REFUSAL)
        _, supported, refusal = T._STEPS[hasattr(m, "_max_count"), phase == "finetune"]
        if not supported(m):
            raise NotImplementedError(refusal)
        return sizes

    def step(self, xs1: Tensor, xs2: Tensor, ys: Tensor, optimizer_net, optimizer_classifier, *, phase: str,
             epoch: int = 0, nr_epochs: int = 1, enforce_weight_sparsity: bool = True, tanh_loss_coeff: float = 1.0,
             sizes: Optional[Sequence[int]] = None, sd_keep: Optional[Dict[int, Tensor]] = None,
             step_optimizers: bool = True) -> Tensor:
        """One iteration of ``phase`` on this rank's rows (both views, labels).  ``sizes``: every rank's row count
        (default: all equal to this rank's, what a ``drop_last`` loader under a distributed sampler gives -- there
        is no size exchange); ``sd_keep``: the GLOBAL masks.  Returns the loss kernel's ``stats[8]`` of the global
        batch, the same on every rank, without a host wait."""
        if xs1.shape[0] != xs2.shape[0] or ys.shape[0] != xs1.shape[0]:
            raise ValueError(f"dist_train: xs1 {tuple(xs1.shape)}, xs2 {tuple(xs2.shape)} and ys {tuple(ys.shape)} "
                             f"must hold the same rows")
        sizes = self.check(phase, xs1.shape[0], sizes)
        return T._train_step(self.module, xs1, xs2, ys, phase=phase, optimizer_classifier=optimizer_classifier,
                             optimizer_net=optimizer_net, w=T._loss_weights(phase == "pretrain", epoch, nr_epochs),
                             enforce_weight_sparsity=enforce_weight_sparsity, tanh_loss_coeff=tanh_loss_coeff,
                             sd_keep=sd_keep, generator=self.generator, step_optimizers=step_optimizers,
                             shard=None if self.world == 1 and not self.force_exchange else Shard(self, sizes))

    def reduce_gradients(self, phase: str, optimizer_classifier, optimizer_net) -> Optional[GradArena]:
        """Sum every rank's gradients: pack them into the arena, ONE all-reduce, and each ``.grad`` becomes a view
        of its slot.  The arena is kept while the parameters with a gradient stay the same."""
        params = [p for p in arena_params(self.module, phase, optimizer_classifier, optimizer_net)
                  if p.grad is not None]
        if not params:
            return None
        if self._arena is None or self._arena.key != tuple(id(p) for p in params):
            self._arena = GradArena(params)
        buf = self._arena.pack()
        if self.world > 1:
            dist.all_reduce(buf, group=self.process_group)
        self._arena.scatter()
        return self._arena


class Shard:
    """A rank's place in one step's global batch -- rows [start, start + rows) of each view's ``batch`` -- and the
    five things ``train._train_step`` asks of it, where such a step differs from one on the whole batch."""

    def __init__(self, owner: ShardedTraining, sizes: Sequence[int]):
        self.owner, self.sizes = owner, list(sizes)
        self.start, self.rows, self.batch = sum(sizes[:owner.rank]), sizes[owner.rank], sum(sizes)
        self.reduce_gradients = owner.reduce_gradients                # (5) the arena's all-reduce before AdamW

    def masks(self, sd_keep: Optional[Dict[int, Tensor]]) -> Dict[int, Tensor]:
        """(1) The rank's rows of the global masks ``sd_keep`` (None: drawn from the shared generator)."""
        return shard_masks(self.owner.draw_masks(self.batch) if sd_keep is None else sd_keep, self.start, self.rows,
                           self.batch)

    def gumbel(self):
        """(2) The Gumbel head of this rank's rows ``[view 1 | view 2]`` on the draw of their global rows: an injected
        ``act.exp_noise`` is the global tensor, sliced; otherwise one Philox launch per view segment, whose first
        row g0 starts at block g0 * h * w * P / 4 (P % 4 == 0 for every head kernel, so that is exact)."""
        seed, start, rows, batch = self.owner.draw_seed(), self.start, self.rows, self.batch

        def draw(logits: Tensor, act) -> Tuple[Tensor, Tensor]:
            if act.exp_noise is not None:
                noise = act.exp_noise.to(device=logits.device, dtype=torch.float32)
                return K.count_gumbel_soft(logits, act.tau, shard_rows(noise, start, rows, batch).contiguous(), 0)
            per = logits[0].numel()
            halves = [K.count_gumbel_soft(logits[v * rows:(v + 1) * rows], act.tau, None, seed,
                                          offset=(v * batch + start) * per // 4) for v in (0, 1)]
            return torch.cat([halves[0][0], halves[1][0]]), torch.cat([halves[0][1], halves[1][1]])
        return draw

    def loss(self, hd, ys: Tensor, loss_args: tuple) -> Tuple[Tensor, Optional[Tensor], Tensor]:
        """(3) ``kernels.train_loss`` on the gathered rows of every rank -> (the global batch's stats, this rank's
        rows of d loss / d out, the gathered pooled rows: (4), what the rows form of the head backward needs)."""
        group = self.owner.process_group
        pooled_all, out_all, ys_all = exchange_rows(hd.pooled, hd.out, ys, self.sizes, group)
        partial = K.train_align_partial(hd.proto)
        if self.owner.world > 1:
            dist.all_reduce(partial, group=group)
        stats, d_out_all = K.train_loss_from_partial(partial, hd.proto.shape[1] * hd.proto.shape[2], pooled_all,
                                                     out_all, ys_all, *loss_args)
        d_out = None if d_out_all is None else shard_rows(d_out_all, self.start, self.rows, self.batch)
        return stats, d_out, pooled_all


def train_pipnet(net, train_loader, optimizer_net, optimizer_classifier, scheduler_net, scheduler_classifier,
                 criterion, epoch, nr_epochs, device, is_count_pipnet=False, pretrain=False, finetune=False,
                 progress_prefix: str = "Train Epoch", enforce_weight_sparsity=True, tanh_loss_coeff=1.0,
                 generator: Optional[torch.Generator] = None, verbose: bool = False, process_group=None) -> dict:
    """``train.train_pipnet`` across the ranks of ``process_group`` (None: the default group): the loader yields
    this rank's rows (equal shards: a ``drop_last`` loader under a distributed sampler), the schedulers advance as
    in ``HipEpoch.run``, and the returned ``train_info`` has the same keys, with the same values on every rank.
    ``net``: the network, or a ``ShardedTraining`` around it (whose shared generator then carries over from epoch
    to epoch); ``generator``, when given, must be in the same state on every rank and replaces the wrapper's."""
    if pretrain and finetune:
        raise NotImplementedError("count_pipnet_amd.train_pipnet: pretrain and finetune are exclusive")
    sharded = net if isinstance(net, ShardedTraining) else ShardedTraining(net, process_group)
    if generator is not None:
        sharded.generator = generator
    m = sharded.module
    if hasattr(m, "_max_count") != bool(is_count_pipnet):
        raise NotImplementedError(T._STEPS[bool(is_count_pipnet), bool(finetune)][2])
    phase = "pretrain" if pretrain else "finetune" if finetune else "train"

    def step(a, b, labels):
        return sharded.step(a, b, labels, optimizer_net, optimizer_classifier, phase=phase, epoch=epoch,
                            nr_epochs=nr_epochs, enforce_weight_sparsity=enforce_weight_sparsity,
                            tanh_loss_coeff=tanh_loss_coeff)

    return T._run_epoch(m, step, train_loader, optimizer_net, optimizer_classifier, scheduler_net, scheduler_classifier,
                        epoch, nr_epochs, device, pretrain, finetune, world=sharded.world,
                        say=f"[{progress_prefix} {epoch}] HIP x{sharded.world}" if verbose and sharded.rank == 0
                        else None)
