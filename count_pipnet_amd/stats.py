"""Class-conditional prototype activation statistics, on the device -- the analysis of
``util/histograms.py`` and the dataset statistic behind CountPIPNet's virtual weights
(``pipnet/count_pipnet.py:226-321``).

The reference runs a forward per batch, copies ``pooled.cpu()`` per batch, concatenates the whole
dataset on the host and then loops in Python over prototypes x classes with boolean masks
(``_collect_activations``, ``plot_prototype_activations_by_class``, ``_generate_zero_report``,
``_generate_summary_heatmap``, ``plot_prototype_activations_histograms``).  Everything it reports
is a function of a few counters and sums per (class, prototype); ``class_prototype_stats``
accumulates those in one streaming pass with no host synchronisation inside the batch loop:

  forward (as ``histograms.net_forward`` picks its mode) -> pipnet_proto_stats_update_f32

Every (class, prototype) entry is accumulated in dataset order by one owner thread, so the
result -- the fp64 sums included -- is bitwise independent of the batch size.  Plotting, colours
and HTML stay with the caller.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import kernels as K
from .backend import use_hip
from .dist import ShardedPass
from .explain_forward import HostCopy, check_first_index, is_count, unwrap_sharded

NEAR_ZERO_THRESHOLD = 0.01      # histograms.py:395
PIPNET_BINS = 50                # histograms.py:397 num_bins_continuous
PIPNET_HIST_MAX = 1.01          # histograms.py:697-698: max(1, max activation) * 1.01 for a softmax score


def pipnet_edges(threshold: float = NEAR_ZERO_THRESHOLD, bins: int = PIPNET_BINS) -> Tensor:
    """The fp32 edges np.histogram(values, bins, range=(threshold, 1.01)) compares fp32 values
    against (histograms.py:697-705 for activations that do not exceed 1)."""
    return torch.from_numpy(np.linspace(threshold, PIPNET_HIST_MAX, bins + 1, dtype=np.float32))


def count_edges(max_count: int) -> Tensor:
    """[0.5, 1.5, ..., max_count + 0.5]: bin i counts the value i + 1, which is
    np.unique(..., return_counts=True) on clamped counts above the threshold (histograms.py:687)."""
    return torch.arange(max_count + 1, dtype=torch.float32) + 0.5


def count_range_edges(max_count: int) -> Tensor:
    """[0, 0.5, 1.5, ..., max_count + 0.5, +inf], for a threshold of -inf: the count ranges of
    plot_prototype_activations_histograms (histograms.py:1058-1065)."""
    return torch.cat((torch.zeros(1), count_edges(max_count), torch.full((1,), float("inf"))))


def _ratio(num: Tensor, den: Tensor) -> Tensor:
    """num / den in fp64, 0 where den is 0 (the reference's ``if n > 0 ... else 0.0``)."""
    den = den.double()
    return torch.where(den > 0, num.double() / den.clamp(min=1), torch.zeros_like(den))


@dataclass
class PrototypeClassStats(HostCopy):
    """Result of ``class_prototype_stats``; tensors stay on the device until ``.cpu()`` is asked
    for.  K = classes, P = prototypes, NB = histogram bins."""
    n_class: Tensor       # [K] int64 images of class k
    n_ge: Tensor          # [K, P] int64 activations >= threshold
    n_gt: Tensor          # [K, P] int64 activations > threshold
    total: Tensor         # [K, P] float64 sum of the activations, in dataset order
    total_gt: Tensor      # [K, P] float64 sum of the activations > threshold, in dataset order
    vmax: Tensor          # [K, P] float32 largest activation (-inf: class without image)
    hist: Tensor          # [K, P, NB] int64 activations > threshold per bin (np.histogram(bins=edges))
    edges: Optional[Tensor]   # [NB + 1] float32, None without histogram
    threshold: float      # the fp32 near-zero threshold compared against
    images: int           # images of the pass

    def mean_per_class(self) -> Tensor:
        """[P, K] float64 mean activation of prototype p over the images of class k
        (histograms.py:591 / :645, the heatmap's :320); 0 where a class has no image."""
        return _ratio(self.total, self.n_class[:, None]).t()

    def nonzero_counts(self) -> Tensor:
        """[P, K] int64 activations >= threshold (histograms.py:590 / :644)."""
        return self.n_ge.t()

    def class_activity(self) -> Tensor:
        """[P, K] float64 share of class k's images with activation > threshold (:660-661)."""
        return _ratio(self.n_gt, self.n_class[:, None]).t()

    def overall_avg_nonzero(self) -> Tensor:
        """[P] float64 mean of the activations > threshold over all images, 0 without any (:521-522)."""
        return _ratio(self.total_gt.sum(dim=0), self.n_gt.sum(dim=0))

    def near_zero(self) -> Tuple[Tensor, Tensor]:
        """([P] int64 images with activation < threshold, [P] float64 their percentage) (:206-209)."""
        n = self.n_class.sum()
        zero = n - self.n_ge.sum(dim=0)
        return zero, _ratio(zero * 100.0, n.expand_as(zero))

    def normalized_hist(self) -> Tensor:
        """[K, P, NB] float64 bin counts over the (class, prototype) pair's activations > threshold
        (:689, :707); 0 where there is none."""
        return _ratio(self.hist, self.n_gt[:, :, None])

    def selected(self, importance: Tensor, importance_threshold: float = 0.1) -> Tensor:
        """[P] bool: importance above the threshold, or every prototype when none is (:479-484)."""
        sel = torch.as_tensor(importance).to(self.n_ge.device) > importance_threshold
        return sel | ~sel.any()

    def outliers(self, plot_outlier_threshold: float = 100.0) -> Tensor:
        """[P] bool: overall non-zero average above the plot threshold (:525-528)."""
        return self.overall_avg_nonzero() > plot_outlier_threshold


def _torch_update(state: K.ProtoStatsState, act: Tensor, labels: Tensor) -> None:
    """pipnet_proto_stats_update_f32 with torch ops: one image at a time, in order, so every sum
    is the kernel's chain of fp64 adds."""
    thr = torch.tensor(state.threshold, dtype=torch.float32, device=act.device)
    nb, e = state.bins, state.edges
    for b in range(act.shape[0]):
        k = int(labels[b])
        if not 0 <= k < state.classes:
            state.bad += 1
            continue
        x = act[b].float()
        gt = x > thr
        state.n_class[k] += 1
        state.n_ge[k] += x >= thr
        state.n_gt[k] += gt
        state.total[k] += x.double()
        state.total_gt[k] += torch.where(gt, x, torch.zeros_like(x)).double()
        state.vmax[k] = torch.fmax(state.vmax[k], x)
        if nb:
            inside = gt & (x >= e[0]) & (x <= e[nb])
            bins = (torch.bucketize(x, e, right=True) - 1).clamp(0, nb - 1)      # x == e[nb]: the last bin
            state.hist[k].scatter_add_(1, bins[:, None], inside[:, None].to(torch.int32))


def _pass(net, loader, max_images: Optional[int], inference: bool, consume, what: str) -> int:
    """Forward every batch of ``loader`` (cut at ``max_images`` as _collect_activations :103-120
    does) and hand (pooled [B,P], labels) to ``consume``; returns the images seen.  Nothing here
    waits for the device."""
    dev = next(net.parameters()).device
    hip = dev.type == "cuda" and use_hip(net)
    seen = 0
    for xs, ys in loader:
        if max_images is not None and seen >= max_images:
            break
        if max_images is not None and xs.shape[0] > max_images - seen:
            xs, ys = xs[:max_images - seen], ys[:max_images - seen]
        if xs.shape[0] == 0:
            continue
        xs = xs.to(dev, non_blocking=True)
        if hip:
            K.require_device(xs, "input images")
        _, pooled, _ = net(xs, inference=inference)
        if pooled.dim() != 2 or pooled.shape[1] != net._num_prototypes:
            raise RuntimeError(f"{what}: the forward returned pooled activations of shape {tuple(pooled.shape)}, "
                               f"expected [batch, {net._num_prototypes}]")
        consume(pooled, ys.to(dev, non_blocking=True).long().contiguous(), hip)
        seen += xs.shape[0]
    return seen


def class_prototype_stats(net, loader, *, num_classes: Optional[int] = None, max_images: Optional[int] = 10000,
                          continuous: bool = False, near_zero_threshold: float = NEAR_ZERO_THRESHOLD,
                          edges=None, first_index: int = 0, process_group=None) -> PrototypeClassStats:
    """One pass over ``loader`` ((images, labels) batches of any size, in dataset order): per
    (class, prototype) the counters, sums, maximum and histogram every figure and report of
    util/histograms.py is computed from.

    ``net``: a PIPNet / CountPIPNet, bare, under a ``.module`` wrapper, or in a ShardedInference; it
    is put in eval mode, as the reference does.  ``first_index`` is the dataset index of the first
    image this loader yields; ``max_images`` cuts at that global index.  In a ShardedInference of more
    than one rank (or with ``process_group`` naming such a group around a bare net) the pass is
    sharded: every rank passes the loader of its own contiguous block (``dist.dataset_shard``, a block
    may be empty) and that block's ``first_index``; the states are exchanged once and merged
    (``kernels.proto_stats_merge``) and every rank returns the statistics of the whole dataset, with
    ``images`` the total.  Every integer field, ``hist`` and ``vmax`` are then bitwise those of one
    process; ``total`` / ``total_gt`` are the ranks' fp64 sums added in rank order, bitwise the
    one-process sums for integer-valued activations (discrete counts) and otherwise within
    2 (n + W) 2^-53 of them, relative (n images of the class, W ranks): the sharded sums depend on the
    partition in their last bits, the one-process sums never on the batching.  The forward mode is
    ``histograms.net_forward``'s (:50-60): PIP-Net and discrete CountPIPNet run with
    ``inference=True``; ``continuous=True`` reads a CountPIPNet's raw counts (``inference=False``,
    the reference's ``plot_always_histograms``).  ``max_images`` cuts the last batch (None: no limit).
    ``num_classes`` defaults to the classifier's rows.  ``edges`` (ascending, fp32) defaults to
    ``pipnet_edges(threshold)`` for PIP-Net and ``count_edges(max_count)`` for discrete counts;
    continuous counts need explicit edges (the reference's range follows each pair's own maximum:
    the result carries ``vmax`` for a second pass).  A label outside [0, num_classes) raises
    ValueError after the pass.  On a ROCm device the statistics are accumulated by one HIP kernel
    per batch; under ``torch_backend()`` or for a CPU net by torch ops in the same order."""
    net, pgroup, world, rank = unwrap_sharded(net, process_group, "class_prototype_stats")
    first_index = check_first_index(first_index, "class_prototype_stats")
    net.eval()
    count = is_count(net)
    if continuous and not count:
        raise ValueError("class_prototype_stats: continuous=True applies to a CountPIPNet only")
    if edges is None:
        if count and continuous:
            raise ValueError("class_prototype_stats: continuous CountPIPNet activations need explicit edges")
        edges = count_edges(net._max_count) if count else pipnet_edges(near_zero_threshold)
    kc = net._classification.weight.shape[0] if num_classes is None else int(num_classes)
    dev = next(net.parameters()).device
    state = K.ProtoStatsState(kc, net._num_prototypes, near_zero_threshold, edges, dev)

    def consume(pooled, ys, hip):
        if hip:
            K.proto_stats_update(state, pooled, ys)
        else:
            _torch_update(state, pooled, ys)

    ex = ShardedPass("class_prototype_stats", pgroup, world, rank, dev)
    seen = 0
    with torch.no_grad(), ex.guard():
        seen = _pass(net, loader, None if max_images is None else max(0, max_images - first_index),
                     not (count and continuous), consume, "class_prototype_stats")
    if ex.sharded:              # one header exchange, one state exchange; every rank holds the merged state
        ex.header(first_index, seen, None, (kc, net._num_prototypes, state.bins, int(count), int(continuous),
                                            -1 if max_images is None else max_images), limit=max_images)
        seen = ex.total
        if seen:
            state = K.proto_stats_merge(ex.gather_state(state))
    if seen == 0:
        raise ValueError("class_prototype_stats: the loader yielded no image")
    bad = int(state.bad)
    if bad:
        raise ValueError(f"class_prototype_stats: {bad} label(s) of the pass lie outside [0, {kc})")
    return PrototypeClassStats(n_class=state.n_class, n_ge=state.n_ge, n_gt=state.n_gt, total=state.total,
                               total_gt=state.total_gt, vmax=state.vmax, hist=state.hist.long(), edges=state.edges,
                               threshold=state.threshold, images=seen)


def mean_intermediate_features(net, loader, *, first_index: int = 0, process_group=None) -> Tensor:
    """[D] float32 mean of ``net._intermediate(clamped_counts)`` over the dataset
    (count_pipnet.py:226-281), streamed: per batch the fp64 column sums are added in image order
    (pipnet_colsum_accum_f64), so no batch's counts are kept and the result does not depend on
    the batching.  ``first_index`` / ``process_group``: as in ``class_prototype_stats``; sharded,
    the ranks' [D] fp64 accumulators are added in rank order (``kernels.colsum_merge_f64``) and
    divided by the total: bitwise the one-process mean where the layer's outputs are integers (one-hot
    codes), else within 2 (n + W) 2^-53 * sum|x| / n of it."""
    from .count_pipnet import intermediate_hip
    net, pgroup, world, rank = unwrap_sharded(net, process_group, "mean_intermediate_features")
    first_index = check_first_index(first_index, "mean_intermediate_features")
    net.eval()
    if not is_count(net):
        raise ValueError("mean_intermediate_features: needs a CountPIPNet")
    acc = []

    def consume(clamped, ys, hip):
        inter = intermediate_hip(net._intermediate, clamped) if hip else net._intermediate(clamped)
        if not acc:
            acc.append(torch.zeros(inter.shape[1], device=inter.device, dtype=torch.float64))
        if hip:
            K.colsum_accum_f64(acc[0], inter)
        else:
            for row in inter.double():
                acc[0] += row

    dev = next(net.parameters()).device
    ex = ShardedPass("mean_intermediate_features", pgroup, world, rank, dev)
    seen = 0
    with torch.no_grad(), ex.guard():
        seen = _pass(net, loader, None, True, consume, "mean_intermediate_features")
    if ex.sharded:              # the width D travels in the header's map slot: an empty rank learns it there
        ex.header(first_index, seen, (1, acc[0].numel()) if acc else None, (net._num_prototypes,))
        seen = ex.total
        if seen:
            mine = acc[0] if acc else torch.zeros(ex.hw[1], device=dev, dtype=torch.float64)
            acc = [K.colsum_merge_f64(ex.gather_tensor(mine))]
    if seen == 0:
        raise ValueError("mean_intermediate_features: the loader yielded no image")
    return (acc[0] / seen).float()


def virtual_weights(net, loader=None, custom_onehot_scale: bool = False, *, first_index: int = 0,
                    process_group=None) -> Tensor:
    """[K, P] virtual classification matrix of a CountPIPNet (count_pipnet.py:283-321): column p is
    ``get_prototype_importance_per_class(p, scalars)``; ``scalars`` are the dataset's mean
    intermediate features for a one-hot intermediate layer with ``custom_onehot_scale`` (that
    needs ``loader``), else None.  ``first_index`` / ``process_group`` go to ``mean_intermediate_features``."""
    from .count_pipnet_utils import OneHotEncoder
    from .local import count_importance_matrix
    wrapped = net
    net = unwrap_sharded(net, process_group, "virtual_weights")[0]
    scalars = None
    if custom_onehot_scale and isinstance(net._intermediate, OneHotEncoder):
        if loader is None:
            raise ValueError("virtual_weights: custom_onehot_scale needs a loader for the dataset mean")
        scalars = mean_intermediate_features(wrapped, loader, first_index=first_index, process_group=process_group)
    with torch.no_grad():
        return count_importance_matrix(net, scalars)
