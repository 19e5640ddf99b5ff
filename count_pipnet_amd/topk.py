"""Top-k patches per prototype, on the device -- the explanation pass of ``util/vis_pipnet.py``.

The reference finds, for every prototype, the k images that activate it most and the patch where
it fires (``vizualize_network_pipnet`` :187-275, ``vizualize_network_count_pipnet`` :652-755) at
batch size 1 with a Python loop over the prototypes: per image and prototype one ``.item()``, one
``feature_map.clone().cpu()`` and two host ``torch.max`` calls.  ``prototype_topk`` computes the
same lists in one pass at any batch size with no host synchronisation inside the loop:

  PIP-Net    backbone + add-on logits -> fused softmax + max-pool + arg-location (the proto map
             is never written) -> threshold + NonNegLinear -> streaming top-k update
  CountPIPNet  the existing forward -> arg-location on its 0/1 map -> top-k update per count group

Image decoding, cropping, grids and plots stay with the caller: the result holds, per prototype,
the dataset indices, scores, latent locations and image-patch coordinates to cut out.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch
from torch import Tensor

from . import kernels as K
from .dist import ShardedPass
from .explain_forward import (PATCH_SIZE, HostCopy, img_coordinates, is_count, located_forward,  # noqa: F401
                              check_first_index, patch_geometry, patch_size, small_map, unwrap, unwrap_sharded)

COUNT_MIN_SCORE = 0.01          # vis_pipnet.py:703: counts below it are not candidates
# vis_pipnet.py:533-538: (first class, last class), 1-based inclusive -> count group
DEFAULT_CLASS_TO_COUNT = {(1, 3): 1, (4, 6): 2, (7, 9): 3}
_pipnet_batch = located_forward     # the located forward's name before it moved: part-purity tests written then import it


@dataclass
class PrototypeTopK(HostCopy):
    """Result of ``prototype_topk``; tensors stay on the device until ``.cpu()`` is asked for.
    G = count groups (1 for PIP-Net); slot j of (p, g) is the j-th best image, empty slots hold
    index -1 (and -1 locations / coordinates, score 0)."""
    scores: Tensor        # [P, G, k] float32
    index: Tensor         # [P, G, k] int64 dataset index (first_index + running image count of the pass)
    h_idx: Tensor         # [P, G, k] int64 latent row of the prototype's maximum
    w_idx: Tensor         # [P, G, k] int64 latent column
    coords: Tensor        # [P, G, k, 4] int64 (h_min, h_max, w_min, w_max) image patch
    abstained: Tensor     # [] int64: images whose largest logit is 0
    selected: Tensor      # [P] bool: importance above the threshold (all when pretraining)
    unused: Tensor        # [P] bool: selected, but no stored score > 0.1
    groups: List[Optional[int]]      # the count value of each group; [None] for PIP-Net
    proto_shape: Tuple[int, int, int, int]   # (1, P, H, W) handed to img_coordinates


def _count_lut(class_to_count: Dict[Tuple[int, int], int]):
    """(count values sorted = the groups, lut[label] = group index or -1) from the reference's
    {(first, last) 1-based inclusive: count} mapping; the first matching range wins, as there."""
    groups = sorted(set(class_to_count.values()))
    n = max(end for _, end in class_to_count)
    lut = torch.full((n,), -1, dtype=torch.int32)
    for label in range(n):
        for (start, end), count in class_to_count.items():
            if start <= label + 1 <= end:
                lut[label] = groups.index(count)
                break
    return groups, lut


def prototype_topk(net, loader, k: int = 10, *, image_size: int, pretraining: bool = False,
                   importance_threshold: float = 0.1,
                   class_to_count: Optional[Dict[Tuple[int, int], int]] = None, first_index: int = 0,
                   process_group=None) -> PrototypeTopK:
    """One pass over ``loader`` ((images, labels) batches of any size, in dataset order): for every
    prototype the k most activating images, where the prototype fires in each, and the image patch
    to cut out -- the lists of vis_pipnet.py:187-275 (PIP-Net) / :652-755 (CountPIPNet, one list per
    count group of the image's class).  The dataset index is ``first_index`` plus the running image
    count: ``first_index`` is the dataset index of the first image this loader yields.

    ``net``: a PIPNet / CountPIPNet on a ROCm device, bare, under a ``.module`` wrapper, or in a
    ShardedInference; it is put in eval mode, as the reference does.  In a ShardedInference of more
    than one rank (or with ``process_group`` naming such a group around a bare net) the pass is
    sharded: every rank passes the loader of its own contiguous block (``dist.dataset_shard``) and
    that block's ``first_index``, the per-rank lists are exchanged once and merged
    (``kernels.topk_merge``), and every rank returns the result of one process over the whole
    dataset, bit for bit; a rank's block may be empty.  PIP-Net scores
    are the clamped pooled activations; CountPIPNet scores are the clamped counts (>= 0.01) and
    ``class_to_count`` maps 1-based inclusive class ranges to count groups (default: classes
    1-3 -> 1, 4-6 -> 2, 7-9 -> 3); a label outside the mapping raises ValueError.  The top-k is kept
    for all prototypes; ``selected`` marks those the reference would visualise.  Nothing inside the
    batch loop waits for the device."""
    net, pgroup, world, rank = unwrap_sharded(net, process_group, "prototype_topk")
    first_index = check_first_index(first_index, "prototype_topk")
    net.eval()
    count = is_count(net)
    dev = next(net.parameters()).device
    pn = net._num_prototypes
    if count:
        groups, lut = _count_lut(DEFAULT_CLASS_TO_COUNT if class_to_count is None else class_to_count)
        lut_dev = lut.to(dev)
        bad = torch.zeros((), device=dev, dtype=torch.bool)     # a device label outside the mapping
    else:
        groups = [None]
    state = K.TopkState(len(groups), pn, k, dev)
    ex = ShardedPass("prototype_topk", pgroup, world, rank, dev)
    with torch.no_grad():
        if pretraining:
            selected = torch.ones(pn, device=dev, dtype=torch.bool)
        elif count:
            selected = torch.tensor([net.get_prototype_importance(p) for p in range(pn)],
                                    device=dev) > importance_threshold
        else:
            selected = net._classification.weight.max(dim=0).values > importance_threshold
        seen, hw, group = 0, None, None
        with ex.guard():
            for xs, ys in loader:
                xs = xs.to(dev, non_blocking=True)
                if count:
                    if ys.is_cuda:       # checked on the device, reported after the pass
                        ysl = ys.to(dev).long()
                        ok = (ysl >= 0) & (ysl < lut_dev.numel())
                        group = torch.where(ok, lut_dev[ysl.clamp(0, lut_dev.numel() - 1)], torch.full_like(ok, -1, dtype=torch.int32))
                        bad |= (group < 0).any()
                    else:
                        ysl = ys.long()
                        ok = (ysl >= 0) & (ysl < lut.numel())
                        if not bool(ok.all()) or bool((lut[ysl] < 0).any()):
                            wrong = [int(y) + 1 for y in ysl if not (0 <= int(y) < lut.numel()) or lut[int(y)] < 0]
                            raise ValueError(f"No class label found for label {wrong[0]}")
                        group = lut[ysl].to(dev, non_blocking=True)
                    group = group.contiguous()
                else:
                    K.require_device(xs, "input images")
                fwd = located_forward(net, xs, small_map(hw))      # the first batch: the map is not known yet
                K.topk_update(state, fwd.scores, fwd.loc, first_index + seen, group, COUNT_MIN_SCORE if count else None,
                              fwd.out)
                hw = fwd.hw
                seen += xs.shape[0]
        flag = count and bool(bad)
        if ex.sharded:          # one header exchange, one state exchange; every rank holds the merged state
            ex.header(first_index, seen, hw, (len(groups), pn, k, int(count)), flag=flag)
            flag, hw = ex.flag, ex.hw
            if not flag and hw is not None:
                state = K.topk_merge(ex.gather_state(state))
        if flag:
            raise ValueError("No class label found for a label of the pass (outside class_to_count)")
        if hw is None:
            raise ValueError("prototype_topk: the loader yielded no batch")
        h_idx, w_idx, coords, shape = patch_geometry(state.loc.permute(1, 0, 2), state.index.permute(1, 0, 2) < 0, pn,
                                                     hw[0], hw[1], image_size)
        scores = state.score.permute(1, 0, 2).contiguous()
        return PrototypeTopK(
            scores=scores, index=state.index.permute(1, 0, 2).contiguous(), h_idx=h_idx, w_idx=w_idx, coords=coords,
            abstained=state.abstained[0], selected=selected, unused=selected & ~(scores > 0.1).flatten(1).any(dim=1),
            groups=groups, proto_shape=shape)
