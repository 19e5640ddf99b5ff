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

import argparse
from dataclasses import dataclass, fields
from typing import Dict, List, Optional, Tuple

import torch
from torch import Tensor

from . import kernels as K
from .convnext_features import as_nhwc
from .pipnet import PRESENCE_THRESHOLD, run_heads, stream_split, sub_batch_logits

PATCH_SIZE = 32
COUNT_MIN_SCORE = 0.01          # vis_pipnet.py:703: counts below it are not candidates
# vis_pipnet.py:533-538: (first class, last class), 1-based inclusive -> count group
DEFAULT_CLASS_TO_COUNT = {(1, 3): 1, (4, 6): 2, (7, 9): 3}


def patch_size(args) -> Tuple[int, int]:
    """(patchsize, skip) of util/func.py:3-15: the image patch a latent location stands for is 32
    pixels wide whatever the backbone, and neighbouring locations lie
    round((image_size - 32) / (wshape - 1)) pixels apart (Python's round: half to even)."""
    return PATCH_SIZE, round((args.image_size - PATCH_SIZE) / (args.wshape - 1))


def img_coordinates(img_size: int, shape, patchsize: int, skip: int, h_idx, w_idx):
    """Latent location -> (h_min, h_max, w_min, w_max) of its image patch, as
    util/vis_pipnet.py:1162-1193 computes it.  ``h_idx`` / ``w_idx``: ints (ints come back) or
    integer tensors of one shape (tensors come back, same device).

    ``shape`` is the 4-D shape ``(1, P, H, W)`` the reference's callers pass
    (``proto_features.shape``), and the function indexes it as the reference does: the tests
    written for a 3-D map -- ``shape[1] == 26 and shape[2] == 26`` for the small-stride ConvNeXt
    rule, ``h_idx == shape[1] - 1`` / ``w_idx == shape[2] - 1`` for the last row / column -- look
    at ``P`` and ``H`` of a 4-D shape.  So the 26 x 26 rule applies only to a 26-prototype net, the
    row clamp fires at ``h_idx == P - 1`` and the column clamp at ``w_idx == H - 1``.  That is the
    reference as run, and parity with it is the contract: ``prototype_topk`` passes ``(1, P, H, W)``.
    """
    scalar = not torch.is_tensor(h_idx)
    h = torch.as_tensor(h_idx, dtype=torch.int64)
    w = torch.as_tensor(w_idx, dtype=torch.int64, device=h.device)
    if shape[1] == 26 and shape[2] == 26:
        # outer latent patches see less of the image: half a step in from the border, and the last
        # one pulled back by that half step
        last = shape[-1] - 1

        def axis(i):
            lo = torch.clamp((i - 1) * skip + 4, min=0)
            lo = torch.where(i < last, lo, lo - 4)
            return lo, lo + patchsize
    else:
        def axis(i):
            return i * skip, torch.clamp(i * skip + patchsize, max=img_size)
    h0, h1 = axis(h)
    w0, w1 = axis(w)
    h1 = torch.where(h == shape[1] - 1, torch.full_like(h1, img_size), h1)
    w1 = torch.where(w == shape[2] - 1, torch.full_like(w1, img_size), w1)
    h0 = torch.where(h1 == img_size, torch.full_like(h0, img_size - patchsize), h0)
    w0 = torch.where(w1 == img_size, torch.full_like(w0, img_size - patchsize), w0)
    if scalar:
        return int(h0), int(h1), int(w0), int(w1)
    return h0, h1, w0, w1


@dataclass
class PrototypeTopK:
    """Result of ``prototype_topk``; tensors stay on the device until ``.cpu()`` is asked for.
    G = count groups (1 for PIP-Net); slot j of (p, g) is the j-th best image, empty slots hold
    index -1 (and -1 locations / coordinates, score 0)."""
    scores: Tensor        # [P, G, k] float32
    index: Tensor         # [P, G, k] int64 dataset index (running image count of the pass)
    h_idx: Tensor         # [P, G, k] int64 latent row of the prototype's maximum
    w_idx: Tensor         # [P, G, k] int64 latent column
    coords: Tensor        # [P, G, k, 4] int64 (h_min, h_max, w_min, w_max) image patch
    abstained: Tensor     # [] int64: images whose largest logit is 0
    selected: Tensor      # [P] bool: importance above the threshold (all when pretraining)
    unused: Tensor        # [P] bool: selected, but no stored score > 0.1
    groups: List[Optional[int]]      # the count value of each group; [None] for PIP-Net
    proto_shape: Tuple[int, int, int, int]   # (1, P, H, W) handed to img_coordinates

    def cpu(self) -> "PrototypeTopK":
        return PrototypeTopK(**{f.name: (getattr(self, f.name).cpu() if torch.is_tensor(getattr(self, f.name))
                                         else getattr(self, f.name)) for f in fields(self)})


def _unwrap(net):
    """Bare module of a DataParallel-style ``.module`` wrapper or a world-size-1 ShardedInference."""
    from .dist import ShardedInference
    while hasattr(net, "module"):
        if isinstance(net, ShardedInference) and net.world != 1:
            raise RuntimeError("prototype_topk: ShardedInference is supported at world size 1 only "
                               "(the dataset index is the running image count of one pass)")
        net = net.module
    return net


def _pipnet_batch(net, xs: Tensor, small_map: Optional[bool], with_raw: bool = False):
    """(clamped pooled [B,P], loc [B,P], logits [B,K], (H, W)) of one batch: PIPNet._forward_hip with
    the arg-location head in place of softmax_pool, the proto map not stored (fp32 logits).
    ``with_raw``: the unclamped pooled values [B,P] (the non-inference forward's) as a fifth item.

    Every image gets the bits of its own batch-1 forward, whatever the batch: on maps of more than
    K.SPLITK_MAX_M pixels the forward's kernels never see the batch size (``small_map`` False: the
    plain forward's path, concurrent sub-batches included); on smaller maps, or while the map size
    is not known yet (None: the first batch), the GEMMs are planned per image
    (K.per_image_gemm_plan) on one stream."""
    cls = net._classification
    b = xs.shape[0]
    dev = xs.device
    pn, kc = cls.weight.shape[1], cls.weight.shape[0]
    pooled = torch.empty((b, pn), device=dev, dtype=torch.float32)
    loc = torch.empty((b, pn), device=dev, dtype=torch.int32)
    clamped = torch.empty((b, pn), device=dev, dtype=torch.float32)
    out = torch.empty((b, kc), device=dev, dtype=torch.float32)

    def head(logits, i0, i1):
        if logits.dtype == torch.bfloat16:      # bf16 build: its own head, then the location on the fp32 map
            proto, _ = K.softmax_pool_bf16(logits, 0)
            K.map_argmax(proto, out=(pooled[i0:i1], loc[i0:i1]))
        else:
            K.softmax_pool_argmax(logits, out=(pooled[i0:i1], loc[i0:i1]))
        K.nonneg_linear(pooled[i0:i1], cls.weight, cls.bias, PRESENCE_THRESHOLD, out=(clamped[i0:i1], out[i0:i1]))

    n = stream_split(net, xs) if small_map is False else 1
    with K.per_image_gemm_plan(b if n == 1 else 1):    # n > 1: the plain forward's concurrent sub-batches
        streams, logits = sub_batch_logits(net, xs, n)
    run_heads(streams, logits, head)
    hw = tuple(logits[0].shape[1:3])
    return (clamped, loc, out, hw, pooled) if with_raw else (clamped, loc, out, hw)


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
                   class_to_count: Optional[Dict[Tuple[int, int], int]] = None) -> PrototypeTopK:
    """One pass over ``loader`` ((images, labels) batches of any size, in dataset order): for every
    prototype the k most activating images, where the prototype fires in each, and the image patch
    to cut out -- the lists of vis_pipnet.py:187-275 (PIP-Net) / :652-755 (CountPIPNet, one list per
    count group of the image's class).  The dataset index is the running image count.

    ``net``: a PIPNet / CountPIPNet on a ROCm device, bare, under a ``.module`` wrapper, or in a
    world-size-1 ShardedInference; it is put in eval mode, as the reference does.  PIP-Net scores
    are the clamped pooled activations; CountPIPNet scores are the clamped counts (>= 0.01) and
    ``class_to_count`` maps 1-based inclusive class ranges to count groups (default: classes
    1-3 -> 1, 4-6 -> 2, 7-9 -> 3); a label outside the mapping raises ValueError.  The top-k is kept
    for all prototypes; ``selected`` marks those the reference would visualise.  Nothing inside the
    batch loop waits for the device."""
    net = _unwrap(net)
    net.eval()
    count = hasattr(net, "_max_count")
    dev = next(net.parameters()).device
    pn = net._num_prototypes
    if count:
        groups, lut = _count_lut(DEFAULT_CLASS_TO_COUNT if class_to_count is None else class_to_count)
        lut_dev = lut.to(dev)
        bad = torch.zeros((), device=dev, dtype=torch.bool)     # a device label outside the mapping
    else:
        groups = [None]
    state = K.TopkState(len(groups), pn, k, dev)
    with torch.no_grad():
        if pretraining:
            selected = torch.ones(pn, device=dev, dtype=torch.bool)
        elif count:
            selected = torch.tensor([net.get_prototype_importance(p) for p in range(pn)],
                                    device=dev) > importance_threshold
        else:
            selected = net._classification.weight.max(dim=0).values > importance_threshold
        seen, hw = 0, None
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
                # small maps: per-image GEMM plan, as in _pipnet_batch (a Gumbel near-tie must not
                # flip with the batch size)
                small = hw is None or hw[0] * hw[1] <= K.SPLITK_MAX_M
                with K.per_image_gemm_plan(xs.shape[0] if small else 1):
                    proto, clamped, out = net(xs, inference=True)
                _, loc = K.map_argmax(as_nhwc(proto))
                K.topk_update(state, clamped, loc, seen, group=group.contiguous(), min_score=COUNT_MIN_SCORE, out=out)
                hw = tuple(proto.shape[2:])
            else:
                K.require_device(xs, "input images")
                clamped, loc, out, hw = _pipnet_batch(net, xs, None if hw is None else hw[0] * hw[1] <= K.SPLITK_MAX_M)
                K.topk_update(state, clamped, loc, seen, out=out)
            seen += xs.shape[0]
        if count and bool(bad):
            raise ValueError("No class label found for a label of the pass (outside class_to_count)")
        if hw is None:
            raise ValueError("prototype_topk: the loader yielded no batch")
        h, w = hw
        shape = (1, pn, h, w)
        _, skip = patch_size(argparse.Namespace(image_size=image_size, wshape=w))
        empty = state.index.permute(1, 0, 2) < 0
        loc = state.loc.permute(1, 0, 2).long().clamp(min=0)
        h_idx, w_idx = loc // w, loc % w
        coords = torch.stack(img_coordinates(image_size, shape, PATCH_SIZE, skip, h_idx, w_idx), dim=-1)
        scores = state.score.permute(1, 0, 2).contiguous()
        return PrototypeTopK(
            scores=scores, index=state.index.permute(1, 0, 2).contiguous(),
            h_idx=h_idx.masked_fill(empty, -1), w_idx=w_idx.masked_fill(empty, -1),
            coords=coords.masked_fill(empty.unsqueeze(-1), -1), abstained=state.abstained[0],
            selected=selected, unused=selected & ~(scores > 0.1).flatten(1).any(dim=1),
            groups=groups, proto_shape=shape)
