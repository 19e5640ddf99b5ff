"""What the explanation passes (``topk``, ``local``, ``purity``, ``stats``, ``attribution``) share: the net under
its wrappers, the rule that keeps a forward's bits independent of its batching, the forward that also says where
each prototype fires, the image patch of a latent location, and the ``.cpu()`` of a result."""
from __future__ import annotations

import argparse
import numbers
from collections import namedtuple
from dataclasses import fields, replace
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import kernels as K
from .convnext_features import as_nhwc
from .pipnet import PRESENCE_THRESHOLD, run_heads, stream_split, sub_batch_logits

PATCH_SIZE = 32


class HostCopy:
    """Mixin of the result dataclasses: ``.cpu()`` is the same result with every tensor field on the host."""
    def cpu(self):
        return replace(self, **{f.name: getattr(self, f.name).cpu() for f in fields(self)
                                if torch.is_tensor(getattr(self, f.name))})


def unwrap(net, what: str):
    """Bare module of a DataParallel-style ``.module`` wrapper or a world-size-1 ShardedInference."""
    from .dist import ShardedInference
    while hasattr(net, "module"):
        if isinstance(net, ShardedInference) and net.world != 1:
            raise RuntimeError(f"{what}: ShardedInference is supported at world size 1 only "
                               "(the dataset index is the running image count of one pass)")
        net = net.module
    return net


def unwrap_sharded(net, process_group, what: str):
    """(bare module, group, world, rank) for the passes that stream the whole dataset and shard over ranks
    (``prototype_topk``, ``class_prototype_stats``, ``mean_intermediate_features``, ``part_purity``): the group
    is ``process_group`` when given, else that of the ShardedInference around the net; world 1, rank 0 without
    either (or without an initialised process group)."""
    import torch.distributed as dist
    from .dist import ShardedInference
    group, wrapped = process_group, False
    while hasattr(net, "module"):
        if isinstance(net, ShardedInference):
            wrapped = True
            if group is None:
                group = net.process_group
        net = net.module
    if not (wrapped or process_group is not None) or not (dist.is_available() and dist.is_initialized()):
        return net, None, 1, 0
    return net, group, dist.get_world_size(group), dist.get_rank(group)


def check_first_index(first_index, what: str) -> int:
    """``first_index`` of a dataset pass as an int: the dataset index of the first image its loader yields."""
    if isinstance(first_index, bool) or not isinstance(first_index, numbers.Integral) or first_index < 0:
        raise ValueError(f"{what}: first_index must be a non-negative integer (the dataset index of the loader's "
                         f"first image), got {first_index!r}")
    return int(first_index)


def is_count(net) -> bool:
    return hasattr(net, "_max_count")


def small_map(hw) -> Optional[bool]:
    """Whether a latent map of ``hw`` = (H, W) has at most K.SPLITK_MAX_M pixels; None while it is not known.
    Anything but False plans the GEMMs per image (K.per_image_gemm_plan) on one stream: there the split-K rule would
    see the batch size (and a Gumbel near-tie flip with it); on larger maps the forward's kernels never do."""
    return None if hw is None else hw[0] * hw[1] <= K.SPLITK_MAX_M


def map_is_small(net, xs: Tensor) -> Optional[bool]:
    """``small_map`` of the map this net gave for inputs of this spatial size; None until ``note_map`` saw one."""
    return small_map(net.__dict__.get("_explain_hw", {}).get(tuple(xs.shape[2:])))


def note_map(net, xs: Tensor, hw) -> None:
    net.__dict__.setdefault("_explain_hw", {})[tuple(xs.shape[2:])] = tuple(hw)     # plain attribute, not a buffer


Located = namedtuple("Located", "scores loc out hw raw")


def located_forward(net, xs: Tensor, small: Optional[bool], with_raw: bool = False) -> Located:
    """(scores [B,P], loc [B,P] int32, logits [B,K], (H, W), raw) of one batch: the inference forward with the flat
    location h * W + w of every prototype's maximum.  Every image gets the bits of its own batch-1 forward, whatever
    the batch; ``small``: ``small_map`` of the latent map.  ``located_forward_maps`` also returns the map.

    PIP-Net: PIPNet._forward_hip with the arg-location head in place of softmax_pool, the proto map not stored
    (fp32 logits); scores are the clamped pooled values, ``raw`` the unclamped ones (the non-inference forward's)
    with ``with_raw``; ``small`` False is the plain forward's path, concurrent sub-batches included.
    CountPIPNet: its own forward (scores: the clamped counts), then the arg-location on its 0/1 map; no ``raw``."""
    return _located(net, xs, small, with_raw, False)[0]


def located_forward_maps(net, xs: Tensor, small: Optional[bool]) -> Tuple[Located, Tensor]:
    """``located_forward`` and the fp32 prototype map [B,P,H,W] (NHWC memory) its scores and locations were read
    from.  PIP-Net: the head writes the map (``softmax_pool_argmax(write_proto=True)``; pooled values, locations
    and logits keep their bits) and the batch runs on one stream, every image still on the plan of its own batch-1
    forward.  CountPIPNet: the map its forward returns."""
    return _located(net, xs, small, False, True)


def _located(net, xs: Tensor, small: Optional[bool], with_raw: bool, with_proto: bool):
    b = xs.shape[0]
    if is_count(net):
        with K.per_image_gemm_plan(b if small is not False else 1):
            proto, clamped, out = net(xs, inference=True)
        _, loc = K.map_argmax(as_nhwc(proto))
        return Located(clamped, loc, out, tuple(proto.shape[2:]), None), proto
    cls = net._classification
    dev = xs.device
    pn, kc = cls.weight.shape[1], cls.weight.shape[0]
    pooled = torch.empty((b, pn), device=dev, dtype=torch.float32)
    loc = torch.empty((b, pn), device=dev, dtype=torch.int32)
    clamped = torch.empty((b, pn), device=dev, dtype=torch.float32)
    out = torch.empty((b, kc), device=dev, dtype=torch.float32)

    maps = []

    def head(logits, i0, i1):
        if logits.dtype == torch.bfloat16:      # bf16 build: its own head, then the location on the fp32 map
            proto, _ = K.softmax_pool_bf16(logits, 0)
            K.map_argmax(proto, out=(pooled[i0:i1], loc[i0:i1]))
        else:
            proto = K.softmax_pool_argmax(logits, write_proto=with_proto, out=(pooled[i0:i1], loc[i0:i1]))[0]
        if with_proto:
            maps.append(proto)
        K.nonneg_linear(pooled[i0:i1], cls.weight, cls.bias, PRESENCE_THRESHOLD, out=(clamped[i0:i1], out[i0:i1]))

    n = stream_split(net, xs) if small is False and not with_proto else 1      # the map: one part, one stream
    with K.per_image_gemm_plan(b if n == 1 else 1):    # n > 1: the plain forward's concurrent sub-batches
        streams, logits = sub_batch_logits(net, xs, n)
    run_heads(streams, logits, head)
    return (Located(clamped, loc, out, tuple(logits[0].shape[1:3]), pooled if with_raw else None),
            maps[0].permute(0, 3, 1, 2) if with_proto else None)


def patch_size(args) -> Tuple[int, int]:
    """(patchsize, skip) of util/func.py:3-15: the image patch a latent location stands for is 32
    pixels wide whatever the backbone, and neighbouring locations lie
    round((image_size - 32) / (wshape - 1)) pixels apart (Python's round: half to even)."""
    return PATCH_SIZE, round((args.image_size - PATCH_SIZE) / (args.wshape - 1))


def patch_skip(image_size: int, w: int) -> int:
    return patch_size(argparse.Namespace(image_size=image_size, wshape=w))[1]


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
    reference as run, and parity with it is the contract: ``patch_geometry`` passes ``(1, P, H, W)``.
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


def patch_geometry(loc: Tensor, empty: Tensor, pn: int, h: int, w: int, image_size: int):
    """(h_idx, w_idx, coords [..., 4], (1, P, H, W)) of the flat locations ``loc`` on an H x W map, as
    ``img_coordinates`` gives them for the 4-D shape; -1 throughout where ``empty``."""
    shape = (1, pn, h, w)
    loc = loc.long().clamp(min=0)
    h_idx, w_idx = loc // w, loc % w
    coords = torch.stack(img_coordinates(image_size, shape, PATCH_SIZE, patch_skip(image_size, w), h_idx, w_idx), dim=-1)
    return h_idx.masked_fill(empty, -1), w_idx.masked_fill(empty, -1), coords.masked_fill(empty.unsqueeze(-1), -1), shape
