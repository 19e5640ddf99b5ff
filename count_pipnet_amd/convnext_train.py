"""Train-mode ConvNeXt backbone on the HIP kernels: the forward that keeps the activations of a
trainable ``features`` suffix and the backward through it (CNBlocks, downsamples, the stem), for
the reference's pretrain / "train + freeze params" / "train everything" phases (main.py:238-256,
360-390) and, without the parameter gradients, for the attribution passes.

The surface is ``resnet_train``'s, name for name and parameter for parameter -- ``supported``,
``units``, ``trainable_start``, ``sd_masks``, ``train_forward``, ``backward`` -- so that
``train._train_step`` asks either backbone the same way.  A unit here is one ``features`` entry.
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional

import torch
import torch.nn as nn
from torch import Tensor

from . import _lib
from . import kernels as K
from .backend import _set_grad, packed
from .convnext_features import (CNBlock, ConvNeXt, LayerNorm2d, MidLayerConvNeXt, convnext_features_hip,
                                stochastic_depth_row_scales)


class Saved(NamedTuple):
    """What ``train_forward`` keeps of one stem / CNBlock / downsample for its backward."""
    kind: str                     # "stem" | "block" | "down"
    mod: nn.Module
    key: str                      # the module's prefix in the weight cache
    act: dict                     # its activations


def supported(model) -> bool:
    return isinstance(model, (ConvNeXt, MidLayerConvNeXt))


def units(model) -> int:
    return len(model.features)


def trainable_start(model) -> int:
    """Index of the first ``features`` entry with a trainable parameter (their count: none has)."""
    for j, mod in enumerate(model.features):
        if any(p.requires_grad for p in mod.parameters()):
            return j
    return len(model.features)


def _cnblocks(seq) -> list:
    return [b for mod in seq if isinstance(mod, nn.Sequential) for b in mod if isinstance(b, CNBlock)]


def stochastic_depth_masks(features: nn.Sequential, batch: int,
                           generator: Optional[torch.Generator] = None) -> Dict[int, Tensor]:
    """Host keep masks (bool [batch]) for every CNBlock with p > 0, keyed by block id in
    module order: StochasticDepth("row") keeps a sample's branch with probability 1 - p."""
    masks: Dict[int, Tensor] = {}
    for bid, blk in enumerate(_cnblocks(features)):
        if blk.stochastic_depth.p > 0.0:
            masks[bid] = torch.rand(batch, generator=generator) >= blk.stochastic_depth.p
    return masks


def sd_masks(model, batch: int, generator: Optional[torch.Generator]) -> Dict[int, Tensor]:
    return stochastic_depth_masks(model.features, batch, generator)


def train_forward(model, xs: Tensor, start: Optional[int], sd_keep: Dict[int, Tensor], *, eval_mode: bool = False,
                  nhwc4: Optional[Tensor] = None):
    """Train-mode forward -> (features NHWC, saved).  ``start`` None: the inference executor with
    stochastic depth, nothing kept.  Otherwise features[:start] run on that executor and
    features[start:] with plain (unfused) kernels whose intermediates are kept: per CNBlock the
    input x, the depthwise output z, the LayerNorm output t, the Linear1 pre-activation h1, GELU
    output g and the Linear2 output y2; per downsample its input and LayerNorm output.
    ``eval_mode``: stochastic depth is the identity (no masks, no 1 / (1 - p) scale: every block
    runs with rs = None), as under ``net.eval()``.  ``nhwc4`` (start = 0 only): the input already in
    the stem conv's 4-channel NHWC form, in place of ``xs``.
    The executor part -- layers that run forward only -- takes the model's ``hip_train_precision``
    (pipnet.set_hip_train_dtype; "fp32" unless set); the kept suffix is always fp32."""
    feats, cache = model.features, model._hip_pack
    precision = getattr(model, "hip_train_precision", "fp32")
    if start is None:
        return convnext_features_hip(feats, xs, cache, sd_keep, precision), []
    saved = []
    if start == 0:   # trainable stem (the "train everything" epochs): conv k4 s4 and LN unfused
        conv, ln = feats[0][0], feats[0][1]
        if conv.kernel_size != (4, 4) or conv.stride != (4, 4) or conv.in_channels != 3 or conv.padding != (0, 0):
            raise RuntimeError(f"HIP training step: unsupported ConvNeXt stem {conv}")
        xp = K.nchw_to_nhwc(xs.contiguous(), 4) if nhwc4 is None else nhwc4      # channels zero-padded 3 -> 4
        wp = packed(cache, "0.conv.train", conv.weight,
                    lambda w: torch.nn.functional.pad(w.permute(0, 2, 3, 1), (0, 1)))
        z = K.conv2d_nhwc(xp, wp, conv.bias, 4, 0, _lib.EPI_BIAS)
        h = K.layernorm(z, ln.weight, ln.bias)
        saved.append(Saved("stem", feats[0], "0", dict(x=xp, z=z)))
        start = 1
    else:
        h = convnext_features_hip(feats[:start], xs, cache, sd_keep, precision)
    scales = {} if eval_mode else stochastic_depth_row_scales(feats, sd_keep, xs.shape[0], xs.device)
    bid = len(_cnblocks(feats[:start]))
    for idx in range(start, len(feats)):
        mod = feats[idx]
        if len(mod) > 0 and isinstance(mod[0], CNBlock):
            for jb, blk in enumerate(mod):
                dw, ln, l1, l2 = blk.block[0], blk.block[2], blk.block[3], blk.block[5]
                b, hh, ww, c = h.shape
                key = f"{idx}.{jb}"
                wdw = packed(cache, key + ".dw", dw.weight, lambda w: w.reshape(c, 49).t())
                z = K.dwconv7_plain(h, wdw, dw.bias)
                t = K.layernorm(z, ln.weight, ln.bias)
                h1 = K.linear(t.view(-1, c), l1.weight, l1.bias, _lib.EPI_BIAS)
                g = K.gelu_fwd(h1)
                y2 = K.linear(g, l2.weight, l2.bias, _lib.EPI_BIAS)
                rs = scales.get(bid) if blk.stochastic_depth.p > 0.0 and not eval_mode else None
                out = K.resid_scale(h.view(-1, c), y2, blk.layer_scale.view(-1), rs, hh * ww).view(b, hh, ww, c)
                saved.append(Saved("block", blk, key, dict(x=h, z=z, t=t, h1=h1, g=g, y2=y2, rs=rs)))
                h = out
                bid += 1
        elif len(mod) == 2 and isinstance(mod[0], LayerNorm2d) and isinstance(mod[1], nn.Conv2d):
            ln, conv = mod[0], mod[1]
            t = K.layernorm(h, ln.weight, ln.bias)
            wp = packed(cache, f"{idx}.conv", conv.weight, lambda w: w.permute(0, 2, 3, 1))
            out = K.conv2x2(t, wp, conv.bias, conv.stride[0])
            saved.append(Saved("down", mod, f"{idx}.conv", dict(x=h, t=t)))
            h = out
        else:
            raise RuntimeError(f"HIP training step: unsupported ConvNeXt features entry {idx}")
    return h, saved


def _block_backward(blk: CNBlock, sv: dict, dy: Tensor, param_grads: bool = True, cache: Optional[dict] = None,
                    key: str = "") -> Tensor:
    """Backward of one CNBlock; returns d input [B,H,W,C], accumulated into ``dy`` in place.
    ``param_grads``: the weight-gradient kernels run and every parameter gets its .grad; without it
    no .grad is touched and the reductions the kernels must write (d_ls, d_gamma, ...) stay scratch.
    ``cache`` (with the block's ``key``) keeps the transposed / flipped weights over many backward
    passes (attribution); None: temporaries, as in training, where the weights change every step."""
    dw, ln, l1, l2 = blk.block[0], blk.block[2], blk.block[3], blk.block[5]
    x = sv["x"]
    b, hh, ww, c = x.shape
    dev = x.device

    def laid_out(name, w, fn):
        return fn(w.detach()).contiguous() if cache is None else packed(cache, key + name, w, fn)

    d_ls, d_b2, d_lnw, d_lnb = (torch.empty(c, device=dev) for _ in range(4))
    dy2 = K.ls_backward(dy.reshape(-1, c), sv["y2"], blk.layer_scale.view(-1), sv["rs"], hh * ww, d_ls, d_b2)
    if param_grads:
        _set_grad(blk.layer_scale, d_ls)
        _set_grad(l2.bias, d_b2)
        if l2.weight.requires_grad:
            _set_grad(l2.weight, K.wgrad(dy2, sv["g"]))
    dh1 = K.linear(dy2, laid_out(".l2.t", l2.weight, lambda w: w.t()), None, _lib.EPI_GELU_BWD, r=sv["h1"])
    if param_grads and l1.weight.requires_grad:
        _set_grad(l1.weight, K.wgrad(dh1, sv["t"].view(-1, c)))
    if param_grads and l1.bias.requires_grad:
        _set_grad(l1.bias, K.colsum(dh1))
    dt = K.linear(dh1, laid_out(".l1.t", l1.weight, lambda w: w.t()), None, _lib.EPI_NONE)
    dz = K.ln_backward(sv["z"].view(-1, c), dt, ln.weight.detach(), d_lnw, d_lnb, want_dz=True).view(b, hh, ww, c)
    if param_grads:
        _set_grad(ln.weight, d_lnw)
        _set_grad(ln.bias, d_lnb)
        dwp, d_dwb = torch.empty(49, c, device=dev), torch.empty(c, device=dev)
        K.dwconv7_wgrad(dz, x, dwp, d_dwb)
        _set_grad(dw.weight, dwp.t())
        _set_grad(dw.bias, d_dwb)
    wflip = laid_out(".dw.flip", dw.weight, lambda w: w.flip(2, 3).reshape(c, 49).t())
    dx = dy.reshape(b, hh, ww, c)                    # residual path; the branch's input grad adds in place
    K.dwconv7_plain(dz, wflip, None, out=dx, accumulate=True)
    return dx


def _stem_backward(mod: nn.Sequential, sv: dict, dy: Tensor) -> None:
    """Stem backward (Conv2d(3, 96, 4, 4) + LayerNorm2d): LN gradients, then the conv's
    weight (stride-4 patch gather, MFMA) and bias gradients; the input images need none."""
    conv, ln = mod[0], mod[1]
    z = sv["z"]
    b, h, w, c = z.shape
    dev = z.device
    d_lnw, d_lnb = torch.empty(c, device=dev), torch.empty(c, device=dev)
    need_dz = conv.weight.requires_grad or (conv.bias is not None and conv.bias.requires_grad)
    dz = K.ln_backward(z.view(-1, c), dy.reshape(-1, c), ln.weight, d_lnw, d_lnb, want_dz=need_dz)
    _set_grad(ln.weight, d_lnw)
    _set_grad(ln.bias, d_lnb)
    if not need_dz:
        return
    if conv.weight.requires_grad:
        gp = torch.empty(c, 4 * 4 * 4, device=dev)
        K.wgrad_conv(dz.view(b, h, w, c), sv["x"], 4, 4, 4, gp)
        _set_grad(conv.weight, gp.view(c, 4, 4, 4)[..., :3].permute(0, 3, 1, 2))
    if conv.bias is not None and conv.bias.requires_grad:
        _set_grad(conv.bias, K.colsum(dz))


def _down_backward(mod: nn.Sequential, sv: dict, dy: Tensor, need_dx: bool, param_grads: bool = True) -> Optional[Tensor]:
    """LayerNorm2d + Conv2d(k2, stride 1|2) backward; returns d input when ``need_dx``.
    ``param_grads=False``: the input gradient only (no weight-gradient kernel, no .grad)."""
    ln, conv = mod[0], mod[1]
    x, t = sv["x"], sv["t"]
    b, h, w, cin = t.shape
    cout, stride = conv.out_channels, conv.stride[0]
    if param_grads and conv.weight.requires_grad:
        gp = torch.empty(cout, 4 * cin, device=t.device)
        K.wgrad_conv2x2(dy, t, stride, gp)
        _set_grad(conv.weight, gp.view(cout, 2, 2, cin).permute(0, 3, 1, 2))
    if param_grads and conv.bias is not None and conv.bias.requires_grad:
        _set_grad(conv.bias, K.colsum(dy.reshape(-1, cout)))
    if not (need_dx or (param_grads and (ln.weight.requires_grad or ln.bias.requires_grad))):
        return None
    wd = conv.weight.detach()
    if stride == 1:        # transposed conv = conv of dy (pad 1) with the flipped, transposed taps
        dt = K.conv2d_nhwc(dy.contiguous(), wd.permute(1, 2, 3, 0).flip(1, 2).contiguous(), None, 1, 1,
                           _lib.EPI_NONE)
    else:                  # stride 2: taps do not overlap -> one GEMM, then place the 2x2 blocks
        oh, ow = dy.shape[1], dy.shape[2]
        gm = K.linear(dy.reshape(-1, cout), wd.permute(2, 3, 1, 0).reshape(4 * cin, cout).contiguous(), None,
                      _lib.EPI_NONE)
        dt = torch.zeros(b, h, w, cin, device=t.device)
        dt[:, :2 * oh, :2 * ow] = gm.view(b, oh, ow, 2, 2, cin).permute(0, 1, 3, 2, 4, 5).reshape(b, 2 * oh, 2 * ow, cin)
    d_lnw, d_lnb = torch.empty(cin, device=t.device), torch.empty(cin, device=t.device)
    dx = K.ln_backward(x.reshape(-1, cin), dt.reshape(-1, cin), ln.weight.detach(), d_lnw, d_lnb, want_dz=need_dx)
    if param_grads:
        _set_grad(ln.weight, d_lnw)
        _set_grad(ln.bias, d_lnb)
    return None if dx is None else dx.view(b, h, w, cin)


def backward(model, saved: list, dfeat: Tensor, param_grads: bool = True) -> Optional[Tensor]:
    """Backward from d features (NHWC) through the saved entries, last to first; every backbone
    parameter with requires_grad gets .grad and each entry is freed once it is done.
    ``param_grads=False``: the input-gradient chain only -- no weight-gradient kernel, no .grad,
    ``saved`` left intact for further passes -- returning the gradient at the first saved entry's input:
    for a saved stem d (stem LayerNorm output), the caller's to take on (attribution._stem_dx)."""
    cache = None if param_grads else model._hip_pack
    dy = dfeat
    for i in range(len(saved) - 1, -1, -1):
        e = saved[i]
        if e.kind == "block":
            dy = _block_backward(e.mod, e.act, dy, param_grads, cache, e.key)
        elif e.kind == "down":
            dy = _down_backward(e.mod, e.act, dy, need_dx=i > 0 or not param_grads, param_grads=param_grads)
        elif param_grads:
            _stem_backward(e.mod, e.act, dy)
        if param_grads:
            saved[i] = None                          # free the activations as we go
    return None if param_grads else dy
