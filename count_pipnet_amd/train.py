"""PIP-Net / CountPIPNet training iterations on the MI355X kernels.

The reference trains with ``pipnet/train.py:train_pipnet`` (train.py:8-150).  In its
finetune phase (main.py:333-345) only the classification layer trains, so one iteration is:
forward of cat([xs1, xs2]) in train mode -> ``calculate_loss`` (train.py:154-250, loss =
2 * class loss; the align / tanh terms are computed for logging) -> backward into the
NonNegLinear weight / bias -> ``optimizer_classifier.step()`` (AdamW, util/args.py:327)
-> scheduler -> the sparsity clamps (train.py:134-140).  Here that iteration is:

  * forward: the same HIP backbone / head as inference, plus torchvision's row stochastic
    depth -- a dropped sample skips the block's branch outright
    (``convnext_features._cnblock``); pooled is not thresholded (inference=False);
  * ``kernels.train_loss`` (csrc/train_ops.hip): align / tanh / class terms, correct count
    and d loss / d out in two launches (the align term reads the proto map once);
  * ``kernels.nonneg_linear_backward`` and ``kernels.adamw_step_`` (AdamW fused with the
    clamps), updating the torch optimizer's own ``state`` tensors (``step``, ``exp_avg``,
    ``exp_avg_sq``) so optimizer, scheduler and their ``state_dict``s stay interchangeable
    with the reference's.

No host synchronisation inside the loop (the reference reads five ``.item()`` per
iteration): loss terms and accuracy accumulate on the device and are read once per epoch.
Stochastic-depth masks come from a host ``torch.Generator`` (the reference draws them with
the device RNG: same distribution, different stream -- RNG parity unpinned; the tests
inject the masks recorded from the reference).

The pretrain / joint / "train everything" phases backpropagate into a trainable backbone
suffix on the same kernels.  A backbone's train-mode forward and backward live in its own module,
both behind one surface (``train_forward``, ``backward``, ...; ``_backbone`` picks the module):
``convnext_train`` (CNBlocks / downsamples / stem) and ``resnet_train`` (the ResNet-50 Bottlenecks
with train-mode BatchNorm; every BN of the backbone, frozen ones included, normalises with batch
statistics and updates its running statistics, as under the reference's ``net.train()``).

Every phase of both models is the one ``_train_step``; the four public ``hip_*_step`` functions
choose its phase and loss weights, the two heads (``_pipnet_head``, ``_count_head``) its middle.
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Tuple

import torch
import torch.nn as nn
from torch import Tensor

from . import _lib, convnext_train, resnet_train
from . import kernels as K
from .backend import _set_grad
from .convnext_train import stochastic_depth_masks  # noqa: F401  (its callers know it from here)

# (align, tanh, class) loss weights of the non-pretrain phases (train.py:56-61)
FINETUNE_LOSS_WEIGHTS = (5.0, 2.0, 2.0)
SPARSITY_DELTA = 1e-3          # train.py:135: W <- max(W - 1e-3, 0) after every step


def _inner(net: nn.Module) -> nn.Module:
    return getattr(net, "module", net)


def _backbone(m: nn.Module):
    """The module with the train-mode forward and backward of ``m``'s backbone: ``convnext_train``
    (ConvNeXt, full or mid-layer), ``resnet_train`` (a Bottleneck ResNet with the stem frozen), or
    None where neither supports it."""
    net = getattr(m, "_net", None)
    return next((b for b in (convnext_train, resnet_train) if b.supported(net)), None)


def _sd_masks(m: nn.Module, batch: int, generator: Optional[torch.Generator]) -> Dict[int, Tensor]:
    """Stochastic-depth keep masks of the backbone (ResNets have none)."""
    return _backbone(m).sd_masks(m._net, batch, generator)


def trainable_suffix_start(net: nn.Module) -> int:
    """Index j of the first ``features`` entry (ConvNeXt) or residual block (ResNet) holding a
    trainable parameter (their count when the backbone is frozen).  Gradients flow through
    every entry from j on."""
    m = _inner(net)
    return _backbone(m).trainable_start(m._net)


def _supported(net: nn.Module, count: bool, finetune: bool) -> bool:
    """True when the iteration runs on the HIP kernels: a PIP-Net (``count``: a CountPIPNet whose
    intermediate layer has a HIP backward) on a backbone with a HIP train-mode forward, fp32 on a
    ROCm device, whose trainable set fits the phase -- ``finetune``: within the classifier (and the
    intermediate layer); otherwise a backbone suffix from unit j on (a ConvNeXt's j = 0: the stem too)."""
    m = _inner(net)
    if hasattr(m, "_max_count") != count or not hasattr(m, "_classification") or _backbone(m) is None:
        return False
    if count:
        from .count_pipnet_utils import (BilinearIntermediate, IdentityIntermediate, LinearFull, LinearIntermediate,
                                         OneHotEncoder)
        if not isinstance(m._intermediate, (IdentityIntermediate, OneHotEncoder, LinearFull, LinearIntermediate,
                                           BilinearIntermediate)):
            return False
    if not all(p.is_cuda and p.dtype == torch.float32 for p in m.parameters()):
        return False
    if not finetune:
        return trainable_suffix_start(m) < _backbone(m).units(m._net)
    cls = m._classification
    allowed = list(cls.parameters()) + list(m._intermediate.parameters()) if count else [cls.weight, cls.bias]
    return {id(p) for p in m.parameters() if p.requires_grad} <= {id(p) for p in allowed}


def hip_finetune_supported(net: nn.Module) -> bool:
    """True when the finetune iteration runs on the HIP kernels: a PIP-Net (not Count) on a
    backbone ``_backbone`` knows (ConvNeXt, or a Bottleneck ResNet with the stem frozen), fp32 on
    a ROCm device, only classifier parameters trainable."""
    return _supported(net, count=False, finetune=True)


def hip_count_finetune_supported(net: nn.Module) -> bool:
    """A CountPIPNet on such a backbone (fp32, ROCm) whose trainable parameters are within the
    classifier and an intermediate layer with a HIP backward (identity, one-hot, linear_full,
    linear, bilinear)."""
    return _supported(net, count=True, finetune=True)


def hip_train_supported(net: nn.Module) -> bool:
    """A PIP-Net on such a backbone (fp32, ROCm) with a trainable backbone part: a ConvNeXt's
    suffix features[j:] (the reference's pretrain / "train + freeze params" phases; j = 0, the
    stem included: the "train everything" epochs after freeze_epochs, main.py:362-373), a
    ResNet's residual blocks from the first trainable one on."""
    return _supported(net, count=False, finetune=False)


def hip_count_train_supported(net: nn.Module) -> bool:
    """A CountPIPNet on such a backbone (fp32, ROCm) with a trainable backbone part as for
    ``hip_train_supported`` and an intermediate layer that has a HIP backward (the reference's
    pretrain, "train + freeze params" and "train everything" phases for CountPIPNet,
    main.py:238-256, 360-390)."""
    return _supported(net, count=True, finetune=False)


class _Head(NamedTuple):
    """What a head's train-mode forward leaves for the loss and the backward."""
    proto: Tensor                 # prototype map, NHWC
    pooled: Tensor                # max-pooled presence scores (PIP-Net) / raw counts (CountPIPNet)
    cls_in: Tensor                # the classifier's input
    out: Tensor
    saved: dict                   # CountPIPNet: tau, the clamped counts, the bilinear layer's activations


def _pipnet_head(m: nn.Module, feats: Tensor) -> _Head:
    """PIPNet.forward(inference=False) after the backbone: add-on softmax, max-pool, classifier."""
    from .pipnet import add_on_logits_hip
    proto, pooled = K.softmax_pool(add_on_logits_hip(m._add_on, feats), pool_mode=0)
    _, out = K.nonneg_linear(pooled, m._classification.weight, m._classification.bias, None)
    return _Head(proto, pooled, pooled, out, {})


def _pipnet_head_backward(m: nn.Module, hd: _Head, d_out: Optional[Tensor], w_align: float, w_tanh: float,
                          tanh_loss_coeff: float, to_logits: bool,
                          pooled_all: Optional[Tensor] = None) -> Optional[Tensor]:
    """d loss / d add-on logits (``to_logits``); a PIP-Net head has no parameter of its own.  ``pooled_all``: ``hd``
    and ``d_out`` are one rank's rows of a batch with these pooled rows (dist_train)."""
    if not to_logits:
        return None
    return K.head_backward(hd.proto, hd.pooled, d_out, m._classification.weight, w_align, w_tanh, pooled_all=pooled_all)


def train_forward_hip(net: nn.Module, xs: Tensor, sd_keep: Optional[Dict[int, Tensor]],
                      update_bn_stats: bool = True):
    """PIPNet.forward(xs, inference=False) with train-mode stochastic depth on the HIP
    kernels: (proto NHWC [B,h,w,P], pooled [B,P], out [B,K]).  Like the module's own forward
    under ``net.train()``, a ResNet backbone's BatchNorms normalise with batch statistics and
    take the running-statistics update; ``update_bn_stats=False`` restores every running
    statistic and counter afterwards (an observer forward that must not advance them)."""
    m = _inner(net)
    saved = None
    if not update_bn_stats:
        saved = [(b, b.clone()) for b in m._net.buffers()]
    with torch.no_grad():
        try:
            feats = _backbone(m).train_forward(m._net, xs, None, sd_keep)[0]
        finally:
            for b, v in saved or ():
                b.copy_(v)
        hd = _pipnet_head(m, feats)
    return hd.proto, hd.pooled, hd.out


def _group_of(optimizer: torch.optim.Optimizer, param: Tensor) -> Optional[dict]:
    for g in optimizer.param_groups:
        if any(p is param for p in g["params"]):
            return g
    return None


def hip_adamw_step(optimizer: torch.optim.Optimizer, param: Tensor, grad: Tensor,
                   post: Optional[Tuple[float, float]] = None) -> bool:
    """``optimizer.step()`` restricted to ``param`` with torch.optim.AdamW's math, on the
    device; state tensors are created exactly as AdamW's ``_init_group`` does (CPU float32
    ``step``).  Returns False when ``param`` is not in any group (nothing to do)."""
    if not isinstance(optimizer, torch.optim.AdamW):
        raise RuntimeError(f"HIP finetune step implements torch.optim.AdamW, got {type(optimizer).__name__}")
    g = _group_of(optimizer, param)
    if g is None:
        return False
    if g.get("amsgrad", False) or g.get("maximize", False) or g.get("capturable", False):
        raise RuntimeError("HIP AdamW step: amsgrad / maximize / capturable groups are not supported")
    st = optimizer.state[param]
    if not st:
        st["step"] = torch.tensor(0.0, dtype=torch.float32)
        st["exp_avg"] = torch.zeros_like(param, memory_format=torch.preserve_format)
        st["exp_avg_sq"] = torch.zeros_like(param, memory_format=torch.preserve_format)
    st["step"] += 1
    beta1, beta2 = g["betas"]
    K.adamw_step_(param.detach(), grad, st["exp_avg"], st["exp_avg_sq"], float(g["lr"]), beta1, beta2,
                  float(g["eps"]), float(g["weight_decay"]), int(st["step"].item()), post)
    return True


# ------------------------------------------------------------------------------------------
# CountPIPNet head (count_pipnet.py:70-110) and its backward
# ------------------------------------------------------------------------------------------
def _count_tail(m: nn.Module, clamped: Tensor):
    """Intermediate layer and classifier of a CountPIPNet on the clamped counts: (activations the
    bilinear backward needs, classifier input, logits)."""
    from .count_pipnet import intermediate_hip
    from .count_pipnet_utils import BilinearIntermediate
    layer = m._intermediate
    saved = {}
    if isinstance(layer, BilinearIntermediate):
        e = K.linear(clamped, layer.embed.weight)
        u = K.linear(e, layer.W.weight)
        v = K.linear(e, layer.V.weight)
        inter = torch.empty_like(u)
        K.linear(e, layer.V.weight, epilogue=_lib.EPI_MUL, r=u, out=inter)
        saved.update(e=e, u=u, v=v)
    else:
        inter = intermediate_hip(layer, clamped)
    _, out = K.nonneg_linear(inter, m._classification.weight, m._classification.bias, None)
    return saved, inter, out


def _count_head(m: nn.Module, feats: Tensor, gumbel=None) -> _Head:
    """CountPIPNet.forward in train mode after the backbone: soft Gumbel-softmax / softmax map,
    spatial sums = raw counts, STE round and clamp, intermediate layer, classifier.  ``saved``
    keeps the head's temperature (``tau``) and the clamped counts with the tail's activations.
    ``gumbel(logits, act) -> (proto, sums)`` draws the Gumbel head's noise in place of the two forms
    below (dist_train: a rank's rows take the draw of their place in the global batch)."""
    from .count_pipnet_utils import GumbelSoftmax
    from .count_pipnet import _fresh_seed
    from .pipnet import add_on_activation, add_on_logits_hip
    act = add_on_activation(m._add_on)
    if isinstance(act, GumbelSoftmax):
        logits = add_on_logits_hip(m._add_on, feats, activation=GumbelSoftmax)
        noise = act.exp_noise
        if gumbel is not None:
            proto, sums = gumbel(logits, act)
        elif noise is not None:
            proto, sums = K.count_gumbel_soft(logits, act.tau, noise.to(device=logits.device,
                                                                        dtype=torch.float32).contiguous(), 0)
        else:
            proto, sums = K.count_gumbel_soft(logits, act.tau, None, _fresh_seed())   # fresh noise per call
        tau = float(act.tau)
    else:
        logits = add_on_logits_hip(m._add_on, feats, activation=nn.Softmax)
        proto, sums = K.softmax_pool(logits, pool_mode=1)
        tau = 1.0
    del logits
    # train mode: STE round in the forward only with use_ste (count_pipnet.py:90-97)
    counts, clamped = K.count_finish(None, sums, m._max_count, bool(m._use_ste))
    saved, inter, out = _count_tail(m, clamped)
    saved.update(tau=tau, clamped=clamped)
    return _Head(proto, counts, inter, out, saved)


def _count_train_forward(m: nn.Module, xs: Tensor, sd_keep: Dict[int, Tensor]):
    """CountPIPNet.forward(xs) in train mode on the HIP kernels: (proto NHWC, raw counts, clamped
    counts, the head's saved dict, classifier input, out)."""
    hd = _count_head(m, _backbone(m).train_forward(m._net, xs, None, sd_keep)[0])
    return hd.proto, hd.pooled, hd.saved["clamped"], hd.saved, hd.cls_in, hd.out


def _intermediate_backward(layer: nn.Module, x: Tensor, saved: dict, d_inter: Tensor,
                           need_dx: bool = False, param_grads: bool = True) -> Optional[Tensor]:
    """Parameter gradients of the intermediate layer (count_pipnet_utils.py:323-539) and, with
    ``need_dx``, the gradient w.r.t. its input x (the clamped counts) -- None where no gradient
    flows (a OneHotEncoder without STE: create_modified_encoding is not differentiable).
    ``param_grads=False``: the input gradient only, no parameter's .grad is touched."""
    from .count_pipnet_utils import (BilinearIntermediate, IdentityIntermediate, LinearFull, LinearIntermediate,
                                     OneHotEncoder)
    if isinstance(layer, IdentityIntermediate):
        return d_inter if need_dx else None
    if isinstance(layer, OneHotEncoder):
        if not (need_dx and layer.use_ste):
            return None
        return K.onehot_ste_backward(x, d_inter, layer.positive_grad_strategy, layer.respect_active_grad)
    if isinstance(layer, LinearFull):
        w = layer.linear.weight
        if param_grads and w.requires_grad:
            _set_grad(w, K.wgrad(d_inter, x))
        if param_grads and layer.linear.bias is not None and layer.linear.bias.requires_grad:
            _set_grad(layer.linear.bias, K.colsum(d_inter))
        return K.linear(d_inter, w.detach().t().contiguous(), None, _lib.EPI_NONE) if need_dx else None
    if isinstance(layer, LinearIntermediate):
        w = layer.linear.weight
        if not ((param_grads and w.requires_grad) or need_dx):
            return None
        dx, dw = K.linear_intermediate_backward(x, d_inter, w, want_dx=need_dx)
        if param_grads and w.requires_grad:
            _set_grad(w, dw.view_as(w))
        return dx
    if isinstance(layer, BilinearIntermediate):
        e, u, v = saved["e"], saved["u"], saved["v"]
        du, dv = K.bilinear_bwd_prep(d_inter, u, v)
        if param_grads and layer.W.weight.requires_grad:
            _set_grad(layer.W.weight, K.wgrad(du, e))
        if param_grads and layer.V.weight.requires_grad:
            _set_grad(layer.V.weight, K.wgrad(dv, e))
        if not ((param_grads and layer.embed.weight.requires_grad) or need_dx):
            return None
        de = K.linear(du, layer.W.weight.detach().t().contiguous())
        ones = torch.ones(de.shape[1], device=de.device)
        K.linear(dv, layer.V.weight.detach().t().contiguous(), None, _lib.EPI_RESID, scale=ones, r=de, out=de)
        if param_grads and layer.embed.weight.requires_grad:
            _set_grad(layer.embed.weight, K.wgrad(de, x))
        return K.linear(de, layer.embed.weight.detach().t().contiguous(), None, _lib.EPI_NONE) if need_dx else None
    raise NotImplementedError(f"HIP count training: no backward for {type(layer).__name__}")


def _count_head_backward(m: nn.Module, hd: _Head, d_out: Optional[Tensor], w_align: float, w_tanh: float,
                         tanh_loss_coeff: float, to_logits: bool,
                         pooled_all: Optional[Tensor] = None) -> Optional[Tensor]:
    """Backward below the classifier: intermediate layer (parameter gradients; ModifiedSTE for a
    one-hot encoder) and, with ``to_logits``, on through ClampSTE / STE_Round -> d counts (+ the
    tanh term) -> d proto (+ the align term) -> soft-max backward scaled by 1 / tau.  Without it
    the intermediate layer runs only when one of its parameters trains, and nothing comes back."""
    layer = m._intermediate
    d_counts = None
    if d_out is not None and (to_logits or any(p.requires_grad for p in layer.parameters())):
        d_inter = K.nonneg_linear_dx(d_out, m._classification.weight.detach())
        d_clamped = _intermediate_backward(layer, hd.saved["clamped"], hd.saved, d_inter, need_dx=to_logits)
        if d_clamped is not None:
            d_counts = K.count_ste_backward(hd.pooled, d_clamped, m._max_count, bool(m._use_ste),
                                            not m._is_clamp_backward_identity or not m._use_ste)
    if not to_logits:
        return None
    return K.count_head_backward(hd.proto, hd.pooled, d_counts, w_align, w_tanh, tanh_loss_coeff, hd.saved["tau"],
                                 counts_all=pooled_all)


# ------------------------------------------------------------------------------------------
# Pretrain / joint phases: a trainable backbone suffix + add-on (+ classifier) on the HIP
# kernels (main.py:238-256 pretrain, :377-390 "train + freeze params")
# ------------------------------------------------------------------------------------------
def _addon_backward(m: nn.Module, feats: Tensor, d_logits: Tensor, param_grads: bool = True) -> Tensor:
    """Backward from d logits (before the prototype softmax) through the add-on (1x1 conv when
    present) -> d features, the backbone's ``backward`` to take on; the conv's weight and bias get
    their .grad.  ``param_grads=False``: the input gradient only -- no weight-gradient kernel, no .grad."""
    mods = list(m._add_on) if isinstance(m._add_on, nn.Sequential) else [m._add_on]
    if len(mods) != 2:                           # no 1x1 prototype conv before the softmax
        return d_logits
    conv = mods[0]
    bsz, hh, ww, cf = feats.shape
    pn = conv.out_channels
    dl = d_logits.view(-1, pn)
    if param_grads and conv.weight.requires_grad:
        _set_grad(conv.weight, K.wgrad(dl, feats.view(-1, cf)))
    if param_grads and conv.bias is not None and conv.bias.requires_grad:
        _set_grad(conv.bias, K.colsum(dl))
    dy = K.linear(dl, conv.weight.detach().view(pn, cf).t().contiguous(), None, _lib.EPI_NONE)
    return dy.view(bsz, hh, ww, cf)


# ------------------------------------------------------------------------------------------
# the iteration: one step for both models and every phase
# ------------------------------------------------------------------------------------------
def _loss_weights(pretrain: bool, epoch: int = 0, nr_epochs: int = 1) -> Tuple[float, float, float]:
    """(align, tanh, class) loss weights of an iteration (train.py:45-61)."""
    return (epoch / nr_epochs, 5.0, 0.0) if pretrain else FINETUNE_LOSS_WEIGHTS


def _step_optimizers(m: nn.Module, optimizer_classifier, optimizer_net, enforce_weight_sparsity: bool) -> None:
    """Device AdamW for every parameter with a .grad in optimizer_classifier (train.py:117-120)
    and in optimizer_net (train.py:122-124) -- None: the phase does not step that one -- then the
    sparsity clamps (train.py:131-140; not in pretrain, where the classifier optimizer rests).
    The classifier weight's and bias's clamps ride on their AdamW launch; one that no such
    launch clamped is clamped on its own, as the reference clamps whatever the optimizers did."""
    cls = m._classification
    clamped = set()
    if optimizer_classifier is not None:
        for g in optimizer_classifier.param_groups:
            for p in g["params"]:
                if p.grad is not None:
                    post = None
                    if enforce_weight_sparsity:
                        post = (SPARSITY_DELTA, 0.0) if p is cls.weight else (0.0, 0.0) if p is cls.bias else None
                    hip_adamw_step(optimizer_classifier, p, p.grad, post)
                    clamped.add(id(p))
    if optimizer_net is not None:
        for g in optimizer_net.param_groups:
            for p in g["params"]:
                if p.grad is not None:
                    hip_adamw_step(optimizer_net, p, p.grad)
    if optimizer_classifier is not None and enforce_weight_sparsity:
        if id(cls.weight) not in clamped:
            K.weight_sparsify_(cls.weight.detach(), SPARSITY_DELTA)
        if cls.bias is not None and id(cls.bias) not in clamped:
            K.clamp_min_(cls.bias.detach(), 0.0)
        K.clamp_min_(cls.normalization_multiplier.detach(), 1.0)


def _classifier_grads(cls: nn.Module, hd: _Head, d_out: Optional[Tensor], finetune: bool) -> None:
    """.grad of the classifier's weight and bias from d loss / d out (None in pretrain: no class term)."""
    has_bias = cls.bias is not None
    if d_out is not None and (finetune or cls.weight.requires_grad or (has_bias and cls.bias.requires_grad)):
        # db is only ever kept under requires_grad (_set_grad), so asking for it is a matter of cost alone:
        # the finetune steps have always skipped a frozen bias's column sum, the other phases compute it
        # whenever there is a bias; each phase goes on launching what it did
        want_bias = has_bias and (cls.bias.requires_grad or not finetune)
        dw, db = K.nonneg_linear_backward(d_out, hd.cls_in, cls.weight, want_bias)
        _set_grad(cls.weight, dw)
        if want_bias:
            _set_grad(cls.bias, db)


def _train_step(m: nn.Module, xs1: Tensor, xs2: Tensor, ys: Tensor, *, phase: str, optimizer_classifier,
                optimizer_net=None, w: Tuple[float, float, float], enforce_weight_sparsity: bool,
                tanh_loss_coeff: float = 1.0, sd_keep: Optional[Dict[int, Tensor]], generator, step_optimizers=True,
                shard=None):
    """One iteration of ``phase`` ("pretrain" | "train" | "finetune", also the loss kernel's mode):
    concatenate the views and draw the stochastic-depth masks; backbone, head and loss; classifier
    gradients; outside finetune the backward through head, add-on and the trainable suffix (whose
    activations the forward then kept); AdamW on the device and the sparsity clamps.
    ``shard`` (a ``dist_train.Shard``): the rows here are one rank's rows of a global batch, and ``sd_keep`` is
    the global batch's; None: they are the whole batch.  It is asked in five places, marked (1) .. (5)."""
    count, finetune = hasattr(m, "_max_count"), phase == "finetune"
    head_backward = _count_head_backward if count else _pipnet_head_backward
    cls, backbone = m._classification, _backbone(m)
    xs = torch.cat([xs1, xs2])
    if shard is not None:
        sd_keep = shard.masks(sd_keep)                                    # (1) the rank's rows of the global masks
    elif sd_keep is None:
        sd_keep = backbone.sd_masks(m._net, xs.shape[0], generator)
    w_align, w_tanh, w_class = w
    loss_args = (cls.normalization_multiplier, enforce_weight_sparsity, tanh_loss_coeff, w_align, w_tanh, w_class,
                 phase)
    with torch.no_grad():
        start = None if finetune else backbone.trainable_start(m._net)    # finetune keeps no activations
        feats, suffix = backbone.train_forward(m._net, xs, start, sd_keep)
        if count:                                                         # (2) the draw of the rows' global place
            hd = _count_head(m, feats, None if shard is None else shard.gumbel())
        else:
            hd = _pipnet_head(m, feats)
        if shard is None:
            (stats, d_out), pooled_all = K.train_loss(hd.proto, hd.pooled, hd.out, ys, *loss_args), None
        else:                                                             # (3) the loss on every rank's rows
            stats, d_out, pooled_all = shard.loss(hd, ys, loss_args)
        _classifier_grads(cls, hd, d_out, finetune)
        d_logits = head_backward(m, hd, d_out, w_align, w_tanh, tanh_loss_coeff, to_logits=not finetune,
                                 pooled_all=pooled_all)                   # (4)
        del hd
        if not finetune:
            backbone.backward(m._net, suffix, _addon_backward(m, feats, d_logits))
        if shard is not None:                                             # (5) the ranks' gradients, summed
            shard.reduce_gradients(phase, optimizer_classifier, optimizer_net)
        if step_optimizers:
            _step_optimizers(m, None if phase == "pretrain" else optimizer_classifier,
                             None if finetune else optimizer_net, enforce_weight_sparsity)
    return stats


def hip_finetune_step(net: nn.Module, xs1: Tensor, xs2: Tensor, ys: Tensor,
                      optimizer_classifier: torch.optim.Optimizer, enforce_weight_sparsity: bool = True,
                      sd_keep: Optional[Dict[int, Tensor]] = None,
                      generator: Optional[torch.Generator] = None) -> Tensor:
    """One finetune iteration on the device (no host sync).  Returns ``kernels.train_loss``'s
    stats: [align, tanh, class, loss, correct, w_align, w_tanh, w_class]."""
    return _train_step(_inner(net), xs1, xs2, ys, phase="finetune", optimizer_classifier=optimizer_classifier,
                       w=_loss_weights(False), enforce_weight_sparsity=enforce_weight_sparsity, sd_keep=sd_keep,
                       generator=generator)


def hip_count_finetune_step(net: nn.Module, xs1: Tensor, xs2: Tensor, ys: Tensor,
                            optimizer_classifier: torch.optim.Optimizer, enforce_weight_sparsity: bool = True,
                            tanh_loss_coeff: float = 1.0, sd_keep: Optional[Dict[int, Tensor]] = None,
                            generator: Optional[torch.Generator] = None) -> Tensor:
    """One CountPIPNet finetune iteration (train.py:75-140 with finetune=True,
    is_count_pipnet=True): train-mode forward (soft Gumbel head, stochastic depth), the loss
    kernel (loss = 2 * class; align / tanh over C * raw counts for logging), backward into the
    classifier and the intermediate layer, AdamW for every parameter the classifier optimizer
    holds (intermediate included when ``train_intermediate`` put it there), the sparsity clamps.
    Returns the loss-kernel stats without synchronising."""
    return _train_step(_inner(net), xs1, xs2, ys, phase="finetune", optimizer_classifier=optimizer_classifier,
                       w=_loss_weights(False), enforce_weight_sparsity=enforce_weight_sparsity,
                       tanh_loss_coeff=tanh_loss_coeff, sd_keep=sd_keep, generator=generator)


def hip_train_step(net: nn.Module, xs1: Tensor, xs2: Tensor, ys: Tensor, optimizer_net, optimizer_classifier,
                   pretrain: bool, epoch: int, nr_epochs: int, enforce_weight_sparsity: bool = True,
                   sd_keep: Optional[Dict[int, Tensor]] = None, generator: Optional[torch.Generator] = None,
                   step_optimizers: bool = True) -> Tensor:
    """One pretrain (``pretrain=True``) or joint iteration (train.py:75-140 with
    finetune=False) for a trainable backbone suffix: train-mode forward keeping the
    suffix's activations, the loss kernel, backward through head, add-on and suffix (every
    parameter with requires_grad gets its .grad), then optimizer_classifier (joint only)
    and optimizer_net steps (AdamW on the device) and the sparsity clamps.  Returns the
    loss-kernel stats without synchronising."""
    m = _inner(net)
    if trainable_suffix_start(m) >= _backbone(m).units(m._net):
        raise NotImplementedError("HIP training step: no trainable backbone parameter (use the finetune step)")
    return _train_step(m, xs1, xs2, ys, phase="pretrain" if pretrain else "train", optimizer_net=optimizer_net,
                       optimizer_classifier=optimizer_classifier, w=_loss_weights(pretrain, epoch, nr_epochs),
                       enforce_weight_sparsity=enforce_weight_sparsity, sd_keep=sd_keep, generator=generator,
                       step_optimizers=step_optimizers)


def hip_count_train_step(net: nn.Module, xs1: Tensor, xs2: Tensor, ys: Tensor, optimizer_net, optimizer_classifier,
                         pretrain: bool, epoch: int, nr_epochs: int, enforce_weight_sparsity: bool = True,
                         tanh_loss_coeff: float = 1.0, sd_keep: Optional[Dict[int, Tensor]] = None,
                         generator: Optional[torch.Generator] = None, step_optimizers: bool = True) -> Tensor:
    """One CountPIPNet pretrain (``pretrain=True``) or joint iteration (train.py:75-140 with
    is_count_pipnet=True, finetune=False): train-mode forward keeping the backbone suffix's
    activations (soft Gumbel-softmax / softmax head, spatial sums = raw counts, STE round and
    clamp, intermediate layer, classifier), the loss kernel (tanh over C * raw counts), then
    the backward: classifier -> intermediate (parameter and input gradients; ModifiedSTE for
    a one-hot encoder) -> ClampSTE / STE_Round -> d counts (+ the tanh term) -> d proto
    (+ the align term) -> soft-max backward scaled by 1/tau -> add-on -> suffix; AdamW steps
    and the sparsity clamps as ``hip_train_step``.  Returns the loss-kernel stats."""
    m = _inner(net)
    if trainable_suffix_start(m) >= _backbone(m).units(m._net):
        raise NotImplementedError("HIP count training step: no trainable backbone parameter (use the finetune step)")
    return _train_step(m, xs1, xs2, ys, phase="pretrain" if pretrain else "train", optimizer_net=optimizer_net,
                       optimizer_classifier=optimizer_classifier, w=_loss_weights(pretrain, epoch, nr_epochs),
                       enforce_weight_sparsity=enforce_weight_sparsity, tanh_loss_coeff=tanh_loss_coeff,
                       sd_keep=sd_keep, generator=generator, step_optimizers=step_optimizers)


# ------------------------------------------------------------------------------------------
# epoch loop (train.py:8-150 drop-in)
# ------------------------------------------------------------------------------------------
class HipEpoch:
    """Runs HIP training iterations back to back with all bookkeeping on the device.

    Per batch (view-1 images, view-2 images, labels): one device step, then the schedules
    advance as in the reference -- the classifier's CosineAnnealingWarmRestarts to the
    fractional epoch position (train.py:120, not in pretrain), the backbone's scheduler once
    per iteration (train.py:124-126, not in finetune).  The five running sums (align, tanh,
    class, loss, accuracy) live in one device vector; ``summary()`` is the single host read.
    ``world``: the batches are one rank's rows of ``world`` equal shards and ``step`` returns the global batch's
    stats (dist_train), so the accuracy is over ``world`` times the labels here."""

    TERMS = ("align", "tanh", "class")

    def __init__(self, step, weights: Tuple[float, float, float], track_acc: bool, world: int = 1):
        self.step, self.weights, self.track_acc, self.world = step, weights, track_acc, world
        self.sums: Optional[Tensor] = None
        self.count = 0
        self.lrs_class: list = []
        self.lrs_net: list = []

    def _add(self, stats: Tensor, labels: int) -> None:
        acc = stats[4:5] / float(2 * labels * self.world) if self.track_acc else torch.zeros_like(stats[4:5])
        row = torch.cat([stats[:4], acc]).double()
        self.sums = row if self.sums is None else self.sums.add_(row)
        self.count += 1

    def run(self, batches, optimizers, epoch: int, device, scheduler_classifier=None, scheduler_net=None) -> None:
        n_batches = len(batches)
        for pos, batch in enumerate(batches):
            a, b, labels = (t.to(device, non_blocking=True) for t in batch)
            for opt in optimizers:
                opt.zero_grad(set_to_none=True)
            self._add(self.step(a, b, labels), labels.shape[0])
            if scheduler_classifier is not None:
                scheduler_classifier.step((epoch - 1) + pos / n_batches)
                self.lrs_class.append(scheduler_classifier.get_last_lr()[0])
            if scheduler_net is not None:
                scheduler_net.step()
                self.lrs_net.append(scheduler_net.get_last_lr()[0])
            else:
                self.lrs_net.append(0.0)

    def summary(self) -> dict:
        vals = self.sums.cpu().tolist() if self.sums is not None else [0.0] * 5
        n = float(max(self.count, 1))
        info = {}
        for j, term in enumerate(self.TERMS):
            info[f"{term}_loss_raw"] = vals[j] / n
            info[f"{term}_loss_weighted"] = vals[j] / n * self.weights[j]
        info.update(train_accuracy=vals[4] / n, loss=vals[3] / n, lrs_net=list(self.lrs_net),
                    lrs_class=list(self.lrs_class))
        return info


_NO_HIP_STEP = ("count_pipnet_amd.train_pipnet: this configuration (phase / trainable parameters / device) has no HIP "
                "step; use the reference train_pipnet with these modules (torch autograd path)")
# (is_count_pipnet, finetune) -> the step, its predicate, what train_pipnet says where the predicate fails
_STEPS = {
    (False, True): (hip_finetune_step, hip_finetune_supported, _NO_HIP_STEP),
    (False, False): (hip_train_step, hip_train_supported, _NO_HIP_STEP),
    (True, True): (hip_count_finetune_step, hip_count_finetune_supported,
                   "count_pipnet_amd.train_pipnet: this CountPIPNet finetune setup has no HIP "
                   "step; run the reference train_pipnet with these modules"),
    (True, False): (hip_count_train_step, hip_count_train_supported,
                    "count_pipnet_amd.train_pipnet: this CountPIPNet training setup (ResNet "
                    "backbone or non-fp32 parameters) runs on the torch path"),
}


def train_pipnet(net, train_loader, optimizer_net, optimizer_classifier, scheduler_net, scheduler_classifier,
                 criterion, epoch, nr_epochs, device, is_count_pipnet=False, pretrain=False, finetune=False,
                 progress_prefix: str = "Train Epoch", enforce_weight_sparsity=True, tanh_loss_coeff=1.0,
                 generator: Optional[torch.Generator] = None, verbose: bool = False) -> dict:
    """Drop-in for train.py:8-150 (same arguments, same ``train_info`` keys; progress output
    reduced to one optional line) for a ConvNeXt or ResNet-50 PIP-Net and a ConvNeXt
    CountPIPNet: the finetune phase (``hip_finetune_step`` / ``hip_count_finetune_step``) and
    the pretrain / joint / "train everything" phases with a trainable backbone suffix
    (``hip_train_step`` / ``hip_count_train_step``).  Anything else (a trainable ResNet stem,
    an intermediate layer without a HIP backward, non-fp32 parameters) raises -- run the
    reference's own loop on these modules (torch autograd path)."""
    if pretrain and finetune:
        raise NotImplementedError("count_pipnet_amd.train_pipnet: pretrain and finetune are exclusive")
    count, finetune = bool(is_count_pipnet), bool(finetune)
    hip_step, supported, refusal = _STEPS[count, finetune]
    if not supported(net):
        raise NotImplementedError(refusal)
    args = (optimizer_classifier,) if finetune else (optimizer_net, optimizer_classifier, pretrain, epoch, nr_epochs)
    kwargs = dict(tanh_loss_coeff=tanh_loss_coeff) if count else {}

    def step(a, b, labels):
        return hip_step(net, a, b, labels, *args, enforce_weight_sparsity=enforce_weight_sparsity,
                        generator=generator, **kwargs)

    return _run_epoch(net, step, train_loader, optimizer_net, optimizer_classifier, scheduler_net, scheduler_classifier,
                      epoch, nr_epochs, device, pretrain, finetune,
                      say=f"[{progress_prefix} {epoch}] HIP" if verbose else None)


def _run_epoch(net, step, train_loader, optimizer_net, optimizer_classifier, scheduler_net, scheduler_classifier,
               epoch, nr_epochs, device, pretrain, finetune, world: int = 1, say: Optional[str] = None) -> dict:
    """The epoch of ``train_pipnet`` here and in ``dist_train`` once ``step(a, b, labels) -> stats`` is chosen:
    train mode, the classifier's ``requires_grad`` flag, ``HipEpoch`` (accuracy over ``world`` shards) with each
    optimizer once, ``train_info``; ``say``: the head of the one progress line, None for none."""
    net.train()
    _inner(net)._classification.requires_grad = not pretrain
    runner = HipEpoch(step, _loss_weights(pretrain, epoch, nr_epochs), track_acc=not pretrain, world=world)
    opts = [o for o in (optimizer_classifier, optimizer_net) if o is not None]
    opts = [o for i, o in enumerate(opts) if all(o is not q for q in opts[:i])]
    runner.run(train_loader, opts, epoch, device, None if pretrain else scheduler_classifier,
               None if finetune else scheduler_net)
    info = runner.summary()
    if say is not None:
        terms = ", ".join(f"{t}={info[t + '_loss_raw']:.4f}" for t in HipEpoch.TERMS)
        print(f"{say}: {runner.count} iterations, {terms}", flush=True)
    return info
