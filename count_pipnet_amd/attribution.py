"""Integrated-gradients pixel attribution, on the device -- ``util/interpret_idg.py`` with
``util/saliency_methods.py`` (IG, LeftIG, IDG).

The reference explains a prototype score (or a class logit) of one image by integrating the
score's input gradient along the straight path from a baseline to the image: 192 path images in
chunks of 16 through torch autograd, per prototype per image (interpret_idg.py:74-77, :101-135).
``attribute`` runs the same three methods with every step on the HIP kernels:

  path images (4-channel NHWC, one launch per chunk) -> eval-mode forward that keeps its activations
  (convnext_train.train_forward) -> add-on -> head (softmax + max-pool with arg-location / hard and soft
  Gumbel-softmax on one noise draw / softmax + sum) -> per target: upstream vector u -> head backward
  -> dx-only backward through add-on and backbone -> stem input gradient, written straight into the
  path's gradient store -> per-step coefficients (LeftIG cutoff included) and the path reduction.

The forward of a chunk runs once for all targets, only the backward repeats (IDG's second pass has
its own path per target).  IG and LeftIG never wait for the device; IDG reads the [T, S] scores of
its first pass once to lay out the second (``idg_schedule``, host).  Under ``torch_backend()``, or
for a CPU net, the same algorithm runs by torch autograd through the module's own forward.
Percentile normalisation and colouring of the maps: ``saliency.py``; plotting stays with the caller.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch
import torch.nn as nn
from torch import Tensor

from . import kernels as K
from .backend import _forced_torch, torch_backend
from .explain_forward import HostCopy, is_count, map_is_small, note_map, unwrap

METHODS = ("ig", "lig", "idg")
KINDS = ("prototype", "class")
LIG_ALPHA_STAR = K.LIG_ALPHA_STAR


@dataclass
class Attribution(HostCopy):
    """Result of ``attribute``; tensors stay on the net's device until ``.cpu()`` is asked for.
    T = targets, S = steps."""
    maps: Tensor          # [T, 3, H, W] float32: what IG / IDG return per target
    scores: Tensor        # [T, S] target value at each step of the gradient pass (the reference's logits)
    alphas: Tensor        # [T, S] path positions of the gradient pass
    weights: Tensor       # [T, S] per-step coefficient applied to the gradients
    cutoff: Tensor        # [T] int64 steps averaged: S unless lig


def idg_schedule(slopes: Tensor, steps: int, step_size: float) -> Tuple[Tensor, Tensor]:
    """IDG's second-pass layout (saliency_methods.py:188-238) from the first pass's slopes [S], on the
    host: (alphas [S], substep [S]).  The slopes are min-max normalised, entry 0 is zeroed, the rest
    is scaled to sum to S and truncated to whole step counts; the steps left over go, one each, to
    the largest values that truncated to 0; the intervals that got steps are laid end to end from 0,
    one uniform step wide each, and divided evenly among their steps.  Same dtype as ``slopes`` throughout (float32 as the reference runs it)."""
    s = slopes.detach().cpu()
    norm = (s - s.min()) / (s.max() - s.min())
    norm[0] = 0
    placed = (norm / norm.sum()) * steps
    counts = placed.to(torch.int32)
    left = int(steps - int(counts.sum()))
    rest = placed.clone()
    rest[counts != 0] = -1
    if left > 0:
        counts[torch.flip(torch.sort(rest)[1], dims=[0])[:left]] = 1
    alphas = torch.zeros(steps, dtype=s.dtype)
    substep = torch.zeros(steps, dtype=s.dtype)
    at, value = 0, 0
    for n in counts.tolist():
        if n != 0:
            alphas[at:at + n] = torch.linspace(value, value + step_size, n + 1, dtype=s.dtype)[:n]
            substep[at:at + n] = torch.tensor(float(n), dtype=s.dtype).reciprocal() * step_size   # torch's scalar / tensor
            at += n
            value += step_size          # an interval without steps does not advance the start (as the reference)
    return alphas, substep


def uniform_slopes(scores: Tensor) -> Tuple[Tensor, float]:
    """(slopes [S], step size) of IDG's first pass on the uniform alphas (saliency_methods.py:173-184)."""
    s = scores.detach().cpu()
    alphas = torch.linspace(0, 1, s.numel(), dtype=s.dtype)
    step = float(alphas[1] - alphas[0])
    slopes = torch.zeros_like(s)
    slopes[1:] = (s[1:] - s[:-1]) / step
    return slopes, step


def _check_args(m: nn.Module, x: Tensor, targets, kind: str, method: str, steps: int, batch_size: int):
    if method not in METHODS:
        raise ValueError(f"attribute: unknown method {method!r} (expected one of {METHODS})")
    if kind not in KINDS:
        raise ValueError(f"attribute: unknown kind {kind!r} (expected one of {KINDS})")
    if steps < 2:
        raise ValueError(f"attribute: steps must be at least 2, got {steps}")
    if batch_size < 1 or steps % batch_size != 0:
        raise ValueError(f"attribute: steps ({steps}) must be evenly divisible by batch_size ({batch_size})")
    if x.dim() == 4 and x.shape[0] == 1:
        x = x[0]
    if x.dim() != 3 or x.shape[0] != 3:
        raise ValueError(f"attribute: x must be one image [3,H,W] or [1,3,H,W], got {tuple(x.shape)}")
    targets = [int(t) for t in targets]
    n = m._num_prototypes if kind == "prototype" else m._classification.weight.shape[0]
    for t in targets:
        if not 0 <= t < n:
            raise ValueError(f"attribute: {kind} target {t} out of range 0..{n - 1}")
    if not targets:
        raise ValueError("attribute: no target given")
    return x, targets


def _hip_supported(m: nn.Module) -> Optional[str]:
    """None when the HIP path serves this net, else what stands in the way."""
    from . import convnext_train
    from .count_pipnet_utils import (BilinearIntermediate, IdentityIntermediate, LinearFull, LinearIntermediate,
                                     OneHotEncoder)
    if not convnext_train.supported(getattr(m, "_net", None)):
        return f"a {type(getattr(m, '_net', None)).__name__} backbone (ConvNeXt only)"
    if getattr(m._net, "hip_precision", "fp32") != "fp32":
        return f"the {m._net.hip_precision} build"
    if not all(p.dtype == torch.float32 for p in m.parameters()):
        return "non-float32 parameters"
    if is_count(m):
        if not isinstance(m._intermediate, (IdentityIntermediate, OneHotEncoder, LinearFull, LinearIntermediate,
                                            BilinearIntermediate)):
            return f"the intermediate layer {type(m._intermediate).__name__} (no HIP backward)"
    elif not (isinstance(m._pool, nn.Sequential) and isinstance(m._pool[0], nn.AdaptiveMaxPool2d)):
        return "a pooling layer other than AdaptiveMaxPool2d(1)"
    return None


def attribute(net, x: Tensor, targets: Sequence[int], *, kind: str = "prototype", method: str = "ig",
              steps: int = 192, batch_size: int = 16, baseline=0.0, exp_noise: Optional[Tensor] = None,
              seed: Optional[int] = None) -> Attribution:
    """IG (``method="ig"``), LeftIG (``"lig"``, alpha_star 0.9) or IDG (``"idg"``) maps of one image
    for T targets -- interpret_idg.py's ATTR_FUNC (:101-109) on its wrappers (:112-135).

    ``net``: a ConvNeXt PIP-Net / CountPIPNet (full or mid-layer, with or without the 1x1 add-on),
    bare, under ``.module`` or in a world-size-1 ShardedInference; it is put in eval mode, as the
    reference does (:178).  ``x``: one normalised image [3,H,W] or [1,3,H,W].  ``kind="prototype"``
    attributes the prototype score -- PIP-Net: ``pooled`` of ``net(x)`` (no presence clamp),
    CountPIPNet: the raw ``counts`` of ``net(x, inference=False)``; ``kind="class"`` attributes
    ``out[:, c]`` of the same forward.  ``baseline``: a float or an image.  With steps S the path is
    ``baseline + alpha_i (x - baseline)``, alphas = linspace(0, 1, S), run in chunks of ``batch_size``:

      ig   mean_i g_i * (x - baseline), g_i the target's gradient at path image i;
      lig  the mean of g[0:cutoff], cutoff = the first step whose score exceeds 0.9 max(score)
           (none: 1; 0 becomes 1);
      idg  a forward-only pass on the uniform alphas gives the score's slopes, ``idg_schedule`` lays
           the S steps out in proportion to them, a second pass takes gradients there:
           mean_i(g_i slope_i substep_i) * (x - baseline), slopes recomputed on the new spacing.

    A CountPIPNet in eval mode counts with the hard straight-through Gumbel-softmax: scores are
    hard counts, the gradient flows through the soft map.  Its noise: a fresh Philox key per call,
    or ``seed``; step i of pass k starts at Philox block (k S + i) h w P / 4, so the draw does not
    depend on ``batch_size``.  ``exp_noise`` [passes * S, P, h, w] injects Exp(1) draws in call
    order (the reference's, concatenated).

    On a ROCm device the call runs on the HIP kernels and, for ig / lig, never waits for the device;
    idg copies its first pass's scores to the host once.  A ResNet backbone, non-fp32 parameters or
    an intermediate layer without a HIP backward raise NotImplementedError there: run the call under
    ``backend.torch_backend()`` (torch autograd through the module's own forward, also the path of
    a CPU net).  Bad arguments raise ValueError (the reference prints and returns zeros).  No
    parameter's ``.grad`` or ``requires_grad`` changes; the call works with grad mode on or off."""
    m = unwrap(net, "attribute")
    x, targets = _check_args(m, x, targets, kind, method, int(steps), int(batch_size))
    steps, batch_size = int(steps), int(batch_size)
    m.eval()
    dev = next(m.parameters()).device
    if _forced_torch() or dev.type != "cuda":
        return _attribute_torch(m, x.to(dev), targets, kind, method, steps, batch_size, baseline, exp_noise, seed)
    why = _hip_supported(m)
    if why is not None:
        raise NotImplementedError(f"count_pipnet_amd.attribute: no HIP path for {why}; run the call under "
                                  "count_pipnet_amd.backend.torch_backend() (torch autograd path)")
    K.require_device(x, "input image")
    with torch.no_grad():
        return _attribute_hip(m, x.contiguous(), targets, kind, method, steps, batch_size, baseline, exp_noise, seed)


# ------------------------------------------------------------------------------------------
# torch autograd path (CPU nets, torch_backend(); the comparison path of tools/attr_bench.py)
# ------------------------------------------------------------------------------------------
def _gumbel_module(m: nn.Module):
    from .count_pipnet_utils import GumbelSoftmax
    from .pipnet import add_on_activation
    act = add_on_activation(m._add_on)
    return act if isinstance(act, GumbelSoftmax) else None


def _target_scores(m: nn.Module, pooled: Tensor, out: Tensor, kind: str, t: int) -> Tensor:
    return pooled[:, t] if kind == "prototype" else out[:, t]


def _torch_pass(m, x, base, alphas, targets, kind, batch_size, noise, want_grad):
    """One pass over the path at ``alphas`` [S] by the module's own forward: (scores [T,S],
    gradients [T,S,3,H,W] or None).  One forward per chunk, one backward per target."""
    steps, t_n = alphas.numel(), len(targets)
    diff = x - base
    scores = torch.zeros(t_n, steps, dtype=x.dtype, device=x.device)
    grads = torch.zeros((t_n, steps) + tuple(x.shape), dtype=x.dtype, device=x.device) if want_grad else None
    act = _gumbel_module(m)
    prev = act.exp_noise if act is not None else None
    try:
        for start in range(0, steps, batch_size):
            end = start + batch_size
            imgs = torch.add(base, torch.mul(alphas[start:end].view(-1, 1, 1, 1), diff))
            if noise is not None and act is not None:
                act.exp_noise = noise[start:end]
            with torch.set_grad_enabled(want_grad), torch_backend():
                imgs.requires_grad_(want_grad)
                _, pooled, out = m(imgs, inference=False)
                for i, t in enumerate(targets):
                    sc = _target_scores(m, pooled, out, kind, t)
                    scores[i, start:end] = sc.detach()
                    if want_grad and sc.requires_grad:
                        g = torch.autograd.grad(sc, imgs, grad_outputs=torch.ones_like(sc),
                                                retain_graph=i + 1 < t_n, allow_unused=True)[0]
                        if g is not None:
                            grads[i, start:end] = g
    finally:
        if act is not None:
            act.exp_noise = prev
    return scores, grads


def _attribute_torch(m, x, targets, kind, method, steps, batch_size, baseline, exp_noise, seed) -> Attribution:
    dt, dev = x.dtype, x.device
    x = x.detach()
    base = baseline.detach().to(device=dev, dtype=dt) if torch.is_tensor(baseline) else torch.full_like(x, float(baseline))
    diff = x - base
    t_n = len(targets)
    if exp_noise is not None:
        exp_noise = exp_noise.detach().to(device=dev, dtype=dt)
    state = None
    if seed is not None and exp_noise is None and _gumbel_module(m) is not None:
        state = torch.random.get_rng_state()
        torch.manual_seed(int(seed))
    try:
        uniform = torch.linspace(0, 1, steps, dtype=dt).to(dev)
        cutoff = torch.full((t_n,), steps, dtype=torch.int64, device=dev)
        if method == "idg":
            s1, _ = _torch_pass(m, x, base, uniform, targets, kind, batch_size,
                                None if exp_noise is None else exp_noise[:steps], False)
            maps, scores, alphas, weights = [], [], [], []
            for i, t in enumerate(targets):
                slopes, step = uniform_slopes(s1[i])
                a, sub = idg_schedule(slopes, steps, step)
                a, sub = a.to(dev), sub.to(dev)
                sc, g = _torch_pass(m, x, base, a, [t], kind, batch_size,
                                    None if exp_noise is None else exp_noise[steps:2 * steps], True)
                sl = torch.zeros(steps, dtype=dt, device=dev)
                sl[1:] = (sc[0, 1:] - sc[0, :-1]) / (a[1:] - a[:-1])
                gw = torch.mul(torch.mul(g[0], sl.view(-1, 1, 1, 1)), sub.view(-1, 1, 1, 1))
                maps.append(gw.mean(dim=0) * diff)
                scores.append(sc[0])
                alphas.append(a)
                weights.append(sl * sub / steps)
            return Attribution(torch.stack(maps), torch.stack(scores), torch.stack(alphas), torch.stack(weights),
                               cutoff)
        scores, grads = _torch_pass(m, x, base, uniform, targets, kind, batch_size, exp_noise, True)
        maps = torch.zeros((t_n,) + tuple(x.shape), dtype=dt, device=dev)
        weights = torch.zeros(t_n, steps, dtype=dt, device=dev)
        for i in range(t_n):
            cut = steps
            if method == "lig":
                thr = scores[i].max() * LIG_ALPHA_STAR
                above = torch.where(scores[i] > thr)[0]
                cut = int(above[0]) if above.numel() else 1
                cut = max(cut, 1)
            maps[i] = grads[i, :cut].mean(dim=0) * diff
            weights[i, :cut] = 1.0 / cut
            cutoff[i] = cut
        return Attribution(maps, scores, uniform.expand(t_n, steps).contiguous(), weights, cutoff)
    finally:
        if state is not None:
            torch.random.set_rng_state(state)


# ------------------------------------------------------------------------------------------
# HIP path
# ------------------------------------------------------------------------------------------
class _Chunk:
    """What one chunk's forward leaves for its backward passes."""
    __slots__ = ("feats", "saved", "soft", "loc", "mode", "tau", "pooled", "out", "counts", "clamped", "inter_saved",
                 "hw")


def _gumbel_heads(logits: Tensor, tau: float, noise: Optional[Tensor], seed: int, block0: int):
    """Hard histogram and soft map of one chunk on the same noise: (hist int32 [B,P], soft [B,h,w,P]).
    The chunk's first step starts at Philox block ``block0`` and step b at block0 + b h w P / 4; where
    h w P is no multiple of 4 that is exact only at one step per launch."""
    b, h, w, p = logits.shape
    per = h * w * p
    if noise is not None or per % 4 == 0 or b == 1:
        _, hist = K.count_gumbel(logits, tau, noise, seed, offset=block0)
        soft, _ = K.count_gumbel_soft(logits, tau, noise, seed, offset=block0)
        return hist, soft
    hists, softs = [], []
    for i in range(b):
        off = block0 + i * per // 4
        hists.append(K.count_gumbel(logits[i:i + 1], tau, None, seed, offset=off)[1])
        softs.append(K.count_gumbel_soft(logits[i:i + 1], tau, None, seed, offset=off)[0])
    return torch.cat(hists), torch.cat(softs)


def _chunk_forward(m, x, baseline, alpha: Tensor, noise: Optional[Tensor], seed: int, step0: int) -> _Chunk:
    """Eval-mode forward of the path images at ``alpha`` (a chunk) keeping the activations."""
    from .count_pipnet_utils import GumbelSoftmax
    from .pipnet import add_on_activation, add_on_logits_hip
    from .convnext_train import train_forward
    from .train import _count_tail
    ck = _Chunk()
    b = alpha.numel()
    images = K.attr_path_images(x, baseline, alpha)
    probe = x.unsqueeze(0)
    small = map_is_small(m, probe)
    # small maps: per-image GEMM plan, so that the bits do not depend on the chunk size (explain_forward.small_map)
    with K.per_image_gemm_plan(b if small is not False else 1):
        ck.feats, ck.saved = train_forward(m._net, None, 0, {}, eval_mode=True, nhwc4=images)
        act = add_on_activation(m._add_on)
        gumbel = isinstance(act, GumbelSoftmax)
        logits = add_on_logits_hip(m._add_on, ck.feats, activation=GumbelSoftmax if gumbel else nn.Softmax)
    _, h, w, p = logits.shape
    ck.hw = (h, w)
    note_map(m, probe, ck.hw)
    ck.loc = ck.counts = ck.clamped = ck.inter_saved = None
    if not is_count(m):
        ck.soft, ck.pooled, ck.loc = K.softmax_pool_argmax(logits, write_proto=True)
        ck.mode, ck.tau = 0, 1.0
        _, ck.out = K.nonneg_linear(ck.pooled, m._classification.weight, m._classification.bias, None)
        return ck
    ck.mode = 1
    if gumbel:
        ck.tau = float(act.tau)
        hist, ck.soft = _gumbel_heads(logits, ck.tau, noise, seed, step0 * (h * w * p) // 4)
        ck.counts, ck.clamped = K.count_finish(hist, None, m._max_count, bool(m._use_ste))
    else:
        ck.tau = 1.0
        ck.soft, sums = K.softmax_pool(logits, pool_mode=1)
        ck.counts, ck.clamped = K.count_finish(None, sums, m._max_count, bool(m._use_ste))
    ck.pooled = ck.counts
    with K.per_image_gemm_plan(b):             # one row per image: the logits do not see the chunk size
        ck.inter_saved, _, ck.out = _count_tail(m, ck.clamped)
    return ck


def _upstream(m, ck: _Chunk, kind: str, t: int) -> Tensor:
    """u [B,P] = d target / d pooled (PIP-Net) or d target / d raw counts (CountPIPNet)."""
    from .train import _intermediate_backward
    b, p = ck.pooled.shape
    dev = ck.pooled.device
    if kind == "prototype":
        u = torch.zeros((b, p), device=dev, dtype=torch.float32)
        u[:, t] = 1.0
        return u
    cls = m._classification
    if not is_count(m):
        return torch.relu(cls.weight.detach()[t]).expand(b, p).contiguous()
    d_out = torch.zeros((b, cls.weight.shape[0]), device=dev, dtype=torch.float32)
    d_out[:, t] = 1.0
    d_inter = K.nonneg_linear_dx(d_out, cls.weight.detach())
    d_clamped = _intermediate_backward(m._intermediate, ck.clamped, ck.inter_saved, d_inter, need_dx=True,
                                       param_grads=False)
    if d_clamped is None:                      # a one-hot encoder without STE passes no gradient
        return torch.zeros((b, p), device=dev, dtype=torch.float32)
    return K.count_ste_backward(ck.counts, d_clamped.contiguous(), m._max_count, bool(m._use_ste),
                                not m._is_clamp_backward_identity or not m._use_ste)


def _stem_dx(m, stem_saved, dy: Tensor, hw_image, out_rows: Tensor) -> None:
    """Stem LayerNorm backward, then the conv's input gradient into ``out_rows`` [B, ld]."""
    conv, ln = stem_saved.mod[0], stem_saved.mod[1]
    z = stem_saved.act["z"]
    b, h, w, c = z.shape
    scratch = torch.empty(2, c, device=z.device)
    dz = K.ln_backward(z.view(-1, c), dy.reshape(-1, c), ln.weight.detach(), scratch[0], scratch[1], want_dz=True)
    K.attr_stem_dx(dz.view(b, h, w, c), conv.weight.detach().contiguous(), hw_image[0], hw_image[1], out=out_rows)


def _chunk_backward(m, ck: _Chunk, kind: str, t: int, hw_image, out_rows: Tensor) -> None:
    from . import convnext_train
    from .train import _addon_backward
    u = _upstream(m, ck, kind, t)
    d_logits = K.attr_head_backward(ck.soft, u, ck.loc, ck.mode, ck.tau)
    dy = convnext_train.backward(m._net, ck.saved, _addon_backward(m, ck.feats, d_logits, False), param_grads=False)
    _stem_dx(m, ck.saved[0], dy, hw_image, out_rows)


def _scores_of(ck: _Chunk, kind: str, t: int) -> Tensor:
    return ck.pooled[:, t] if kind == "prototype" else ck.out[:, t]


def _attribute_hip(m, x, targets, kind, method, steps, batch_size, baseline, exp_noise, seed) -> Attribution:
    from .count_pipnet import _fresh_seed
    dev = x.device
    _, hh, ww = x.shape
    if hh < 4 or ww < 4:
        raise ValueError(f"attribute: the image must be at least 4 x 4, got {(hh, ww)}")
    t_n, n = len(targets), 3 * hh * ww
    ld = (n + 3) // 4 * 4                       # rows of the gradient store start 16-byte aligned
    if torch.is_tensor(baseline):
        if tuple(baseline.shape[-3:]) != (3, hh, ww) or baseline.numel() != n:
            raise ValueError(f"attribute: baseline image {tuple(baseline.shape)} vs image {tuple(x.shape)}")
        baseline = baseline.detach().to(device=dev, dtype=torch.float32).reshape(3, hh, ww).contiguous()
    else:
        baseline = float(baseline)
    gumbel = _gumbel_module(m) is not None
    if exp_noise is not None and gumbel:
        exp_noise = exp_noise.detach().to(device=dev, dtype=torch.float32).contiguous()
        need = (2 if method == "idg" else 1) * steps
        if exp_noise.dim() != 4 or exp_noise.shape[0] < need:
            raise ValueError(f"attribute: exp_noise must be [{need}, P, h, w], got {tuple(exp_noise.shape)}")
    else:
        exp_noise = None
    key = 0
    if gumbel and exp_noise is None:
        key = int(seed) if seed is not None else _fresh_seed()

    def noise(step0: int, count: int):
        return None if exp_noise is None else exp_noise[step0:step0 + count]

    uniform = torch.linspace(0, 1, steps, dtype=torch.float32).to(dev, non_blocking=True)   # the host's linspace bits
    scores = torch.empty((t_n, steps), device=dev, dtype=torch.float32)
    grads = torch.empty((t_n, steps, ld), device=dev, dtype=torch.float32)
    weights = torch.empty((t_n, steps), device=dev, dtype=torch.float32)
    cutoff = torch.empty((t_n,), device=dev, dtype=torch.int64)
    maps = torch.empty((t_n, 3, hh, ww), device=dev, dtype=torch.float32)
    alphas = uniform.expand(t_n, steps).contiguous()
    substep = None
    if method == "idg":
        first = torch.empty((t_n, steps), device=dev, dtype=torch.float32)
        for start in range(0, steps, batch_size):           # pass 1: forward only, all targets at once
            ck = _chunk_forward(m, x, baseline, uniform[start:start + batch_size], noise(start, batch_size), key, start)
            for i, t in enumerate(targets):
                first[i, start:start + batch_size] = _scores_of(ck, kind, t)
            del ck
        first_host = first.cpu()                             # the one wait of the call
        lay = []
        for i in range(t_n):
            slopes, step = uniform_slopes(first_host[i])
            lay.append(idg_schedule(slopes, steps, step))
        alphas = torch.stack([a for a, _ in lay]).to(dev)
        substep = torch.stack([s for _, s in lay]).to(dev)
        for i, t in enumerate(targets):                      # pass 2: every target has its own path
            for start in range(0, steps, batch_size):
                ck = _chunk_forward(m, x, baseline, alphas[i, start:start + batch_size],
                                    noise(steps + start, batch_size), key, steps + start)
                scores[i, start:start + batch_size] = _scores_of(ck, kind, t)
                _chunk_backward(m, ck, kind, t, (hh, ww), grads[i, start:start + batch_size])
                del ck
    else:
        for start in range(0, steps, batch_size):            # one forward per chunk, one backward per target
            ck = _chunk_forward(m, x, baseline, uniform[start:start + batch_size], noise(start, batch_size), key, start)
            for i, t in enumerate(targets):
                scores[i, start:start + batch_size] = _scores_of(ck, kind, t)
                _chunk_backward(m, ck, kind, t, (hh, ww), grads[i, start:start + batch_size])
            del ck
    for i in range(t_n):
        K.attr_path_weights(scores[i], method, None if substep is None else alphas[i],
                            None if substep is None else substep[i], out=(weights[i], cutoff[i]))
        K.attr_path_reduce(grads[i], weights[i], x, baseline, out=maps[i])
    return Attribution(maps, scores, alphas, weights, cutoff)
