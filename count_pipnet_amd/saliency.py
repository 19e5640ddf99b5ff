"""Attribution maps to saliency images, on the device -- the second half of ``util/interpret_idg.py``.

``attribution.attribute`` returns the raw [T,3,H,W] maps of IG / LeftIG / IDG.  The reference goes on, in numpy on
the host: it picks the prototypes that matter for the image (:319-378), folds each map to 2-D (:413-415),
normalises it by a percentile with two fallbacks (``normalize_attribution_map``, :183-204), adds the maps into one
coloured overlay with a max-alpha channel (:419-427, :454-457), un-normalises the input image (:442-446) and, in
logit mode, writes the ``Blues``-coloured map (:626-641).  This module takes the maps to those pixels without
leaving the device:

  maps -> abs-sum over the channels -> per map: exact min / max / percentile (a radix select, one workgroup per
  map) -> rule + clip((x - vmin) / den, 0, 1) -> float64 colour blend / byte colour map; image -> clip(x std + mean)

Every stage is bitwise what the reference's numpy (2.2.6) / torch statements give on the same input.  Under
``backend.torch_backend()``, and for CPU tensors and nets, the same functions run plain torch operations with the
same results.  Figures, legends, titles, captum's ``blended_heat_map`` and PNG encoding stay with the caller.

Two statements about the reference as it runs under numpy 2.2.6, both restated here:
  * ``np.percentile`` of a float32 map computes in float32 throughout: q / 100, the virtual index
    (N - 1) * (q / 100), its fractional part gamma and the interpolation (``percentile_plan``);
  * ``denominator > 1e-3`` compares a float32 scalar with a Python float, that is with float32(1e-3).
One departure: logit mode divides by zero where the percentile equals the minimum; that map is rule 2 (zeros) here.
The select orders -0.0 below +0.0 (numpy leaves the order of equal values open); its value for a map that holds
NaN is unspecified (numpy gives NaN) -- the folded maps of this module are sums of absolute values.
"""
from __future__ import annotations

import contextlib
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import kernels as K
from .attribution import Attribution, attribute
from .backend import _forced_torch, torch_backend
from .explain_forward import HostCopy, is_count, unwrap

# plotly.express.colors.qualitative.Plotly (interpret_idg.py:386), reused modulo its length (:420)
PLOTLY_QUALITATIVE = ["#636EFA", "#EF553B", "#00CC96", "#AB63FA", "#FFA15A", "#19D3F3", "#FF6692", "#B6E880", "#FF97FF",
                      "#FECB52"]
IMAGENET_MEAN = (0.485, 0.456, 0.406)           # interpret_idg.py:442-443
IMAGENET_STD = (0.229, 0.224, 0.225)
RULE_PERCENTILE, RULE_GLOBAL_MAX, RULE_ZERO = 0, 1, 2
MIN_PERCENTILE_RANGE = 1e-3                     # interpret_idg.py:193, compared as float32
MIN_GLOBAL_RANGE = 1e-5                         # interpret_idg.py:200


@dataclass
class SaliencyMaps(HostCopy):
    """Result of ``normalize_maps``; T = maps."""
    folded: Tensor        # [T, H, W] float32 sum over the channels of |map|
    vmin: Tensor          # [T] minimum of the folded map
    vq: Tensor            # [T] its percentile
    vtop: Tensor          # [T] its maximum
    rule: Tensor          # [T] int32: 0 percentile range, 1 global-max fallback, 2 zero map
    normalized: Tensor    # [T, H, W] float32 in [0, 1]


@dataclass
class ActivePrototypes(HostCopy):
    """Result of ``active_prototypes``."""
    indices: List[int]    # prototypes with contribution > threshold, largest contribution first
    contributions: Tensor  # [P] float32: score * weight of the target class, every prototype


@dataclass
class PrototypeSaliency(HostCopy):
    """Result of ``interpret_prototypes``; the tensor fields are None when no prototype is active."""
    active: ActivePrototypes
    attribution: Optional[Attribution]
    saliency: Optional[SaliencyMaps]
    overlay: Optional[Tensor]       # [H, W, 4] float64 RGBA
    image: Optional[Tensor]         # [H, W, 3] float32 in [0, 1]

    def cpu(self):
        def host(v):
            return v if v is None else v.cpu()
        return PrototypeSaliency(self.active.cpu(), host(self.attribution), host(self.saliency), host(self.overlay),
                                 host(self.image))


@dataclass
class LogitSaliency(HostCopy):
    """Result of ``interpret_logit``."""
    attribution: Attribution
    saliency: SaliencyMaps
    image: Tensor                   # [H, W, 3] float32 in [0, 1]
    rgba: Optional[Tensor]          # [H, W, 4] uint8 with a ``lut``

    def cpu(self):
        return LogitSaliency(self.attribution.cpu(), self.saliency.cpu(), self.image.cpu(),
                             None if self.rgba is None else self.rgba.cpu())


def palette_colours(count: int) -> Tensor:
    """[count, 3] float64 host tensor: the hex triples of ``PLOTLY_QUALITATIVE`` / 255.0, reused modulo ten."""
    rows = []
    for i in range(count):
        code = PLOTLY_QUALITATIVE[i % len(PLOTLY_QUALITATIVE)]
        rows.append([int(code[1:3], 16) / 255.0, int(code[3:5], 16) / 255.0, int(code[5:7], 16) / 255.0])
    return torch.tensor(rows, dtype=torch.float64).reshape(count, 3)


def percentile_plan(n: int, percentile: float) -> Tuple[int, float]:
    """(k, gamma): np.percentile's split of its virtual index for a float32 array of ``n`` values, as numpy 2.2.6
    computes it -- in float32: q = float32(percentile) / float32(100), index = float32(n - 1) * q, k = floor(index),
    gamma = index - k.  At or past the last element numpy takes the last value for both neighbours and leaves
    gamma = index + 1; the interpolation of two equal values ignores it."""
    q = np.float32(percentile) / np.float32(100)
    index = np.float32(n - 1) * q
    if index >= np.float32(n - 1):
        return n - 1, float(np.float32(np.float64(index) + 1.0))
    k = int(np.floor(index))
    return k, float(np.float32(np.float64(index) - k))


def _hip(t: Tensor) -> bool:
    return t.is_cuda and not _forced_torch()


def _check_percentile(percentile) -> float:
    p = float(percentile)
    if not 0.0 <= p <= 100.0:
        raise ValueError(f"saliency: percentile must lie in [0, 100], got {percentile}")
    return p


def _fold_torch(maps: Tensor) -> Tensor:
    return (maps[:, 0].abs() + maps[:, 1].abs()) + maps[:, 2].abs()


def _order_stats_torch(folded: Tensor, k: int, gamma: float):
    t = folded.shape[0]
    s = torch.sort(folded.reshape(t, -1), dim=1).values
    lo, hi = s[:, k], s[:, min(k + 1, s.shape[1] - 1)]
    g = torch.tensor(gamma, dtype=torch.float32, device=folded.device)
    d = hi - lo
    vq = torch.add(hi, -torch.mul(d, 1 - g)) if gamma >= 0.5 else torch.add(lo, torch.mul(d, g))
    return s[:, 0].contiguous(), s[:, -1].contiguous(), lo.contiguous(), hi.contiguous(), vq


def _normalize_torch(folded: Tensor, vmin: Tensor, vq: Tensor, vtop: Tensor, fallback: bool):
    dev = folded.device
    den = vq - vmin
    if fallback:
        first = den > torch.tensor(MIN_PERCENTILE_RANGE, dtype=torch.float32, device=dev)
        den2 = vtop - vmin
        second = den2 > torch.tensor(MIN_GLOBAL_RANGE, dtype=torch.float32, device=dev)
        rule = torch.where(first, 0, torch.where(second, 1, 2)).to(torch.int32)
        den = torch.where(first, den, den2)
    else:
        rule = torch.where(vq == vmin, 2, 0).to(torch.int32)
    zero = (rule == RULE_ZERO).view(-1, 1, 1)
    safe = torch.where(rule == RULE_ZERO, torch.ones_like(den), den).view(-1, 1, 1)
    norm = torch.clamp((folded - vmin.view(-1, 1, 1)) / safe, 0, 1)
    return rule, torch.where(zero, torch.zeros_like(norm), norm)


def normalize_maps(maps: Tensor, percentile: float = 98.0, *, fallback: bool = True) -> SaliencyMaps:
    """Fold and normalise T attribution maps: interpret_idg.py:413-417 with ``normalize_attribution_map``
    (``fallback=True``), or logit mode :627-635 (``fallback=False``).

    ``maps``: float32 [T,3,H,W], or already folded [T,H,W]; on a ROCm device (HIP kernels, nothing waits) or on
    the CPU (torch).  Per map: folded = sum_c |map_c|; vmin, vtop; vq = np.percentile(folded, percentile) by exact
    selection; then ``clip((folded - vmin) / den, 0, 1)`` with den = vq - vmin where that is > 1e-3 (rule 0), else
    vtop - vmin where that is > 1e-5 (rule 1), else a zero map (rule 2) -- both tests in float32.  Without
    ``fallback`` den = vq - vmin, and a map whose percentile equals its minimum is rule 2.  T = 0 gives empty
    results."""
    if not torch.is_tensor(maps) or maps.dtype != torch.float32:
        raise ValueError(f"normalize_maps: maps must be a float32 tensor, got "
                         f"{maps.dtype if torch.is_tensor(maps) else type(maps).__name__}")
    if maps.dim() not in (3, 4) or (maps.dim() == 4 and maps.shape[1] != 3):
        raise ValueError(f"normalize_maps: maps must be [T,3,H,W] or [T,H,W], got {tuple(maps.shape)}")
    p = _check_percentile(percentile)
    t, h, w = maps.shape[0], maps.shape[-2], maps.shape[-1]
    if h * w < 1:
        raise ValueError(f"normalize_maps: empty maps {tuple(maps.shape)}")
    if h * w >= 1 << 31:
        raise ValueError(f"normalize_maps: {h * w} values per map; the select counts in 32 bits")
    maps = maps.detach()
    k, gamma = percentile_plan(h * w, p)
    if _hip(maps):
        maps = maps.contiguous()
        folded = K.saliency_abs_sum(maps) if maps.dim() == 4 else maps
        vmin, vtop, _, _, vq = K.saliency_order_stats(folded, k, gamma)
        rule, norm = K.saliency_normalize(folded, vmin, vq, vtop, fallback)
        return SaliencyMaps(folded, vmin, vq, vtop, rule, norm)
    folded = _fold_torch(maps) if maps.dim() == 4 else maps
    if t == 0:
        e = torch.empty(0, dtype=torch.float32, device=maps.device)
        return SaliencyMaps(folded, e, e.clone(), e.clone(), e.to(torch.int32), torch.empty_like(folded))
    vmin, vtop, _, _, vq = _order_stats_torch(folded, k, gamma)
    rule, norm = _normalize_torch(folded, vmin, vq, vtop, fallback)
    return SaliencyMaps(folded, vmin, vq, vtop, rule, norm)


def blend_maps(normalized: Tensor, colours: Optional[Tensor] = None) -> Tensor:
    """[H,W,4] float64 RGBA overlay of T normalised maps [T,H,W] (interpret_idg.py:419-427, :454-457): RGB =
    ``clip(sum_i colour_i * normalized_i, 0, 1)`` accumulated in float64 in the order i = 0 .. T-1, alpha =
    ``max_i normalized_i`` from 0.  ``colours`` [T,3] float64; default ``palette_colours(T)``."""
    if not torch.is_tensor(normalized) or normalized.dtype != torch.float32 or normalized.dim() != 3:
        raise ValueError("blend_maps: normalized must be a float32 [T,H,W] tensor")
    t, h, w = normalized.shape
    if h * w < 1:
        raise ValueError(f"blend_maps: empty maps {tuple(normalized.shape)}")
    if colours is None:
        colours = palette_colours(t)
    colours = torch.as_tensor(colours)
    if colours.dtype != torch.float64 or tuple(colours.shape) != (t, 3):
        raise ValueError(f"blend_maps: colours must be float64 [{t}, 3], got {colours.dtype} {tuple(colours.shape)}")
    normalized = normalized.detach()
    colours = colours.to(normalized.device).contiguous()
    if _hip(normalized):
        return K.saliency_blend(normalized.contiguous(), colours)
    rgb = torch.zeros((h, w, 3), dtype=torch.float64, device=normalized.device)
    alpha = torch.zeros((h, w, 1), dtype=torch.float64, device=normalized.device)
    for i in range(t):
        v = normalized[i].to(torch.float64).unsqueeze(-1)
        rgb = rgb + colours[i] * v
        alpha = torch.maximum(alpha, v)
    return torch.cat((torch.clamp(rgb, 0, 1), alpha), dim=-1)


def unnormalize_image(x: Tensor, mean: Sequence[float] = IMAGENET_MEAN, std: Sequence[float] = IMAGENET_STD) -> Tensor:
    """[H,W,3] float32 ``clip(x * std + mean, 0, 1)`` of one normalised image [3,H,W] or [1,3,H,W]
    (interpret_idg.py:442-446); the product and the sum are two float32 roundings, as torch's two operations."""
    if not torch.is_tensor(x) or x.dtype != torch.float32:
        raise ValueError("unnormalize_image: x must be a float32 tensor")
    if x.dim() == 4 and x.shape[0] == 1:
        x = x[0]
    if x.dim() != 3 or x.shape[0] != 3 or x.shape[1] * x.shape[2] < 1:
        raise ValueError(f"unnormalize_image: x must be one image [3,H,W] or [1,3,H,W], got {tuple(x.shape)}")
    mean, std = [float(v) for v in mean], [float(v) for v in std]
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("unnormalize_image: mean and std must hold three values each")
    x = x.detach()
    if _hip(x):
        return K.saliency_unnormalize(x.contiguous(), mean, std)
    m = torch.tensor(mean, dtype=torch.float32, device=x.device).view(3, 1, 1)
    s = torch.tensor(std, dtype=torch.float32, device=x.device).view(3, 1, 1)
    return torch.clamp(torch.add(torch.mul(x, s), m).permute(1, 2, 0), 0, 1).contiguous()


def colormap_rgba8(normalized: Tensor, lut: Tensor) -> Tensor:
    """[..., 4] uint8: entry ``min(int(v * 256), 255)`` of the byte table ``lut`` (uint8 [256,4]) for every value
    v in [0, 1] -- what ``plt.imsave(..., cmap=...)`` writes for a map whose minimum is 0 and maximum is 1
    (identity Normalize, ``xa *= N``, ``xa[xa == N] = N - 1``, truncation, byte LUT).  The caller passes the table,
    e.g. ``(matplotlib.colormaps["Blues"]._lut[:256] * 255).astype(np.uint8)``."""
    if not torch.is_tensor(normalized) or normalized.dtype != torch.float32:
        raise ValueError("colormap_rgba8: normalized must be a float32 tensor")
    if not torch.is_tensor(lut) or lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 4):
        raise ValueError("colormap_rgba8: lut must be a uint8 [256,4] tensor")
    normalized = normalized.detach()
    lut = lut.to(normalized.device).contiguous()
    if _hip(normalized):
        return K.saliency_colormap_rgba8(normalized.contiguous(), lut)
    idx = torch.clamp(torch.mul(normalized, 256.0), 0, 255).to(torch.int64)
    return lut[idx]


def _one_image(x: Tensor, what: str) -> Tensor:
    if x.dim() == 4 and x.shape[0] == 1:
        x = x[0]
    if x.dim() != 3 or x.shape[0] != 3:
        raise ValueError(f"{what}: x must be one image [3,H,W] or [1,3,H,W], got {tuple(x.shape)}")
    return x


def active_prototypes(net, x: Tensor, target_class: int, threshold: float = 0.1, *,
                      exp_noise: Optional[Tensor] = None) -> ActivePrototypes:
    """The prototypes that matter for class ``target_class`` of one image (interpret_idg.py:319-378).

    PIP-Net: ``pooled`` of ``net(x)`` (no presence clamp) times the raw row ``_classification.weight[target_class]``.
    CountPIPNet: the clamped counts of ``net(x, inference=True)`` times the row of ``local.count_importance_matrix``
    (with the one-hot encoding of the counts as scalars when the intermediate layer is a OneHotEncoder).  Entries
    ``> threshold`` are kept, largest contribution first; equal contributions in ascending index order (the
    reference's ``argsort`` leaves ties open).  Torch operations on the net's device and one read of the index
    list, the only wait.  ``exp_noise`` [1,P,h,w] injects the Exp(1) draw of a Gumbel-softmax net's forward."""
    from .attribution import _gumbel_module
    from .count_pipnet_utils import OneHotEncoder
    from .local import count_importance_matrix
    m = unwrap(net, "active_prototypes")
    x = _one_image(x, "active_prototypes")
    kc = m._classification.weight.shape[0]
    c = int(target_class)
    if not 0 <= c < kc:
        raise ValueError(f"active_prototypes: target_class {target_class} out of range 0..{kc - 1}")
    m.eval()
    dev = next(m.parameters()).device
    xs = x.detach().to(dev).unsqueeze(0)
    forced = _forced_torch() or dev.type != "cuda"
    act = _gumbel_module(m)
    prev = act.exp_noise if act is not None else None
    try:
        if act is not None and exp_noise is not None:
            act.exp_noise = exp_noise.detach().to(device=dev, dtype=torch.float32)
        with torch.no_grad():
            if is_count(m):
                with torch_backend() if forced else contextlib.nullcontext():
                    _, clamped, _ = m(xs, inference=True)
                scalars = m._intermediate(clamped).squeeze(0) if isinstance(m._intermediate, OneHotEncoder) else None
                weight = count_importance_matrix(m, scalars).to(device=dev, dtype=torch.float32)
                contributions = clamped.squeeze(0) * weight[c]
            else:
                with torch_backend() if forced else contextlib.nullcontext():
                    _, pooled, _ = m(xs)
                contributions = pooled.squeeze(0) * m._classification.weight.detach()[c]
            keep = torch.where(contributions > threshold)[0]
            order = torch.sort(contributions[keep], descending=True, stable=True)[1]
            indices = keep[order].tolist()               # the one device-to-host read
    finally:
        if act is not None:
            act.exp_noise = prev
    return ActivePrototypes(indices, contributions)


def interpret_prototypes(net, x: Tensor, target_class: int, *, method: str = "ig", steps: int = 192,
                         batch_size: int = 16, baseline=0.0, threshold: float = 0.1, percentile: float = 98.0,
                         colours: Optional[Tensor] = None, exp_noise: Optional[Tensor] = None,
                         seed: Optional[int] = None, selection_noise: Optional[Tensor] = None) -> PrototypeSaliency:
    """interpret_idg.py's ``interpret_prototypes`` for one image, up to the pixels it plots: ``active_prototypes``,
    ``attribute(kind="prototype")`` on them, ``normalize_maps``, ``blend_maps`` and ``unnormalize_image``.

    Which nets the HIP path serves is ``attribute``'s decision, and its refusals are raised from there.  With no
    active prototype the result holds the selection only and nothing more is launched (the reference prints and
    returns).  ``exp_noise`` / ``seed``: ``attribute``'s; ``selection_noise``: ``active_prototypes``' ``exp_noise``.
    ``colours`` [T,3] float64 for the T active prototypes in their order; default the Plotly palette."""
    p = _check_percentile(percentile)
    x = _one_image(x, "interpret_prototypes")
    active = active_prototypes(net, x, target_class, threshold, exp_noise=selection_noise)
    if not active.indices:
        return PrototypeSaliency(active, None, None, None, None)
    if colours is not None:
        colours = torch.as_tensor(colours)
        if colours.dtype != torch.float64 or tuple(colours.shape) != (len(active.indices), 3):
            raise ValueError(f"interpret_prototypes: colours must be float64 [{len(active.indices)}, 3], got "
                             f"{colours.dtype} {tuple(colours.shape)}")
    attr = attribute(net, x, active.indices, kind="prototype", method=method, steps=steps, batch_size=batch_size,
                     baseline=baseline, exp_noise=exp_noise, seed=seed)
    sal = normalize_maps(attr.maps, p, fallback=True)
    overlay = blend_maps(sal.normalized, colours)
    image = unnormalize_image(x.detach().to(device=attr.maps.device, dtype=torch.float32))
    return PrototypeSaliency(active, attr, sal, overlay, image)


def interpret_logit(net, x: Tensor, target_class: int, *, method: str = "idg", steps: int = 192, batch_size: int = 16,
                    baseline=0.0, percentile: float = 99.0, lut: Optional[Tensor] = None,
                    exp_noise: Optional[Tensor] = None, seed: Optional[int] = None) -> LogitSaliency:
    """One image of interpret_idg.py's ``interpret_logits_for_dataset`` (:608-641): ``attribute(kind="class")``,
    ``normalize_maps(fallback=False)`` at the 99th percentile, ``unnormalize_image`` and, with a byte table
    ``lut`` (uint8 [256,4]), ``colormap_rgba8`` -- the pixels of ``plt.imsave(..., cmap=...)``."""
    p = _check_percentile(percentile)
    x = _one_image(x, "interpret_logit")
    if lut is not None and (not torch.is_tensor(lut) or lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 4)):
        raise ValueError("interpret_logit: lut must be a uint8 [256,4] tensor")
    attr = attribute(net, x, [int(target_class)], kind="class", method=method, steps=steps, batch_size=batch_size,
                     baseline=baseline, exp_noise=exp_noise, seed=seed)
    sal = normalize_maps(attr.maps, p, fallback=False)
    image = unnormalize_image(x.detach().to(device=attr.maps.device, dtype=torch.float32))
    rgba = None if lut is None else colormap_rgba8(sal.normalized[0], lut)
    return LogitSaliency(attr, sal, image, rgba)
