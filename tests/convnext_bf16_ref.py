"""CPU restatement of the plain bf16 ConvNeXt build (set_hip_dtype(net, "bf16")).

``oracle/ref_cpu.convnext_features`` with the build's four roundings and RNE-bf16 weights
(include/pipnet_amd.h, pipnet_conv2d_nhwc_bf16_mix):

* stem: fp32, unchanged; the residual stream stays fp32;
* CNBlock: dwconv7 + LayerNorm in fp32, rounded once to bf16 [1]; Linear1 = bf16 x RNE-bf16
  weights, fp32 accumulation, + fp32 bias, erf-GELU in fp32, rounded once to bf16 [2]; Linear2 =
  that x RNE-bf16 weights, fp32 accumulation, + fp32 bias, * fp32 layer_scale, + fp32 residual;
* downsample: LayerNorm2d in fp32, rounded once to bf16 [3]; the 2x2 conv with RNE-bf16 weights
  [4 = the weight rounding, shared by all three GEMM kinds], fp32 accumulation, fp32 bias and output;
* everything after the backbone (add-on conv, heads, classifier) is the fp32 oracle's.

bf16 values are carried as fp32 tensors holding bf16-representable numbers, so torch's fp32 CPU
kernels do the fp32-accumulated products.  TEST INFRASTRUCTURE ONLY, like the oracle itself.
"""
from __future__ import annotations

from typing import Dict

import torch
import torch.nn.functional as F

from oracle import ref_cpu

Tensor = torch.Tensor


def bf(x: Tensor) -> Tensor:
    """Round to nearest even to bf16, kept as fp32."""
    return x.to(torch.bfloat16).to(torch.float32)


def convnext_features_bf16(x: Tensor, sd: Dict[str, Tensor], prefix: str, net: str = "convnext_tiny_26",
                           use_mid_layers: bool = False, num_stages: int = 2) -> Tensor:
    p = prefix + "features."
    x = F.conv2d(x, sd[p + "0.0.weight"], sd[p + "0.0.bias"], stride=4)
    x = ref_cpu._ln2d(x, sd[p + "0.1.weight"], sd[p + "0.1.bias"])
    last = 7 if not use_mid_layers else min(num_stages, 7)
    idx = 1
    for cin, cout, n in ref_cpu.CONVNEXT_TINY:
        if idx > last:
            break
        for j in range(n):
            q = f"{p}{idx}.{j}."
            y = F.conv2d(x, sd[q + "block.0.weight"], sd[q + "block.0.bias"], padding=3, groups=cin)
            y = y.permute(0, 2, 3, 1)
            y = bf(F.layer_norm(y, (cin,), sd[q + "block.2.weight"], sd[q + "block.2.bias"], ref_cpu.LN_EPS))
            y = F.linear(y, bf(sd[q + "block.3.weight"])) + sd[q + "block.3.bias"]
            y = bf(F.gelu(y))
            y = F.linear(y, bf(sd[q + "block.5.weight"])) + sd[q + "block.5.bias"]
            y = y.permute(0, 3, 1, 2)
            x = sd[q + "layer_scale"] * y + x
        idx += 1
        if cout is None or idx > last:
            break
        q = f"{p}{idx}."
        x = bf(ref_cpu._ln2d(x, sd[q + "0.weight"], sd[q + "0.bias"]))
        x = F.conv2d(x, bf(sd[q + "1.weight"]), None, stride=ref_cpu.downsample_stride(net, cin)) \
            + sd[q + "1.bias"].view(1, -1, 1, 1)
        idx += 1
    return x


def backbone_bf16(x: Tensor, sd: Dict[str, Tensor], cfg) -> Tensor:
    """ref_cpu.backbone for the bf16 ConvNeXt build."""
    if "convnext" not in cfg.net:
        raise ValueError(f"convnext_bf16_ref: {cfg.net} is not a ConvNeXt backbone")
    return convnext_features_bf16(x, sd, "_net.", cfg.net, getattr(cfg, "use_mid_layers", False),
                                  getattr(cfg, "num_stages", 2))


def pre_head_logits(feats: Tensor, sd: Dict[str, Tensor], cfg) -> Tensor:
    """The head's input: backbone features through the optional fp32 1x1 add-on conv."""
    if getattr(cfg, "num_features", 0):
        feats = F.conv2d(feats, sd["_add_on.0.weight"], sd["_add_on.0.bias"])
    return feats


def pipnet_head(logits: Tensor, sd: Dict[str, Tensor]):
    """(raw pooled, inference logits) of the PIP-Net head over pre-head logits (ref_cpu.pipnet_forward)."""
    raw = torch.softmax(logits, dim=1).amax(dim=(2, 3))
    out = ref_cpu.non_neg_linear(torch.where(raw < 0.1, torch.zeros_like(raw), raw),
                                 sd["_classification.weight"], sd.get("_classification.bias"))
    return raw, out
