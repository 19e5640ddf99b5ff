"""CPU restatement of a training step's FROZEN ConvNeXt layers in plain bf16 (set_hip_train_dtype(net, "bf16")).

``oracle/ref_cpu.convnext_features`` in train mode (stochastic depth masks) where the first ``frozen`` entries of
``features`` run the plain bf16 build's arithmetic (tests/convnext_bf16_ref.py: dwconv7 + LayerNorm rounded once
to bf16, Linear1 on RNE-bf16 weights with fp32 accumulation, GELU rounded once to bf16, Linear2 likewise, the
downsample's LayerNorm rounded once and its conv on RNE-bf16 weights) and every later entry the fp32 oracle's.  The
residual update of a block is the device epilogue's (PIPNET_EPI_F32_RESID_ROWSCALE), in its multiplication order:

    x + rs_b * (layer_scale * y),   rs_b = keep_b / (1 - p)   (fp32; a block with p == 0: x + layer_scale * y)

``frozen`` counts ``features`` entries as ``convnext_train.trainable_start`` does (0 = the stem, which is fp32 in
every build): None = the whole backbone (the finetune phase), j = entries [0, j) (the frozen prefix of a pretrain /
joint step).  TEST INFRASTRUCTURE ONLY, like the oracle itself.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn.functional as F

from convnext_bf16_ref import bf
from oracle import ref_cpu

Tensor = torch.Tensor


def convnext_features_train_bf16(x: Tensor, sd: Dict[str, Tensor], prefix: str, net: str = "convnext_tiny_26",
                                 use_mid_layers: bool = False, num_stages: int = 2,
                                 sd_keep: Optional[Dict[int, Tensor]] = None, frozen: Optional[int] = None) -> Tensor:
    p = prefix + "features."
    x = F.conv2d(x, sd[p + "0.0.weight"], sd[p + "0.0.bias"], stride=4)
    x = ref_cpu._ln2d(x, sd[p + "0.1.weight"], sd[p + "0.1.bias"])
    last = 7 if not use_mid_layers else min(num_stages, 7)
    idx, bid = 1, -1

    def low(i):                                   # entry i runs the bf16 arithmetic
        return frozen is None or i < frozen

    def rnd(t, i):
        return bf(t) if low(i) else t

    for cin, cout, n in ref_cpu.CONVNEXT_TINY:
        if idx > last:
            break
        for j in range(n):
            bid += 1
            q = f"{p}{idx}.{j}."
            y = F.conv2d(x, sd[q + "block.0.weight"], sd[q + "block.0.bias"], padding=3, groups=cin)
            y = y.permute(0, 2, 3, 1)
            y = rnd(F.layer_norm(y, (cin,), sd[q + "block.2.weight"], sd[q + "block.2.bias"], ref_cpu.LN_EPS), idx)
            if low(idx):                          # fp32 accumulation, then the fp32 bias (the device epilogue)
                y = F.linear(y, bf(sd[q + "block.3.weight"])) + sd[q + "block.3.bias"]
                y = bf(F.gelu(y))
                y = F.linear(y, bf(sd[q + "block.5.weight"])) + sd[q + "block.5.bias"]
            else:                                 # the oracle's own calls
                y = F.gelu(F.linear(y, sd[q + "block.3.weight"], sd[q + "block.3.bias"]))
                y = F.linear(y, sd[q + "block.5.weight"], sd[q + "block.5.bias"])
            y = sd[q + "layer_scale"] * y.permute(0, 3, 1, 2)
            prob = ref_cpu.sd_drop_prob(bid)
            if sd_keep is not None and prob > 0.0:
                rs = torch.as_tensor(sd_keep[bid]).to(torch.float32) / (1.0 - prob)      # keep_b / (1 - p), fp32
                y = rs.view(-1, 1, 1, 1) * y
            x = x + y
        idx += 1
        if cout is None or idx > last:
            break
        q = f"{p}{idx}."
        x = rnd(ref_cpu._ln2d(x, sd[q + "0.weight"], sd[q + "0.bias"]), idx)
        stride = ref_cpu.downsample_stride(net, cin)
        if low(idx):
            x = F.conv2d(x, bf(sd[q + "1.weight"]), None, stride=stride) + sd[q + "1.bias"].view(1, -1, 1, 1)
        else:
            x = F.conv2d(x, sd[q + "1.weight"], sd[q + "1.bias"], stride=stride)
        idx += 1
    return x


def backbone_train_bf16(x: Tensor, sd: Dict[str, Tensor], cfg, sd_keep=None, frozen: Optional[int] = None) -> Tensor:
    """ref_cpu.backbone(x, sd, cfg, sd_keep) with the first ``frozen`` features entries (None: all) in bf16."""
    if "convnext" not in cfg.net:
        raise ValueError(f"convnext_train_lowp_ref: {cfg.net} is not a ConvNeXt backbone")
    return convnext_features_train_bf16(x, sd, "_net.", cfg.net, getattr(cfg, "use_mid_layers", False),
                                        getattr(cfg, "num_stages", 2), sd_keep, frozen)


def pipnet_train_forward(feats: Tensor, sd: Dict[str, Tensor], cfg):
    """PIPNet.forward(inference=False) after the backbone: (proto, pooled, out), as ref_cpu.pipnet_forward."""
    if getattr(cfg, "num_features", 0):
        feats = F.conv2d(feats, sd["_add_on.0.weight"], sd["_add_on.0.bias"])
    proto = torch.softmax(feats, dim=1)
    pooled = torch.amax(proto, dim=(2, 3))
    out = ref_cpu.non_neg_linear(pooled, sd["_classification.weight"], sd.get("_classification.bias"))
    return proto, pooled, out


def count_soft_forward(feats: Tensor, sd: Dict[str, Tensor], cfg, exp_noise: Optional[Tensor]):
    """CountPIPNet.forward in train mode up to the raw counts: (soft Gumbel-softmax / softmax map, its spatial sums)
    -- count_pipnet_utils.py:36-38 with the Exp(1) draw injected, count_pipnet.py:88."""
    if getattr(cfg, "num_features", 0):
        feats = F.conv2d(feats, sd["_add_on.0.weight"], sd["_add_on.0.bias"])
    if getattr(cfg, "activation", "gumbel_softmax") == "softmax":
        proto = torch.softmax(feats, dim=1)
    else:
        proto = ((feats - exp_noise.log()) / float(getattr(cfg, "tau", 1.0))).softmax(1)
    return proto, proto.sum(dim=(2, 3))
