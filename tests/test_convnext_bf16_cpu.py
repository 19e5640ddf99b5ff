"""The plain bf16 ConvNeXt build on the CPU: the public switch, and its error budget measured
from the reference alone.

The budget: tests/convnext_bf16_ref.py (the oracle with the build's four roundings and RNE-bf16
weights) against the fp32 oracle on each end-to-end case the GPU suite runs
(tests/test_gpu_convnext_bf16.py).  The bounds below are written once, here, at about 2x what this
module measures (the convention of the ResNet bf16 build, tests/test_gpu_bf16.py): the device
accumulates in another order, which re-randomises every later rounding, so a device run is another
draw from the same error distribution, not the same numbers.  Each test prints what it measured.

Measured with this restatement (torch CPU, 8 threads), bounds beside them:

| case                                  | pooled          | presence flips, distance from 0.1 | logit / scale             | class margin    | decisive |
| C2 golden model, 16 x 224^2, seed 11  | 0.0140 (0.03)   | 22 flips within 0.0041 (0.008)    | 0.272 / 23.1 = 0.012 (0.03) | 0.0794 (0.16) | 3 of 16 (>= 2) |
| pipnet_mid_addon, 16 x 64^2, seed 5   | 0.0122 (0.025)  | 1 flip at 0.0008 (0.002)          | 0.127 / 12.9 = 0.010 (0.02) | 0.0313 (0.06) | 8 of 16 (>= 6) |
| c1_count_identity / count_onehot / count_linear_full | pre-head logit error 0.0484 / 0.0475 / 0.0415 on scales 9.2 / 7.9 / 6.8 (0.05) |

The C2 images are synth_images seed 11, not the seed 7 of the parity suite: a decisive image is one
whose fp32 top-two class gap exceeds the margin bound, the comparison needs at least 2 of them, and
with seed 7 the reference alone gives 1 (margin error 0.0758, gaps 0.249, 0.130, 0.117, ...); seed 11
gives 3 (gaps 0.194, 0.187, 0.162).  Over eight image seeds (7, 11, 3, 5, 13, 17, 1, 2) the
restatement's C2 errors spread over pooled 0.013-0.023, logit / scale 0.012-0.024 (mostly common to
every class of an image: the classifier rows are N(1, 0.1)) and margin 0.063-0.128, which is why the
logit bound is 2x their mean (0.0166) and not 2x the seed-11 draw alone.

CountPIPNet: the device run is held to the head's decisions, not to a logit error.  A pixel counts
as decisive when the oracle's top-two gap of the (Gumbel-perturbed) logits exceeds
COUNT_GAP_FACTOR = 4 x COUNT_LOGIT_TOL; flipping such a pixel's argmax takes two logit errors that sum
to more than the gap, i.e. one of more than 2 x COUNT_LOGIT_TOL -- so the 2x safety factor of the
PIP-Net bounds sits in the gap factor, and COUNT_LOGIT_TOL itself is the reference's own largest
error rounded up (0.0484 -> 0.05).  At 4 x 0.05 = 0.2, 86.7 / 87.1 / 80.5 % of the pixels are
decisive (>= 80 % required) and the restatement's argmax agrees on every one of them.
"""
import functools

import pytest
import torch

from convnext_bf16_ref import backbone_bf16, pipnet_head, pre_head_logits
from golden_util import golden_args, golden_inputs, golden_noise, golden_state_dict, load_golden, proto_shape
from oracle import ref_cpu

# ---- committed bounds (module docstring: the measurements and where each bound comes from) ----
# PIP-Net cases: name -> bounds and the images the comparison runs on
PIPNET_CASES = {
    "c2_pipnet_convnext26": dict(images=16, size=224, seed=11, min_decisive=2,
                                 pooled=0.03, band=0.008, logit=0.03, margin=0.16),
    "pipnet_mid_addon": dict(images=16, size=64, seed=5, min_decisive=6,
                             pooled=0.025, band=0.002, logit=0.02, margin=0.06),
}
# CountPIPNet cases: absolute error of the pre-head logits; a pixel is decisive when the oracle's
# top-two gap of the perturbed logits exceeds COUNT_GAP_FACTOR x that bound
COUNT_LOGIT_TOL = 0.05
COUNT_GAP_FACTOR = 4.0
COUNT_MIN_DECISIVE = 0.80
COUNT_CASES = ("c1_count_identity", "count_onehot", "count_linear_full")


def compare_pipnet(pooled, out, r_raw, r_out, bounds, check=True):
    """Inference-mode (pooled, logits) of a bf16 evaluation against the fp32 oracle's raw pooled values
    and logits: the measured figures, asserted under ``bounds`` when ``check`` -- the structure of
    tests/test_gpu_bf16.py::_check_bf16_vs_fp32."""
    pooled, out, r_raw, r_out = (t.double() for t in (pooled, out, r_raw, r_out))
    r_inf = torch.where(r_raw < 0.1, torch.zeros_like(r_raw), r_raw)
    flipped = (pooled > 0) != (r_raw >= 0.1)
    flip = (r_raw - 0.1).abs()[flipped].max().item() if flipped.any() else 0.0
    both = (pooled > 0) & (r_inf > 0)
    perr = (pooled - r_inf).abs()[both].max().item() if both.any() else 0.0
    d = out - r_out
    scale = r_out.abs().max().clamp(min=1.0).item()
    top = r_out.argmax(1)
    merr = (d - d.gather(1, top[:, None])).abs().max(1).values
    srt = r_out.sort(dim=1).values
    gap = srt[:, -1] - srt[:, -2]
    decisive = gap > bounds["margin"]
    got = {"pooled_err": perr, "flip_dist": flip, "flips": int(flipped.sum()), "logit_err": d.abs().max().item(),
           "logit_scale": scale, "margin_err": merr.max().item(), "decisive": int(decisive.sum()),
           "images": int(out.shape[0])}
    if check:
        assert flip <= bounds["band"], ("presence flag flipped outside the band", got)
        assert perr <= bounds["pooled"], got
        assert got["logit_err"] <= bounds["logit"] * scale, got
        assert got["margin_err"] <= bounds["margin"], got
        assert got["decisive"] >= bounds["min_decisive"], (got, gap)
        assert torch.equal(out.argmax(1)[decisive], top[decisive]), (out.argmax(1), top, gap)
    return got


@functools.lru_cache(maxsize=None)
def pipnet_case(name):
    """(meta, images, state dict, args, oracle raw pooled, oracle logits) of a PIP-Net case, computed once."""
    from count_pipnet_amd.synthetic import synth_images
    meta, _ = load_golden(name)
    c = PIPNET_CASES[name]
    xs = synth_images(c["images"], c["size"], seed=c["seed"])
    sd, args = golden_state_dict(meta), golden_args(meta)
    with torch.no_grad():
        r_raw, r_out = pipnet_head(pre_head_logits(ref_cpu.backbone(xs, sd, args), sd, args), sd)
    return meta, xs, sd, args, r_raw, r_out


@functools.lru_cache(maxsize=None)
def count_case(name):
    """(meta, record, images, state dict, args, noise, oracle pre-head logits) of a CountPIPNet case."""
    meta, rec = load_golden(name)
    xs, sd, args = golden_inputs(meta), golden_state_dict(meta), golden_args(meta)
    gumbel = meta["case"]["activation"] == "gumbel_softmax"
    noise = golden_noise(meta, proto_shape(meta, rec)) if gumbel else None
    with torch.no_grad():
        z = pre_head_logits(ref_cpu.backbone(xs, sd, args), sd, args)
    return meta, rec, xs, sd, args, noise, z


def perturbed(z, noise, args):
    """What the head takes the argmax of: the logits, plus the Gumbel noise of a gumbel head."""
    return z if noise is None else (z - noise.log()) / float(getattr(args, "tau", 1.0))


def decisive_pixels(z_ref, noise, args):
    """[B,h,w] mask: the oracle's top-two gap exceeds COUNT_GAP_FACTOR x COUNT_LOGIT_TOL."""
    top2 = perturbed(z_ref, noise, args).topk(2, dim=1).values
    tau = float(getattr(args, "tau", 1.0)) if noise is not None else 1.0
    return (top2[:, 0] - top2[:, 1]) * tau > COUNT_GAP_FACTOR * COUNT_LOGIT_TOL


# ------------------------------------------------------------------------------------------
def _net(name):
    from model_util import build_model
    return build_model(load_golden(name)[0])


@pytest.mark.parametrize("name", ["c2_pipnet_convnext26", "pipnet_mid_addon", "c1_count_identity"])
def test_set_hip_dtype_bf16_reaches_convnext(name):
    from count_pipnet_amd.convnext_features import ConvNeXt, MidLayerConvNeXt
    from count_pipnet_amd.pipnet import set_hip_dtype
    net = _net(name)
    backbones = [m for m in net.modules() if isinstance(m, (ConvNeXt, MidLayerConvNeXt))]
    assert backbones
    for dtype in ("bf16", torch.bfloat16):
        assert set_hip_dtype(net, dtype) is net
        assert all(m.hip_precision == "bf16" for m in backbones)
        set_hip_dtype(net, "fp32")
        assert all(m.hip_precision == "fp32" for m in backbones)
    set_hip_dtype(net, "bf16x3")
    assert all(m.hip_precision == "bf16x3" for m in backbones)
    set_hip_dtype(net, torch.float32)
    assert all(m.hip_precision == "fp32" for m in backbones)


def test_set_hip_dtype_bf16_keeps_resnet_switch():
    from count_pipnet_amd.pipnet import set_hip_dtype
    from count_pipnet_amd.resnet_features import ResNet_features
    net = _net("c3_pipnet_resnet50")
    set_hip_dtype(net, "bf16")
    assert all(m.hip_dtype == torch.bfloat16 for m in net.modules() if isinstance(m, ResNet_features))
    set_hip_dtype(net, "fp32")
    assert all(m.hip_dtype == torch.float32 for m in net.modules() if isinstance(m, ResNet_features))


def test_set_hip_dtype_without_a_backbone_raises():
    from count_pipnet_amd.pipnet import set_hip_dtype
    plain = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 1), torch.nn.ReLU())
    for dtype in ("bf16", torch.bfloat16, "bf16x3"):
        with pytest.raises(ValueError):
            set_hip_dtype(plain, dtype)
    with pytest.raises(ValueError):
        set_hip_dtype(plain, "fp16")


def test_args_hip_dtype_bf16_builds_a_bf16_convnext():
    from count_pipnet_amd.pipnet import get_pipnet
    meta, _ = load_golden("pipnet_mid_addon")
    args = golden_args(meta)
    args.hip_dtype = "bf16"
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        net, _ = get_pipnet(meta["case"]["num_classes"], args)
    assert net._net.hip_precision == "bf16"


def test_unknown_precision_still_raises():
    from count_pipnet_amd.convnext_features import PRECISIONS, convnext_features_hip_steps
    assert PRECISIONS == ("fp32", "bf16x3", "bf16")
    net = _net("pipnet_mid_addon")
    with pytest.raises(ValueError):
        next(convnext_features_hip_steps(net._net.features, torch.zeros(1, 3, 64, 64), {}, precision="nope"))


@pytest.mark.parametrize("name", sorted(PIPNET_CASES))
def test_bf16_budget_pipnet_from_the_reference_alone(name):
    torch.set_num_threads(8)
    meta, xs, sd, args, r_raw, r_out = pipnet_case(name)
    with torch.no_grad():
        raw, out = pipnet_head(pre_head_logits(backbone_bf16(xs, sd, args), sd, args), sd)
    pooled = torch.where(raw < 0.1, torch.zeros_like(raw), raw)
    got = compare_pipnet(pooled, out, r_raw, r_out, PIPNET_CASES[name], check=False)
    print(f"bf16 budget, restatement vs fp32 oracle, {name}:", got)
    compare_pipnet(pooled, out, r_raw, r_out, PIPNET_CASES[name])


@pytest.mark.parametrize("name", COUNT_CASES)
def test_bf16_budget_count_from_the_reference_alone(name):
    torch.set_num_threads(8)
    meta, rec, xs, sd, args, noise, z_ref = count_case(name)
    with torch.no_grad():
        z = pre_head_logits(backbone_bf16(xs, sd, args), sd, args)
    err = (z - z_ref).abs().max().item()
    dec = decisive_pixels(z_ref, noise, args)
    frac = dec.double().mean().item()
    agree = perturbed(z, noise, args).argmax(1) == perturbed(z_ref, noise, args).argmax(1)
    print(f"bf16 budget, restatement vs fp32 oracle, {name}: pre-head logit err {err:.4f} on scale "
          f"{z_ref.abs().max().item():.2f}, decisive pixels {frac:.3f}, argmax agrees on "
          f"{agree.double().mean().item():.4f} of all pixels")
    assert err <= COUNT_LOGIT_TOL, err
    assert frac >= COUNT_MIN_DECISIVE, frac
    assert agree[dec].all()
