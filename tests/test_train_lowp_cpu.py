"""Low-precision frozen layers of a training step (set_hip_train_dtype) on the CPU: the switch, the labels of the
new launches, and the bf16 error budget measured from the reference alone.

The budget: tests/convnext_train_lowp_ref.py (the fp32 oracle's train-mode forward with the frozen entries in the
plain bf16 build's arithmetic and the device epilogue's residual update x + rs_b * (layer_scale * y)) against
``ref_cpu.pipnet_forward(..., inference=False, sd_keep=masks)`` on the cases the GPU suite runs
(tests/test_gpu_train_lowp.py imports CASES, BOUNDS and the case builders from here).  Every block with p > 0 has at
least one dropped and one kept sample (``forced_masks``): the fixtures' recorded masks almost never drop, p <= 0.03
in the mid-layer models.  The bounds are written once, here, at about 2x what this module measures (the convention
of tests/test_convnext_bf16_cpu.py: a device run accumulates in another order, so it is another draw from the same
error distribution).  Each test prints what it measured.

Measured with this restatement (torch CPU, 8 threads).  The three loss terms are signed sums over the batch, so
their error swings by more than 10x from one draw of images to the next (class term of finetune_mid_addon: 1.6e-5 to
1.5e-4); each figure below is therefore the LARGEST of six image seeds (3, 11, 5, 7, 13, 17 at 224^2; 5, 3, 7, 11,
13, 17 at 64^2; the first is the seed the tests run), the case's own seed beside it, and the bound twice the largest:

| case, frozen entries                     | pooled                 | logit / max logit       | align                     | tanh                      | class                     |
| finetune_c2, 6 x 224^2, whole backbone   | 0.0134, own 0.0104 (0.027) | 0.0022, own 0.0007 (0.0044) | 0.00108, own 0.00093 (0.0022) | 0.00050, own 0.00050 (0.0010) | 0.00016, own 0.00015 (0.00032) |
| finetune_mid_addon, 16 x 64^2, whole     | 0.0085, own 0.0072 (0.017) | 0.0027, own 0.0016 (0.0055) | 0.00053, own 0.00031 (0.0011) | 0.00016, own 0.00006 (0.00033) | 0.00015, own 0.00004 (0.00031) |
| joint_c2, 6 x 224^2, features[:6]        | 0.0106, own 0.0083 (0.021) | 0.0015, own 0.0004 (0.0029) | 0.00090, own 0.00040 (0.0018) | 0.00043, own 0.00043 (0.00086) | 0.00010, own 0.00010 (0.00021) |
| joint_mid_addon, 16 x 64^2, features[:2] | 0.0059, own 0.0049 (0.012) | 0.0015, own 0.0012 (0.0030) | 0.00034, own 0.00009 (0.00067) | 0.00012, own 0.00002 (0.00023) | 0.00006, own 0.00005 (0.00012) |
| count_finetune_onehot, 6 x 64^2, whole   | soft map 0.0106, own 0.0093 (0.021); raw counts 0.0523, own 0.0374, on a scale of 16.9 (0.105) |

(max logit: 40.8 for the C2 model, 13.8 for the mid-layer one.)
"""
import argparse
import contextlib
import functools
import io
import re

import pytest
import torch

from convnext_train_lowp_ref import backbone_train_bf16, count_soft_forward, pipnet_train_forward
from golden_util import golden_args, golden_state_dict, load_golden, load_train_golden
from oracle import ref_cpu, train_ref

# ---- committed bounds (module docstring: the measurements) ----
# PIP-Net: max |pooled error|, max |logit error| / max |logit|, |error| of the three raw loss terms
BOUNDS = {
    "finetune_c2": dict(pooled=0.027, logit=0.0044, align=0.0022, tanh=0.0010, cls=0.00032),
    "finetune_mid_addon": dict(pooled=0.017, logit=0.0055, align=0.0011, tanh=0.00033, cls=0.00031),
    "joint_c2": dict(pooled=0.021, logit=0.0029, align=0.0018, tanh=0.00086, cls=0.00021),
    "joint_mid_addon": dict(pooled=0.012, logit=0.0030, align=0.00067, tanh=0.00023, cls=0.00012),
}
# CountPIPNet finetune: max |error| of the soft map and of the raw counts (spatial sums of the soft map)
COUNT_BOUNDS = dict(proto=0.021, counts=0.105)
# case -> (fixture whose model it is, images, image size, image seed, frozen features entries: None = all)
CASES = {
    "finetune_c2": ("train_finetune_c2", 6, 224, 3, None),
    "finetune_mid_addon": ("train_finetune_mid_addon", 16, 64, 5, None),
    "joint_c2": ("train_joint_c2", 6, 224, 3, 6),
    "joint_mid_addon": ("train_joint_mid_addon", 16, 64, 5, 2),
}
COUNT_CASE = ("train_count_finetune_onehot", 6, 64, 7)


def forced_masks(cfg, batch, gen):
    """Stochastic-depth keep masks {block id: bool [batch]} for every block with p > 0 of the case's backbone: the
    draw of test_train_forward_stochastic_depth_matches_oracle (keep with 1 - p, then drop 30 % more), then one
    sample of every block forced dropped and the next one forced kept."""
    stages = ref_cpu.CONVNEXT_TINY
    if getattr(cfg, "use_mid_layers", False):
        stages = stages[:(min(cfg.num_stages, 7) + 1) // 2]
    masks = {}
    for bid in range(sum(n for _, _, n in stages)):
        p = ref_cpu.sd_drop_prob(bid)
        if p > 0.0:
            m = (torch.rand(batch, generator=gen) >= p) & (torch.rand(batch, generator=gen) < 0.7)
            m[bid % batch], m[(bid + 1) % batch] = False, True
            masks[bid] = m
    return masks


@functools.lru_cache(maxsize=None)
def pipnet_case(case):
    """(forward meta, images, labels of one view, masks, state dict, args, multiplier, the fp32 oracle's (proto,
    pooled, out), frozen entries) of a PIP-Net case, computed once."""
    fixture, images, size, seed, frozen = CASES[case]
    meta, rec, fwd_meta = load_train_golden(fixture)
    sd, cfg = golden_state_dict(fwd_meta), golden_args(fwd_meta)
    g = torch.Generator().manual_seed(seed)
    xs = torch.randn(images, 3, size, size, generator=g)
    masks = forced_masks(cfg, images, g)
    ys = torch.randint(0, fwd_meta["case"]["num_classes"], (images // 2,), generator=g)
    mult = float(sd["_classification.normalization_multiplier"][0])
    torch.set_num_threads(8)
    with torch.no_grad():
        ref = ref_cpu.pipnet_forward(xs, sd, cfg, inference=False, sd_keep=masks)
    return fwd_meta, xs, ys, masks, sd, cfg, mult, ref, frozen


def compare_train(got, ref, ys, mult, bounds, check=True):
    """Train-mode (proto NCHW, pooled, out) against the fp32 oracle's: the measured figures, asserted under
    ``bounds`` when ``check``."""
    (proto, pooled, out), (rp, rpool, rout) = ([t.detach().cpu().float() for t in x] for x in (got, ref))
    scale = rout.abs().max().clamp(min=1.0).item()
    a, b = train_ref.loss_terms(proto, pooled, out, ys, mult), train_ref.loss_terms(rp, rpool, rout, ys, mult)
    fig = dict(pooled=(pooled - rpool).abs().max().item(), logit=(out - rout).abs().max().item() / scale,
               logit_scale=scale, **{k: abs(float(a[k]) - float(b[k])) for k in ("align", "tanh", "cls")})
    if check:
        for k, bound in bounds.items():
            assert fig[k] <= bound, (k, fig[k], bound, fig)
    return fig


@functools.lru_cache(maxsize=None)
def count_case():
    """(forward meta, images, masks, state dict, args, Exp(1) noise, the fp32 oracle's (soft map, raw counts))."""
    from count_pipnet_amd.synthetic import synth_exponential
    fixture, images, size, seed = COUNT_CASE
    meta, rec, fwd_meta = load_train_golden(fixture)
    sd, cfg = golden_state_dict(fwd_meta), golden_args(fwd_meta)
    g = torch.Generator().manual_seed(seed)
    xs = torch.randn(images, 3, size, size, generator=g)
    masks = forced_masks(cfg, images, g)
    torch.set_num_threads(8)
    with torch.no_grad():
        feats = ref_cpu.backbone(xs, sd, cfg, masks)
        noise = synth_exponential((images, cfg.num_features) + tuple(feats.shape[2:]), meta["noise_seed"])
        ref = count_soft_forward(feats, sd, cfg, noise)
    return fwd_meta, xs, masks, sd, cfg, noise, ref


# ------------------------------------------------------------------------------------------ the switch
def _net(name):
    from model_util import build_model
    return build_model(load_golden(name)[0])


@pytest.mark.parametrize("name", ["c2_pipnet_convnext26", "pipnet_mid_addon", "c1_count_identity"])
def test_set_hip_train_dtype_reaches_convnext(name):
    from count_pipnet_amd.convnext_features import ConvNeXt, MidLayerConvNeXt
    from count_pipnet_amd.pipnet import set_hip_dtype, set_hip_train_dtype
    net = _net(name)
    backbones = [m for m in net.modules() if isinstance(m, (ConvNeXt, MidLayerConvNeXt))]
    assert backbones and not any(hasattr(m, "hip_train_precision") for m in backbones)     # the default: unset = fp32
    for dtype in ("bf16", "bf16x3"):
        set_hip_dtype(net, dtype)                              # the inference switch alone never sets it
        assert not any(hasattr(m, "hip_train_precision") for m in backbones)
    set_hip_dtype(net, "fp32")
    for dtype in ("bf16", "bf16x3"):
        assert set_hip_train_dtype(net, dtype) is net
        assert all(m.hip_train_precision == dtype and m.hip_precision == "fp32" for m in backbones)
        set_hip_train_dtype(net, "fp32")
        assert all(m.hip_train_precision == "fp32" for m in backbones)
    set_hip_train_dtype(net, "bf16")
    set_hip_dtype(net, "bf16x3")                               # ... and never clears it
    assert all(m.hip_train_precision == "bf16" and m.hip_precision == "bf16x3" for m in backbones)
    for bad in ("fp16", "split_bf16", torch.bfloat16, None):
        with pytest.raises(ValueError):
            set_hip_train_dtype(net, bad)
    assert all(m.hip_train_precision == "bf16" for m in backbones)


def test_set_hip_train_dtype_refuses_a_resnet_and_a_plain_module():
    from count_pipnet_amd.pipnet import set_hip_train_dtype
    net = _net("c3_pipnet_resnet50")
    assert set_hip_train_dtype(net, "fp32") is net
    for dtype in ("bf16", "bf16x3"):
        with pytest.raises(ValueError, match="ResNet"):
            set_hip_train_dtype(net, dtype)
    assert not any(hasattr(m, "hip_train_precision") for m in net.modules())
    with pytest.raises(ValueError):
        set_hip_train_dtype(torch.nn.Sequential(torch.nn.Conv2d(3, 8, 1)), "bf16")


def test_args_hip_train_dtype_in_both_factories():
    from count_pipnet_amd.count_pipnet import get_count_network
    from count_pipnet_amd.pipnet import get_pipnet
    for name, factory in (("pipnet_mid_addon", get_pipnet), ("count_onehot", get_count_network)):
        meta, _ = load_golden(name)
        for dtype in ("bf16x3", "bf16", None):
            args = argparse.Namespace(**vars(golden_args(meta)))
            if dtype:
                args.hip_train_dtype = dtype
            with contextlib.redirect_stdout(io.StringIO()):
                net, _ = factory(meta["case"]["num_classes"], args)
            assert getattr(net._net, "hip_train_precision", "fp32") == (dtype or "fp32")
            assert getattr(net._net, "hip_precision", "fp32") == "fp32"
    meta, _ = load_golden("c3_pipnet_resnet50")
    args = golden_args(meta)
    args.hip_train_dtype = "bf16"
    with pytest.raises(ValueError), contextlib.redirect_stdout(io.StringIO()):
        get_pipnet(meta["case"]["num_classes"], args)


def test_train_forward_reads_the_train_precision_only(monkeypatch):
    """convnext_train.train_forward hands the model's train precision, and only it, to both executor calls."""
    from count_pipnet_amd import convnext_train
    from count_pipnet_amd.pipnet import set_hip_dtype, set_hip_train_dtype
    net = _net("pipnet_mid_addon")
    seen = []

    def fake(features, x, cache, sd_keep=None, precision="fp32"):
        seen.append((len(features), precision))
        raise StopIteration                                    # no device here: the arguments are the test

    monkeypatch.setattr(convnext_train, "convnext_features_hip", fake)
    for inference, train, want in (("bf16", None, "fp32"), ("fp32", "bf16x3", "bf16x3"), ("bf16x3", "bf16", "bf16")):
        set_hip_dtype(net, inference)
        if train:
            set_hip_train_dtype(net, train)
        for start in (None, 2):
            with pytest.raises(StopIteration):
                convnext_train.train_forward(net._net, torch.zeros(1, 3, 64, 64), start, {})
        assert seen[-2:] == [(len(net._net.features), want), (2, want)], seen


# ------------------------------------------------------------------------------------------ the labels
def test_rowscale_kernel_names_exist_in_library():
    """The labels of the new launches (pipnet_linear_bf16_mix_rowscale_label / pipnet_linear_s3_rowscale_label) name
    kernels the built library instantiates, at the four Linear2 shapes and on every tile the entries accept; the
    tile and the rest of the name are F32_RESID's for the same layer, and what F32_RESID refuses is refused."""
    import shutil
    import subprocess
    from count_pipnet_amd import _lib, build
    from count_pipnet_amd import kernels as K
    build.build()
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-C", build.LIB], capture_output=True, text=True, check=True).stdout
    syms = set(re.findall(r"void (pipnet_\w+::\w+<.*>)\(", out))
    rowscale = {s for s in syms if re.search(r"kernel<(pipnet_bf16::Cfg<[^>]*>, )?13, ", s) and "__device_stub__" not in s}
    assert len(rowscale) == 5 and all(re.search(r"13, 0, ", s) for s in rowscale), rowscale   # the dense loader only
    seen = set()
    for s3 in (False, True):
        for b, h, cin, cout in [(64, 56, 384, 96), (64, 28, 768, 192), (64, 27, 1536, 384), (64, 26, 3072, 768),
                                (3, 9, 384, 96), (1, 7, 3072, 768), (3, 63, 96, 200), (3, 63, 128, 520)]:
            m = b * h * h
            for tile in K.LOWP_ROWSCALE_TILES:
                name = K.linear_lowp_rowscale_kernel_name(m, cin, cout, tile, s3)
                assert name in rowscale, (s3, m, cin, cout, tile, name)
                plain = K.bf16_conv_kernel_name(1, m, 1, cin, cout, 1, 1, 1, 0, _lib.EPI_F32_RESID, tile, s3=s3,
                                                mix=not s3)
                assert plain in syms and name == re.sub(r"\b11, 0, ", "13, 0, ", plain, count=1), (name, plain)
                seen.add(name)
            for tile in (1, 2, 3, 6, 8, 9, 11):                # the persistent tile (9) among them
                with pytest.raises(RuntimeError):
                    K.linear_lowp_rowscale_kernel_name(m, cin, cout, tile, s3)
    assert seen == rowscale                                    # every instantiation is reachable
    lib = _lib.load()
    args = (None, 189, 128, None, None, None, None, 200, None, 63, None)
    for entry in (lib.pipnet_linear_bf16_mix_rowscale, lib.pipnet_linear_s3_rowscale):
        assert entry(*args, 9, None) == 1 and entry(*args, 3, None) == 1 and entry(*args, -1, None) == 1  # null operands
    for entry in (lib.pipnet_conv2d_nhwc_bf16_mix, lib.pipnet_conv2d_nhwc_s3):     # no `epilogue` argument takes 13
        assert entry(None, 1, 189, 1, 128, None, None, None, None, 200, 1, 1, 1, 0, 13, None, -1, None) == 1


# ------------------------------------------------------------------------------------------ the budget
def test_restatement_without_frozen_entries_is_the_oracle():
    """frozen = 0: no entry is rounded and every call is the oracle's own; x + rs * (ls * y) is its
    (ls * y) * rs + x bit for bit."""
    fwd_meta, xs, ys, masks, sd, cfg, mult, ref, _ = pipnet_case("finetune_mid_addon")
    with torch.no_grad():
        got = pipnet_train_forward(backbone_train_bf16(xs, sd, cfg, masks, frozen=0), sd, cfg)
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    assert all((~m).any() and m.any() for m in masks.values()) and len(masks) == 5


@pytest.mark.parametrize("case", sorted(CASES))
def test_bf16_train_budget_from_the_reference_alone(case):
    fwd_meta, xs, ys, masks, sd, cfg, mult, ref, frozen = pipnet_case(case)
    assert all((~m).any() and m.any() for m in masks.values())
    with torch.no_grad():
        got = pipnet_train_forward(backbone_train_bf16(xs, sd, cfg, masks, frozen), sd, cfg)
    fig = compare_train(got, ref, ys, mult, BOUNDS[case], check=False)
    print(f"bf16 frozen layers, restatement vs fp32 oracle, {case} (frozen entries: {frozen}):", fig)
    compare_train(got, ref, ys, mult, BOUNDS[case])


def test_bf16_train_budget_count_from_the_reference_alone():
    fwd_meta, xs, masks, sd, cfg, noise, (r_proto, r_counts) = count_case()
    assert all((~m).any() and m.any() for m in masks.values())
    with torch.no_grad():
        proto, counts = count_soft_forward(backbone_train_bf16(xs, sd, cfg, masks, None), sd, cfg, noise)
    fig = dict(proto=(proto - r_proto).abs().max().item(), counts=(counts - r_counts).abs().max().item(),
               counts_scale=r_counts.abs().max().item())
    print("bf16 frozen layers, restatement vs fp32 oracle, count_finetune_onehot:", fig)
    assert fig["proto"] <= COUNT_BOUNDS["proto"] and fig["counts"] <= COUNT_BOUNDS["counts"], fig
