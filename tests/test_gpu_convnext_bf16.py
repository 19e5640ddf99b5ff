"""The plain bf16 build of the ConvNeXt backbone (set_hip_dtype(net, "bf16")) through the C ABI.

Kernel level: the producers are bitwise RNE(fp32 kernel's output); the bf16 GEMM with the ConvNeXt
epilogues is held to an fp64 evaluation of the same bf16-valued operands -- one bf16 ulp + 1e-6 and
>= 99 % identical bits for the bf16 GELU output (the bar of tests/test_gpu_bf16.py), 2e-6 of
max |ref| for the fp32 outputs (the fp32-accumulation bar of tests/test_gpu_split.py).

End to end: against the fp32 oracle under the budget tests/test_convnext_bf16_cpu.py measures from
the reference alone and commits (bounds, cases and image seeds are imported from there).
"""
import pytest
import torch
import torch.nn.functional as F

import test_convnext_bf16_cpu as budget
from count_pipnet_amd import _lib
from count_pipnet_amd import kernels as K
from golden_util import golden_inputs, load_golden
from model_util import build_model

pytestmark = pytest.mark.gpu

EPIS = {"bias_gelu": _lib.EPI_BIAS_GELU, "f32_bias": _lib.EPI_F32_BIAS, "f32_resid": _lib.EPI_F32_RESID}
MIX_TILES = (0, 4, 5, 7)             # every tile the automatic rule can pick for these epilogues


# ---- producers ----
@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("h,w", [(5, 7), (9, 9), (24, 24)])
@pytest.mark.parametrize("c", [96, 192, 384, 768])
def test_dwconv7_ln_bf16_is_rne_of_fp32_kernel(gpu, c, h, w, b):
    g = torch.Generator().manual_seed(c + 10 * h + w + b)
    x = torch.randn(b, h, w, c, generator=g).to(gpu)
    wdw = (torch.randn(49, c, generator=g) * 0.1).to(gpu)
    bias, lw, lb = (torch.randn(c, generator=g).to(gpu) for _ in range(3))
    y = K.dwconv7_ln_bf16(x, wdw, bias, lw, lb)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (b, h, w, c)
    assert torch.equal(y, K.dwconv7_ln(x, wdw, bias, lw, lb).to(torch.bfloat16))
    assert torch.equal(y, K.dwconv7_ln_s3(x, wdw, bias, lw, lb)[..., :c])       # the split form's hi plane


@pytest.mark.parametrize("rows", [1, 3, 37, 1000])
@pytest.mark.parametrize("c", [96, 192, 384, 768])
def test_layernorm_bf16_is_rne_of_fp32_kernel(gpu, c, rows):
    g = torch.Generator().manual_seed(rows * c)
    x = torch.randn(rows, c, generator=g).to(gpu)
    w, b = torch.randn(c, generator=g).to(gpu), torch.randn(c, generator=g).to(gpu)
    y = K.layernorm_bf16(x, w, b)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (rows, c)
    assert torch.equal(y, K.layernorm(x, w, b).to(torch.bfloat16))
    assert torch.equal(y, K.layernorm_s3(x, w, b)[..., :c])


# ---- GEMM / conv ----
def _gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / 2 ** 0.5))


def _run_mix(gpu, b, h, w, cin, cout, kh, stride, epi, tile, seed):
    """One conv_bf16_mix launch and its fp64 reference over the same bf16-valued operands."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, h, w, cin, generator=g).to(torch.bfloat16)
    wt = torch.randn(cout, kh, kh, cin, generator=g) * (kh * kh * cin) ** -0.5
    bias = torch.randn(cout, generator=g) * 0.1
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), wt.to(torch.bfloat16).double().permute(0, 3, 1, 2),
                   stride=stride).permute(0, 2, 3, 1) + bias.double()
    wp = K.pack_conv_weight_bf16(wt.to(gpu))
    code = EPIS[epi]
    if epi == "f32_resid":
        scale = torch.rand(cout, generator=g) + 0.5
        r = torch.randn(ref.shape, generator=g, dtype=torch.float32)
        rd = r.to(gpu)
        y = K.conv_bf16_mix(x.to(gpu), wp, kh, kh, bias.to(gpu), stride, 0, code, scale=scale.to(gpu), r=rd, out=rd,
                            tile=tile)
        assert y.data_ptr() == rd.data_ptr()                 # in place on the residual stream
        ref = r.double() + scale.double() * ref
    else:
        y = K.conv_bf16_mix(x.to(gpu), wp, kh, kh, bias.to(gpu), stride, 0, code, tile=tile)
    torch.cuda.synchronize()
    assert tuple(y.shape) == tuple(ref.shape)
    return y.cpu(), ref


def _check_mix(y, ref, epi):
    if epi == "bias_gelu":
        assert y.dtype == torch.bfloat16
        want = _gelu64(ref).float().to(torch.bfloat16).double()
        err = (y.double() - want).abs()
        assert torch.all(err <= want.abs() * 2.0 ** -7 + 1e-6), err.max()
        assert (err == 0).double().mean() >= 0.99, (err == 0).double().mean()
    else:
        assert y.dtype == torch.float32
        err = (y.double() - ref).abs().max().item()
        assert err <= 2e-6 * ref.abs().max().item(), (err, ref.abs().max().item())


@pytest.mark.parametrize("epi", sorted(EPIS))
@pytest.mark.parametrize("b,h,cin,cout,kh,stride", [
    (3, 9, 96, 384, 1, 1),        # K = 96 -> 128: zero K tail
    (2, 11, 384, 96, 1, 1),       # narrow N
    (2, 13, 192, 768, 1, 1),
    (1, 7, 768, 3072, 1, 1),
    (1, 7, 3072, 768, 1, 1),      # longest K
    (3, 10, 128, 136, 1, 1),      # ragged N
    (4, 28, 96, 192, 2, 2),
    (2, 27, 192, 384, 2, 1),      # odd map
    (2, 13, 384, 768, 2, 1),
])
def test_conv_bf16_mix_automatic_tile(gpu, b, h, cin, cout, kh, stride, epi):
    y, ref = _run_mix(gpu, b, h, h, cin, cout, kh, stride, epi, -1, seed=b * 1000 + h * 10 + kh + cout)
    _check_mix(y, ref, epi)


@pytest.mark.parametrize("epi", sorted(EPIS))
@pytest.mark.parametrize("cin,cout,kh", [(96, 200, 1), (128, 520, 1), (64, 200, 2)])
@pytest.mark.parametrize("tile", MIX_TILES)
def test_conv_bf16_mix_every_tile_ragged(gpu, tile, cin, cout, kh, epi):
    """M = 3 * 7 * 9 = 189 output pixels (ragged in every tile height), N = 200 / 520 (ragged in every
    tile width, several column tiles), dense and 2x2 gathers, K = 96 -> 128 padded."""
    y, ref = _run_mix(gpu, 3, 7 + kh - 1, 9 + kh - 1, cin, cout, kh, 1, epi, tile, seed=tile * 31 + cout + kh)
    _check_mix(y, ref, epi)


@pytest.mark.parametrize("tile", [1, 2, 3, 6, 8, 9, 10, 11, 12])
def test_conv_bf16_mix_refuses_other_tiles(gpu, tile):
    x = torch.zeros(1, 4, 4, 256, device=gpu, dtype=torch.bfloat16)
    wp = K.pack_conv_weight_bf16(torch.zeros(256, 1, 1, 256, device=gpu))
    for code in EPIS.values():
        kw = dict(scale=torch.ones(256, device=gpu), r=torch.zeros(1, 4, 4, 256, device=gpu)) \
            if code == _lib.EPI_F32_RESID else {}
        with pytest.raises(RuntimeError):
            K.conv_bf16_mix(x, wp, 1, 1, None, 1, 0, code, tile=tile, **kw)


def test_conv_bf16_mix_operand_errors(gpu):
    x = torch.zeros(1, 4, 4, 64, device=gpu, dtype=torch.bfloat16)
    wp = K.pack_conv_weight_bf16(torch.zeros(64, 1, 1, 64, device=gpu))
    K.conv_bf16_mix(x, wp, 1, 1, None, 1, 0, _lib.EPI_F32_BIAS)                  # the well-formed call
    with pytest.raises(RuntimeError):                                            # fp32 x
        K.conv_bf16_mix(x.float(), wp, 1, 1, None, 1, 0, _lib.EPI_F32_BIAS)
    with pytest.raises(RuntimeError):                                            # CPU weight
        K.conv_bf16_mix(x, wp.cpu(), 1, 1, None, 1, 0, _lib.EPI_F32_BIAS)
    with pytest.raises(RuntimeError):                                            # wrong packed K
        K.conv_bf16_mix(x, wp, 2, 2, None, 1, 0, _lib.EPI_F32_BIAS)
    with pytest.raises(RuntimeError):                                            # Cin = 40: not % 32
        K.conv_bf16_mix(torch.zeros(1, 4, 4, 40, device=gpu, dtype=torch.bfloat16),
                        K.pack_conv_weight_bf16(torch.zeros(64, 1, 1, 40, device=gpu)), 1, 1, None, 1, 0,
                        _lib.EPI_F32_BIAS)
    r, scale = torch.zeros(1, 4, 4, 64, device=gpu), torch.ones(64, device=gpu)
    with pytest.raises(RuntimeError):                                            # residual epilogue without r
        K.conv_bf16_mix(x, wp, 1, 1, None, 1, 0, _lib.EPI_F32_RESID, scale=scale)
    with pytest.raises(RuntimeError):                                            # ... without scale
        K.conv_bf16_mix(x, wp, 1, 1, None, 1, 0, _lib.EPI_F32_RESID, r=r)
    with pytest.raises(RuntimeError):                                            # an epilogue of another entry
        K.conv_bf16_mix(x, wp, 1, 1, None, 1, 0, _lib.EPI_BIAS_RELU)
    with pytest.raises(RuntimeError):                                            # bias on the CPU
        K.conv_bf16_mix(x, wp, 1, 1, torch.zeros(64), 1, 0, _lib.EPI_F32_BIAS)


def test_conv_bf16_mix_batch_invariant(gpu):
    """The tile may change with M (0 / 4 walk K alike); the bits of a pixel's result must not."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(40, 28, 28, 96, generator=g).to(torch.bfloat16).to(gpu)
    wp = K.pack_conv_weight_bf16((torch.randn(192, 1, 1, 96, generator=g) * 0.1).to(gpu))
    bias = torch.randn(192, generator=g).to(gpu)
    for code in (_lib.EPI_BIAS_GELU, _lib.EPI_F32_BIAS):
        full = K.conv_bf16_mix(x, wp, 1, 1, bias, 1, 0, code)
        part = K.conv_bf16_mix(x[2:5].contiguous(), wp, 1, 1, bias, 1, 0, code)
        assert torch.equal(full[2:5], part)


# ---- end to end ----
def _bf16_net(name, gpu):
    from count_pipnet_amd.pipnet import set_hip_dtype
    meta, rec = load_golden(name)
    return meta, rec, set_hip_dtype(build_model(meta), "bf16").to(gpu)


@pytest.mark.parametrize("name", sorted(budget.PIPNET_CASES))
def test_bf16_pipnet_vs_fp32_oracle(gpu, name):
    """The case's committed-seed images through the HIP bf16 build and the fp32 oracle: presence flags,
    pooled values, logits, class-margin error and the argmax of every decisive image under the
    committed budget."""
    torch.set_num_threads(8)
    _, xs, _, _, r_raw, r_out = budget.pipnet_case(name)
    _, _, net = _bf16_net(name, gpu)
    with torch.no_grad():
        proto, pooled, out = net(xs.to(gpu), inference=True)
    assert proto.dtype == torch.float32                       # the head and proto_features stay fp32
    got = budget.compare_pipnet(pooled.cpu(), out.cpu(), r_raw, r_out, budget.PIPNET_CASES[name], check=False)
    print(f"bf16 budget, HIP build vs fp32 oracle, {name}:", got)
    budget.compare_pipnet(pooled.cpu(), out.cpu(), r_raw, r_out, budget.PIPNET_CASES[name])


@pytest.mark.parametrize("name", ["c1_count_identity", "count_linear_full"])
def test_bf16_count_pipnet_vs_fp32_oracle(gpu, name):
    """The golden inputs and noise: the head's per-pixel decision agrees with the fp32 oracle on every
    decisive pixel (>= 80 % of all pixels are), and an image's clamped counts move by no more than
    its number of non-decisive pixels."""
    torch.set_num_threads(8)
    meta, rec, xs, sd, args, noise, z_ref = budget.count_case(name)
    _, _, net = _bf16_net(name, gpu)
    if noise is not None:
        net._add_on[-1].exp_noise = noise.to(gpu)
    with torch.no_grad():
        proto, counts, _ = net(xs.to(gpu), inference=True)
    dec = budget.decisive_pixels(z_ref, noise, args)
    assert dec.double().mean().item() >= budget.COUNT_MIN_DECISIVE
    want = budget.perturbed(z_ref, noise, args).argmax(1)
    got = proto.float().cpu().argmax(1)
    agree = got == want
    print(f"bf16 HIP build vs fp32 oracle, {name}: decisive pixels {dec.double().mean().item():.3f}, "
          f"argmax agrees on {agree.double().mean().item():.4f} of all pixels")
    assert agree[dec].all(), (~agree & dec).sum()
    slack = (~dec).flatten(1).sum(1).double()
    dcount = (counts.cpu().double() - torch.from_numpy(rec["inf_pooled"]).double()).abs().max(1).values
    assert torch.all(dcount <= slack), (dcount, slack)


def _c2_net(gpu):
    return _bf16_net("c2_pipnet_convnext26", gpu)[2]


def test_bf16_c2_properties(gpu):
    from count_pipnet_amd.synthetic import synth_images
    net = _c2_net(gpu)
    xs = synth_images(8, 224, seed=7).to(gpu)
    with torch.no_grad():
        proto, pooled, out = net(xs, inference=True)
        proto3, pooled3, out3 = net(xs[2:5].contiguous(), inference=True)
    assert proto.shape == (8, 768, 26, 26) and pooled.shape == (8, 768) and out.shape == (8, 200)
    assert proto.dtype == torch.float32
    assert torch.allclose(proto.sum(dim=1), torch.ones(8, 26, 26, device=gpu), atol=2e-6)
    raw_max = proto.amax(dim=(2, 3))
    assert torch.equal(pooled, torch.where(raw_max < 0.1, torch.zeros_like(raw_max), raw_max))
    w = net._classification.weight
    assert torch.allclose(out, pooled @ torch.relu(w).t(), rtol=1e-5, atol=1e-4)
    assert torch.equal(proto[2:5], proto3) and torch.equal(pooled[2:5], pooled3) and torch.equal(out[2:5], out3)
    with torch.no_grad():                                     # classifier mutation between calls
        w.copy_(torch.clamp(w - 1e-3, min=0.0))
        _, pooled_b, out_b = net(xs, inference=True)
    assert torch.equal(pooled_b, pooled) and not torch.equal(out_b, out)
    assert torch.allclose(out_b, pooled_b @ torch.relu(w).t(), rtol=1e-5, atol=1e-4)
    with torch.no_grad():                                     # the packed bf16 weights follow the parameter
        net._net.features[1][0].block[3].weight.mul_(2)
        _, pooled_c, _ = net(xs, inference=True)
    assert not torch.equal(pooled_c, pooled)


def test_bf16_mode_switch_on_one_net(gpu):
    from count_pipnet_amd.pipnet import set_hip_dtype
    meta, _ = load_golden("pipnet_mid_addon")
    net = build_model(meta).to(gpu)
    xs = golden_inputs(meta).to(gpu)
    outs = []
    for mode in ("fp32", "bf16", "fp32"):
        set_hip_dtype(net, mode)
        with torch.no_grad():
            outs.append([t.clone() for t in net(xs, inference=True)])
    for a, b in zip(outs[0], outs[2]):
        assert torch.equal(a, b)
    assert not torch.equal(outs[0][0], outs[1][0]) and not torch.equal(outs[0][2], outs[1][2])


def test_bf16_graph_replay_equals_eager(gpu):
    from count_pipnet_amd.graph import GraphedForward
    meta, _, net = _bf16_net("pipnet_mid_addon", gpu)
    xs = golden_inputs(meta).to(gpu)
    assert xs.shape == (4, 3, 64, 64)
    with torch.no_grad():
        ref = [t.clone() for t in net(xs, inference=True)]
    g = GraphedForward(net)
    for _ in range(2):
        outs = g(xs)
        torch.cuda.synchronize()
        for a, b in zip(outs, ref):
            assert torch.equal(a, b)


def test_bf16_attribution_is_still_refused(gpu):
    from count_pipnet_amd.attribution import attribute
    _, _, net = _bf16_net("pipnet_mid_addon", gpu)
    with pytest.raises(NotImplementedError, match="the bf16 build"):
        attribute(net, torch.zeros(3, 64, 64, device=gpu), [0], steps=8, batch_size=4)


def test_bf16_kernel_names_exist_in_library():
    """The names the library gives for the C2 stage GEMMs and downsample convs (64 images of 224^2)
    are kernels it instantiates -- needs the built library, not a device."""
    from test_capi_symbols import _kernel_symbols
    from count_pipnet_amd import build
    build.build()
    syms = _kernel_symbols()
    names = set()
    for hw, c in ((56, 96), (28, 192), (27, 384), (26, 768)):
        names.add(K.bf16_conv_kernel_name(64, hw, hw, c, 4 * c, 1, 1, 1, 0, _lib.EPI_BIAS_GELU, mix=True))
        names.add(K.bf16_conv_kernel_name(64, hw, hw, 4 * c, c, 1, 1, 1, 0, _lib.EPI_F32_RESID, mix=True))
    for hw, c, s in ((56, 96, 2), (28, 192, 1), (27, 384, 1)):
        names.add(K.bf16_conv_kernel_name(64, hw, hw, c, 2 * c, 2, 2, s, 0, _lib.EPI_F32_BIAS, mix=True))
    assert names and names <= syms, names - syms
    for tile in MIX_TILES:
        assert K.bf16_conv_kernel_name(3, 7, 9, 96, 200, 1, 1, 1, 0, _lib.EPI_BIAS_GELU, tile, mix=True) in syms
    with pytest.raises(RuntimeError):
        K.bf16_conv_kernel_name(3, 7, 9, 96, 256, 1, 1, 1, 0, _lib.EPI_BIAS_GELU, 9, mix=True)
    with pytest.raises(RuntimeError):                         # the ResNet epilogues stay with their own entry
        K.bf16_conv_kernel_name(3, 7, 9, 96, 256, 1, 1, 1, 0, _lib.EPI_BIAS_RELU, mix=True)
