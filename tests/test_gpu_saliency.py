"""Attribution images on the GPU (count_pipnet_amd.saliency, csrc/saliency_ops.hip).

* every kernel bit for bit against tests/saliency_ref.py on the same inputs, over the size / T / percentile grids
  of tests/saliency_cases.py plus N = 257 (one past a block) and N = 4099 (a loop, unaligned rows), every output
  inside sentinel-filled padding that must stay untouched;
* the select on ties, all-equal and mixed-sign maps; the normalisation rules one float32 ulp either side of 1e-3
  and 1e-5; the operand checks;
* ``interpret_prototypes`` / ``interpret_logit`` on the device stage by stage against ``saliency_ref`` applied to
  the call's own maps, run to run, against the CPU net's selection, without touching the net;
* the normalised device maps against the reference's recording (tests/golden/saliency/<case>.npz) within
  12 eps / (D - 6 eps) + four float32 roundings, eps the bound tests/test_gpu_attribution.py holds the maps to.

Measured |deviation| / bound on an MI355X (printed as SALIENCY_RATIO): 0.007 .. 0.021 over the 24 maps.
"""
import numpy as np
import pytest
import torch

import saliency_ref as R
from attr_util import KINDS, METHODS, attr_image, attr_noise, load_attr
from count_pipnet_amd import kernels as K
from count_pipnet_amd import saliency as S
from count_pipnet_amd.attribution import attribute
from golden_util import load_golden
from model_util import build_model
from saliency_cases import (COUNTS, END_TO_END, PERCENTILES, SIZES, as_tensor, decisive_choice, direct_contributions,
                            load_saliency, same_bits, sample_maps, selection_noise)

pytestmark = pytest.mark.gpu

GPU_SIZES = SIZES + [(1, 257), (1, 4099)]
MAP_BOUND = 8                    # tests/test_gpu_attribution.py: err_hip <= MAP_BOUND * ref_err
PAD = 8                          # sentinel elements either side of every output
FIELDS = ("folded", "vmin", "vq", "vtop", "rule", "normalized")
_SENTINEL = {torch.float32: -7.0, torch.float64: -7.0, torch.int32: -7, torch.uint8: 0xA5}
_NETS = {}


class Padded:
    """A sentinel-filled buffer and the contiguous view of ``shape`` that starts PAD + shift elements in."""

    def __init__(self, shape, dtype, dev, shift=0):
        self.n = int(np.prod(shape))
        self.first = PAD + shift
        self.buf = torch.full((self.n + 2 * PAD + shift,), _SENTINEL[dtype], dtype=dtype, device=dev)
        self.view = self.buf[self.first:self.first + self.n].view(shape)

    def untouched(self) -> bool:
        s = _SENTINEL[self.buf.dtype]
        return bool((self.buf[:self.first] == s).all()) and bool((self.buf[self.first + self.n:] == s).all())


def _lut():
    return load_saliency("steps")[1]["blues_lut"]


# ---- kernels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", COUNTS)
@pytest.mark.parametrize("hw", GPU_SIZES)
def test_abs_sum_kernel(gpu, hw, t):
    """16-byte path (aligned, N % 4 == 0), scalar path (a row or the output off by one float): the same bits."""
    maps = sample_maps(t, *hw)
    want = R.fold(maps)
    dev = as_tensor(maps, gpu)
    assert same_bits(K.saliency_abs_sum(dev), want)
    for shift in (0, 1):
        out = Padded((t,) + hw, torch.float32, gpu, shift)
        assert K.saliency_abs_sum(dev, out=out.view) is out.view
        assert same_bits(out.view, want) and out.untouched(), (hw, t, shift)
    src = Padded((t, 3) + hw, torch.float32, gpu, 1)            # unaligned input rows
    src.view.copy_(dev)
    assert same_bits(K.saliency_abs_sum(src.view), want)


def _check_stats(gpu, folded: np.ndarray, q, exact_zero_sign=True):
    k, _, gamma = R.percentile_split(folded.shape[1] * folded.shape[2], q)
    want = R.order_stats(folded, q)
    t = folded.shape[0]
    outs = [Padded((t,), torch.float32, gpu) for _ in range(5)]
    got = K.saliency_order_stats(as_tensor(folded, gpu), k, float(gamma), out=tuple(o.view for o in outs))
    for name, g, w, o in zip(("vmin", "vtop", "lo", "hi", "vq"), got, want, outs):
        if exact_zero_sign:
            assert same_bits(g, w), (name, q, folded.shape)
        else:
            assert np.array_equal(g.cpu().numpy(), w), (name, q, folded.shape)
        assert o.untouched(), name
    return want


@pytest.mark.parametrize("t", COUNTS)
@pytest.mark.parametrize("hw", GPU_SIZES)
def test_order_stats_kernel(gpu, hw, t):
    folded = R.fold(sample_maps(t, *hw))
    for q in PERCENTILES:
        _check_stats(gpu, folded, q)


def test_order_stats_ties_and_digit_boundaries(gpu):
    """N = 1024.  0x3F7FFFFF | 0x3F800000 sit either side of rank k at q = 50 (the keys part in the second
    digit); the same with 2.0 above (they part in the first digit); k and k + 1 inside a run of equal values;
    a constant map; values that differ in the last digit only."""
    n = 1024
    below, one = np.nextafter(np.float32(1), np.float32(0)), np.float32(1)
    assert below.view(np.uint32) == 0x3F7FFFFF and one.view(np.uint32) == 0x3F800000
    rows = [np.r_[np.full(512, below), np.full(512, one)],
            np.r_[np.full(512, below), np.full(512, np.float32(2))],
            np.r_[np.full(300, np.float32(0.5)), np.full(724, one)],
            np.full(n, np.float32(0.375)),
            np.float32(1) + np.arange(n, dtype=np.float32) * np.float32(2.0 ** -23)]
    g = np.random.default_rng(11)
    folded = np.stack([g.permutation(r.astype(np.float32)) for r in rows]).reshape(len(rows), 32, 32)
    for q in PERCENTILES:
        vmin, vtop, lo, hi, vq = _check_stats(gpu, folded, q)
        if q == 50:
            assert (lo[0], hi[0]) == (below, one) and (lo[1], hi[1]) == (below, np.float32(2))
            assert (lo[2], hi[2]) == (one, one) and lo[3] == hi[3] == vq[3] == np.float32(0.375)
    full = S.normalize_maps(as_tensor(folded, gpu), 98)
    want = R.normalize_maps(folded, 98)
    for f in FIELDS:
        assert same_bits(getattr(full, f), want[f]), f
    assert want["rule"][3] == 2


def test_order_stats_mixed_sign(gpu):
    """Negative values, both zeros: the keys order every finite float; -0.0 and +0.0 may swap against numpy's
    partition, so the select is compared with == here."""
    g = np.random.default_rng(5)
    folded = (g.standard_normal((3, 17, 31)) * 3).astype(np.float32)
    folded[1, :4] = np.float32(0.0)
    folded[1, 4:8] = np.float32(-0.0)
    folded[2] = -np.abs(folded[2])
    for q in PERCENTILES + [33.3]:
        _check_stats(gpu, folded, q, exact_zero_sign=False)


def _ulp_cases():
    """Six 8 x 8 maps with vmin = 0: ranks 61 and 62 (the neighbours of the 98th percentile of 64 values) hold v,
    rank 63 holds the maximum.  v one ulp below / at / one ulp above float32(1e-3); then v = 0 and the maximum one
    ulp below / at / one ulp above float32(1e-5)."""
    a, b = np.float32(1e-3), np.float32(1e-5)
    dn, up = (lambda v: np.nextafter(v, np.float32(0))), (lambda v: np.nextafter(v, np.float32(1)))
    pairs = [(dn(a), 0.5), (a, 0.5), (up(a), 0.5), (0.0, dn(b)), (0.0, b), (0.0, up(b))]
    g = np.random.default_rng(3)
    maps = []
    for v, top in pairs:
        m = np.zeros(64, dtype=np.float32)
        m[61:63], m[63] = v, top
        maps.append(g.permutation(m).reshape(8, 8))
    assert R.percentile_split(64, 98)[0] == 61
    return np.stack(maps), [1, 1, 0, 2, 2, 1], np.array([v for v, _ in pairs], dtype=np.float32)


def test_normalize_rules_one_ulp_either_side_of_the_constants(gpu):
    folded, rules, vq = _ulp_cases()
    want = R.normalize_maps(folded, 98)
    assert want["rule"].tolist() == rules
    assert np.array_equal(want["vq"], vq) and not want["vmin"].any()      # the ranges are the values themselves
    got = S.normalize_maps(as_tensor(folded, gpu), 98)
    for f in FIELDS:
        assert same_bits(getattr(got, f), want[f]), f
    logit = S.normalize_maps(as_tensor(folded, gpu), 98, fallback=False)
    want = R.normalize_maps(folded, 98, fallback=False)
    assert want["rule"].tolist() == [0, 0, 0, 2, 2, 2]
    for f in FIELDS:
        assert same_bits(getattr(logit, f), want[f]), f


@pytest.mark.parametrize("t", COUNTS)
@pytest.mark.parametrize("hw", GPU_SIZES)
def test_normalize_blend_and_colour_map_kernels(gpu, hw, t):
    maps = sample_maps(t, *hw)
    lut = _lut()
    for q in PERCENTILES:
        for fallback in (True, False):
            want = R.normalize_maps(maps, q, fallback)
            got = S.normalize_maps(as_tensor(maps, gpu), q, fallback=fallback)
            for f in FIELDS:
                assert same_bits(getattr(got, f), want[f]), (hw, t, q, fallback, f)
    # the normalisation kernel on the restatement's own statistics, its outputs inside padding
    want = R.normalize_maps(maps, 98)
    rule, norm = Padded((t,), torch.int32, gpu), Padded((t,) + hw, torch.float32, gpu, 1)
    K.saliency_normalize(as_tensor(want["folded"], gpu), as_tensor(want["vmin"], gpu), as_tensor(want["vq"], gpu),
                         as_tensor(want["vtop"], gpu), True, out=(rule.view, norm.view))
    assert same_bits(rule.view, want["rule"]) and same_bits(norm.view, want["normalized"])
    assert rule.untouched() and norm.untouched()
    ndev = as_tensor(want["normalized"], gpu)
    # blend: the palette (T = 12 wraps it) and caller's colours
    assert same_bits(S.blend_maps(ndev), R.blend(want["normalized"]))
    colours = np.random.default_rng(t + 1).random((t, 3))
    out = Padded(hw + (4,), torch.float64, gpu, 1)
    K.saliency_blend(ndev, as_tensor(colours, gpu), out=out.view)
    assert same_bits(out.view, R.blend(want["normalized"], colours)) and out.untouched()
    # byte colour map: one 4-byte store per pixel
    rgba = Padded((t,) + hw + (4,), torch.uint8, gpu)
    K.saliency_colormap_rgba8(ndev, as_tensor(lut, gpu), out=rgba.view)
    assert same_bits(rgba.view, R.colormap(want["normalized"], lut)) and rgba.untouched()
    assert same_bits(S.colormap_rgba8(ndev, as_tensor(lut)), R.colormap(want["normalized"], lut))


def test_colour_map_takes_every_table_entry(gpu):
    """v * 256 at, just below and just above every integer; 1.0 is entry 255; an odd table offset."""
    lut = np.random.default_rng(9).integers(0, 256, (256, 4), dtype=np.uint8)
    edges = np.arange(257, dtype=np.float32) / np.float32(256)
    v = np.concatenate([edges, np.nextafter(edges[1:], np.float32(0)), np.nextafter(edges[:-1], np.float32(1))])
    want = R.colormap(v, lut)
    assert set(np.minimum((v * 256).astype(np.int64), 255).tolist()) == set(range(256))
    assert same_bits(K.saliency_colormap_rgba8(as_tensor(v, gpu), as_tensor(lut, gpu)), want)
    odd = torch.zeros(1025, dtype=torch.uint8, device=gpu)
    odd[1:] = as_tensor(lut, gpu).reshape(-1)
    assert same_bits(K.saliency_colormap_rgba8(as_tensor(v, gpu), odd[1:].view(256, 4)), want)


@pytest.mark.parametrize("hw", GPU_SIZES)
def test_unnormalize_kernel(gpu, hw):
    x = (np.random.default_rng(hw[0] * 100 + hw[1]).standard_normal((3,) + hw) * 1.5).astype(np.float32)
    want = R.unnormalize(x)
    out = Padded(hw + (3,), torch.float32, gpu, 1)
    K.saliency_unnormalize(as_tensor(x, gpu), R.MEAN, R.STD, out=out.view)
    assert same_bits(out.view, want) and out.untouched()
    assert same_bits(S.unnormalize_image(as_tensor(x, gpu)[None]), want)
    other = R.unnormalize(x, (0.5, 0.25, 0.125), (0.1, 0.2, 0.3))
    assert same_bits(S.unnormalize_image(as_tensor(x, gpu), (0.5, 0.25, 0.125), (0.1, 0.2, 0.3)), other)


def test_torch_backend_on_the_device_gives_the_same_bits(gpu):
    from count_pipnet_amd.backend import torch_backend
    maps = sample_maps(3, 7, 9)
    want = R.normalize_maps(maps, 98)
    with torch_backend():
        got = S.normalize_maps(as_tensor(maps, gpu), 98)
        rgba = S.blend_maps(got.normalized)
    assert got.normalized.is_cuda
    for f in FIELDS:
        assert same_bits(getattr(got, f), want[f]), f
    assert same_bits(rgba, R.blend(want["normalized"]))


def test_operand_checks_raise_before_any_launch(gpu):
    maps = as_tensor(sample_maps(2, 8, 8), gpu)
    folded = K.saliency_abs_sum(maps)
    stats = K.saliency_order_stats(folded, 10, 0.5)
    vmin, vtop, _, _, vq = stats
    lut = as_tensor(_lut(), gpu)
    colours = torch.zeros(2, 3, dtype=torch.float64, device=gpu)
    x = torch.zeros(3, 8, 8, device=gpu)
    bad_calls = [
        lambda: K.saliency_abs_sum(maps.cpu()), lambda: K.saliency_abs_sum(maps.double()),
        lambda: K.saliency_abs_sum(maps.transpose(2, 3)), lambda: K.saliency_abs_sum(maps[:, :2]),
        lambda: K.saliency_abs_sum(maps, out=torch.empty(2, 8, 9, device=gpu)),
        lambda: K.saliency_order_stats(folded.cpu(), 10, 0.5), lambda: K.saliency_order_stats(folded.double(), 10, 0.5),
        lambda: K.saliency_order_stats(folded.transpose(1, 2), 10, 0.5),
        lambda: K.saliency_order_stats(folded, 64, 0.5), lambda: K.saliency_order_stats(folded, -1, 0.5),
        lambda: K.saliency_normalize(folded, vmin.cpu(), vq, vtop),
        lambda: K.saliency_normalize(folded, vmin, vq[:1], vtop),
        lambda: K.saliency_normalize(folded.transpose(1, 2), vmin, vq, vtop),
        lambda: K.saliency_normalize(folded, vmin, vq, vtop.double()),
        lambda: K.saliency_blend(folded.cpu(), colours), lambda: K.saliency_blend(folded, colours.float()),
        lambda: K.saliency_blend(folded, colours[:1]), lambda: K.saliency_blend(folded.transpose(1, 2), colours),
        lambda: K.saliency_unnormalize(x.cpu(), R.MEAN, R.STD),
        lambda: K.saliency_unnormalize(x.double(), R.MEAN, R.STD),
        lambda: K.saliency_unnormalize(x.transpose(1, 2), R.MEAN, R.STD),
        lambda: K.saliency_unnormalize(x, R.MEAN[:2], R.STD),
        lambda: K.saliency_colormap_rgba8(folded.cpu(), lut), lambda: K.saliency_colormap_rgba8(folded, lut[:255]),
        lambda: K.saliency_colormap_rgba8(folded, lut.cpu()), lambda: K.saliency_colormap_rgba8(folded, lut.int()),
        lambda: K.saliency_colormap_rgba8(folded.transpose(1, 2), lut),
        lambda: K.saliency_colormap_rgba8(folded, lut, out=Padded((2, 8, 8, 4), torch.uint8, gpu, 1).view),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"call {i} was accepted")
    torch.cuda.synchronize()


# ---- end to end on the device -----------------------------------------------------------------------------------
def _case(name, dev):
    """(meta, arrays, net on the device, image, noise, CPU net) of an attribution fixture; built once."""
    if name not in _NETS:
        meta, rec = load_attr(name)
        noise = attr_noise(meta)
        _NETS[name] = (meta, rec, build_model(meta).to(dev), attr_image(meta), noise, build_model(meta))
    return _NETS[name]


def _prototype_call(name, dev):
    meta, rec, net, x, noise, cpu_net = _case(name, dev)
    sel = selection_noise(noise)
    contrib = direct_contributions(cpu_net, x, sel)
    c, thr = decisive_choice(contrib)
    assert float((contrib[c] - thr).abs().min()) >= 1e-3
    kw = dict(method="ig", steps=8, batch_size=4, threshold=thr, exp_noise=None if noise is None else noise.to(dev),
              selection_noise=sel)
    return net, cpu_net, x, c, thr, sel, kw


@pytest.mark.parametrize("name", END_TO_END)
def test_interpret_prototypes_on_the_device(gpu, name):
    net, cpu_net, x, c, thr, sel, kw = _prototype_call(name, gpu)
    res = S.interpret_prototypes(net, x.to(gpu), c, **kw)
    assert res.attribution.maps.is_cuda and res.overlay.is_cuda and res.image.is_cuda
    assert res.active.indices == S.active_prototypes(cpu_net, x, c, thr, exp_noise=sel).indices      # the CPU net's
    t = len(res.active.indices)
    assert t >= 2
    host = res.cpu()
    maps = host.attribution.maps.numpy()
    want = R.normalize_maps(maps, 98)
    for f in FIELDS:
        assert same_bits(getattr(host.saliency, f), want[f]), f
    assert same_bits(host.overlay, R.blend(want["normalized"]))
    assert same_bits(host.image, R.unnormalize(x.numpy()))
    again = S.interpret_prototypes(net, x.to(gpu), c, **kw).cpu()                                     # run to run
    assert again.active.indices == host.active.indices and torch.equal(again.attribution.maps, host.attribution.maps)
    assert torch.equal(again.overlay, host.overlay) and torch.equal(again.saliency.normalized, host.saliency.normalized)
    empty = S.interpret_prototypes(net, x.to(gpu), c, **{**kw, "threshold": 1e9})
    assert empty.active.indices == [] and empty.attribution is None and empty.overlay is None


@pytest.mark.parametrize("name", END_TO_END)
def test_interpret_logit_on_the_device(gpu, name):
    meta, rec, net, x, noise, _ = _case(name, gpu)
    lut = _lut()
    c = int(rec["class_targets"][0])
    kw = dict(method="idg", steps=8, batch_size=4, exp_noise=None if noise is None else noise.to(gpu),
              lut=as_tensor(lut, gpu))
    res = S.interpret_logit(net, x.to(gpu), c, **kw)
    assert res.rgba.is_cuda and res.rgba.shape == (64, 64, 4)
    host = res.cpu()
    want = R.normalize_maps(host.attribution.maps.numpy(), 99, fallback=False)
    for f in FIELDS:
        assert same_bits(getattr(host.saliency, f), want[f]), f
    assert same_bits(host.image, R.unnormalize(x.numpy()))
    assert same_bits(host.rgba, R.colormap(want["normalized"][0], lut))
    again = S.interpret_logit(net, x.to(gpu), c, **kw).cpu()
    assert torch.equal(again.rgba, host.rgba) and torch.equal(again.attribution.maps, host.attribution.maps)


@pytest.mark.parametrize("grad_mode", [True, False])
def test_no_side_effects_on_the_net(gpu, grad_mode):
    net, cpu_net, x, c, thr, sel, kw = _prototype_call("pipnet_mid_addon", gpu)
    xs = x.to(gpu).unsqueeze(0)
    with torch.no_grad():
        before = [t.clone() for t in net(xs, inference=True)]
    flags = [p.requires_grad for p in net.parameters()]
    assert any(flags)
    with torch.set_grad_enabled(grad_mode):
        res = S.interpret_prototypes(net, xs, c, **kw)
        logit = S.interpret_logit(net, xs, c, method="ig", steps=8, batch_size=4)
        assert torch.is_grad_enabled() == grad_mode
    assert not res.overlay.requires_grad and not logit.saliency.normalized.requires_grad and not net.training
    assert all(p.grad is None for p in net.parameters())
    assert [p.requires_grad for p in net.parameters()] == flags
    with torch.no_grad():
        after = net(xs, inference=True)
    for a, b in zip(before, after):
        assert torch.equal(a, b)


def test_refused_nets_are_refused_by_attribute(gpu):
    meta, _ = load_golden("pipnet_resnet50_small")
    net = build_model(meta).to(gpu)
    x = torch.zeros(3, 64, 64, device=gpu)
    with pytest.raises(NotImplementedError, match="torch_backend"):
        S.interpret_logit(net, x, 0, steps=8, batch_size=4)
    with pytest.raises(NotImplementedError, match="torch_backend"):
        S.interpret_prototypes(net, x, 0, steps=8, batch_size=4, threshold=-1.0)
    with pytest.raises(ValueError):
        S.interpret_logit(_case("pipnet_mid_addon", gpu)[2], x, 0, method="gig", steps=8, batch_size=4)


# ---- end to end against the reference's recording ------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", END_TO_END)
def test_normalised_maps_match_the_reference_recording(gpu, name, kind, method):
    """The device maps lie within eps = MAP_BOUND * ref_err * max|ref64| of the float64 reference per channel.
    Folding is 1-Lipschitz per channel (3 eps on the folded map), order statistics are 1-Lipschitz in the sup
    norm (numerator and denominator move by at most 6 eps each), so a normalised value moves by at most
    12 eps / (D - 6 eps), D the recorded denominator, plus four float32 roundings of values in [0, 1].  The
    generator kept only targets whose rule cannot flip."""
    meta, rec, net, x, noise, _ = _case(name, gpu)
    _, srec = load_saliency(name)
    key = f"{kind}_{method}"
    assert srec[key + "_keep"].all()
    res = attribute(net, x.to(gpu), rec[f"{kind}_targets"].tolist(), kind=kind, method=method, steps=meta["steps"],
                    batch_size=meta["batch_size"], baseline=meta["baseline"],
                    exp_noise=None if noise is None else noise.to(gpu))
    sal = S.normalize_maps(res.maps, 98 if kind == "prototype" else 99, fallback=kind == "prototype").cpu()
    worst = 0.0
    for i in range(2):
        eps = MAP_BOUND * float(rec[key + "_ref_err"][i]) * float(np.abs(rec[key + "_ref64"][i]).max())
        assert eps == float(srec[key + "_eps"][i])
        d = float(srec[key + "_den"][i])
        bound = 12 * eps / (d - 6 * eps) + 4 * 2.0 ** -24
        dev = float(np.abs(sal.normalized[i].double().numpy() - srec[key + "_normalized"][i].astype(np.float64)).max())
        print(f"SALIENCY_RATIO {name} {key}[{i}] deviation {dev:.3e} bound {bound:.3e} ratio {dev / bound:.3f}")
        assert int(sal.rule[i]) == int(srec[key + "_rule"][i]), (name, key, i)
        worst = max(worst, dev / bound)
    assert worst <= 1.0, (name, key, worst)
