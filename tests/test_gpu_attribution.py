"""Integrated-gradients attribution on the GPU (count_pipnet_amd.attribution, csrc/attribution.hip).

* every new kernel against torch autograd / torch arithmetic in float64 on the same inputs;
* ``attribute`` on the HIP path against every fixture of tests/golden/attr (the reference's own
  IG / LeftIG / IDG runs): CountPIPNet scores, cutoffs and IDG placements exactly, maps to
  ``MAP_BOUND * ref_err`` of the recorded float64 reference;
* invariance (chunk size, multi-target, run to run), no side effects, unsupported setups.

Measured err_hip / ref_err per fixture map on an MI355X: 0.80 .. 2.42 (the table of DESIGN.md).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from attr_util import KINDS, METHODS, attr_image, attr_names, attr_noise, load_attr, rel_err
from count_pipnet_amd import kernels as K
from count_pipnet_amd.attribution import attribute
from golden_util import load_golden
from model_util import build_model

pytestmark = pytest.mark.gpu

NAMES = attr_names()
# (fixture, kind) pairs with recorded targets (the full backbone's fixture records prototype targets only)
CASES = [(n, k) for n in NAMES for k in KINDS if len(load_attr(n)[1][f"{k}_targets"])]
# err_hip <= MAP_BOUND * ref_err: the smallest power of two that is at least twice the worst ratio
# measured over all 54 fixture maps (2.42, count_linear_full prototype idg; the others 0.80 .. 1.43;
# the factor two: another summation order on another ROCm build); never above 16.
MAP_BOUND = 8
_NETS = {}


def _case(name, dev):
    """(meta, arrays, net on the device, image, noise) of a fixture; built once, never changed."""
    if name not in _NETS:
        meta, rec = load_attr(name)
        noise = attr_noise(meta)
        _NETS[name] = (meta, rec, build_model(meta).to(dev), attr_image(meta).to(dev),
                       None if noise is None else noise.to(dev))
    return _NETS[name]


def _rel(a: torch.Tensor, ref64: torch.Tensor) -> float:
    """max|a - ref| / max|ref|; a reference that is zero throughout (P = 1: the softmax is constant)
    asks for an exact zero."""
    diff, top = float((a.double().cpu() - ref64.cpu()).abs().max()), float(ref64.abs().max())
    if top == 0.0:
        return 0.0 if diff == 0.0 else float("inf")
    return diff / top


# ---- kernels ------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(1, 1), (6, 6), (8, 5)])
@pytest.mark.parametrize("p", [1, 16, 33, 768])
def test_head_backward_kernel(gpu, p, hw):
    """Max and sum modes against float64 autograd through softmax + pooling on the same logits:
    1e-6 of the map's maximum (the soft map handed to the kernel is one exp and one reduction deep).
    Logits of scale 0.5: no softmax value comes near 1, where s (1 - s) asks for digits of 1 - s that
    a float32 soft map no longer holds (an input-conditioning matter, the same for any float32 backward)."""
    h, w = hw
    g = torch.Generator().manual_seed(1000 * p + 10 * h + w)
    for b in (1, 3):
        logits = (torch.randn(b, h, w, p, generator=g) * 0.5).to(gpu)
        dense = torch.randn(b, p, generator=g)
        onehot = torch.zeros(b, p)
        onehot[:, p // 2] = 1.0
        for u in (onehot, dense):
            u_dev = u.to(gpu)
            for tau in (1.0, 0.5):
                l64 = logits.double().cpu().requires_grad_(True)
                # max mode: nn.Softmax(dim=1) + AdaptiveMaxPool2d (tie-free random logits)
                soft, pooled, loc = K.softmax_pool_argmax(logits, write_proto=True)
                got = K.attr_head_backward(soft, u_dev, loc, 0, tau)
                s64 = l64.softmax(dim=-1)
                (ref,) = torch.autograd.grad((s64.flatten(1, 2).amax(dim=1) * u.double()).sum(), l64)
                assert _rel(got, ref) <= 1e-6, ("max", p, hw, b, tau)
                # sum mode: softmax(logits / tau) + spatial sum (1 / tau is a power of two: the scaling is exact)
                soft, _ = K.softmax_pool((logits / tau).contiguous(), pool_mode=1)
                got = K.attr_head_backward(soft, u_dev, None, 1, tau)
                y64 = (l64 / tau).softmax(dim=-1)
                (ref,) = torch.autograd.grad((y64.sum(dim=(1, 2)) * u.double()).sum(), l64)
                assert _rel(got, ref) <= 1e-6, ("sum", p, hw, b, tau)


@pytest.mark.parametrize("hw", [(8, 8), (8, 12), (20, 20)])
@pytest.mark.parametrize("b", [1, 3])
def test_stem_dx_kernel(gpu, b, hw):
    """Input gradient of Conv2d(3, 96, 4, 4) against float64 autograd: 1e-6 of the maximum (96 fp32 terms)."""
    h, w = hw
    g = torch.Generator().manual_seed(7 * h + w + b)
    wt = torch.randn(96, 3, 4, 4, generator=g) * 0.1
    dz = torch.randn(b, h // 4, w // 4, 96, generator=g)
    x64 = torch.zeros(b, 3, h, w, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x64, wt.double(), stride=4)
    (ref,) = torch.autograd.grad(y, x64, grad_outputs=dz.double().permute(0, 3, 1, 2))
    got = K.attr_stem_dx(dz.to(gpu), wt.to(gpu), h, w)
    assert got.shape == (b, 3, h, w) and _rel(got, ref) <= 1e-6
    # into padded rows of a larger store (the path's gradient store): same bits, the padding untouched
    n = 3 * h * w
    store = torch.full((b + 1, n + 4), -7.0, device=gpu)
    K.attr_stem_dx(dz.to(gpu), wt.to(gpu), h, w, out=store[:b])
    assert torch.equal(store[:b, :n].reshape(b, 3, h, w), got)
    assert bool((store[:b, n:] == -7.0).all()) and bool((store[b] == -7.0).all())


def test_stem_dx_kernel_ragged_image(gpu):
    """Rows / columns beyond the last whole 4 x 4 patch get a zero gradient."""
    g = torch.Generator().manual_seed(5)
    wt = torch.randn(96, 3, 4, 4, generator=g) * 0.1
    dz = torch.randn(2, 2, 3, 96, generator=g)
    x64 = torch.zeros(2, 3, 10, 13, dtype=torch.float64, requires_grad=True)
    (ref,) = torch.autograd.grad(F.conv2d(x64, wt.double(), stride=4), x64,
                                 grad_outputs=dz.double().permute(0, 3, 1, 2))
    got = K.attr_stem_dx(dz.to(gpu), wt.to(gpu), 10, 13)
    assert _rel(got, ref) <= 1e-6
    assert bool((got[:, :, 8:] == 0).all()) and bool((got[:, :, :, 12:] == 0).all())


@pytest.mark.parametrize("hw", [(8, 8), (8, 12), (20, 20)])
@pytest.mark.parametrize("s", [1, 3, 8])
def test_path_images_kernel(gpu, s, hw):
    """baseline + alpha (x - baseline) as one fused multiply-add per element: exactly the float64
    value of alpha * float32(x - b) + b rounded once; channel 3 of the NHWC output is zero."""
    h, w = hw
    g = torch.Generator().manual_seed(100 * s + h + w)
    x = torch.randn(3, h, w, generator=g)
    alpha = torch.rand(s, generator=g)
    alpha[0] = 0.0
    alpha[-1] = 1.0 if s > 1 else alpha[-1]
    for base in (0.25, torch.randn(3, h, w, generator=g)):
        bt = base if torch.is_tensor(base) else torch.full_like(x, base)
        diff = (x - bt).double()
        want = (alpha.double().view(-1, 1, 1, 1) * diff + bt.double()).float()          # [S,3,H,W]
        got = K.attr_path_images(x.to(gpu), base.to(gpu) if torch.is_tensor(base) else base, alpha.to(gpu)).cpu()
        assert got.shape == (s, h, w, 4)
        assert torch.equal(got[..., :3].permute(0, 3, 1, 2), want)
        assert bool((got[..., 3] == 0).all())


def _ulp_close(a: torch.Tensor, ref: torch.Tensor) -> bool:
    up = torch.nextafter(ref, torch.full_like(ref, float("inf")))
    dn = torch.nextafter(ref, torch.full_like(ref, float("-inf")))
    return bool(((a == ref) | (a == up) | (a == dn)).all())


@pytest.mark.parametrize("s", [2, 8])
def test_path_weights_kernel(gpu, s):
    """Cutoffs exactly, weights to 1 ulp of the float64 formulas, the three methods."""
    g = torch.Generator().manual_seed(s)
    rand = torch.randn(s, generator=g)
    rising = torch.linspace(0.1, 2.0, s)
    vectors = {"random": rand, "rising": rising, "nonpositive": -torch.rand(s, generator=g) - 0.5,
               "zero_max": torch.cat([torch.zeros(1), -torch.ones(s - 1)]), "first_step": torch.linspace(2.0, 1.9, s)}
    for name, sc in vectors.items():
        w, cut = K.attr_path_weights(sc.to(gpu), "ig")
        assert int(cut) == s and _ulp_close(w.cpu(), torch.full((s,), 1.0 / s, dtype=torch.float64).float())
        w, cut = K.attr_path_weights(sc.to(gpu), "lig")
        above = torch.where(sc > sc.max() * torch.tensor(0.9))[0]          # the reference's float32 test
        want = max(int(above[0]) if len(above) else 1, 1)
        if name in ("nonpositive", "zero_max", "first_step"):
            assert want == 1
        assert int(cut) == want, (name, int(cut), want)
        ref = torch.zeros(s, dtype=torch.float64)
        ref[:want] = 1.0 / want
        assert _ulp_close(w.cpu(), ref.float())
        # idg on a non-uniform layout
        sub = torch.rand(s, generator=g) * 0.2 + 0.01
        alphas = torch.cumsum(sub, 0) - sub[0]
        w, cut = K.attr_path_weights(sc.to(gpu), "idg", alphas.to(gpu), sub.to(gpu))
        slope = torch.zeros(s, dtype=torch.float64)
        slope[1:] = (sc[1:].double() - sc[:-1].double()) / (alphas[1:].double() - alphas[:-1].double())
        assert int(cut) == s and _ulp_close(w.cpu(), (slope * sub.double() / s).float()), name
    assert K.attr_path_weights(rising.to(gpu), "lig")[1].dtype == torch.int64


@pytest.mark.parametrize("hw", [(5, 7), (16, 16)])
@pytest.mark.parametrize("s", [1, 3, 8])
def test_path_reduce_kernel(gpu, s, hw):
    """(x - b) * sum_i w_i g_i against float64: 1e-6 of the maximum; rows padded to a multiple of four
    floats take the 16-byte path with a scalar tail, unpadded odd rows the scalar path -- same bits."""
    h, w = hw
    n = 3 * h * w
    g = torch.Generator().manual_seed(10 * s + h)
    x = torch.randn(3, h, w, generator=g)
    grads = torch.randn(s, n, generator=g)
    wt = torch.randn(s, generator=g)
    for base in (0.0, torch.randn(3, h, w, generator=g)):
        bt = base if torch.is_tensor(base) else torch.full_like(x, base)
        ref = (x - bt).double() * (wt.double().view(-1, 1) * grads.double()).sum(0).view(3, h, w)
        bdev = base.to(gpu) if torch.is_tensor(base) else base
        plain = K.attr_path_reduce(grads.to(gpu), wt.to(gpu), x.to(gpu), bdev)
        ld = (n + 3) // 4 * 4
        store = torch.zeros(s, ld, device=gpu)
        store[:, :n] = grads.to(gpu)
        padded = K.attr_path_reduce(store, wt.to(gpu), x.to(gpu), bdev)
        assert plain.shape == (3, h, w) and _rel(plain, ref) <= 1e-6
        assert torch.equal(plain, padded)


# ---- end to end against the reference's runs -----------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name,kind", CASES)
def test_attribute_matches_reference(gpu, name, kind, method):
    meta, rec, net, x, noise = _case(name, gpu)
    key = f"{kind}_{method}"
    res = attribute(net, x, rec[f"{kind}_targets"].tolist(), kind=kind, method=method, steps=meta["steps"],
                    batch_size=meta["batch_size"], baseline=meta["baseline"], exp_noise=noise).cpu()
    assert res.maps.shape == (2, 3, meta["case"]["size"], meta["case"]["size"]) and res.maps.dtype == torch.float32
    count = meta["case"]["model"] == "count_pipnet"
    got, want = res.scores.numpy(), rec[key + "_scores"]
    print(f"ATTR_SCORES {name} {key} max rel diff {float(np.abs(got - want).max() / np.abs(want).max()):.2e}")
    if count and meta["case"]["activation"] == "gumbel_softmax" and kind == "prototype":
        assert np.array_equal(got, want), (name, key)              # hard counts: exact
    elif count and kind == "class" and meta["case"]["intermediate_layer"] in ("onehot", "identity"):
        # the logit of hard counts: a sum of at most P * max_count = 48 non-negative float32 products,
        # taken in another order than the recording's CPU GEMM: 48 * 2^-24 relative.  (LinearFull's
        # signed weights cancel: its logits are held as a float32 forward, below.)
        assert np.allclose(got, want, rtol=48 * 2.0 ** -24, atol=0), (name, key)
    else:
        assert np.allclose(got, want, rtol=1e-4, atol=1e-6), (name, key)     # a float32 forward of the whole net
    assert np.array_equal(res.cutoff.numpy(), rec[key + "_cutoff"]), (name, key)
    assert np.array_equal(res.alphas.numpy(), rec[key + "_alphas"]), (name, key)          # the IDG placements
    ratios = []
    for i in range(2):
        err, ref_err = rel_err(res.maps[i], rec[key + "_ref64"][i]), float(rec[key + "_ref_err"][i])
        ratios.append(err / ref_err)
        print(f"ATTR_RATIO {name} {key}[{i}] err_hip {err:.3e} ref_err {ref_err:.3e} ratio {err / ref_err:.2f}")
    assert max(ratios) <= MAP_BOUND, (name, key, ratios)


# ---- invariance -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["count_onehot", "c1_count_identity"])
def test_chunk_size_invariance(gpu, name):
    """batch_size 4 against 8: identical CountPIPNet scores under a fixed seed (the noise of a step
    does not depend on the chunking); on the fixture's noise both stay within the bound."""
    meta, rec, net, x, noise = _case(name, gpu)
    for kind in KINDS:
        ts = rec[f"{kind}_targets"].tolist()
        a = attribute(net, x, ts, kind=kind, method="lig", steps=8, batch_size=4, seed=1234)
        b = attribute(net, x, ts, kind=kind, method="lig", steps=8, batch_size=8, seed=1234)
        assert torch.equal(a.scores, b.scores) and torch.equal(a.cutoff, b.cutoff), (name, kind)
        c = attribute(net, x, ts, kind=kind, method="ig", steps=8, batch_size=8, exp_noise=noise)
        assert np.allclose(c.scores.cpu().numpy(), rec[f"{kind}_ig_scores"], rtol=48 * 2.0 ** -24, atol=0)
        for i in range(2):
            assert rel_err(c.maps[i], rec[f"{kind}_ig_ref64"][i]) <= MAP_BOUND * float(rec[f"{kind}_ig_ref_err"][i])


@pytest.mark.parametrize("name,method", [("pipnet_mid_addon", "ig"), ("count_onehot", "idg"),
                                         ("count_linear_full", "lig")])
def test_multi_target_equals_single_target_bitwise(gpu, name, method):
    meta, rec, net, x, noise = _case(name, gpu)
    for kind in KINDS:
        ts = rec[f"{kind}_targets"].tolist()
        kw = dict(kind=kind, method=method, steps=8, batch_size=4, exp_noise=noise)
        both = attribute(net, x, ts, **kw)
        again = attribute(net, x, ts, **kw)
        for f in ("maps", "scores", "alphas", "weights", "cutoff"):
            assert torch.equal(getattr(both, f), getattr(again, f)), (name, kind, f)      # run to run
        for i, t in enumerate(ts):
            one = attribute(net, x, [t], **kw)
            for f in ("maps", "scores", "alphas", "weights", "cutoff"):
                assert torch.equal(getattr(both, f)[i], getattr(one, f)[0]), (name, kind, t, f)


# ---- side effects, unsupported setups ---------------------------------------------------------------
@pytest.mark.parametrize("grad_mode", [True, False])
def test_no_side_effects_on_the_net(gpu, grad_mode):
    meta, rec, net, x, noise = _case("pipnet_mid_addon", gpu)
    xs = x.unsqueeze(0)
    with torch.no_grad():
        before = [t.clone() for t in net(xs, inference=True)]
    flags = [p.requires_grad for p in net.parameters()]
    assert any(flags)
    with torch.set_grad_enabled(grad_mode):
        res = attribute(net, xs, rec["class_targets"].tolist(), kind="class", method="idg", steps=8, batch_size=4)
        assert torch.is_grad_enabled() == grad_mode
    assert not res.maps.requires_grad and not net.training
    assert all(p.grad is None for p in net.parameters())
    assert [p.requires_grad for p in net.parameters()] == flags
    with torch.no_grad():
        after = net(xs, inference=True)
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    assert np.array_equal(res.cutoff.cpu().numpy(), rec["class_idg_cutoff"])


def test_argument_errors_on_the_device(gpu):
    meta, rec, net, x, noise = _case("pipnet_mid_addon", gpu)
    with pytest.raises(ValueError):
        attribute(net, x, [0], steps=10, batch_size=4)
    with pytest.raises(ValueError):
        attribute(net, x, [net._num_prototypes], steps=8, batch_size=4)
    with pytest.raises(ValueError):
        attribute(net, x, [0], steps=8, batch_size=4, baseline=torch.zeros(3, 8, 8))


def test_resnet_backbone_is_refused(gpu):
    meta, _ = load_golden("pipnet_resnet50_small")
    net = build_model(meta).to(gpu)
    x = torch.zeros(3, 64, 64, device=gpu)
    with pytest.raises(NotImplementedError, match="torch_backend"):
        attribute(net, x, [0], steps=8, batch_size=4)
