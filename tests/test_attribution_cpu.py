"""count_pipnet_amd.attribute on its torch path (CPU) against the reference's own IG / LeftIG / IDG
runs (tests/golden/attr, recorded by tests/golden/gen_golden_attr.py), the host IDG schedule, the
argument errors and the no-side-effect contract."""
import numpy as np
import pytest
import torch

from attr_util import KINDS, METHODS, attr_image, attr_names, attr_noise, load_attr, rel_err
from count_pipnet_amd.attribution import Attribution, attribute, idg_schedule, uniform_slopes
from count_pipnet_amd.backend import torch_backend
from model_util import build_model

NAMES = attr_names()
# (fixture, kind) pairs with recorded targets (the full backbone's fixture records prototype targets only)
CASES = [(n, k) for n in NAMES for k in KINDS if len(load_attr(n)[1][f"{k}_targets"])]
_NETS = {}


def _case(name):
    """(meta, arrays, net, image, noise) of a fixture; built once and shared, never changed."""
    if name not in _NETS:
        meta, rec = load_attr(name)
        _NETS[name] = (meta, rec, build_model(meta), attr_image(meta), attr_noise(meta))
    return _NETS[name]


@pytest.fixture
def one_thread():
    """The fixtures' float32 scores were recorded single-threaded; they are compared exactly."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def test_fixture_set():
    assert set(NAMES) == {"pipnet_mid_addon", "count_onehot", "c1_count_identity", "count_linear_full",
                          "pipnet_convnext26_64"}
    for name in NAMES:
        meta, rec = load_attr(name)
        assert (meta["steps"], meta["batch_size"], meta["baseline"]) == (8, 4, 0.0)
        for kind in KINDS:
            if (name, kind) == ("pipnet_convnext26_64", "class"):     # no class target of 768 prototypes is decisive
                assert rec["class_targets"].shape == (0,)
                continue
            assert rec[f"{kind}_targets"].shape == (2,)
            for method in METHODS:
                assert rec[f"{kind}_{method}_ref64"].shape == (2, 3, meta["case"]["size"], meta["case"]["size"])
                assert (rec[f"{kind}_{method}_ref_err"] > 0).all() and (rec[f"{kind}_{method}_ref_err"] < 1e-4).all()


@pytest.mark.parametrize("name", NAMES)
def test_idg_schedule_reproduces_recorded_layout(name):
    """The host schedule gives the reference's alphas and substeps bit for bit from its slopes."""
    meta, rec = load_attr(name)
    for kind in KINDS:
        for i in range(len(rec[f"{kind}_targets"])):
            slopes = torch.from_numpy(rec[f"{kind}_idg_slopes"][i])
            alphas, sub = idg_schedule(slopes, meta["steps"], float(rec[f"{kind}_idg_step_size"][i]))
            assert np.array_equal(alphas.numpy(), rec[f"{kind}_idg_alphas"][i]), (name, kind, i)
            assert np.array_equal(sub.numpy(), rec[f"{kind}_idg_substeps"][i]), (name, kind, i)


def test_uniform_slopes():
    s = torch.tensor([0.0, 1.0, 3.0, 2.0])
    slopes, step = uniform_slopes(s)
    lin = torch.linspace(0, 1, 4)
    assert step == float(lin[1] - lin[0])
    assert torch.equal(slopes, torch.tensor([0.0, 1.0 / step, 2.0 / step, -1.0 / step]))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name,kind", CASES)
def test_torch_path_matches_reference(name, kind, method, one_thread):
    """Maps within 2 ref_err of the float64 reference; scores and cutoffs exactly the float32 run's."""
    meta, rec, net, x, noise = _case(name)
    key = f"{kind}_{method}"
    with torch_backend():
        res = attribute(net, x, rec[f"{kind}_targets"].tolist(), kind=kind, method=method, steps=meta["steps"],
                        batch_size=meta["batch_size"], baseline=meta["baseline"], exp_noise=noise)
    assert isinstance(res, Attribution) and res.maps.shape == (2,) + tuple(x.shape)
    assert np.array_equal(res.scores.numpy(), rec[key + "_scores"]), (name, key)
    assert res.cutoff.dtype == torch.int64 and np.array_equal(res.cutoff.numpy(), rec[key + "_cutoff"])
    assert np.array_equal(res.alphas.numpy(), rec[key + "_alphas"])
    for i in range(2):
        err, ref_err = rel_err(res.maps[i], rec[key + "_ref64"][i]), float(rec[key + "_ref_err"][i])
        print(f"{name} {key}[{i}] err {err:.3e} ref_err {ref_err:.3e} ratio {err / ref_err:.2f}")
        assert err <= 2 * ref_err, (name, key, i, err, ref_err)
    # the coefficients are what the reduction applies: weights sum to 1 for ig / lig
    if method != "idg":
        assert torch.allclose(res.weights.sum(dim=1), torch.ones(2), atol=1e-6)
        assert ((res.weights > 0).sum(dim=1) == res.cutoff).all()


def test_argument_errors():
    meta, rec, net, x, noise = _case("pipnet_mid_addon")
    with torch_backend():
        for kw in (dict(steps=10, batch_size=4), dict(steps=1, batch_size=1), dict(method="gig"),
                   dict(kind="logit"), dict(steps=8, batch_size=0)):
            with pytest.raises(ValueError):
                attribute(net, x, [0], **{"steps": 8, "batch_size": 4, **kw})
        for kind, bad in (("prototype", net._num_prototypes), ("class", 10), ("prototype", -1)):
            with pytest.raises(ValueError):
                attribute(net, x, [bad], kind=kind, steps=8, batch_size=4)
        with pytest.raises(ValueError):
            attribute(net, x, [], steps=8, batch_size=4)
        with pytest.raises(ValueError):
            attribute(net, x[:2], [0], steps=8, batch_size=4)


@pytest.mark.parametrize("grad_mode", [True, False])
def test_no_side_effects_on_the_net(grad_mode):
    """No .grad appears, requires_grad flags stay, the net ends in eval mode, grad mode on or off."""
    meta, rec, net, x, noise = _case("count_onehot")
    frozen = next(net._net.parameters())
    was = frozen.requires_grad
    frozen.requires_grad_(False)
    flags = [p.requires_grad for p in net.parameters()]
    try:
        net.train()
        with torch.set_grad_enabled(grad_mode), torch_backend():
            res = attribute(net, x.unsqueeze(0), [int(rec["class_targets"][0])], kind="class", method="lig",
                            steps=8, batch_size=4, exp_noise=noise)
            assert torch.is_grad_enabled() == grad_mode
        assert not net.training
        assert all(p.grad is None for p in net.parameters())
        assert [p.requires_grad for p in net.parameters()] == flags and not frozen.requires_grad
        assert not res.maps.requires_grad
        assert np.array_equal(res.scores[0].numpy(), rec["class_lig_scores"][0])
    finally:
        frozen.requires_grad_(was)


def test_tensor_baseline_and_cpu_copy():
    """A zero image as baseline is the float baseline 0.0; .cpu() returns the same type."""
    meta, rec, net, x, noise = _case("pipnet_mid_addon")
    t = [int(rec["prototype_targets"][0])]
    with torch_backend():
        a = attribute(net, x, t, steps=8, batch_size=4, baseline=0.0)
        b = attribute(net, x, t, steps=8, batch_size=4, baseline=torch.zeros_like(x))
    assert torch.equal(a.maps, b.maps)
    assert isinstance(a.cpu(), Attribution) and torch.equal(a.cpu().maps, a.maps)
