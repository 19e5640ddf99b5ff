"""Attribution images without a GPU (count_pipnet_amd.saliency on its torch route, tests/saliency_ref.py).

* the numpy restatement ``saliency_ref`` against what the reference's own statements recorded
  (tests/golden/saliency/steps.npz, written by tests/golden/gen_golden_saliency.py), bit for bit;
* the torch route of every public function against ``saliency_ref``, bit for bit, over the size / T /
  percentile grids of tests/saliency_cases.py;
* ``active_prototypes`` against a direct restatement of interpret_idg.py:319-378 on the module's own forward;
* ``interpret_prototypes`` / ``interpret_logit`` on CPU nets stage by stage, the empty result, the argument errors.
"""
import numpy as np
import pytest
import torch

import saliency_ref as R
from attr_util import attr_image, attr_noise, load_attr
from count_pipnet_amd import saliency as S
from count_pipnet_amd.attribution import Attribution
from model_util import build_model
from saliency_cases import (COUNTS, END_TO_END, PERCENTILES, SIZES, as_tensor, decisive_choice, direct_contributions,
                            load_saliency, same_bits, sample_maps, selection_noise)

_NETS = {}


def _case(name):
    """(meta, arrays, net, image, noise) of an attribution fixture; built once and shared, never changed."""
    if name not in _NETS:
        meta, rec = load_attr(name)
        _NETS[name] = (meta, rec, build_model(meta), attr_image(meta), attr_noise(meta))
    return _NETS[name]


# ---- the restatement against the reference's own results ---------------------------------------------
def test_ref_fold_and_percentile_equal_the_recording():
    meta, rec = load_saliency("steps")
    folded = R.fold(rec["maps"])
    assert folded.dtype == np.float32 and np.array_equal(folded, rec["folded"])
    assert rec["percentiles"].tolist() == [float(q) for q in PERCENTILES]
    for j, q in enumerate(PERCENTILES):
        vmin, vtop, lo, hi, vq = R.order_stats(rec["folded"], q)
        assert vq.dtype == np.float32 and np.array_equal(vq, rec["vq"][:, j]), q
        assert np.array_equal(vmin, rec["vmin"]) and np.array_equal(vtop, rec["vtop"])
        live = np.array([np.percentile(f, q) for f in rec["folded"]])          # the installed numpy, fixture maps
        assert live.dtype == np.float32 and np.array_equal(vq, live), (q, np.__version__)


def test_ref_normalisation_rules_equal_the_recording():
    meta, rec = load_saliency("steps")
    assert rec["rule_98"].tolist() == [0, 1, 2]           # percentile range, global-max fallback, constant map
    out = R.normalize_maps(rec["maps"], 98)
    assert np.array_equal(out["rule"], rec["rule_98"])
    assert out["normalized"].dtype == np.float32 and np.array_equal(out["normalized"], rec["normalized_98"])
    assert float(out["normalized"][2].max()) == 0.0 and float(out["normalized"][1].max()) == 1.0


def test_ref_blend_image_and_colour_map_equal_the_recording():
    meta, rec = load_saliency("steps")
    assert meta["palette"] == R.PALETTE == S.PLOTLY_QUALITATIVE
    rgba = R.blend(rec["blend_in"])
    assert rgba.dtype == np.float64 and np.array_equal(rgba, rec["blend_rgba"])
    img = R.unnormalize(rec["image"])
    assert img.dtype == np.float32 and np.array_equal(img, rec["image_unnormalized"])
    logit = R.normalize_maps(rec["maps"][:1], 99, fallback=False)
    assert np.array_equal(logit["normalized"][0], rec["logit_normalized"])
    assert rec["blues_lut"].shape == (256, 4) and rec["blues_lut"].dtype == np.uint8
    assert np.array_equal(R.colormap(rec["logit_normalized"], rec["blues_lut"]), rec["logit_rgba"])


# ---- the torch route against the restatement ---------------------------------------------------------
@pytest.mark.parametrize("t", COUNTS)
@pytest.mark.parametrize("hw", SIZES)
def test_normalize_maps_equals_ref(hw, t):
    maps = sample_maps(t, *hw)
    for q in PERCENTILES:
        for fallback in (True, False):
            want = R.normalize_maps(maps, q, fallback)
            got = S.normalize_maps(as_tensor(maps), q, fallback=fallback)
            assert isinstance(got, S.SaliencyMaps) and isinstance(got.cpu(), S.SaliencyMaps)
            for f in ("folded", "vmin", "vq", "vtop", "rule", "normalized"):
                assert same_bits(getattr(got, f), want[f]), (hw, t, q, fallback, f)
            if t:                                                               # already folded input: same result
                again = S.normalize_maps(as_tensor(want["folded"]), q, fallback=fallback)
                assert same_bits(again.normalized, want["normalized"]) and same_bits(again.rule, want["rule"])
    if t >= 3 and hw[0] * hw[1] > 2:
        assert R.normalize_maps(maps, 98)["rule"][:3].tolist() == [0, 1, 2]    # the grid meets every rule


@pytest.mark.parametrize("t", COUNTS)
@pytest.mark.parametrize("hw", SIZES)
def test_blend_and_colour_map_equal_ref(hw, t):
    norm = R.normalize_maps(sample_maps(t, *hw), 98)["normalized"]
    got = S.blend_maps(as_tensor(norm))
    assert got.shape == hw + (4,) and same_bits(got, R.blend(norm))
    if t:
        colours = np.random.default_rng(t).random((t, 3))
        assert same_bits(S.blend_maps(as_tensor(norm), as_tensor(colours)), R.blend(norm, colours))
    lut = load_saliency("steps")[1]["blues_lut"]
    assert same_bits(S.colormap_rgba8(as_tensor(norm), as_tensor(lut)), R.colormap(norm, lut))


def test_palette_wraps_after_ten():
    c = S.palette_colours(12)
    assert c.dtype == torch.float64 and same_bits(c, R.palette(12))
    assert torch.equal(c[10], c[0]) and torch.equal(c[11], c[1]) and not torch.equal(c[0], c[1])
    assert c[0].tolist() == [0x63 / 255.0, 0x6E / 255.0, 0xFA / 255.0]


@pytest.mark.parametrize("hw", SIZES)
def test_unnormalize_image_equals_ref(hw):
    x = (np.random.default_rng(hw[0] * 100 + hw[1]).standard_normal((3,) + hw) * 1.5).astype(np.float32)
    want = R.unnormalize(x)
    assert same_bits(S.unnormalize_image(as_tensor(x)), want)
    assert same_bits(S.unnormalize_image(as_tensor(x)[None]), want)
    assert float(want.min()) == 0.0 or hw == (1, 1) or float(want.max()) == 1.0      # the clip is exercised
    other = R.unnormalize(x, (0.5, 0.25, 0.125), (0.1, 0.2, 0.3))
    assert same_bits(S.unnormalize_image(as_tensor(x), (0.5, 0.25, 0.125), (0.1, 0.2, 0.3)), other)


def test_percentile_plan_is_numpys_float32_split():
    """k and gamma as numpy 2.2.6 derives them for a float32 array -- the recorded percentiles hang on both."""
    for n in (1, 2, 63, 64, 65, 256, 4096, 4099, 50176):
        for q in PERCENTILES + [12.5, 99.9]:
            k, gamma = S.percentile_plan(n, q)
            rk, rk1, rg = R.percentile_split(n, q)
            assert (k, np.float32(gamma)) == (rk, rg) and 0 <= k < n
    assert S.percentile_plan(4096, 98)[0] == 4013 and S.percentile_plan(1, 98) == (0, 1.0)
    assert S.percentile_plan(10, 100)[0] == 9


# ---- active prototypes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", END_TO_END)
def test_active_prototypes_equal_the_direct_restatement(name):
    meta, rec, net, x, noise = _case(name)
    contrib = direct_contributions(net, x, selection_noise(noise))
    c, thr = decisive_choice(contrib)
    row = contrib[c]
    assert float((row - thr).abs().min()) >= 1e-3                        # nothing hangs on the comparison
    kept = row[row > thr]
    assert len(kept) >= 2 and len(torch.unique(kept)) == len(kept)      # no tie among the kept
    want = torch.where(row > thr)[0]
    want = want[torch.argsort(row[want], descending=True)].tolist()
    got = S.active_prototypes(net, x, c, thr, exp_noise=selection_noise(noise))
    assert isinstance(got, S.ActivePrototypes) and got.indices == want
    assert torch.equal(got.contributions, row) and got.indices == R.active(row.numpy(), thr)
    assert S.active_prototypes(net, x.unsqueeze(0), c, 1e9, exp_noise=selection_noise(noise)).indices == []
    with pytest.raises(ValueError):
        S.active_prototypes(net, x, contrib.shape[0], thr)
    with pytest.raises(ValueError):
        S.active_prototypes(net, x[:2], c, thr)


def test_active_prototypes_orders_ties_by_index():
    assert R.active(np.array([0.5, 0.9, 0.5, 0.0, 0.9], dtype=np.float32), 0.1) == [1, 4, 0, 2]


# ---- the two pipelines on CPU nets ---------------------------------------------------------------------
@pytest.mark.parametrize("name", END_TO_END)
def test_interpret_prototypes_stage_by_stage(name):
    meta, rec, net, x, noise = _case(name)
    sel = selection_noise(noise)
    c, thr = decisive_choice(direct_contributions(net, x, sel))
    kw = dict(method="ig", steps=8, batch_size=4, threshold=thr, exp_noise=noise, selection_noise=sel)
    res = S.interpret_prototypes(net, x, c, **kw)
    assert isinstance(res, S.PrototypeSaliency) and isinstance(res.attribution, Attribution)
    assert res.active.indices == S.active_prototypes(net, x, c, thr, exp_noise=sel).indices
    t = len(res.active.indices)
    assert t >= 2 and res.attribution.maps.shape == (t, 3, 64, 64)
    want = R.normalize_maps(res.attribution.maps.numpy(), 98)
    for f in ("folded", "vmin", "vq", "vtop", "rule", "normalized"):
        assert same_bits(getattr(res.saliency, f), want[f]), f
    assert same_bits(res.overlay, R.blend(want["normalized"]))
    assert same_bits(res.image, R.unnormalize(x.numpy()))
    assert isinstance(res.cpu(), S.PrototypeSaliency)
    colours = np.random.default_rng(3).random((t, 3))
    other = S.interpret_prototypes(net, x, c, percentile=50, colours=as_tensor(colours), **kw)
    assert same_bits(other.overlay, R.blend(R.normalize_maps(res.attribution.maps.numpy(), 50)["normalized"], colours))
    # a threshold above every contribution: the selection alone, nothing else computed
    empty = S.interpret_prototypes(net, x, c, **{**kw, "threshold": 1e9})
    assert empty.active.indices == [] and empty.attribution is None and empty.saliency is None
    assert empty.overlay is None and empty.image is None and isinstance(empty.cpu(), S.PrototypeSaliency)
    with pytest.raises(ValueError):
        S.interpret_prototypes(net, x, c, **{**kw, "colours": torch.zeros(t + 1, 3, dtype=torch.float64)})
    with pytest.raises(ValueError):
        S.interpret_prototypes(net, x, c, **{**kw, "method": "gig"})          # attribute's refusal, unchanged


@pytest.mark.parametrize("name", END_TO_END)
def test_interpret_logit_stage_by_stage(name):
    meta, rec, net, x, noise = _case(name)
    lut = load_saliency("steps")[1]["blues_lut"]
    c = int(rec["class_targets"][0])
    res = S.interpret_logit(net, x, c, method="idg", steps=8, batch_size=4, exp_noise=noise, lut=as_tensor(lut))
    assert isinstance(res, S.LogitSaliency) and res.attribution.maps.shape == (1, 3, 64, 64)
    want = R.normalize_maps(res.attribution.maps.numpy(), 99, fallback=False)
    for f in ("folded", "vmin", "vq", "vtop", "rule", "normalized"):
        assert same_bits(getattr(res.saliency, f), want[f]), f
    assert same_bits(res.image, R.unnormalize(x.numpy()))
    assert res.rgba.shape == (64, 64, 4) and same_bits(res.rgba, R.colormap(want["normalized"][0], lut))
    assert S.interpret_logit(net, x, c, method="ig", steps=8, batch_size=4, exp_noise=noise).rgba is None
    assert isinstance(res.cpu(), S.LogitSaliency)


def test_logit_mode_writes_a_zero_map_where_the_reference_divides_by_zero():
    flat = np.full((1, 3, 4, 4), 0.5, dtype=np.float32)
    out = S.normalize_maps(as_tensor(flat), 99, fallback=False)
    assert out.rule.tolist() == [2] and float(out.normalized.abs().max()) == 0.0


def test_argument_errors():
    maps = as_tensor(sample_maps(2, 4, 4))
    lut = as_tensor(load_saliency("steps")[1]["blues_lut"])
    for q in (-0.5, 100.5, float("nan")):
        with pytest.raises(ValueError):
            S.normalize_maps(maps, q)
    for bad in (maps[0, 0], maps[:, :2], maps.double(), maps.numpy(), maps[None]):
        with pytest.raises(ValueError):
            S.normalize_maps(bad)
    norm = S.normalize_maps(maps).normalized
    for colours in (torch.zeros(3, 3, dtype=torch.float64), torch.zeros(2, 4, dtype=torch.float64), torch.zeros(2, 3)):
        with pytest.raises(ValueError):
            S.blend_maps(norm, colours)
    with pytest.raises(ValueError):
        S.blend_maps(maps)
    for table in (lut[:255], lut.float(), lut[:, :3], lut.numpy()):
        with pytest.raises(ValueError):
            S.colormap_rgba8(norm, table)
    with pytest.raises(ValueError):
        S.colormap_rgba8(norm.double(), lut)
    for x in (torch.zeros(4, 4), torch.zeros(2, 3, 4, 4), torch.zeros(3, 4, 4, dtype=torch.float64)):
        with pytest.raises(ValueError):
            S.unnormalize_image(x)
    meta, rec, net, x, noise = _case("pipnet_mid_addon")
    with pytest.raises(ValueError):
        S.interpret_prototypes(net, x, 0, steps=8, batch_size=4, percentile=101)
    with pytest.raises(ValueError):
        S.interpret_logit(net, x, 0, steps=8, batch_size=4, percentile=-1)
    with pytest.raises(ValueError):
        S.interpret_logit(net, x, 0, steps=8, batch_size=4, lut=lut[:100])
