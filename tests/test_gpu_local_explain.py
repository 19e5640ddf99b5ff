"""Device-side local explanations (count_pipnet_amd.local, pipnet_local_explain_f32) on the GPU.

* the selection kernel against the restatement of the reference loop (tests/local_explain_ref.py,
  util/visualize_prediction.py:63-88 / :138-168), every output element compared exactly;
* explain_predictions end to end on PIP-Net and CountPIPNet against the restatement fed the
  existing forward's own batch-1 outputs, whatever the batching;
* class ranks and kept sets against the CPU oracle where the oracle's own values are decisive.
"""
import argparse

import numpy as np
import pytest
import torch

from count_pipnet_amd import _lib
from count_pipnet_amd import kernels as K
from count_pipnet_amd.local import count_importance_matrix, explain_predictions
from count_pipnet_amd.synthetic import synth_exponential, synth_images
from count_pipnet_amd.topk import img_coordinates, patch_size
from golden_util import golden_args, load_golden
from local_explain_ref import pack, reference_lists
from model_util import build_model
from oracle import ref_cpu

pytestmark = pytest.mark.gpu

MAP = 4                      # planted maps of the kernel tests are MAP x MAP
I_SENTINEL, F_SENTINEL = -77, -12345.0


# ---- the kernel against the restatement ---------------------------------------------------------
def boundary_pairs(limit=3):
    """(score, weight) float32 pairs whose exact product is above 0.01 while its float32 rounding is
    not above float32(0.01): an fp32 keep test drops them, the reference's Python floats keep them.
    A fixed scan: scores 0.1 + i * 0.000437, the weight next to 0.01 / score and its neighbours."""
    lim32 = np.float32(0.01)
    pairs = []
    for i in range(1, 4000):
        s = np.float32(0.1 + i * 0.000437)
        w0 = np.float32(0.01 / float(s))
        for w in (w0, np.nextafter(w0, np.float32(1)), np.nextafter(w0, np.float32(0))):
            prod = float(s) * float(w)                        # exact: two 24-bit significands
            if prod > 0.01 and np.float32(prod) <= lim32:
                pairs.append((s, w))
                break
        if len(pairs) == limit:
            break
    return pairs


def _case(shape, seed):
    """(pooled [B,P], loc [B,P] int32, out [B,K], weight [K,P] -- possibly a view with ldw > P --,
    facts planted) for one (B,P,K,C,M) of the list below."""
    b, p, k, c, m = shape
    g = torch.Generator().manual_seed(seed)
    loc = torch.randint(0, MAP * MAP, (b, p), generator=g, dtype=torch.int32)
    out = torch.randn(b, k, generator=g)
    weight = torch.randn(k, p, generator=g) * 0.2
    facts = {}
    if shape == (1, 1, 1, 1, 1):
        pooled = torch.full((1, 1), 0.7)
        weight = torch.full((1, 1), 0.5)
    elif shape == (3, 16, 9, 3, 16):
        pooled = torch.randint(0, 4, (b, p), generator=g).float()          # counts 0..3: ties everywhere
        pooled[2] = 0.0                                                     # an image with nothing found
        out[0] = torch.tensor([1.0, 0.5, 3.0, 7.0, -2.0, 9.0, 3.0, 0.0, 3.0])      # ranks 2, 3, 4 hold 3.0
        out[1, 4] = -0.0                                                    # -0 == +0: class 4 before 7
        out[1, 7] = 0.0
        facts["ldw"] = p + 3
    elif shape in ((2, 64, 5, 5, 8), (2, 65, 65, 65, 8)):
        pooled = torch.rand(b, p, generator=g) * 0.9 + 0.1                  # all active
        if p == 65:
            pooled[0, 17] = 0.0                                             # image 0: exactly 64, image 1: 65
            out[0, 3] = out[0, 40]                                          # a tie inside the full order
        pooled[1, 5] = pooled[1, 60]                                        # a score tie across the wave boundary
        weight = torch.randn(k, p, generator=g)                             # most products pass: n > M
    elif shape == (2, 768, 200, 3, 64):
        pooled = torch.rand(b, p, generator=g)
        pooled = torch.where(pooled < 0.7, torch.zeros(()), pooled)         # PIP-Net like: ~30 % present
        weight = torch.rand(k, p, generator=g) * 2.0
        weight = torch.where(torch.rand(k, p, generator=g) < 0.05, weight, torch.zeros(()))   # ~5 % non-zero
        out[0, 123] = 50.0                                                  # image 0's best class
        out[1, 7] = out[1, 150] = 40.0                                      # ... and a tie at image 1's top
        pairs = boundary_pairs()
        facts["pairs"] = pairs
        facts["pair_protos"] = [100 + 64 * j for j in range(len(pairs))]
        for pj, (s, w) in zip(facts["pair_protos"], pairs):
            pooled[0, pj] = float(s)
            weight[123, pj] = float(w)
        facts["ldw"] = p + 8
    else:
        assert shape == (1, 2048, 10, 10, 64)
        pooled = torch.rand(b, p, generator=g) + 0.001                      # 2048 active: the largest sort
        pooled[0, 1000] = pooled[0, 11]
        weight = torch.randn(k, p, generator=g) * 0.01                      # products on both sides of 0.01
    if "ldw" in facts:
        big = torch.zeros(k, facts["ldw"])
        big[:, :p] = weight
        weight = big
    return pooled, loc, out, weight, facts


def _planted_maps(pooled, loc):
    """[B,P,MAP,MAP] maps holding the score (1.0 where it is 0 or less) at ``loc`` only: the reference's
    two-step max finds ``loc``."""
    b, p = pooled.shape
    proto = torch.zeros(b, p, MAP * MAP)
    proto.scatter_(2, loc.long().unsqueeze(-1), torch.where(pooled > 0, pooled, torch.ones(())).unsqueeze(-1))
    return proto.view(b, p, MAP, MAP)


def _raw_call(gpu, pooled, loc, out, weight_dev, p, c, m, min_abs=0.01):
    """pipnet_local_explain_f32 into sentinel-filled outputs."""
    b, k = out.shape
    i32 = dict(device=gpu, dtype=torch.int32)
    res = (torch.full((b, c), I_SENTINEL, **i32), torch.full((b, c), F_SENTINEL, device=gpu),
           torch.full((b, c), I_SENTINEL, **i32), torch.full((b, c, m), I_SENTINEL, **i32),
           torch.full((b, c, m), F_SENTINEL, device=gpu), torch.full((b, c, m), F_SENTINEL, device=gpu),
           torch.full((b, c, m), F_SENTINEL, device=gpu), torch.full((b, c, m), I_SENTINEL, **i32))
    _lib.call("pipnet_local_explain_f32", pooled.data_ptr(), loc.data_ptr(), out.data_ptr(), weight_dev.data_ptr(),
              weight_dev.stride(0), b, p, k, c, m, float(min_abs), *[t.data_ptr() for t in res],
              torch.cuda.current_stream(gpu).cuda_stream)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in res)


SHAPES = [(1, 1, 1, 1, 1), (3, 16, 9, 3, 16), (2, 64, 5, 5, 8), (2, 65, 65, 65, 8), (2, 768, 200, 3, 64),
          (1, 2048, 10, 10, 64)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_local_explain_kernel_matches_reference_loop(gpu, shape):
    b, p, k, c, m = shape
    pooled, loc, out, weight, facts = _case(shape, seed=sum(shape))
    w_view = weight[:, :p]
    proto = _planted_maps(pooled, loc)
    want = pack([reference_lists(proto[i:i + 1], pooled[i:i + 1], out[i:i + 1], w_view, c) for i in range(b)], m)

    w_dev = weight.to(gpu)[:, :p]                      # a row view when ldw > P
    assert w_dev.stride(0) == facts.get("ldw", p)
    args = (pooled.to(gpu), loc.to(gpu), out.to(gpu))
    raw = _raw_call(gpu, *args, w_dev, p, c, m)
    for t in raw:                                      # the kernel wrote every element
        assert not (t == (I_SENTINEL if t.dtype == torch.int32 else F_SENTINEL)).any()
    wrapped = tuple(t.cpu() for t in K.local_explain(*args, w_dev, c, m))
    for a, r in zip(wrapped, raw):
        assert a.dtype == r.dtype and torch.equal(a, r)

    cls, cls_logit, n, e_proto, e_sim, e_w, e_simw, e_loc = (t.numpy() for t in raw)
    assert np.array_equal(cls, want["classes"]) and np.array_equal(n, want["count"])
    assert np.array_equal(cls_logit, want["logits"])
    assert np.array_equal(e_proto, want["prototype"])
    assert np.array_equal(e_sim, want["similarity"]) and np.array_equal(e_w, want["weight"])
    assert np.array_equal(e_simw, want["simweight"])
    assert np.array_equal(e_loc, np.where(want["prototype"] < 0, -1, want["h_idx"] * MAP + want["w_idx"]))

    # what the shape is there for did occur
    active = (pooled != 0).sum(dim=1).tolist()
    srt = torch.sort(out, dim=1, descending=True).values
    if shape == (3, 16, 9, 3, 16):
        assert active[2] == 0 and (n[2] == 0).all() and (e_proto[2] == -1).all()
        assert srt[0, c - 1] == srt[0, c] and cls[0].tolist() == [5, 3, 2]          # the tie at the cut: lower index
        assert max(np.unique(pooled[0].numpy(), return_counts=True)[1]) > 1
    if p == 64:
        assert active == [64, 64] and c == k
    if p == 65:
        assert active == [64, 65] and c == k
    if p in (64, 65):
        assert (n > m).any() and (e_proto[n > m] >= 0).all()                         # truncated, the count is the true one
    if p == 768:
        assert facts["pairs"], "the scan found no boundary pair"
        assert cls[0, 0] == 123 and n[0, 0] <= m
        for pj, (s, w) in zip(facts["pair_protos"], facts["pairs"]):
            assert float(s) * float(w) > 0.01 and np.float32(float(s) * float(w)) <= np.float32(0.01)
            assert s * w <= np.float32(0.01)                                         # the fp32 product: dropped
            assert pj in e_proto[0, 0].tolist(), (pj, s, w)                          # the kernel keeps it
        assert (weight[:, :p] != 0).float().mean().item() < 0.06
    if p == 2048:
        assert active == [2048] and 0 < n.min() and (n > m).any()


def test_local_explain_non_finite_values_stay_in_bounds(gpu):
    """NaN / inf scores and logits may land anywhere in the order; every index stays in range, every
    element is written and the counts -- which do not depend on the order -- are still exact."""
    b, p, k, c, m = 2, 70, 7, 3, 8
    g = torch.Generator().manual_seed(9)
    pooled = torch.rand(b, p, generator=g)
    pooled[0, [0, 13, 64, 69]] = torch.tensor([float("nan"), float("inf"), -float("inf"), float("nan")])
    pooled[1] = float("nan")
    out = torch.randn(b, k, generator=g)
    out[0, [1, 4, 5]] = torch.tensor([float("nan"), float("inf"), -float("inf")])
    out[1] = float("nan")
    weight = torch.randn(k, p, generator=g) * 0.1
    weight[2, 5] = float("nan")
    weight[3, 6] = float("inf")
    loc = torch.randint(0, MAP * MAP, (b, p), generator=g, dtype=torch.int32)
    raw = _raw_call(gpu, pooled.to(gpu), loc.to(gpu), out.to(gpu), weight.to(gpu), p, c, m)
    for t in raw:
        assert not (t == (I_SENTINEL if t.dtype == torch.int32 else F_SENTINEL)).any()
    cls, _, n, e_proto, _, _, _, e_loc = raw
    assert ((cls >= 0) & (cls < k)).all() and all(len(set(row.tolist())) == c for row in cls)
    with np.errstate(invalid="ignore"):
        prod = np.abs(pooled.numpy().astype(np.float64)[:, None, :] * weight.numpy().astype(np.float64)[None])
        n_ref = (prod > 0.01).sum(axis=2)                               # a NaN product is never kept
    assert torch.equal(n.long(), torch.from_numpy(n_ref).gather(1, cls.long()))
    filled = torch.arange(m)[None, None, :] < n.clamp(max=m)[..., None]
    assert ((e_proto >= 0) & (e_proto < p))[filled].all() and (e_proto[~filled] == -1).all()
    loc_of = loc[:, None, :].expand(b, c, p).gather(2, e_proto.long().clamp(min=0))
    assert torch.equal(e_loc[filled], loc_of[filled])
    assert (e_loc[~filled] == -1).all()


def test_local_explain_wrapper_rejects_bad_arguments(gpu):
    pooled, loc, out, weight, _ = _case((2, 64, 5, 5, 8), seed=1)
    pooled, loc, out, weight = pooled.to(gpu), loc.to(gpu), out.to(gpu), weight.to(gpu)
    with pytest.raises(RuntimeError):
        K.local_explain(pooled.cpu(), loc, out, weight, 3, 8)
    with pytest.raises(RuntimeError):
        K.local_explain(pooled, loc.long(), out, weight, 3, 8)
    with pytest.raises(RuntimeError):
        K.local_explain(pooled, loc, out, weight[:, :63], 3, 8)
    with pytest.raises(RuntimeError):
        K.local_explain(pooled, loc, out, weight.t().contiguous().t(), 3, 8)      # column stride != 1
    with pytest.raises(RuntimeError):
        K.local_explain(pooled, loc, out, weight, 6, 8)                            # more classes than there are
    with pytest.raises(RuntimeError):
        K.local_explain(pooled, loc, out, weight, 3, 0)
    with pytest.raises(RuntimeError):
        K.local_explain(pooled, loc, out, weight, 3, 8, min_abs=-0.5)
    empty = K.local_explain(pooled[:0], loc[:0], out[:0], weight, 3, 8)
    assert tuple(empty[3].shape) == (0, 3, 8)


# ---- end to end ---------------------------------------------------------------------------------
FIELDS = ("classes", "logits", "count", "prototype", "similarity", "weight", "simweight", "h_idx", "w_idx",
          "coords", "rect")


def _explain(net, xs, bs, top, before_batch=None, **kw):
    """explain_predictions over ``xs`` in batches of ``bs`` -> {field: host tensor of all images}."""
    parts = []
    for i in range(0, xs.shape[0], bs):
        if before_batch is not None:
            before_batch(i, i + bs)
        parts.append(explain_predictions(net, xs[i:i + bs], top, image_size=64, **kw).cpu())
    res = {f: torch.cat([getattr(part, f) for part in parts]) for f in FIELDS}
    res["proto_shape"] = parts[0].proto_shape
    return res


def _assert_matches_reference(res, outputs, weight, top, max_entries):
    """Every field of the (host) result equals the restatement on the batch-1 forwards ``outputs``."""
    want = pack([reference_lists(proto, pooled, out, weight, top) for proto, pooled, out in outputs], max_entries)
    for f in ("classes", "logits", "count", "prototype", "similarity", "weight", "simweight", "h_idx", "w_idx"):
        assert np.array_equal(res[f].numpy(), want[f]), f
    assert res["classes"].dtype == res["count"].dtype == res["prototype"].dtype == torch.int64
    shape = res["proto_shape"]
    assert shape == (1,) + tuple(outputs[0][0].shape[1:])
    _, skip = patch_size(argparse.Namespace(image_size=64, wshape=shape[3]))
    b, c, m = want["prototype"].shape
    for i in range(b):
        for r in range(c):
            for j in range(m):
                if want["prototype"][i, r, j] < 0:
                    assert (res["coords"][i, r, j] == -1).all() and (res["rect"][i, r, j] == -1).all()
                    continue
                h, w = int(want["h_idx"][i, r, j]), int(want["w_idx"][i, r, j])
                assert tuple(res["coords"][i, r, j].tolist()) == img_coordinates(64, shape, 32, skip, h, w)
                assert tuple(res["rect"][i, r, j].tolist()) == (w * skip, h * skip, min(64, w * skip + 32),
                                                                min(64, h * skip + 32))           # :87
    return want


def _reweight_(net):
    """Classifier weights of the golden model are all in 0.7..1.3: every present prototype would pass.
    A third of the columns to 0 and a third scaled so that their products straddle 0.01."""
    with torch.no_grad():
        w = net._classification.weight
        w[:, 0::3] = 0.0
        w[:, 1::3] *= 0.03


@pytest.fixture(scope="module")
def pipnet_case(gpu):
    meta, _ = load_golden("pipnet_mid_addon")
    net = build_model(meta).to(gpu)
    _reweight_(net)
    xs = torch.cat([synth_images(4, 64, seed=700 + i) for i in range(3)])
    xd = xs.to(gpu)
    with torch.no_grad():
        outputs = [tuple(t.float().cpu() for t in net(xd[i:i + 1], inference=True)) for i in range(12)]
    return meta, net, xs, xd, outputs


@pytest.mark.parametrize("top", [3, None])
def test_explain_predictions_pipnet_matches_reference_loop(gpu, pipnet_case, top):
    meta, net, _, xd, outputs = pipnet_case
    weight = net._classification.weight.detach().cpu()
    results = [_explain(net, xd, bs, top) for bs in (1, 5, 12)]
    want = _assert_matches_reference(results[0], outputs, weight, top, 64)
    assert want["classes"].shape == (12, 3 if top else 10)
    assert ((want["count"] > 0) & (want["count"] < 32)).any()
    active = np.array([int((o[1] != 0).sum()) for o in outputs])
    assert (want["count"] < active[:, None]).any(), "the weights decide nothing"
    for res in results[1:]:
        for f in FIELDS:
            assert torch.equal(res[f], results[0][f]), f                    # bitwise, whatever the batch
    # max_entries below the count: the list is cut, the count is not
    cut = _explain(net, xd, 12, top, max_entries=4)
    assert torch.equal(cut["count"], results[0]["count"]) and (cut["count"] > 4).any()
    assert torch.equal(cut["prototype"], results[0]["prototype"][:, :, :4])


def test_explain_predictions_pipnet_wrappers_and_arguments(gpu, pipnet_case):
    from count_pipnet_amd.dist import ShardedInference
    meta, net, _, xd, outputs = pipnet_case
    base = _explain(net, xd, 12, 3)

    class Holder:
        def __init__(self, module):
            self.module = module

    for wrapped in (Holder(net), ShardedInference(net)):
        res = _explain(wrapped, xd, 12, 3)
        for f in FIELDS:
            assert torch.equal(res[f], base[f]), f
    # weight= replaces the classifier's
    other = torch.rand(10, 32, generator=torch.Generator().manual_seed(4)) * 0.05
    res = _explain(net, xd, 5, 3, weight=other.to(gpu))
    _assert_matches_reference(res, outputs, other, 3, 64)
    with pytest.raises(ValueError):
        explain_predictions(net, xd[:1], 3, image_size=64, weight=other[:, :31].to(gpu))
    with pytest.raises(ValueError):
        explain_predictions(net, xd[:1], 11, image_size=64)
    with pytest.raises(ValueError):
        explain_predictions(net, xd[:1], 0, image_size=64)


def test_explain_predictions_pipnet_against_cpu_oracle(gpu, pipnet_case):
    """Class ranks and kept sets against oracle/ref_cpu.py on the 12 images, where the oracle is
    decisive: a class rank when the oracle's neighbouring logits at ranks 0..C differ by more than
    2e-3 (twice the project's 1e-3 parity); an (image, class, prototype) decision when |sim * w| is
    farther than 2e-3 * w from 0.01 and the score farther than 2e-3 from the 0.1 presence
    threshold.  At most 15 % of the (image, class rank) pairs and 5 % of the decisions may be
    excluded; the oracle alone, on the CPU: 5.6 % (C = 3) / 6.7 % (all 10 classes) of the pairs and
    1.4 % of the decisions on these images with these weights."""
    meta, net, xs, xd, _ = pipnet_case
    sd = {key: v.cpu() for key, v in net.state_dict().items()}
    with torch.no_grad():
        r_proto, r_pooled, r_out = ref_cpu.pipnet_forward(xs, sd, golden_args(meta), inference=True)
    r_raw = r_proto.amax(dim=(2, 3))
    w = sd["_classification.weight"]
    n, kc, pn = 12, 10, 32
    r_sorted, r_order = torch.sort(r_out, dim=1, descending=True, stable=True)
    gap = r_sorted[:, :-1] - r_sorted[:, 1:]                       # between rank r and r + 1
    for top in (3, None):
        c = top or kc
        res = _explain(net, xd, 5, top)
        decisive = torch.ones(n, c, dtype=torch.bool)
        for r in range(c):
            if r > 0:
                decisive[:, r] &= gap[:, r - 1] > 2e-3
            if r < kc - 1:
                decisive[:, r] &= gap[:, r] > 2e-3
        excluded = 1.0 - decisive.float().mean().item()
        print(f"top_classes {top}: class ranks excluded: {100 * excluded:.1f} %")
        assert excluded <= 0.15
        assert torch.equal(res["classes"][decisive], r_order[:, :c][decisive])
    # kept sets by class, from the all-classes result
    prod = r_pooled.double()[:, None, :] * w.double()[None]                             # [n, K, P]
    decisive = ((prod.abs() - 0.01).abs() > 2e-3 * w.double().abs()[None]) & ((r_raw - 0.1).abs() > 2e-3)[:, None, :]
    excluded = 1.0 - decisive.float().mean().item()
    print(f"decisions excluded: {100 * excluded:.1f} %")
    assert excluded <= 0.05
    kept = torch.zeros(n, kc, pn, dtype=torch.bool)
    assert (res["count"] <= 64).all()
    for i in range(n):
        for r in range(kc):
            protos = res["prototype"][i, r]
            kept[i, res["classes"][i, r], protos[protos >= 0]] = True
    assert torch.equal(kept[decisive], (prod.abs() > 0.01)[decisive])


# ---- end to end, CountPIPNet --------------------------------------------------------------------
def _count_case(gpu, name, image_seed, noise_seed):
    meta, _ = load_golden(name)
    net = build_model(meta).to(gpu)
    n = 12
    xd = torch.cat([synth_images(4, 64, seed=image_seed + i) for i in range(3)]).to(gpu)
    noise = synth_exponential((n, 16, 8, 8), seed=noise_seed).to(gpu)
    head = net._add_on[-1]

    def slice_noise(i0, i1):
        head.exp_noise = noise[i0:i1]

    outputs = []
    with torch.no_grad():
        for i in range(n):
            slice_noise(i, i + 1)
            outputs.append(tuple(t.float().cpu() for t in net(xd[i:i + 1], inference=True)))
    return net, xd, slice_noise, outputs


def test_explain_predictions_count_identity(gpu):
    """c1_count_identity: the classifier reads the counts themselves, so the default weight is
    ``_classification.weight`` itself."""
    net, xd, slice_noise, outputs = _count_case(gpu, "c1_count_identity", 820, 78)
    weight = net._classification.weight.detach()
    assert torch.equal(count_importance_matrix(net), weight)
    for top in (3, None):
        res = _explain(net, xd, 5, top, before_batch=slice_noise)
        want = _assert_matches_reference(res, outputs, weight.cpu(), top, 64)
        assert (want["count"] > 0).any()
        assert max(np.unique(outputs[0][1].numpy(), return_counts=True)[1]) > 1      # counts tie


def test_explain_predictions_count_onehot(gpu):
    """count_onehot (classifier input width 3 P): the default weight is the model's per-class
    prototype importance; injected noise sliced per image as in test_gpu_topk.py."""
    net, xd, slice_noise, outputs = _count_case(gpu, "count_onehot", 800, 77)
    with torch.no_grad():
        importance = torch.stack([net.get_prototype_importance_per_class(p) for p in range(16)], dim=1)
    assert tuple(importance.shape) == (9, 16) and net._classification.weight.shape[1] == 48
    assert torch.equal(count_importance_matrix(net), importance)
    results = [_explain(net, xd, bs, 3, before_batch=slice_noise) for bs in (1, 5, 12)]
    want = _assert_matches_reference(results[0], outputs, importance.cpu(), 3, 64)
    assert (want["count"] > 0).any()
    imp = importance.cpu()
    filled = results[0]["prototype"] >= 0
    cls = results[0]["classes"].unsqueeze(-1).expand_as(results[0]["prototype"])
    assert torch.equal(results[0]["weight"][filled], imp[cls[filled], results[0]["prototype"][filled]])
    for res in results[1:]:
        for f in FIELDS:
            assert torch.equal(res[f], results[0][f]), f
    # weight= overrides the default, a wrong shape is an error (the classifier's own [9, 48] too)
    slice_noise(0, 5)
    other = torch.rand(9, 16, generator=torch.Generator().manual_seed(5)) * 0.02
    res = _explain(net, xd, 5, None, before_batch=slice_noise, weight=other.to(gpu))
    _assert_matches_reference(res, outputs, other, None, 64)
    slice_noise(0, 1)
    with pytest.raises(ValueError):
        explain_predictions(net, xd[:1], 3, image_size=64, weight=net._classification.weight.detach())
