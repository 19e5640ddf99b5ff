"""The explanation passes (top-k, local explanations, part purity, attribution) as the library sees them.

``CASES`` maps a name to a function ``(gpu) -> (calls, digest)``: the pass runs on a fresh net under
``train_trace_cases.record_calls()`` and ``digest`` is ``result_digest`` of its ``.cpu()`` result(s).  The inputs are
the 64-pixel fixtures of tests/test_gpu_topk.py, test_gpu_local_explain.py, test_gpu_part_purity.py and
test_gpu_attribution.py, 8 x 8 maps throughout.  The ``large_*`` cases are the branch those never reach: the
``pipnet_mid_addon`` architecture on 184-pixel images (a 23 x 23 = 529 pixel map, above ``K.SPLITK_MAX_M``) with two
sub-batch streams, 68 images in two batches of 34 -- the first with the map size still unknown (per-image plan, one
stream), the second on the plain forward's path with two side streams -- and, as ``*_bs1``, one image at a time.

tests/golden/gen_explain_call_trace.py records both on the parent commit into tests/golden/explain_call_trace.json;
tests/test_gpu_explain_trace.py holds the tree to it.
"""
import hashlib
import tempfile
from dataclasses import fields

import numpy as np
import torch

from attr_util import attr_image, attr_noise, load_attr
from count_pipnet_amd import kernels as K
from count_pipnet_amd.attribution import attribute
from count_pipnet_amd.local import explain_predictions
from count_pipnet_amd.pipnet import set_hip_dtype, set_stream_split
from count_pipnet_amd.purity import PartAnnotations, part_purity
from count_pipnet_amd.synthetic import synth_exponential, synth_images
from count_pipnet_amd.topk import prototype_topk
from golden_util import eval_loader_batches, load_golden
from model_util import build_model
from part_purity_util import FIXTURES, fixture_annotations, load_purity_fixture, random_table
from train_trace_cases import record_calls

# (kernel name, argument position) pairs that differ between two runs of the parent and are left out
MASKED = ()
LARGE_SIZE, LARGE_IMAGES, LARGE_BATCH = 184, 68, 34


def result_digest(*results):
    """sha256 over the (host) results' fields in field order: a tensor by name, dtype, shape and bytes, anything
    else by name and ``repr``."""
    h = hashlib.sha256()
    for res in results:
        for f in fields(res):
            v = getattr(res, f.name)
            if torch.is_tensor(v):
                h.update(f"{f.name}|{v.dtype}|{tuple(v.shape)}|".encode() + v.contiguous().numpy().tobytes() + b"\0")
            else:
                h.update(f"{f.name}|{v!r}\0".encode())
    return h.hexdigest()


def _recorded(run):
    """(calls, digest) of ``run() -> results still on the device``."""
    with record_calls(MASKED) as calls:
        results = run()
    return calls, result_digest(*[r.cpu() for r in results])


def _batches(xs, bs):
    ys = torch.zeros(xs.shape[0], dtype=torch.int64)
    return [(xs[i:i + bs], ys[i:i + bs]) for i in range(0, xs.shape[0], bs)]


def _images12(seed):
    return torch.cat([synth_images(4, 64, seed=seed + i) for i in range(3)])


def _pipnet(gpu):
    return build_model(load_golden("pipnet_mid_addon")[0]).to(gpu)


def _count_onehot(gpu):
    """(net, images, labels, set_noise): count_onehot with the injected Exp(1) draws of the count tests."""
    net = build_model(load_golden("count_onehot")[0]).to(gpu)
    noise = synth_exponential((12, 16, 8, 8), seed=77).to(gpu)
    head = net._add_on[-1]

    def set_noise(i0, i1):
        head.exp_noise = noise[i0:i1]

    ys = torch.randint(0, 9, (12,), generator=torch.Generator().manual_seed(8))
    return net, _images12(800), ys, set_noise


# ---- prototype_topk --------------------------------------------------------------------------------
def topk_pipnet(bs):
    def case(gpu):
        net = _pipnet(gpu)
        return _recorded(lambda: [prototype_topk(net, _batches(_images12(700), bs), 3, image_size=64)])
    return case


def topk_count(gpu):
    net, xs, ys, set_noise = _count_onehot(gpu)

    def loader():
        for i in range(0, 12, 5):
            set_noise(i, i + 5)
            yield xs[i:i + 5], ys[i:i + 5]

    return _recorded(lambda: [prototype_topk(net, loader(), 3, image_size=64)])


# ---- explain_predictions: two calls on a fresh net, the map size unknown and then known --------------
def local_pipnet(gpu):
    net = _pipnet(gpu)
    with torch.no_grad():               # as tests/test_gpu_local_explain.py: the weights decide something
        net._classification.weight[:, 0::3] = 0.0
        net._classification.weight[:, 1::3] *= 0.03
    xd = _images12(700).to(gpu)
    return _recorded(lambda: [explain_predictions(net, xd[:5], 3, image_size=64),
                              explain_predictions(net, xd[5:], 3, image_size=64)])


def local_count(gpu):
    net, xs, _, set_noise = _count_onehot(gpu)
    xd = xs.to(gpu)

    def run():
        out = []
        for i0, i1 in ((0, 5), (5, 12)):
            set_noise(i0, i1)
            out.append(explain_predictions(net, xd[i0:i1], 3, image_size=64))
        return out

    return _recorded(run)


# ---- part_purity -----------------------------------------------------------------------------------
def _purity_fixture():
    meta, rec, fwd_meta = load_purity_fixture(FIXTURES[0])
    with tempfile.TemporaryDirectory() as folder:
        ann = fixture_annotations(meta, rec, folder)
    return meta, rec, fwd_meta, ann


def purity(mode):
    def case(gpu):
        meta, rec, fwd_meta, ann = _purity_fixture()
        c = fwd_meta["case"]
        net = build_model(fwd_meta).to(gpu)
        with torch.no_grad():
            net._classification.weight.copy_(torch.from_numpy(rec["weight"]))
        batches = eval_loader_batches(c["size"], c["num_classes"], meta["batches"], meta["batch_size"], meta["label_seed"])
        xs = torch.cat([x for x, _ in batches])[:meta["images"]]
        return _recorded(lambda: [part_purity(net, _batches(xs, 5), ann, image_size=c["size"], mode=mode,
                                              threshold=meta["threshold"], k=meta["k"],
                                              relevance_threshold=meta["relevance"])])
    return case


def purity_bf16_all(gpu):
    """The bf16 build (ResNet-50 at 64 x 64) with the fixture's annotations; about 2 % of the (image, prototype)
    pairs give a row (the threshold is the 0.98 quantile of the plain forward's pooled scores)."""
    _, _, _, ann = _purity_fixture()
    fwd_meta, _ = load_golden("pipnet_resnet50_small")
    c = fwd_meta["case"]
    net = build_model(fwd_meta).to(gpu)
    set_hip_dtype(net, "bf16")
    xs = torch.cat([x for x, _ in eval_loader_batches(c["size"], c["num_classes"], 3, 5, 312)])[:ann.images]
    with torch.no_grad():
        thr = float(np.quantile(net(xs.to(gpu), inference=False)[1].float().cpu().numpy(), 0.98))
    return _recorded(lambda: [part_purity(net, _batches(xs, 5), ann, image_size=c["size"], mode="all", threshold=thr,
                                          k=3)])


# ---- attribute: two chunks on a fresh net -----------------------------------------------------------------
def attr(name, kind, method):
    def case(gpu):
        meta, rec = load_attr(name)
        net = build_model(meta).to(gpu)
        noise = attr_noise(meta)
        x = attr_image(meta).to(gpu)
        return _recorded(lambda: [attribute(net, x, rec[f"{kind}_targets"].tolist(), kind=kind, method=method, steps=8,
                                            batch_size=4, baseline=meta["baseline"],
                                            exp_noise=None if noise is None else noise.to(gpu))])
    return case


# ---- the large-map branch ------------------------------------------------------------------------------
def large_annotations():
    """Seeded part annotations of the 68 images, built the way tests/part_purity_util.py builds its tables."""
    t = random_table(np.random.default_rng(LARGE_IMAGES), LARGE_IMAGES, 15, 3, LARGE_SIZE)
    return PartAnnotations(
        xy=torch.from_numpy(t["xy"]), vis=torch.from_numpy(t["vis"]), size=torch.from_numpy(t["size"]),
        merged=torch.from_numpy(t["merged"]), is_left=torch.from_numpy(t["is_left"]),
        pair_index=torch.from_numpy(t["pair_index"]), part_ids=t["ids"], part_names=t["names"],
        merged_ids=[t["ids"][q] for q in t["keep"]], merged_names=[t["names"][q] for q in t["keep"]],
        image_keys=[f"c/{i}.jpg" for i in range(LARGE_IMAGES)])


def large(what, bs):
    def case(gpu):
        net = set_stream_split(_pipnet(gpu), 2)
        xs = synth_images(LARGE_IMAGES, LARGE_SIZE, seed=900)
        if what == "topk":
            return _recorded(lambda: [prototype_topk(net, _batches(xs, bs), 3, image_size=LARGE_SIZE)])
        ann = large_annotations()
        return _recorded(lambda: [part_purity(net, _batches(xs, bs), ann, image_size=LARGE_SIZE, mode="topk", k=3)])
    return case


CASES = {
    "topk_pipnet_bs5": topk_pipnet(5), "topk_pipnet_bs12": topk_pipnet(12), "topk_count_bs5": topk_count,
    "local_pipnet": local_pipnet, "local_count": local_count,
    "purity_all": purity("all"), "purity_topk": purity("topk"), "purity_bf16_all": purity_bf16_all,
    "attr_ig_pipnet": attr("pipnet_mid_addon", "prototype", "ig"), "attr_idg_count": attr("count_onehot", "class", "idg"),
    "large_topk": large("topk", LARGE_BATCH), "large_purity_topk": large("purity", LARGE_BATCH),
    "large_topk_bs1": large("topk", 1), "large_purity_topk_bs1": large("purity", 1),
}
# pairs the parent gave the same bits for: batches of 34 (the second as two concurrent halves), one image at a time
BATCH_INVARIANT = [("large_topk", "large_topk_bs1"), ("large_purity_topk", "large_purity_topk_bs1")]
assert 22 * 22 <= K.SPLITK_MAX_M < 23 * 23          # stride 8: 184 px (23 x 23) is the smallest input above the rule's bound
