"""Part purity on the device (csrc/part_purity.hip, count_pipnet_amd/purity.py): the update kernel
against the numpy reduction on planted inputs, batch-split invariance of every state tensor, the
rows kernel and finish against the dict restatement, the recorded reference data through the
kernels, and the end-to-end passes over the fixture models."""
import numpy as np
import pytest
import torch

from count_pipnet_amd import kernels as K
from count_pipnet_amd.pipnet import set_hip_dtype
from count_pipnet_amd.purity import part_purity
from count_pipnet_amd.explain_forward import located_forward
from golden_util import eval_loader_batches, load_golden
from model_util import build_model
from part_purity_util import (FIXTURES, annotations_table, assert_finish_matches, assert_matches_recording,
                              assert_state_equal, first_appearance, fixture_annotations, geometry, load_purity_fixture,
                              new_state, np_finish, np_rows, np_update, random_table, recorded_rows, restate_rows,
                              result_from_finish, rows_all, rows_topk)

pytestmark = pytest.mark.gpu

THR = 0.5
FIN_KEYS = ("in_csv", "max_purity", "max_part", "max_sum", "most_part", "most_sum", "most_purity", "purity")
# (B, P, Q, pairs, H = W, small-stride rule; None: the rule of the map size): one image, one part, a
# 1 x 1 map; odd sizes; C2's width on its 26 x 26 map; the 26-prototype net on that map, with and
# without the rule (both branches of the patch geometry at one size); C5's width, more column blocks
KERNEL_CASES = [(1, 16, 1, 0, 1, None), (7, 100, 15, 3, 7, None), (64, 768, 15, 3, 26, None),
                (5, 26, 15, 3, 26, None), (5, 26, 15, 3, 26, False), (5, 2048, 4, 1, 14, None)]


def _dev_table(table, gpu):
    return tuple(torch.from_numpy(table[k]).to(gpu) for k in ("xy", "vis", "size", "merged", "is_left", "pair_index"))


def _state_np(st):
    return dict(n=st.n.cpu().numpy(), hits=st.hits.cpu().numpy(), first_key=st.first_key.cpu().numpy().view(np.uint64),
                rows=st.rows.cpu().numpy(), bad=int(st.bad))


def _fin_np(res):
    return {k: v.cpu().numpy() for k, v in zip(FIN_KEYS, res)}


def _planted(rng, b, p, hw, thr=THR, fire=0.12):
    """pooled [b, p] float32 with about ``fire`` of the entries above the threshold, the threshold
    and one ulp on either side scattered in; loc [b, p] over the whole map, its corners included."""
    pooled = rng.random((b, p), dtype=np.float32)
    pooled = np.where(rng.random((b, p)) < fire, np.float32(thr) + pooled * np.float32(0.5), pooled * np.float32(thr))
    t = np.float32(thr)
    marks = np.array([t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1))], dtype=np.float32)
    flat = pooled.reshape(-1)
    pos = rng.choice(flat.size, size=min(flat.size, 9), replace=False)
    flat[pos] = np.resize(marks, pos.size)
    loc = rng.integers(0, hw * hw, (b, p)).astype(np.int32)
    lf = loc.reshape(-1)
    lf[rng.choice(lf.size, size=min(lf.size, 4), replace=False)] = np.resize([0, hw - 1, hw * (hw - 1), hw * hw - 1],
                                                                              min(lf.size, 4))
    return pooled.astype(np.float32), loc


def _update(gpu, pooled, loc, relevant, i0, thr, geo, table, splits=None):
    st = K.PartPurityState(pooled.shape[1], len(table["keep"]), gpu)
    dt = _dev_table(table, gpu)
    pd, ld = torch.from_numpy(pooled).to(gpu), torch.from_numpy(loc).to(gpu)
    rd = torch.from_numpy(relevant.astype(np.uint8)).to(gpu)
    i = 0
    for s in splits or [pooled.shape[0]]:
        K.part_purity_update(st, pd[i:i + s], ld[i:i + s].contiguous(), rd, i0 + i, thr, geo, dt)
        i += s
    assert i == pooled.shape[0]
    return st


@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_update_kernel_matches_the_numpy_reduction(gpu, case):
    b, p, q, pairs, hw, small = case
    rng = np.random.default_rng(sum(c or 0 for c in case))
    size = 224 if hw == 26 else 64
    geo = geometry(hw, hw, size, small)
    table = random_table(rng, b + 5, q, pairs, size)
    pooled, loc = _planted(rng, b, p, hw)
    relevant = rng.random(p) < 0.9
    i0 = 3
    st = _update(gpu, pooled, loc, relevant, i0, THR, geo, table)
    want = np_update(new_state(p, len(table["keep"])), pooled, loc, relevant, i0, THR, geo, table)
    got = _state_np(st)
    assert_state_equal(got, want, case)
    assert got["bad"] == 0 and want["rows"].sum() > 0
    assert (got["rows"][~relevant] == 0).all()
    fin = _fin_np(K.part_purity_finish(st))
    ref = restate_rows(rows_all(pooled, loc, relevant, i0, THR, geo, b + 5), table, size)
    assert_finish_matches(fin, ref, table, case)
    wf = np_finish(want)
    for k in FIN_KEYS:
        assert np.array_equal(fin[k], wf[k], equal_nan=True), k


def test_update_kernel_strided_view_masks_threshold_and_bad_indices(gpu):
    b, p, q, hw = 23, 100, 15, 7
    rng = np.random.default_rng(5)
    geo = geometry(hw, hw, 64)
    table = random_table(rng, b, q, 3)
    wide, loc = _planted(rng, b, 137, hw)
    loc = np.ascontiguousarray(loc[:, :p])
    pooled = np.ascontiguousarray(wide[:, 5:5 + p])
    relevant = rng.random(p) < 0.9
    dt = _dev_table(table, gpu)
    rd = torch.from_numpy(relevant.astype(np.uint8)).to(gpu)
    want = np_update(new_state(p, 12), pooled, loc, relevant, 0, THR, geo, table)
    # a sliced view: row stride 137 > P, storage offset 5
    st = K.PartPurityState(p, 12, gpu)
    K.part_purity_update(st, torch.from_numpy(wide).to(gpu)[:, 5:5 + p], torch.from_numpy(loc).to(gpu), rd, 0, THR, geo, dt)
    assert_state_equal(_state_np(st), want, "lda > P")
    # no relevant prototype; a threshold nothing passes: the state stays as initialised
    none = np.zeros(p, dtype=bool)
    for rel, thr in ((none, THR), (relevant, 2.0)):
        got = _state_np(_update(gpu, pooled, loc, rel, 0, thr, geo, table))
        assert_state_equal(got, new_state(p, 12), (rel.any(), thr))
        assert got["bad"] == 0
    # dataset indices below 0 and from N on count into ``bad`` only
    for i0, bad in ((-4, 4), (b - 6, 17), (b, b)):
        got = _state_np(_update(gpu, pooled, loc, relevant, i0, THR, geo, table))
        w = np_update(new_state(p, 12), pooled, loc, relevant, i0, THR, geo, table)
        assert_state_equal(got, w, i0)
        assert got["bad"] == bad == w["bad"]


def test_state_is_bitwise_independent_of_the_batch_split(gpu):
    b, p, hw = 23, 768, 26
    rng = np.random.default_rng(23)
    geo = geometry(hw, hw, 224)
    table = random_table(rng, b, 15, 3, 224)
    pooled, loc = _planted(rng, b, p, hw)
    relevant = rng.random(p) < 0.9
    runs = [_update(gpu, pooled, loc, relevant, 0, THR, geo, table, s) for s in (None, [1] * 23, [5, 2, 9, 7])]
    for other in runs[1:]:
        for x, y in zip(runs[0].tensors(), other.tensors()):
            assert x.dtype == y.dtype and torch.equal(x, y)
    assert_state_equal(_state_np(runs[0]), np_update(new_state(p, 12), pooled, loc, relevant, 0, THR, geo, table))


def test_rows_kernel_and_finish_match_the_restatement_with_ties_and_empty_slots(gpu):
    """Seeded tables with ties in purity, in hit count and at purity 0 (tests/part_purity_util.py
    random_table), top-k states with empty slots and an index past the table."""
    seen_bad = 0
    for seed in range(40):
        rng = np.random.default_rng(1000 + seed)
        q = (1, 4, 15)[seed % 3]
        pairs = int(rng.integers(0, min(3, q // 2) + 1))
        n_img, pn, k = int(rng.integers(1, 7)), int(rng.integers(1, 150)), int(rng.integers(1, 33))
        table = random_table(rng, n_img, q, pairs)
        hw = int(rng.integers(1, 9))
        geo = geometry(hw, hw, 64, small=seed % 4 == 0)
        relevant = rng.random(pn) < 0.85
        index = rng.integers(-1, n_img + (seed % 7 == 0), (pn, k)).astype(np.int64)
        loc = rng.integers(0, hw * hw, (pn, k)).astype(np.int32)
        st = K.PartPurityState(pn, len(table["keep"]), gpu)
        K.part_purity_rows(st, torch.from_numpy(index).to(gpu), torch.from_numpy(loc).to(gpu),
                           torch.from_numpy(relevant.astype(np.uint8)).to(gpu), geo, _dev_table(table, gpu))
        want = np_rows(new_state(pn, len(table["keep"])), index, loc, relevant, geo, table)
        got = _state_np(st)
        assert_state_equal(got, want, seed)
        assert got["bad"] == want["bad"]
        seen_bad += want["bad"]
        ref = restate_rows(rows_topk(index, loc, relevant, geo, n_img), table, 64)
        assert_finish_matches(_fin_np(K.part_purity_finish(st)), ref, table, seed)
    assert seen_bad > 0


@pytest.mark.parametrize("mode", ["all", "topk"])
@pytest.mark.parametrize("name", FIXTURES)
def test_recorded_reference_data_through_the_kernels(gpu, name, mode, tmp_path):
    """The pooled / loc values the reference saw, through update (or top-k + rows) and finish: the
    recorded dicts exactly, the logged means and stds within P * 2^-52 (an fp64 sum of at most P
    values in [0, 1], reordered)."""
    meta, rec, fwd_meta = load_purity_fixture(name)
    ann = fixture_annotations(meta, rec, tmp_path)
    table = annotations_table(ann)
    size = fwd_meta["case"]["size"]
    _, h, w = meta["map_shape"]
    geo = geometry(h, w, size)
    pooled, loc = rec[f"{mode}_pooled"], rec[f"{mode}_loc"]
    pn = pooled.shape[1]
    relevant = rec["weight"].max(axis=0) > np.float32(meta["relevance"])
    rd = torch.from_numpy(relevant.astype(np.uint8)).to(gpu)
    dt = ann.to(gpu).table()
    if mode == "all":
        st = _update(gpu, pooled, loc, relevant, 0, meta["threshold"], geo, table)
        rows = rows_all(pooled, loc, relevant, 0, meta["threshold"], geo, ann.images)
        order = first_appearance(rows)
    else:
        ts = K.TopkState(1, pn, meta["k"], gpu)
        K.topk_update(ts, torch.from_numpy(pooled).to(gpu), torch.from_numpy(loc).to(gpu), 0)
        st = K.PartPurityState(pn, len(table["keep"]), gpu)
        K.part_purity_rows(st, ts.index[0].contiguous(), ts.loc[0].contiguous(), rd, geo, dt)
        rows = rows_topk(ts.index[0].cpu().numpy(), ts.loc[0].cpu().numpy(), relevant, geo, ann.images)
        order = sorted(first_appearance(rows))
    assert rows == recorded_rows(rec, mode)
    fin = _fin_np(K.part_purity_finish(st))
    assert int(st.bad) == 0
    assert_matches_recording(result_from_finish(fin, order, table), meta, mode, ulps=pn)
    assert_finish_matches(fin, restate_rows(rows, table, size), table, (name, mode))


def _own_forward(net, xs, gpu):
    """(raw pooled [N,P], loc [N,P]) of the batch-1 forwards, image by image."""
    with torch.no_grad():
        outs = [located_forward(net, xs[i:i + 1].to(gpu), None, with_raw=True) for i in range(xs.shape[0])]
    hw = outs[0][3]
    return (torch.cat([o[4] for o in outs]).cpu().numpy(), torch.cat([o[1] for o in outs]).cpu().numpy(), hw)


def _loader(xs, bs):
    ys = torch.zeros(xs.shape[0], dtype=torch.int64)
    return [(xs[i:i + bs], ys[i:i + bs]) for i in range(0, xs.shape[0], bs)]


def _end_to_end(gpu, net, xs, ann, table, size, mode, thr, k, relevance):
    """part_purity at batch sizes 1, 5 and the whole set: bitwise equal, and exact against the
    restatement applied to the forward's own pooled / loc.  Returns (result, restatement)."""
    pooled, loc, (h, w) = _own_forward(net, xs, gpu)
    geo = geometry(h, w, size)
    relevant = (net._classification.weight.detach().max(dim=0).values > relevance).cpu().numpy()
    if mode == "all":
        rows = rows_all(pooled, loc, relevant, 0, thr, geo, ann.images)
    else:
        order = np.argsort(-pooled, axis=0, kind="stable")[:k].T
        rows = rows_topk(order.astype(np.int64), np.take_along_axis(loc.T, order, axis=1), relevant, geo, ann.images)
    ref = restate_rows(rows, table, size)
    results = [part_purity(net, _loader(xs, bs), ann, image_size=size, mode=mode, threshold=thr, k=k,
                           relevance_threshold=relevance).cpu() for bs in (1, 5, xs.shape[0])]
    for res in results:
        assert res.geometry == geo and res.images == ann.images
        assert [(str(r[0]),) + r[1:] for r in res.patch_rows()] == rows
        assert_finish_matches({f: getattr(res, f).numpy() for f in FIN_KEYS}, ref, table, mode)
        assert [str(p) for p in res.csv_order()] == ref["order"] and res.summary() == ref["logged"]
        for f in ("n", "hits", "first_key", "rows", "row_loc", "relevant") + FIN_KEYS:
            a, b = getattr(res, f), getattr(results[0], f)
            assert a.dtype == b.dtype and torch.equal(torch.nan_to_num(a, nan=-1.0) if a.is_floating_point() else a,
                                                      torch.nan_to_num(b, nan=-1.0) if b.is_floating_point() else b), f
        if mode == "topk":
            assert torch.equal(res.row_index, results[0].row_index)
    return results[0], ref


@pytest.mark.parametrize("mode", ["all", "topk"])
@pytest.mark.parametrize("name", FIXTURES)
def test_part_purity_end_to_end_equals_the_recorded_reference(gpu, name, mode, tmp_path):
    """fp32 build on the fixture model: exact against the restatement on the forward's own outputs,
    bitwise equal across batch sizes, and equal to the recorded reference result without
    exclusions (the fixture is decisive by construction)."""
    meta, rec, fwd_meta = load_purity_fixture(name)
    ann = fixture_annotations(meta, rec, tmp_path)
    table = annotations_table(ann)
    case = fwd_meta["case"]
    net = build_model(fwd_meta).to(gpu)
    with torch.no_grad():
        net._classification.weight.copy_(torch.from_numpy(rec["weight"]))
    batches = eval_loader_batches(case["size"], case["num_classes"], meta["batches"], meta["batch_size"],
                                  meta["label_seed"])
    xs = torch.cat([x for x, _ in batches])[:meta["images"]]
    res, ref = _end_to_end(gpu, net, xs, ann, table, case["size"], mode, meta["threshold"], meta["k"], meta["relevance"])
    assert [(str(r[0]),) + r[1:] for r in res.patch_rows()] == recorded_rows(rec, mode)
    assert_matches_recording(ref, meta, mode, ulps=net._num_prototypes)
    fin = {f: getattr(res, f).numpy() for f in FIN_KEYS}
    got = result_from_finish(fin, res.csv_order(), table)
    got["logged"] = res.summary()
    assert_matches_recording(got, meta, mode, ulps=net._num_prototypes)
    # wrappers: ShardedInference at world size 1
    from count_pipnet_amd.dist import ShardedInference
    res_w = part_purity(ShardedInference(net), _loader(xs, 7), ann, image_size=case["size"], mode=mode,
                        threshold=meta["threshold"], k=meta["k"]).cpu()
    assert torch.equal(res_w.n, res.n) and torch.equal(res_w.first_key, res.first_key)
    # a loader that ends early: the annotations cover images the pass never saw
    with pytest.raises(ValueError, match="saw"):
        part_purity(net, _loader(xs[:5], 5), ann, image_size=case["size"], mode=mode)


@pytest.mark.parametrize("mode", ["all", "topk"])
def test_part_purity_end_to_end_bf16_build_against_its_own_forward(gpu, mode, tmp_path):
    """The bf16 build (ResNet-50 at 64 x 64) with the fixture's annotation table: the same
    end-to-end properties against its own forward outputs only."""
    meta, rec, _ = load_purity_fixture(FIXTURES[0])
    ann = fixture_annotations(meta, rec, tmp_path)
    table = annotations_table(ann)
    fwd_meta, _ = load_golden("pipnet_resnet50_small")
    case = fwd_meta["case"]
    net = build_model(fwd_meta).to(gpu)
    set_hip_dtype(net, "bf16")
    xs = torch.cat([x for x, _ in eval_loader_batches(case["size"], case["num_classes"], 3, 5, 312)])[:ann.images]
    pooled, _, _ = _own_forward(net, xs, gpu)
    thr = float(np.quantile(pooled, 0.98))              # about 2 % of the (image, prototype) pairs give a row
    res, ref = _end_to_end(gpu, net, xs, ann, table, case["size"], mode, thr, 3, 1e-5)
    assert int(res.rows.sum()) >= 30 and len(ref["order"]) >= 10
