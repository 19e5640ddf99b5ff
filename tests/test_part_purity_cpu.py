"""Part purity without a GPU: the dict restatement against the recorded reference run, the
(n, hits, first_key) reduction against the restatement on seeded random tables, the annotation
parser, the CSV writer / host evaluator, the centring correction and the 32-pixel patch invariant."""
import numpy as np
import pytest
import torch

from count_pipnet_amd.purity import (CSV_HEADER, PartAnnotations, PartPurity, eval_patch_csv, image_key,
                                     write_patch_csv)
from count_pipnet_amd.topk import img_coordinates
from part_purity_ref import restate
from part_purity_util import (FIXTURES, annotations_table, assert_finish_matches, assert_matches_recording,
                              fixture_annotations, geometry, load_purity_fixture, new_state, np_finish, np_patch,
                              np_rows, np_update, random_table, recorded_rows, restate_rows, rows_all, rows_topk,
                              write_annotation_files)


def _fixture_reduction(meta, rec, table, mode):
    """The numpy reduction over the recorded pooled / loc of ``mode``: (state, finish, relevant, geo, index, loc)."""
    pooled, loc = rec[f"{mode}_pooled"], rec[f"{mode}_loc"]
    relevant = rec["weight"].max(axis=0) > np.float32(meta["relevance"])
    _, h, w = meta["map_shape"]
    geo = geometry(h, w, load_size(meta))
    state = new_state(pooled.shape[1], len(table["keep"]))
    if mode == "all":
        np_update(state, pooled, loc, relevant, 0, meta["threshold"], geo, table)
        return state, np_finish(state), relevant, geo, None, loc
    order = np.argsort(-pooled, axis=0, kind="stable")[:meta["k"]].T       # score descending, earlier image first
    index = order.astype(np.int64)
    kloc = np.take_along_axis(loc.T, order, axis=1).astype(np.int32)
    np_rows(state, index, kloc, relevant, geo, table)
    return state, np_finish(state), relevant, geo, index, kloc


def load_size(meta):
    from golden_util import load_golden
    return load_golden(meta["forward_case"])[0]["case"]["size"]


@pytest.mark.parametrize("mode", ["all", "topk"])
@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_the_recorded_dicts_and_logged_tuple(name, mode, tmp_path):
    meta, rec, _ = load_purity_fixture(name)
    table = annotations_table(fixture_annotations(meta, rec, tmp_path))
    ref = restate_rows(recorded_rows(rec, mode), table, load_size(meta))
    assert_matches_recording(ref, meta, mode, ulps=0)
    assert meta["modes"][mode]["header"] == CSV_HEADER
    if mode == "all":
        assert meta["empty_dict"] and all(not ref["presences"][p] for p in meta["empty_dict"])
        assert len(ref["order"]) < int((rec["weight"].max(axis=0) > 1e-5).sum())      # a relevant prototype without row


@pytest.mark.parametrize("mode", ["all", "topk"])
@pytest.mark.parametrize("name", FIXTURES)
def test_reduction_and_result_object_reproduce_the_recording(name, mode, tmp_path):
    """The recorded pooled / loc through the numpy reduction: the recorded CSV rows, dicts and logged
    tuple; and PartPurity's host side (csv order, summary, patch rows) on that state."""
    meta, rec, _ = load_purity_fixture(name)
    ann = fixture_annotations(meta, rec, tmp_path)
    table = annotations_table(ann)
    size = load_size(meta)
    state, fin, relevant, geo, index, loc = _fixture_reduction(meta, rec, table, mode)
    rows = (rows_all(rec["all_pooled"], rec["all_loc"], relevant, 0, meta["threshold"], geo, ann.images)
            if mode == "all" else rows_topk(index, loc, relevant, geo, ann.images))
    assert rows == recorded_rows(rec, mode)
    ref = restate_rows(rows, table, size)
    assert_finish_matches(fin, ref, table, (name, mode))
    t = {k: torch.from_numpy(np.asarray(v)) for k, v in fin.items()}
    fires = (rec["all_pooled"].astype(np.float64) > meta["threshold"]) & relevant[None]
    res = PartPurity(mode=mode, n=torch.from_numpy(state["n"]), hits=torch.from_numpy(state["hits"]),
                     first_key=torch.from_numpy(state["first_key"].view(np.int64)), rows=torch.from_numpy(state["rows"]),
                     relevant=torch.from_numpy(relevant), merged_names=ann.merged_names, images=ann.images, geometry=geo,
                     row_loc=torch.from_numpy(np.where(fires, rec["all_loc"], -1).astype(np.int32) if mode == "all" else loc),
                     row_index=None if mode == "all" else torch.from_numpy(index), **t)
    assert [str(p) for p in res.csv_order()] == meta["modes"][mode]["order"]
    assert list(res.summary()) == meta["modes"][mode]["logged"]            # same values, same order: same bits
    assert [(str(r[0]),) + r[1:] for r in res.patch_rows()] == recorded_rows(rec, mode)
    # CSV writer -> host evaluator: the recorded result again, through the file
    paths = ["/data/" + p for p in meta["image_paths"]]
    csvfile = write_patch_csv(res, paths, str(tmp_path / "patches.csv"))
    got = eval_patch_csv(csvfile, ann, size)
    assert list(got.presences) == meta["modes"][mode]["order"]
    assert got.max_part == meta["modes"][mode]["max_part"]
    assert {k: [v[0], v[1]] for k, v in got.most_part.items()} == meta["modes"][mode]["most_part"]
    assert list(got.summary()) == meta["modes"][mode]["logged"]
    assert got.max_purity == ref["max_purity"] and got.max_sum == ref["max_sum"] and got.presences == ref["presences"]


SEEDS = range(2400)


def test_reduction_equals_restatement_on_random_tables():
    """n / hits / first_key + finish == the dict restatement, over seeded tables with Q in {1, 4, 15},
    0..3 pairs and ties in purity, in hit count and at purity 0; both row sources."""
    ties = dict(purity=0, hits=0, zero=0, left_only=0, empty=0)
    for seed in SEEDS:
        rng = np.random.default_rng(seed)
        q = (1, 4, 15)[seed % 3]
        pairs = int(rng.integers(0, min(3, q // 2) + 1))
        n_img, pn = int(rng.integers(1, 7)), 3
        table = random_table(rng, n_img, q, pairs)
        h, w = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        geo = geometry(h, w, 64, small=bool(seed % 5 == 0))
        relevant = rng.random(pn) < 0.85
        state = new_state(pn, len(table["keep"]))
        if seed % 2:
            pooled = rng.random((n_img, pn)).astype(np.float32)
            loc = rng.integers(0, h * w, (n_img, pn)).astype(np.int32)
            np_update(state, pooled, loc, relevant, 0, 0.4, geo, table)
            rows = rows_all(pooled, loc, relevant, 0, 0.4, geo, n_img)
        else:
            k = int(rng.integers(1, 5))
            index = rng.integers(-1, n_img, (pn, k)).astype(np.int64)          # -1: empty slots
            loc = rng.integers(0, h * w, (pn, k)).astype(np.int32)
            np_rows(state, index, loc, relevant, geo, table)
            rows = rows_topk(index, loc, relevant, geo, n_img)
        ref = restate_rows(rows, table, 64)
        assert_finish_matches(np_finish(state), ref, table, seed)
        for key, flags in ref["presences"].items():
            pur = [float(np.mean(s)) for s in flags.values()]
            hit = [int(np.sum(s)) for s in flags.values()]
            best = max(pur, default=0.0)
            ties["empty"] += not flags
            ties["purity"] += best > 0 and pur.count(best) > 1
            ties["hits"] += best > 0 and len({h_ for p_, h_ in zip(pur, hit) if p_ == best}) > 1
            ties["zero"] += bool(pur) and best == 0.0 and len(pur) > 1
        lefts = np.flatnonzero(table["is_left"])
        for lq in lefts:
            rq = [r for r in np.flatnonzero(table["merged"] == table["merged"][lq]) if r != lq][0]
            ties["left_only"] += int((table["vis"][:, lq] & ~table["vis"][:, rq].astype(bool)).any())
    assert all(v >= 20 for v in ties.values()), ties


def test_parser_matches_by_last_two_components_and_reads_sizes_from_the_header(tmp_path):
    from PIL import Image
    meta, rec, _ = load_purity_fixture(FIXTURES[0])
    files = write_annotation_files(meta, tmp_path)
    paths = []
    for rel, (w, h) in zip(meta["image_paths"], rec["sizes"]):
        path = tmp_path / "root" / rel
        path.parent.mkdir(parents=True, exist_ok=True)
        Image.new("RGB", (int(w), int(h))).save(path)
        paths.append(str(path))
    assert any("normal_" in p for p in paths) and image_key("a/b/c/normal_x.png") == "c/x.png"
    assert image_key("C:\\data\\c\\normal_x.png") == "c/x.png"           # a Windows-style path
    ann = PartAnnotations.from_cub(files["part_locs"], files["parts"], files["images"], paths)
    want = fixture_annotations(meta, rec, tmp_path)
    for f in ("xy", "vis", "size", "merged", "is_left", "pair_index"):
        assert torch.equal(getattr(ann, f), getattr(want, f)), f
    assert ann.merged_names == [n for n in ann.part_names if "left" not in n] and len(ann.merged_names) == 12
    assert ann.image_keys[1] == image_key(paths[1]) and "normal_" not in ann.image_keys[1]
    # the table: left ids share their right partner's merged part, pair order = file order of the lefts
    names = ann.part_names
    for q, nm in enumerate(names):
        if "left" in nm:
            assert ann.is_left[q] and ann.merged[q] == ann.merged[names.index(nm.replace("left", "right"))]
    assert ann.pair_index[ann.is_left.bool()].tolist() == [0, 1, 2]
    planted = {what.split(" (")[0] for _, _, what in meta["planted"]}
    assert {"no visible part", "left eye only", "right eye only", "both eyes"} <= planted
    empty_img = meta["planted"][0][0]
    assert int(ann.vis[empty_img].sum()) == 0 and ann.visible_parts(empty_img) == {}


def test_parser_errors(tmp_path):
    meta, rec, _ = load_purity_fixture(FIXTURES[0])
    files = write_annotation_files(meta, tmp_path)
    paths = ["/data/" + p for p in meta["image_paths"]]
    sizes = [tuple(int(v) for v in s) for s in rec["sizes"]]
    args = (files["part_locs"], files["parts"], files["images"])
    PartAnnotations.from_cub(*args, paths, image_sizes=sizes)
    with pytest.raises(ValueError, match="is not in"):
        PartAnnotations.from_cub(*args, paths[:3] + ["/data/001.X/unknown.png"], image_sizes=sizes[:4])
    with pytest.raises(ValueError, match="image sizes"):
        PartAnnotations.from_cub(*args, paths, image_sizes=sizes[:-1])
    no_partner = tmp_path / "parts_no_partner.txt"
    no_partner.write_text(meta["files"]["parts"].replace("right wing", "other wing"))
    with pytest.raises(ValueError, match="no partner"):
        PartAnnotations.from_cub(files["part_locs"], str(no_partner), files["images"], paths, image_sizes=sizes)
    lines = meta["files"]["part_locs"].splitlines()
    lines[3], lines[4] = lines[4], lines[3]                     # ids 5, 4 of the first image
    swapped = tmp_path / "locs_swapped.txt"
    swapped.write_text("\n".join(lines) + "\n")
    with pytest.raises(ValueError, match="ascending"):
        PartAnnotations.from_cub(str(swapped), files["parts"], files["images"], paths, image_sizes=sizes)
    missing = tmp_path / "locs_missing.txt"
    missing.write_text("\n".join(l for l in meta["files"]["part_locs"].splitlines() if not l.startswith("2 ")) + "\n")
    with pytest.raises(ValueError, match="no line"):
        PartAnnotations.from_cub(str(missing), files["parts"], files["images"], paths, image_sizes=sizes)


def test_part_purity_refuses_a_count_net_a_wrong_mode_and_a_loader_of_another_length(tmp_path):
    from count_pipnet_amd.purity import part_purity
    meta, rec, _ = load_purity_fixture(FIXTURES[0])
    ann = fixture_annotations(meta, rec, tmp_path)

    class CountNet(torch.nn.Module):
        _max_count = 3

    with pytest.raises(NotImplementedError, match="CountPIPNet"):
        part_purity(CountNet(), [], ann, image_size=64)
    with pytest.raises(ValueError, match="mode"):
        part_purity(torch.nn.Linear(1, 1), [], ann, image_size=64, mode="best")

    class Loader(list):
        dataset = list(range(ann.images + 1))

    with pytest.raises(ValueError, match="images"):
        part_purity(torch.nn.Linear(1, 1), Loader(), ann, image_size=64)


def test_centring_correction_on_oversized_patches(tmp_path):
    """A 50 x 32 patch is cut to rows 9 .. 41 of 0 .. 50 (9 = 18 // 2 off either end); an odd excess
    leaves one pixel more: 0 .. 45 -> 6 .. 39."""
    names = ["left eye", "crown", "right eye"]
    ids = ["1", "2", "3"]
    sizes = [(64, 64), (128, 32)]
    files = {"parts": "".join(f"{i} {n}\n" for i, n in zip(ids, names)),
             "images": "1 a/x.png\n2 a/y.png\n",
             "part_locs": "1 1 10.0 5.0 1\n1 2 10.0 9.0 1\n1 3 10.0 41.5 1\n"
                          "2 1 12.0 20.5 1\n2 2 100.0 3.0 1\n2 3 0.0 0.0 0\n"}
    for k, v in files.items():
        (tmp_path / (k + ".txt")).write_text(v)
    ann = PartAnnotations.from_cub(str(tmp_path / "part_locs.txt"), str(tmp_path / "parts.txt"),
                                   str(tmp_path / "images.txt"), ["r/a/x.png", "r/a/y.png"], image_sizes=sizes)
    rows = [(7, 0, 0, 50, 0, 32),          # rows 9..41: crown (y 9) in, left eye (y 5) out, right eye (41.5) out
            (7, 1, 0, 45, 0, 77),          # image 128 x 32: rows 6..39 -> y 3..19.5; cols 22..55 -> x 44..110
            (9, 0, 0, 32, 0, 32)]          # not oversized: left eye (5) in -> folded into right eye; crown stays first
    csvfile = write_patch_csv(rows, ["r/a/x.png", "r/a/y.png"], str(tmp_path / "p.csv"))
    got = eval_patch_csv(csvfile, ann, 64)
    assert got.presences == {"7": {"2": [1, 1], "3": [0, 0]}, "9": {"2": [1], "3": [1]}}
    assert got.max_part == {"7": "crown", "9": "crown"} and got.max_purity == {"7": 1.0, "9": 1.0}
    assert got.most_part == {"7": ("2", 2), "9": ("2", 1)}
    parts = [ann.visible_parts(i) for i in range(2)]
    ref = restate([(str(p),) + tuple(r) for p, *r in rows], parts, sizes, ids, names, 64)
    assert ref["presences"] == got.presences and ref["logged"] == got.summary()
    uncut = restate([(str(p),) + tuple(r) for p, *r in rows], parts, sizes, ids, names, 64, centre=False)
    assert uncut["presences"]["7"] == {"2": [1, 1], "3": [1, 1]}          # the whole patch would have bought purity


def test_patches_are_always_32_pixels_square():
    """img_coordinates yields 32 x 32 for every map size 1..28 (the centring correction never fires
    for the project's own patches), for the map shape (P, H, W) the evaluation hands it and for the
    4-D shape of the visualisation; the kernels' geometry (numpy twin) is the former."""
    for size in (64, 224):
        for h in range(1, 29):
            for w in range(1, 29):
                geo = geometry(h, w, size)
                hh, ww = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
                for shape in ((5, h, w), (26, h, w), (1, 26, h, w), (1, 7, h, w)):
                    h0, h1, w0, w1 = img_coordinates(size, shape, 32, geo[3], hh.flatten(), ww.flatten())
                    assert bool(((h1 - h0) == 32).all()) and bool(((w1 - w0) == 32).all()), (size, shape)
                    if len(shape) == 3 and shape[0] == 5:
                        mine = [np_patch(geo, l) for l in range(h * w)]
                        assert mine == list(zip(h0.tolist(), h1.tolist(), w0.tolist(), w1.tolist())), (size, h, w)


def test_patch_geometry_equals_the_recorded_reference_coordinates():
    """The reference's get_img_coordinates under the 3-D map shape (P, H, W) its part evaluation
    hands on, recorded for every latent location of the fixture's map and of the full backbones'
    maps: a 26 x 26 map takes the small-stride rule whatever the number of prototypes."""
    meta, rec, _ = load_purity_fixture(FIXTURES[0])
    keys = [k for k in rec if k.startswith("coords_")]
    assert len(keys) == 5
    for key in keys:
        pn, hw, size = (int(v) for v in key.split("_")[1:])
        geo = geometry(hw, hw, size)
        assert geo[4] == (hw == 26)
        assert [np_patch(geo, l) for l in range(hw * hw)] == [tuple(r) for r in rec[key].tolist()], key
        l = torch.arange(hw * hw)
        mine = img_coordinates(size, (pn, hw, hw), 32, geo[3], l // hw, l % hw)
        assert torch.equal(torch.stack(mine, dim=1), torch.from_numpy(rec[key]).long()), key
