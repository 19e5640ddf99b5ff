"""Explanation images on the GPU (count_pipnet_amd.gallery, csrc/gallery_ops.hip), bit for bit:

* pipnet_patch_compose_rgb8 against numpy slices: every byte alignment of a 3-byte pixel, windows cut at the
  bottom and the right, sentinel bytes outside the cells, one launch of 2048 * 10 items, the host refusals;
* pipnet_draw_rects_rgb8 against the rule tests/test_gallery_cpu.py holds against Pillow;
* prototype_gallery / explanation_images end to end on an ImageFolder of PNG files against tests/gallery_ref.py
  applied to the same pass result, whatever the batch size, and without touching the net.
"""
import os

import numpy as np
import pytest
import torch

import gallery_ref as R
from count_pipnet_amd import kernels as K
from count_pipnet_amd.data import DecodedImageFolder, DeviceEvalLoader, DeviceEvalTransform, pack_images
from count_pipnet_amd.gallery import explanation_images, prototype_gallery
from count_pipnet_amd.local import LocalExplanation, explain_predictions
from count_pipnet_amd.topk import prototype_topk
from golden_util import load_golden
from input_util import synth_photo
from model_util import build_model

pytestmark = pytest.mark.gpu

SIZES = [(5, 7), (64, 64), (57, 83)]
SENTINEL = 0xA5


# ---- compose kernel ---------------------------------------------------------------------------------------------
def np_compose(frames, items, canvases):
    out = canvases.copy()
    for f, h0, h1, w0, w1, c, y, x in items:
        cut = frames[f, h0:h1, w0:w1]
        out[c, y:y + cut.shape[0], x:x + cut.shape[1]] = cut
    return out


def _frames(n, fh, fw, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, fh, fw, 3), dtype=np.uint8)


def _items(fh, fw):
    """Cells that do not overlap on two 40 x 175 canvases (odd width: rows start at every byte alignment)."""
    items = [(0, 0, 1, 0, 1, 0, 0, 0), (1, fh - 1, fh, fw - 1, fw, 0, 0, 1), (2, fh // 2, fh // 2 + 1, 1, 2, 0, 0, 2),
             (0, 1, 2, fw - 2, fw - 1, 0, 1, 3), (1, 0, 1, 3, 4, 0, 2, 5)]                    # 1 x 1 at x = 0, 1, 2, 3, 5
    hb, wr = max(fh - 20, 0), max(fw - 20, 0)
    items += [(0, 0, 32, 0, 32, 0, 4, 0),                        # 32 x 32 (cut by a small frame)
              (1, hb, hb + 32, wr, wr + 32, 0, 4, 33),           # cut at the bottom and the right
              (2, min(3, fh - 1), 35, min(2, fw - 1), 34, 0, 4, 67),
              (2, min(3, fh - 1), 35, min(2, fw - 1), 34, 0, 4, 101),                           # two items, one source
              (1, hb, hb + 32, 0, 32, 0, 5, 135)]                # cut at the bottom only, odd row
    items += [(0, 0, 32, wr, wr + 32, 1, 3, x) for x in (1, 36, 71, 106, 143)]                # one frame into many cells
    return items


@pytest.mark.parametrize("fh,fw", SIZES)
def test_patch_compose_matches_numpy_slices_at_every_alignment(gpu, fh, fw):
    frames = _frames(3, fh, fw, fh * fw)
    canvases = np.full((2, 40, 175, 3), SENTINEL, np.uint8)
    items = _items(fh, fw)
    want = np_compose(frames, items, canvases)
    assert (want != canvases).any() and (want == SENTINEL).sum() > want.size // 4
    assert {((c * 40 + y) * 175 + x) * 3 % 4 for *_, c, y, x in items} == {0, 1, 2, 3}
    dev = torch.from_numpy(canvases).to(gpu)
    got = K.patch_compose_rgb8(torch.from_numpy(frames).to(gpu), items, dev)
    assert got is dev
    assert np.array_equal(got.cpu().numpy(), want)              # cells and the sentinel bytes around them
    # the table as a tensor or an array, one item at a time: the same canvases
    dev2 = torch.from_numpy(canvases).to(gpu)
    for it in items:
        K.patch_compose_rgb8(torch.from_numpy(frames).to(gpu), torch.tensor([it]), dev2)
    assert torch.equal(dev2, got)


def test_patch_compose_empty_table_launches_nothing(gpu):
    frames = torch.from_numpy(_frames(2, 8, 8, 1)).to(gpu)
    canvases = torch.full((1, 9, 11, 3), SENTINEL, dtype=torch.uint8, device=gpu)
    for empty in ([], np.zeros((0, 8), np.int32), torch.zeros((0, 8), dtype=torch.int64)):
        assert K.patch_compose_rgb8(frames, empty, canvases) is canvases
    assert (canvases == SENTINEL).all()
    none = torch.empty((0, 8, 8, 3), dtype=torch.uint8, device=gpu)
    K.patch_compose_rgb8(none, [], canvases)                     # no frames, no items
    with pytest.raises(RuntimeError):
        K.patch_compose_rgb8(none, [(0, 0, 1, 0, 1, 0, 0, 0)], canvases)


def test_patch_compose_one_launch_of_2048_grids(gpu):
    """A 2048-prototype k = 10 gallery in one call: 20480 items of 32 x 32 into [2048, 32, 331, 3]."""
    pn, k, f = 2048, 10, 64
    rng = np.random.default_rng(5)
    frames = _frames(f, 64, 64, 9)
    src = rng.integers(0, f, pn * k)
    org = rng.integers(0, 33, (pn * k, 2))
    items = [(int(src[i]), int(org[i, 0]), int(org[i, 0]) + 32, int(org[i, 1]), int(org[i, 1]) + 32, i // k, 0,
              (i % k) * 33 + 1) for i in range(pn * k)]
    canvases = np.full((pn, 32, k * 33 + 1, 3), R.PAD, np.uint8)
    want = np_compose(frames, items, canvases)
    got = K.patch_compose_rgb8(torch.from_numpy(frames).to(gpu), items, torch.from_numpy(canvases).to(gpu))
    assert torch.equal(got, torch.from_numpy(want).to(gpu))
    assert (got[:, :, ::33] == R.PAD).all()


@pytest.mark.parametrize("bad", [
    (3, 0, 4, 0, 4, 0, 0, 0), (-1, 0, 4, 0, 4, 0, 0, 0),             # frame index
    (0, 0, 4, 0, 4, 2, 0, 0), (0, 0, 4, 0, 4, -1, 0, 0),             # canvas index
    (0, -1, 4, 0, 4, 0, 0, 0), (0, 0, 4, -2, 4, 0, 0, 0),            # window origin
    (0, 0, 4, 0, 4, 0, -1, 0), (0, 0, 4, 0, 4, 0, 0, -1),            # cell origin
    (0, 0, 4, 0, 4, 0, 7, 0), (0, 0, 4, 0, 4, 0, 0, 10),             # the window does not fit at (y, x)
    (0, 0, 99, 0, 99, 0, 1, 0),                                       # cut to the 8 x 8 frame, still too tall at y = 1
    (0, 0, 4, 0, 4, 0, 0, 1 << 31),                                   # no int32
])
def test_patch_compose_refuses_rows_out_of_range_before_it_launches(gpu, bad):
    frames = torch.from_numpy(_frames(3, 8, 8, 2)).to(gpu)
    canvases = torch.full((2, 8, 12, 3), SENTINEL, dtype=torch.uint8, device=gpu)
    good = (1, 0, 4, 0, 4, 1, 2, 3)
    with pytest.raises(RuntimeError):
        K.patch_compose_rgb8(frames, [good, bad], canvases)
    torch.cuda.synchronize()
    assert (canvases == SENTINEL).all()                              # the good row was not written either
    K.patch_compose_rgb8(frames, [good, (0, 0, 99, 0, 99, 0, 0, 0)], canvases)      # cut to the frame: fits
    assert torch.equal(canvases[0, :, :8], frames[0]) and (canvases[0, :, 8:] == SENTINEL).all()


def test_patch_compose_checks_its_operands(gpu):
    frames = torch.from_numpy(_frames(1, 8, 8, 3)).to(gpu)
    canvases = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=gpu)
    item = [(0, 0, 4, 0, 4, 0, 0, 0)]
    for f, c in [(frames.float(), canvases), (frames.cpu(), canvases), (frames, canvases.cpu()),
                 (frames[:, :, ::2], canvases), (frames[..., :2], canvases), (frames, canvases[0])]:
        with pytest.raises(RuntimeError):
            K.patch_compose_rgb8(f, item, c)
    with pytest.raises(RuntimeError):
        K.patch_compose_rgb8(frames, [(0.5, 0, 4, 0, 4, 0, 0, 0)], canvases)


# ---- rectangle kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fh,fw", SIZES)
@pytest.mark.parametrize("width", [1, 2, 3])
def test_draw_rects_matches_the_outline_rule(gpu, fh, fw, width):
    frames = _frames(2, fh, fw, fh + fw + width)
    m = 2 * width
    rects = [(0, 0, max(fw - 1, m), max(fh - 1, m)), (0, 0, max(fw, m), max(fh, m)),      # x1 == fw: the patch boxes
             (fw - 1 - m, fh - 1 - m, fw - 1, fh - 1), (0, 0, m, m), (fw - 3, fh - 3, fw + 29, fh + 29),
             (-5, -4, m - 2, m + 1), (-9, -9, fw + 9, fh + 9), (fw + 2, 1, fw + 2 + m, 1 + m),
             (1, 0, 1 + m, fh + 40), (fw - 32, fh - 32, fw, fh)]
    src = [i % 2 for i in range(len(rects))]
    got = K.draw_rects_rgb8(torch.from_numpy(frames).to(gpu), src, rects, width).cpu().numpy()
    assert got.shape == (len(rects), fh, fw, 3)
    for n, rect in enumerate(rects):
        assert np.array_equal(got[n], R.draw_rect(frames[src[n]], rect, width)), rect
    other = K.draw_rects_rgb8(torch.from_numpy(frames).to(gpu), torch.tensor(src), np.array(rects), width, (1, 2, 3))
    assert np.array_equal(other[3].cpu().numpy(), R.draw_rect(frames[src[3]], rects[3], width, (1, 2, 3)))


def test_draw_rects_refusals_and_empty_table(gpu):
    frames = torch.from_numpy(_frames(2, 16, 16, 4)).to(gpu)
    assert tuple(K.draw_rects_rgb8(frames, [], np.zeros((0, 4), np.int64)).shape) == (0, 16, 16, 3)
    with pytest.raises(ValueError):
        K.draw_rects_rgb8(frames, [0, 1], [(0, 0, 15, 15), (2, 2, 5, 12)], 2)        # 4 pixels wide, 2 * 2 + 1 needed
    for src, rects, kw in [([2], [(0, 0, 8, 8)], {}), ([-1], [(0, 0, 8, 8)], {}), ([0, 1], [(0, 0, 8, 8)], {}),
                           ([0], [(0, 0, 8, 8)], dict(colour=(0, 256, 0))), ([0], [(0, 0, 1 << 31, 8)], {})]:
        with pytest.raises(RuntimeError):
            K.draw_rects_rgb8(frames, src, rects, 2, **kw)


# ---- end to end -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """18 lossless PNG files, 40..90 pixels a side, two in each of 9 classes; the resized frames by the oracle."""
    from PIL import Image
    root = tmp_path_factory.mktemp("gallery_folder")
    rng = np.random.default_rng(21)
    for i in range(18):
        d = root / f"class_{i // 2}"
        os.makedirs(d, exist_ok=True)
        h, w = (int(v) for v in rng.integers(40, 91, 2))
        Image.fromarray(synth_photo(h, w, 300 + i, "smooth" if i % 3 else "noise")).save(d / f"img_{i:02d}.png")
    ds = DecodedImageFolder(str(root))
    assert len(ds) == 18 and ds.targets == [i // 2 for i in range(18)]
    cache = {}

    def frame_of(i):
        if i not in cache:
            cache[i] = R.frame(ds[i][0], 64)
        return cache[i]

    return ds, frame_of


def _topk(net, ds, gpu, k):
    torch.manual_seed(5)                    # a CountPIPNet draws its Gumbel noise from this generator
    loader = DeviceEvalLoader(ds, DeviceEvalTransform(64), gpu, batch_size=5, shuffle=False)
    return prototype_topk(net, loader, k, image_size=64).cpu()


def _snapshot(net):
    return {n: t.detach().clone() for n, t in net.state_dict().items()}, {n: m.training for n, m in net.named_modules()}


def _assert_untouched(net, snap):
    state, flags = snap
    now = net.state_dict()
    assert list(now) == list(state) and all(torch.equal(now[n], state[n]) for n in state)
    assert {n: m.training for n, m in net.named_modules()} == flags


def _assert_gallery(g, want):
    for name, exp in want.items():
        got = getattr(g, name)
        if name == "frames" and got is None:
            continue
        assert got.device.type == "cpu", name
        assert np.array_equal(got.numpy(), exp), name
        assert got.numpy().dtype == exp.dtype, name


TOPK_FIELDS = ("scores", "index", "h_idx", "w_idx", "coords", "selected", "unused", "abstained")


@pytest.mark.parametrize("name,k", [("pipnet_mid_addon", 3), ("c1_count_identity", 4)])
def test_prototype_gallery_matches_the_reference_grids(gpu, folder, name, k):
    ds, frame_of = folder
    net = build_model(load_golden(name)[0]).to(gpu)
    res = _topk(net, ds, gpu, k)
    snap = _snapshot(net)
    want = R.expected_gallery(res, frame_of, 64)
    assert (want["cells"] >= 2).any(), "no grid with two patches: the padded layout is untested"
    assert want["ok"].all() and (want["height"][want["cells"] >= 2] == 32).all()
    first = prototype_gallery(net, ds, res, image_size=64, batch_size=4, keep_frames=True)
    assert first.grids.is_cuda and first.frames.is_cuda and first.grids.shape == (res.scores.shape[0], 32, k * 33 + 1, 3)
    _assert_gallery(first.cpu(), want)
    for kwargs in (dict(net_or_none=None, device=gpu, batch_size=1), dict(net_or_none=net, batch_size=64),
                   dict(net_or_none=None, batch_size=7, keep_frames=True)):
        g = prototype_gallery(kwargs.pop("net_or_none"), ds, res.cpu(), image_size=64, **kwargs)
        assert (g.frames is None) != kwargs.get("keep_frames", False)
        _assert_gallery(g.cpu(), want)
    _assert_untouched(net, snap)
    again = _topk(net, ds, gpu, k)
    for f in TOPK_FIELDS:
        assert torch.equal(getattr(again, f), getattr(res, f)), f
    # the documented way to the picture
    p = int(np.argmax(want["cells"]))
    g = first.cpu()
    picture = g.grids[p, :g.height[p], :g.width[p]].numpy()
    assert picture.shape == (32, int(want["cells"][p]) * 33 + 1, 3) and (picture[:, ::33] == R.PAD).all()
    other = prototype_gallery(net, ds, res, image_size=64, pad_value=7).cpu()
    assert (other.grids[p, :, ::33] == 7).all() and torch.equal(other.grids[p, :, 1:33], g.grids[p, :, 1:33])


def test_prototype_gallery_single_patch_unequal_windows_and_a_repeated_image(gpu, folder):
    """Hand-built pass results, where the branches are certain: one entry (make_grid returns the patch unpadded, the
    crop takes its first and last row), windows of different sizes (make_grid raises: ok False, no grid), equal cut
    windows, and the reference's k = 10, 10 / 1 / 1 selection that shows one image twice."""
    ds, frame_of = folder
    cut = (40, 72, 0, 32)                                        # 24 rows left on a 64-pixel frame
    pip = R.build_topk(5, [None], 3, {(0, 0): [(0.9, 4, (3, 35, 30, 62))], (1, 0): [(0.9, 1), (0.8, 2, cut)],
                                      (2, 0): [(0.9, 6, cut), (0.5, 6, cut)], (3, 0): [(0.7, 17), (0.6, 0), (0.5, 9)],
                                      (4, 0): [(0.05, 3)]})
    want = R.expected_gallery(pip, frame_of, 64)
    assert want["cells"].tolist() == [1, 0, 2, 3, 0] and want["ok"].tolist() == [True, False, True, True, True]
    assert want["height"].tolist() == [30, 0, 24, 32, 0] and want["width"].tolist() == [32, 0, 67, 100, 0]
    assert want["frame_index"].tolist() == [0, 4, 6, 9, 17]
    assert np.array_equal(want["grids"][0, :30, :32], frame_of(4)[4:34, 30:62])
    for bs in (1, 2, 64):
        _assert_gallery(prototype_gallery(None, ds, pip, image_size=64, device=gpu, batch_size=bs, keep_frames=True).cpu(),
                        want)
    lists = {(0, 0): [(0.95 - 0.05 * j, j) for j in range(10)], (0, 1): [(0.72, 12)], (0, 2): [(0.2, 15)]}
    count = R.build_topk(2, [1, 2, 3], 10, lists)
    want = R.expected_gallery(count, frame_of, 64)
    assert want["entry_index"][0].tolist() == [0, 1, 2, 3, 3, 4, 12, 5, 6, 15] and want["cells"].tolist() == [10, 0]
    g = prototype_gallery(None, ds, count, image_size=64, device=gpu).cpu()
    _assert_gallery(g, want)
    assert torch.equal(g.grids[0, :, 3 * 33 + 1:4 * 33], g.grids[0, :, 4 * 33 + 1:5 * 33])
    with pytest.raises(ValueError):
        prototype_gallery(None, ds, R.build_topk(1, [None], 2, {(0, 0): [(0.9, 18)]}), image_size=64, device=gpu)


def _assert_images(imgs, want):
    for name, exp in want.items():
        assert np.array_equal(getattr(imgs, name).numpy(), exp), name


@pytest.mark.parametrize("name", ["pipnet_mid_addon", "c1_count_identity"])
def test_explanation_images_match_the_reference_in_both_input_forms(gpu, folder, name):
    ds, frame_of = folder
    net = build_model(load_golden(name)[0]).to(gpu)
    idx = [3, 0, 17, 5, 5, 9, 12]
    torch.manual_seed(5)
    xs, u8 = DeviceEvalTransform(64)(pack_images([ds[i][0] for i in idx]), gpu, want_u8=True)
    res = explain_predictions(net, xs, 3, image_size=64, max_entries=4)
    snap = _snapshot(net)
    frames = np.stack([frame_of(i) for i in idx])
    assert np.array_equal(u8.cpu().numpy(), frames)
    want = R.expected_explanations(res.cpu(), frames)
    n = want["entry"].shape[0]
    assert n == int(res.count.clamp(max=4).sum()) and n >= 4
    assert (res.count.cpu() > 4).any(), "no truncated list: min(count, max_entries) is untested"
    a = explanation_images(u8, res, image_size=64, batch_size=3)
    assert a.patches.is_cuda and a.rects.is_cuda and tuple(a.rects.shape) == (n, 64, 64, 3)
    _assert_images(a.cpu(), want)
    _assert_images(explanation_images(ds, res, image_size=64, indices=idx, batch_size=2).cpu(), want)
    _assert_images(explanation_images(ds, res.cpu(), image_size=64, indices=torch.tensor(idx)).cpu(), want)
    assert (a.rects.cpu().numpy() != frames[want["entry"][:, 0]]).any(axis=(1, 2, 3)).all()       # every frame is marked
    _assert_images(explanation_images(u8, res, image_size=64, rect_width=1).cpu(),
                   R.expected_explanations(res.cpu(), frames, 1))
    _assert_untouched(net, snap)
    for bad in (dict(indices=idx), {}):
        with pytest.raises(ValueError):
            explanation_images(u8 if bad else ds, res, image_size=64, **bad)
    with pytest.raises(ValueError):
        explanation_images(u8[:3], res, image_size=64)
    with pytest.raises(ValueError):
        explanation_images(u8, res, image_size=64, rect_width=16)                  # a 32-pixel box, 33 needed


def test_explanation_images_cut_windows_and_empty_results(gpu, folder):
    """A hand-built result: windows cut by the frame are padded to 32 x 32 with their true size beside them, slots
    beyond ``count`` and beyond ``max_entries`` are passed over, an image without entries gives no row."""
    ds, frame_of = folder
    b, c, m = 3, 2, 2
    z = lambda *s: torch.zeros(*s, dtype=torch.int64)      # noqa: E731
    count = torch.tensor([[2, 0], [0, 0], [5, 1]])
    coords = torch.full((b, c, m, 4), -1, dtype=torch.int64)
    rect = torch.full((b, c, m, 4), -1, dtype=torch.int64)
    coords[0, 0, 0], rect[0, 0, 0] = torch.tensor((40, 72, 50, 82)), torch.tensor((50, 40, 64, 64))    # 24 x 14
    coords[0, 0, 1], rect[0, 0, 1] = torch.tensor((0, 32, 0, 32)), torch.tensor((0, 0, 32, 32))
    coords[2, 0, 0], rect[2, 0, 0] = torch.tensor((32, 64, 32, 64)), torch.tensor((35, 35, 64, 64))
    coords[2, 0, 1], rect[2, 0, 1] = torch.tensor((5, 37, 60, 92)), torch.tensor((60, 5, 64, 37))       # 32 x 4
    coords[2, 1, 0], rect[2, 1, 0] = torch.tensor((63, 95, 63, 95)), torch.tensor((59, 59, 64, 64))     # 1 x 1
    res = LocalExplanation(classes=z(b, c), logits=torch.zeros(b, c), count=count, prototype=z(b, c, m),
                           similarity=torch.zeros(b, c, m), weight=torch.zeros(b, c, m), simweight=torch.zeros(b, c, m),
                           h_idx=z(b, c, m), w_idx=z(b, c, m), coords=coords, rect=rect, proto_shape=(1, 4, 8, 8))
    idx = [2, 7, 11]
    frames = np.stack([frame_of(i) for i in idx])
    want = R.expected_explanations(res, frames)
    assert want["entry"].tolist() == [[0, 0, 0], [0, 0, 1], [2, 0, 0], [2, 0, 1], [2, 1, 0]]
    assert want["patch_hw"].tolist() == [[24, 14], [32, 32], [32, 32], [32, 4], [1, 1]]
    got = explanation_images(ds, res, image_size=64, indices=idx, batch_size=2)
    assert got.patches.device == gpu or got.patches.is_cuda
    _assert_images(got.cpu(), want)
    res.count[:] = 0
    none = explanation_images(torch.from_numpy(frames).to(gpu), res, image_size=64).cpu()
    assert tuple(none.entry.shape) == (0, 3) and tuple(none.patches.shape) == (0, 32, 32, 3)
    assert tuple(none.patch_hw.shape) == (0, 2) and tuple(none.rects.shape) == (0, 64, 64, 3)
