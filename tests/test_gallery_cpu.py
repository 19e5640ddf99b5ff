"""The host half of count_pipnet_amd.gallery, without a GPU: the selection of the shown entries against the
statement-by-statement restatement of the reference (tests/gallery_ref.py) and against lists worked out by hand,
the grid layout against the numpy ``make_grid``, the rectangle rule against Pillow itself, and the uint8 facts
that make the whole path integer copying."""
import numpy as np
import pytest
import torch

import gallery_ref as R
from count_pipnet_amd import gallery
from count_pipnet_amd import kernels as K


def _shown(res):
    got = gallery.select_entries(res)
    assert len(got) == res.scores.shape[0]
    return {p: e for p, e in enumerate(got) if e}


def _score(j):
    return 0.95 - 0.05 * j


COUNT_CASES = {
    # k = 10 with 10 / 1 / 1 entries: samples_per_group 3, one extra; group 1 takes slots 0-3, the fill step offers
    # its slot 3 again (extra_samples is 0 by then) -> the image of slot 3 twice
    "duplicate": (10, {(0, 0): [(_score(j), j) for j in range(10)], (0, 1): [(0.72, 20)], (0, 2): [(0.2, 30)]},
                  {0: [(0, 0), (0, 1), (0, 2), (0, 3), (0, 3), (0, 4), (1, 0), (0, 5), (0, 6), (2, 0)]}),
    "k3_three_groups": (3, {(0, 0): [(0.3, 1), (0.2, 2)], (0, 1): [(0.9, 3)], (0, 2): [(0.5, 4), (0.4, 5)]},
                        {0: [(1, 0), (2, 0), (0, 0)]}),
    "one_group": (3, {(0, 1): [(0.6, 7), (0.5, 8)]}, {0: [(1, 0), (1, 1)]}),
    # integer counts tie across groups: the final sort is stable, the groups' order survives among equals
    "ties": (4, {(0, 0): [(2.0, 1), (1.0, 2)], (0, 1): [(2.0, 3), (2.0, 4), (1.0, 5)]},
             {0: [(0, 0), (1, 0), (1, 1), (0, 1)]}),
    "ties_fill": (5, {(0, 0): [(2.0, 1), (1.0, 2)], (0, 2): [(2.0, 3), (2.0, 4), (1.0, 5)]},
                  {0: [(0, 0), (2, 0), (2, 1), (0, 1), (2, 2)]}),
    # prototype 0 has no entry at all, prototype 1 one
    "no_entry": (3, {(1, 2): [(1.0, 4)]}, {1: [(2, 0)]}),
}


@pytest.mark.parametrize("name", sorted(COUNT_CASES))
def test_count_selection_matches_the_reference_statements_and_the_hand_worked_lists(name):
    k, lists, want = COUNT_CASES[name]
    res = R.build_topk(2, [1, 2, 3], k, lists)
    assert R.selection(res) == want
    assert _shown(res) == want


def test_count_selection_duplicate_shows_one_image_twice():
    k, lists, want = COUNT_CASES["duplicate"]
    res = R.build_topk(2, [1, 2, 3], k, lists)
    shown = _shown(res)[0]
    assert len(shown) == 10 and shown.count((0, 3)) == 2 and len(set(shown)) == 9


def test_count_selection_passes_over_unselected_prototypes():
    res = R.build_topk(3, [1, 2, 3], 3, {(0, 0): [(1.0, 1)], (1, 0): [(1.0, 2)], (2, 1): [(3.0, 3)]},
                       selected=[True, False, True])
    assert R.selection(res) == {0: [(0, 0)], 2: [(1, 0)]} == _shown(res)


def test_count_selection_random_tables_match_the_restatement():
    g = torch.Generator().manual_seed(11)
    for k in (1, 2, 3, 7, 10):
        lists = {}
        for p in range(24):
            for gi in range(3):
                n = int(torch.randint(0, k + 1, (1,), generator=g))
                sc = sorted((float(torch.randint(1, 4, (1,), generator=g)) for _ in range(n)), reverse=True)   # ties
                lists[(p, gi)] = [(s, 100 * gi + 10 * p + j) for j, s in enumerate(sc)]
        res = R.build_topk(24, [1, 2, 3], k, lists, selected=[p % 5 != 0 for p in range(24)])
        assert _shown(res) == R.selection(res)


def test_pipnet_selection_shows_used_selected_prototypes_in_slot_order():
    lists = {(0, 0): [(0.9, 5), (0.4, 2)], (1, 0): [(0.05, 1), (0.01, 3)], (2, 0): [(0.8, 4)]}
    res = R.build_topk(4, [None], 3, lists, selected=[True, True, False, True])
    assert res.unused.tolist() == [False, True, False, True]          # 1: nothing above 0.1; 3: selected, nothing stored
    assert R.selection(res) == {0: [(0, 0), (0, 1)]} == _shown(res)


# ---- the grid ---------------------------------------------------------------------------------------------------
def _compose(frames, windows, layout, k, pad=R.PAD):
    canvas = np.full((R.PATCH, k * (R.PATCH + 1) + 1, 3), pad, np.uint8)
    for fr, (h0, h1, w0, w1, y, x) in zip(frames, layout[2]):
        canvas[y:y + h1 - h0, x:x + w1 - w0] = fr[h0:h1, w0:w1]
    return canvas


@pytest.mark.parametrize("n,k", [(1, 4), (2, 4), (4, 4), (10, 10), (1, 1)])
def test_grid_layout_is_make_grid_and_crop(n, k):
    rng = np.random.default_rng(n + k)
    frames = [rng.integers(0, 256, (40, 40, 3), dtype=np.uint8) for _ in range(n)]
    windows = [(int(a), int(a) + 32, int(b), int(b) + 32) for a, b in rng.integers(0, 9, (n, 2))]
    want = R.patch_grid([fr[h0:h1, w0:w1] for fr, (h0, h1, w0, w1) in zip(frames, windows)], k)
    height, width, items = layout = gallery.grid_layout(windows)
    assert (height, width) == want.shape[:2] == ((30, 32) if n == 1 else (32, n * 33 + 1))
    canvas = _compose(frames, windows, layout, k)
    assert np.array_equal(canvas[:height, :width], want)
    rest = np.ones(canvas.shape[:2], bool)
    rest[:height, :width] = False
    assert (canvas[rest] == R.PAD).all()
    if n >= 2:
        assert [it[5] for it in items] == [j * 33 + 1 for j in range(n)] and (want[:, ::33] == R.PAD).all()


def test_grid_layout_refuses_windows_of_different_sizes_as_make_grid_does():
    rng = np.random.default_rng(3)
    fr = rng.integers(0, 256, (40, 40, 3), dtype=np.uint8)
    windows = [(0, 32, 0, 32), (8, 40, 10, 40)]                        # the second is cut to 32 x 30
    assert R.patch_grid([fr[h0:h1, w0:w1] for h0, h1, w0, w1 in windows], 4) is None
    assert gallery.grid_layout(windows) is None
    assert gallery.grid_layout([windows[1], windows[1]])[:2] == (32, 2 * 31 + 1)      # equal but smaller: a grid


def test_window_follows_python_slices():
    fr = np.arange(40 * 40).reshape(40, 40)
    for coords in [(0, 32, 8, 40), (20, 52, 30, 62), (8, 40, 39, 71), (40, 72, 0, 32), (-8, 24, 0, 32)]:
        h0, h1, w0, w1 = gallery._window(coords, 40)
        assert np.array_equal(fr[h0:h1, w0:w1], fr[coords[0]:coords[1], coords[2]:coords[3]]), coords
        assert 0 <= h0 <= h1 <= 40 and 0 <= w0 <= w1 <= 40


# ---- the rectangle ------------------------------------------------------------------------------------------------
def _pillow(frame, rect, width):
    from PIL import Image, ImageDraw
    im = Image.fromarray(frame)
    ImageDraw.Draw(im).rectangle([(rect[0], rect[1]), (rect[2], rect[3])], outline="yellow", width=width)
    return np.asarray(im)


@pytest.mark.parametrize("width", [1, 2, 3])
@pytest.mark.parametrize("fh,fw", [(5, 7), (64, 64), (57, 83)])
def test_rectangle_rule_is_pillows(width, fh, fw):
    rng = np.random.default_rng(fh + width)
    frame = rng.integers(0, 256, (fh, fw, 3), dtype=np.uint8)
    m = 2 * width                                        # x1 - x0 of the narrowest accepted box
    rects = [(0, 0, max(fw - 1, m), max(fh - 1, m)), (0, 0, max(fw, m), max(fh, m)),   # the frame; x1 == fw: on the edge
             (fw - 1 - m, fh - 1 - m, fw - 1, fh - 1), (0, 0, m, m),                # narrowest box, in two corners
             (fw - 3, fh - 3, fw + 29, fh + 29), (-5, -4, m - 2, m + 1), (-9, -9, fw + 9, fh + 9),   # past the edge
             (fw + 2, 1, fw + 2 + m, 1 + m)]                                         # wholly outside
    if fw > 3 * m and fh > 3 * m:
        rects += [(m, m - 1, 2 * m + 1, 2 * m + 3), (1, 2, fw - 3, fh - 2), (3, 1, 3 + m, fh - 1)]   # inside
    for rect in rects:
        K.rect_outline_check([rect], width)
        assert np.array_equal(R.draw_rect(frame, rect, width), _pillow(frame, rect, width)), rect


@pytest.mark.parametrize("width", [1, 2, 3])
def test_boxes_below_2w_plus_1_are_refused(width):
    m = 2 * width
    K.rect_outline_check([(4, 4, 4 + m, 4 + m)], width)                       # 2w + 1 pixels each way
    for rect in [(4, 4, 4 + m - 1, 40), (4, 4, 40, 4 + m - 1), (4, 4, 4, 4), (9, 9, 3, 3)]:
        with pytest.raises(ValueError):
            K.rect_outline_check([(0, 0, 31, 31), rect], width)
    with pytest.raises(ValueError):
        K.rect_outline_check([(0, 0, 31, 31)], 0)


def test_yellow_is_pillows():
    from PIL import ImageColor
    assert ImageColor.getrgb("yellow") == K.YELLOW == (255, 255, 0)


# ---- uint8 in, uint8 out --------------------------------------------------------------------------------------------
def test_to_tensor_to_pil_round_trip_is_the_identity_on_uint8():
    """ToTensor: ``.to(float32).div(255)``; ToPILImage: ``.mul(255).byte()``; make_grid fills with the fp32 40/255."""
    v = torch.arange(256, dtype=torch.uint8)
    assert torch.equal(v.to(torch.float32).div(255).mul(255).byte(), v)
    fill = torch.zeros(3).new_full((5,), 40 / 255.)
    assert fill.dtype == torch.float32 and (fill.mul(255).byte() == R.PAD).all()
    assert gallery.GRID_PAD_VALUE == R.PAD == 40 and gallery.PATCH_SIZE == R.PATCH
