"""The arithmetic of the prototype feature-map overlays (count_pipnet_amd.gallery.prototype_map_overlays,
csrc/overlay_ops.hip) against the statements the reference runs for ``*_overlay.png`` (util/vis_pipnet.py:454-475),
on the CPU:

* the prefilter and zoom of tests/overlay_ref.py against ``scipy.ndimage.zoom``;
* its mask, colour index and overlay against ``resized > 0.1`` and ``cmap(resized[y, x])`` of matplotlib's viridis,
  pixel by pixel, and on the values where the index rule can go wrong;
* the recorded colour table against matplotlib's;
* ``select_map_entries`` against the reference's statements (restated in tests/overlay_ref.py) and against lists
  written out by hand;
* what the public calls refuse before they need a device, and the entry point in the header and the library.

tests/test_gpu_overlay.py then holds the kernel against tests/overlay_ref.py, bit for bit.
"""
import os

import numpy as np
import pytest
import torch

import overlay_ref as R
from count_pipnet_amd import _lib, build
from count_pipnet_amd import kernels as K
from count_pipnet_amd.gallery import feature_map_overlays, prototype_map_overlays, select_map_entries
from gallery_ref import build_topk

GOLDEN_LUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "viridis_lut.npy")
SHAPES = [(3, 3, 8), (4, 4, 32), (5, 7, 33), (8, 8, 64), (13, 13, 64), (26, 26, 224), (28, 28, 224)]


def lut():
    return np.load(GOLDEN_LUT)[:, :3].copy()


def softmax_like(h, w, seed):
    """Sparse peaks as a softmax over prototypes leaves them: most of the map near 0, a few pixels up to 1, so the
    spline overshoots above 1 beside a peak and undershoots below 0 around it."""
    rng = np.random.default_rng(seed)
    m = (rng.random((h, w)) ** 12).astype(np.float32)
    for _ in range(max(1, h * w // 24)):
        m[rng.integers(h), rng.integers(w)] = np.float32(1.0) - np.float32(rng.random() * 0.05)
    r, c = rng.integers(h), rng.integers(w - 1)
    m[r, c], m[r, c + 1] = 1.0, 0.99                       # two neighbours at the top: the spline passes 1 between them
    return m


def maps_of(h, w):
    spike = np.zeros((h, w), np.float32)
    spike[h // 2, w - 1] = 1.0
    return [("softmax0", softmax_like(h, w, 11 * h + w)), ("softmax1", softmax_like(h, w, 1000 + 7 * h + w)),
            ("spike", spike), ("constant", np.full((h, w), 0.37, np.float32)), ("zero", np.zeros((h, w), np.float32))]


# ---- zoom -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,s", SHAPES)
def test_zoom_matches_scipy(h, w, s):
    """Every pixel within one float32 ulp of scipy's plus 2^-40 max|m| (about 200 float64 roundings on coefficients
    bounded by 9 max|m| stay under 2^-42 max|m|), and among the pixels of at least 2^-20 max|m| at most one in a
    thousand different at all: the restatement's doubles sit within a few 2^-52 of scipy's (its compiled filter
    rounds some steps differently), which moves a float32 only on a tie.  The thousandth is counted over the five
    maps of a shape together; seen here: 1 of 899 on the spike map at 5 x 7 -> 33, whose step of 6 / 32 makes
    short dyadic weights and so ties, 0 of 3,258 on that shape's other maps, 0 on every other shape."""
    ndimage = pytest.importorskip("scipy.ndimage")
    over = under = False
    differ = counted = 0
    for name, m in maps_of(h, w):
        ref = ndimage.zoom(m, (s / h, s / w))
        got = R.zoom(m, s)
        assert ref.dtype == np.float32 and got.dtype == np.float32 and ref.shape == got.shape == (s, s), name
        top = float(np.abs(m).max())
        ulp = np.spacing(np.abs(ref)).astype(np.float64)
        err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
        worst = float((err - ulp).max())
        print(f"{name} {h}x{w}->{s}: {int((got != ref).sum())} of {ref.size} differ, max |err| {float(err.max()):.3e}")
        assert (err <= ulp + 2.0 ** -40 * top).all(), (name, worst)
        big = np.abs(ref) >= 2.0 ** -20 * top
        if top > 0:
            differ, counted = differ + int((got[big] != ref[big]).sum()), counted + int(big.sum())
            print(f"    of at least 2^-20 max|m|: {int((got[big] != ref[big]).sum())} of {int(big.sum())} differ")
        else:
            assert not got.any() and not ref.any()
        over, under = over or bool((ref > 1).any()), under or bool((ref < 0).any())
    assert differ <= 1e-3 * counted, (differ, counted)
    assert over and under, "the maps never overshoot: values above 1 and below 0 are untested"


def test_prefilter_matches_scipy_spline_filter():
    ndimage = pytest.importorskip("scipy.ndimage")
    for h, w in [(3, 3), (5, 7), (26, 26)]:
        m = softmax_like(h, w, h * w)
        ref = ndimage.spline_filter(m.astype(np.float64), order=3, mode="mirror")
        got = R.prefilter(m)
        assert np.abs(got - ref).max() <= 2.0 ** -42 * 9 * float(np.abs(m).max())


# ---- mask, colour, overlay ----------------------------------------------------------------------------------------
def test_fixture_is_matplotlibs_table():
    matplotlib = pytest.importorskip("matplotlib")
    table = np.load(GOLDEN_LUT)
    assert table.shape == (256, 4) and table.dtype == np.float64
    assert np.array_equal(table, matplotlib.colormaps["viridis"](np.arange(256)))
    assert (table[:, 3] == 1.0).all()


def edge_values():
    tenth = np.float32(0.1)
    vals = [1.0, np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(1), np.float32(2)), tenth,
            np.nextafter(tenth, np.float32(0)), np.nextafter(tenth, np.float32(1)), 255 / 256,
            np.nextafter(np.float32(255 / 256), np.float32(0)), np.nextafter(np.float32(255 / 256), np.float32(1)),
            1.25, 2.0, 7.5, 255.0, 256.0, 1e9, 0.0, -0.0, -0.3, 0.0999, 0.5, 26 / 256,
            np.nextafter(np.float32(26 / 256), np.float32(0))]
    vals += [k / 256 for k in range(20, 40)] + list(np.linspace(0.09, 1.1, 301))
    return np.array(vals, dtype=np.float32)


def test_mask_colour_and_overlay_match_matplotlib_pixel_by_pixel():
    matplotlib = pytest.importorskip("matplotlib")
    cmap = matplotlib.colormaps["viridis"]
    table = lut()
    r = R.zoom(softmax_like(5, 7, 3), 33)
    for resized in (r, edge_values().reshape(1, -1)):
        # the reference's statements, vis_pipnet.py:464-475
        mask = resized > 0.1
        overlay = np.zeros((*resized.shape, 4))
        for y in range(resized.shape[0]):
            for x in range(resized.shape[1]):
                if mask[y, x]:
                    color = cmap(resized[y, x])
                    overlay[y, x] = (*color[:3], 0.7)
        assert mask.any() and not mask.all()
        assert np.array_equal(R.mask_of(resized), mask)
        got = R.overlay_of(resized, table)
        assert got.dtype == np.float64 and np.array_equal(got, overlay)
        colour = R.colour_of(resized)
        assert colour.dtype == np.uint8 and (colour[~mask] == 0).all()
        assert np.array_equal(table[colour[mask]], overlay[mask][:, :3])
    c = R.colour_of(edge_values())
    assert c[0] == 255 and c[1] == 255 and c[2] == 255 and c[3] == 0 and c[4] == 0 and c[5] == 25      # 1.0, 0.1
    assert c[6] == 255 and c[7] == 254 and c[9] == 255 and c[13] == 255 and c[14] == 255               # 255 / 256, > 1
    assert R.overlay_of(np.float32([0.5]), table, 0.25)[0, 3] == 0.25


# ---- selection ------------------------------------------------------------------------------------------------------
def descending(n, top=0.9, step=0.05, base=0):
    return [(top - step * j, base + j) for j in range(n)]


def test_pipnet_selection_takes_the_highest_the_middle_and_the_lowest_above_the_threshold():
    lists = {(0, 0): descending(1), (1, 0): descending(2), (2, 0): descending(3), (3, 0): descending(10),
             (4, 0): [(0.9, 1), (0.6, 2), (0.3, 3), (0.2, 4), (0.05, 5), (0.0, 6)],        # a tail below 0.1
             (5, 0): [(0.09, 1), (0.05, 2), (0.0, 3)],                                     # all below: unused
             (6, 0): descending(4), (7, 0): [],                                            # unselected; empty
             (8, 0): [(0.9, 1), (0.05, 2)], (9, 0): [(0.5, 1), (0.04, 2), (0.03, 3)],
             (10, 0): [(0.9, 1), (0.8, 2), (0.7, 3), (0.05, 4)]}
    selected = [True] * 11
    selected[6] = False
    res = build_topk(11, [None], 10, lists, selected=selected)
    assert res.unused.tolist() == [False] * 5 + [True, False, True] + [False] * 3
    want = [[(0, 0)], [(0, 0), (0, 1)], [(0, 0), (0, 1), (0, 2)], [(0, 0), (0, 5), (0, 9)], [(0, 0), (0, 3)], [], [],
            [], [(0, 0)], [(0, 0), (0, 1)], [(0, 0), (0, 2)]]
    got = select_map_entries(res)
    assert got == want
    ref = R.map_selection(res)
    assert got == [ref.get(p, []) for p in range(11)]
    for most in (1, 2, 5):
        ref = R.map_selection(res, most)
        assert select_map_entries(res, most) == [ref.get(p, []) for p in range(11)] == [e[:most] for e in want]


def test_count_selection_takes_slot_0_of_every_non_empty_group_in_ascending_count():
    lists = {(0, 0): descending(3), (0, 2): descending(2, base=10),                        # group 1 empty
             (1, 0): [(2.0, 4), (2.0, 5), (1.0, 6)], (1, 1): [(3.0, 7)], (1, 2): [(0.02, 8)],  # ties at slot 0
             (2, 1): [(1.0, 9)], (3, 0): descending(2)}
    res = build_topk(5, [1, 2, 3], 3, lists, selected=[True, True, True, False, True])
    want = [[(0, 0), (2, 0)], [(0, 0), (1, 0), (2, 0)], [(1, 0)], [], []]
    assert select_map_entries(res) == want
    ref = R.map_selection(res)
    assert want == [ref.get(p, []) for p in range(5)]
    assert select_map_entries(res, 2) == [e[:2] for e in want]
    ref = R.map_selection(res, 2)
    assert [e[:2] for e in want] == [ref.get(p, []) for p in range(5)]
    four = build_topk(1, [1, 2, 3, 4], 2, {(0, g): descending(1, base=g) for g in range(4)})
    assert select_map_entries(four) == [[(0, 0), (1, 0), (2, 0)]]


def test_selection_refuses_a_bad_limit():
    res = build_topk(1, [None], 2, {(0, 0): descending(2)})
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError):
            select_map_entries(res, bad)


# ---- refusals that need no device -----------------------------------------------------------------------------------
def test_public_calls_refuse_bad_operands_before_they_need_a_device():
    proto = torch.zeros(2, 5, 4, 6)                            # [B, P, h, w]
    table = torch.from_numpy(lut())
    ok = dict(size=16)
    for args, kwargs in [
        ((proto[0], [(0, 0)], table), ok),                                   # not four-dimensional
        ((proto.double(), [(0, 0)], table), ok),                             # dtype
        ((torch.zeros(2, 5, 2, 6), [(0, 0)], table), ok),                    # h = 2
        ((torch.zeros(2, 5, 4, 2), [(0, 0)], table), ok),                    # w = 2
        ((proto, [(0, 0)], table.float()), ok),                              # lut dtype
        ((proto, [(0, 0)], table[:255]), ok),                                # lut shape
        ((proto, [(0, 0)], table.numpy()), ok),                              # no tensor
        ((proto, [(2, 0)], table), ok), ((proto, [(0, 5)], table), ok), ((proto, [(-1, 0)], table), ok),
        ((proto, [(0, 0, 0)], table), ok), ((proto, [(0.5, 0)], table), ok), ((proto, [0, 1], table), ok),
        ((proto, [(0, 0)], table), dict(size=1)), ((proto, [(0, 0)], table), dict(size=16.0)),
        ((proto, [(0, 0)], table), dict(size=1 << 14)), ((proto, [(0, 0)], table), dict(size=True)),
        ((proto, [(0, 0)], table), dict(size=16, batch_size=0)),
        ((proto, [(0, 0)], table), dict(size=16, batch_size=2.0)),
        ((proto, [(0, 0)], table), dict(size=16, alpha=1.5)), ((proto, [(0, 0)], table), dict(size=16, alpha=None)),
        ((torch.zeros(1, 1, 90, 90), [(0, 0)], table), dict(size=224)),       # the map does not fit the LDS
    ]:
        with pytest.raises(ValueError):
            feature_map_overlays(*args, **kwargs)
    with pytest.raises(RuntimeError):
        feature_map_overlays(proto, [(0, 0)], table, size=16)                # everything right but the device
    with pytest.raises(RuntimeError):
        K.map_overlay(proto.permute(0, 2, 3, 1).contiguous(), [(0, 0)], table, 16)
    res = build_topk(2, [None], 2, {(0, 0): descending(2)})
    for kwargs in (dict(image_size=64, batch_size=0), dict(image_size=1), dict(image_size=64, max_per_prototype=0)):
        with pytest.raises(ValueError):
            prototype_map_overlays(None, None, res, table, **kwargs)
    with pytest.raises(ValueError):
        prototype_map_overlays(None, None, res, table.float(), image_size=64)


def test_the_size_rule_is_the_librarys():
    """ceil2(h * (w | 1)) * 8 + 6144 + 48 + 4 * S bytes within 64 KiB: one output row beside the map."""
    table = torch.from_numpy(lut())
    for h, w, s in [(26, 26, 224), (3, 3, 8), (26, 26, 1024), (85, 85, 224), (83, 83, 1024), (3, 2000, 224)]:
        assert K.overlay_shapes(torch.zeros(0, h, w, 1), table, s) == (0, h, w, 1, s)
    for h, w, s in [(86, 86, 224), (84, 84, 1024), (3, 2500, 224), (26, 26, 14000)]:
        with pytest.raises(ValueError, match="LDS"):
            K.overlay_shapes(torch.zeros(0, h, w, 1), table, s)


# ---- the entry point ----------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_refuses_bad_arguments_without_a_device():
    build.build()
    lib = _lib.load()
    assert hasattr(lib, "pipnet_map_overlay") and "pipnet_map_overlay" in _lib.SIGNATURES
    assert lib.pipnet_amd_abi_version() == 4 and _lib.ABI_VERSION == 4
    P, I32, F64 = _lib.P, _lib.I32, _lib.F64
    assert _lib.SIGNATURES["pipnet_map_overlay"] == [P, I32, I32, I32, I32, P, I32, P, I32, F64, P, P, P, P, P, P]
    p16 = 16

    def status(b=1, h=4, w=4, p=5, n=1, s=16, proto=p16, items=p16, table=p16, overlay=p16):
        return lib.pipnet_map_overlay(proto, b, h, w, p, items, n, table, s, 0.7, None, None, None, None, overlay, None)

    for kw in (dict(h=2), dict(w=2), dict(s=1), dict(p=0), dict(n=-1), dict(b=-1), dict(b=0), dict(proto=None),
               dict(items=None), dict(table=None), dict(overlay=8), dict(table=8), dict(h=90, w=90, s=224),
               dict(s=1 << 15), dict(n=1 << 24)):
        assert status(**kw) == 1, kw
    assert status(n=0) == 0 and status(n=0, proto=None, items=None, table=None, b=0) == 0       # nothing to launch
    assert status(n=0, h=2) == 1                                                                # still checked
