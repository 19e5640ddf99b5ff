"""Prototype feature-map overlays on the GPU (count_pipnet_amd.gallery, csrc/overlay_ops.hip): every output against
tests/overlay_ref.py, bit for bit -- the arithmetic is IEEE + - * / in one stated order (include/pipnet_amd.h), so
equality is the requirement, in float64 and float32 alike.

* pipnet_map_overlay through ``feature_map_overlays`` at every size where the kernel takes another path: the
  smallest map, a map that is not square, a picture whose side is no multiple of 4 (one element per lane) and one that
  is (16-byte stores), more bands than one (33, 64, 224 rows), P below and at a multiple of 4, one entry, the chunk
  edge of ``batch_size``, repeated pairs, an NCHW-contiguous input, no overlay, an empty mask, values above 1;
* the refusals that need the device;
* ``prototype_map_overlays`` end to end on an ImageFolder of PNG files and a small ConvNeXt PIP-Net.

tests/test_overlay_cpu.py holds tests/overlay_ref.py against scipy and matplotlib.
"""
import os

import numpy as np
import pytest
import torch

import overlay_ref as R
from count_pipnet_amd import kernels as K
from count_pipnet_amd.data import DecodedImageFolder, DeviceEvalLoader, DeviceEvalTransform
from count_pipnet_amd.gallery import feature_map_overlays, prototype_map_overlays, select_map_entries
from count_pipnet_amd.topk import prototype_topk
from golden_util import load_golden
from input_util import synth_photo
from model_util import build_model

pytestmark = pytest.mark.gpu

GOLDEN_LUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "viridis_lut.npy")
FIELDS = ("maps", "resized", "mask", "colour", "overlay")


@pytest.fixture(scope="module")
def table():
    return np.load(GOLDEN_LUT)[:, :3].copy()


def proto_maps(b, p, h, w, seed):
    """[b, p, h, w] float32: sparse peaks as a softmax leaves them (the spline passes 1 between two neighbours at the
    top and falls below 0 around a peak); prototype 1 of image 0 is all zero, prototype 2 of image 0 a constant
    (0.26: row 66 of the table, far from a step of the index)."""
    rng = np.random.default_rng(seed)
    m = (rng.random((b, p, h, w)) ** 10).astype(np.float32)
    for bi in range(b):
        for pi in range(p):
            r, c = rng.integers(h), rng.integers(w - 1)
            m[bi, pi, r, c], m[bi, pi, r, c + 1] = 1.0, 0.99
    m[0, 1] = 0.0
    m[0, 2] = 0.26
    return m


_RENDERED = {}


def expected(m, table, size, alpha=R.ALPHA):
    """overlay_ref's arrays for the [N, h, w] maps, every distinct map rendered once per module."""
    out = {f: [] for f in FIELDS}
    for one in m:
        key = (one.tobytes(), one.shape, size, alpha)
        if key not in _RENDERED:
            _RENDERED[key] = R.render(one, table, size, alpha)
        for f in FIELDS[1:]:
            out[f].append(_RENDERED[key][f])
        out["maps"].append(one)
    return {f: np.stack(v) for f, v in out.items()}


def assert_bits(got, want, fields=FIELDS):
    for f in fields:
        g = getattr(got, f).cpu().numpy()
        assert g.dtype == want[f].dtype and g.shape == want[f].shape, f
        assert np.array_equal(g, want[f]), (f, int((g != want[f]).sum()))


def pairs_for(n, b, p):
    """n pairs: the zero and the constant map first, then all over the tensor, every third one a repeat."""
    base = [(0, 1), (0, 2), (b - 1, p - 1), (0, 0)]
    rng = np.random.default_rng(n + 7 * p)
    more = [(int(rng.integers(b)), int(rng.integers(p))) for _ in range(n)]
    for i in range(2, len(more), 3):
        more[i] = more[i - 1]
    return (base + more)[:n]


@pytest.mark.parametrize("h,w,s", [(3, 3, 8), (5, 7, 33), (8, 8, 64), (13, 13, 64), (26, 26, 224)])
@pytest.mark.parametrize("p", [5, 16])
def test_kernel_matches_the_reference_bit_for_bit(gpu, table, h, w, s, p):
    b = 3
    m = proto_maps(b, p, h, w, 100 * h + w + p)
    lut = torch.from_numpy(table).to(gpu)
    nhwc = torch.from_numpy(m).to(gpu).contiguous(memory_format=torch.channels_last)      # a forward's own layout
    nchw = torch.from_numpy(m).to(gpu)                                                    # copied once
    assert nhwc.permute(0, 2, 3, 1).is_contiguous() and not nchw.permute(0, 2, 3, 1).is_contiguous()
    for n in (1, 3, 65) if s < 224 else (1, 3):             # the chunk edge at the small sizes
        pairs = pairs_for(n, b, p)
        want = expected(np.stack([m[bi, pi] for bi, pi in pairs]), table, s)
        got = feature_map_overlays(nhwc, pairs, lut, size=s, batch_size=64)
        assert all(getattr(got, f).is_cuda for f in FIELDS)
        assert_bits(got, want)
        if n == 65:
            assert want["mask"].any() and not want["mask"].all() and (want["resized"] > 1).any()
            assert (want["resized"] < 0).any() and len(set(pairs)) < n
            assert_bits(feature_map_overlays(nchw, np.array(pairs), lut, size=s, batch_size=7), want)
            bare = feature_map_overlays(nhwc, pairs, lut, size=s, want_overlay=False)
            assert bare.overlay is None
            assert_bits(bare, want, FIELDS[:4])
        if n == 3:
            assert not want["mask"][0].any() and not want["overlay"][0].any()               # the all-zero map
            assert want["mask"][1].all() and (want["colour"][1] == 66).all()                # the constant 0.26
            other = feature_map_overlays(nhwc, pairs, lut, size=s, alpha=0.5)
            assert_bits(other, expected(want["maps"], table, s, 0.5))


def test_kernel_matches_the_reference_at_c2_dimensions(gpu, table):
    """26 x 26 -> 224: seven bands of 32 rows, 16-byte stores, a 768-wide tensor read at stride 768."""
    m = np.zeros((2, 768, 26, 26), np.float32)
    picked = [(0, 0), (1, 767), (1, 5)]
    m[[bi for bi, _ in picked], [pi for _, pi in picked]] = proto_maps(1, 3, 26, 26, 26)[0]
    lut = torch.from_numpy(table).to(gpu)
    nhwc = torch.from_numpy(m).to(gpu).contiguous(memory_format=torch.channels_last)
    want = expected(np.stack([m[bi, pi] for bi, pi in picked]), table, 224)
    assert_bits(feature_map_overlays(nhwc, picked, lut, size=224), want)
    # the wrapper, with members left out and items already on the device
    items = torch.tensor(picked, dtype=torch.int32, device=gpu)
    proto = nhwc.permute(0, 2, 3, 1)
    only = K.map_overlay(proto, items, lut, 224, out=K.MapOverlay(torch.empty((3, 26, 26), device=gpu), None, None,
                                                                   None, None))
    assert only.resized is None and np.array_equal(only.maps.cpu().numpy(), want["maps"])
    colour = torch.full((3, 224, 224), 7, dtype=torch.uint8, device=gpu)
    K.map_overlay(proto, picked, lut, 224, out=K.MapOverlay(None, None, None, colour, None))
    assert np.array_equal(colour.cpu().numpy(), want["colour"])
    assert_bits(K.map_overlay(proto, items, lut, 224), want)
    empty = K.map_overlay(proto, [], lut, 224)
    assert tuple(empty.overlay.shape) == (0, 224, 224, 4) and tuple(empty.maps.shape) == (0, 26, 26)


def test_refusals_on_the_device(gpu, table):
    lut = torch.from_numpy(table).to(gpu)
    good = torch.zeros((2, 5, 4, 6), device=gpu)
    for args, kwargs in [((torch.zeros((2, 5, 2, 6), device=gpu), [(0, 0)], lut), dict(size=16)),      # h = 2
                         ((good, [(0, 0)], lut), dict(size=1)),                                        # S = 1
                         ((good, [(0, 0), (2, 0)], lut), dict(size=16)),                               # a pair out of range
                         ((good, [(0, 5)], lut), dict(size=16)),
                         ((good, [(0, 0)], lut.float()), dict(size=16))]:                              # lut dtype
        with pytest.raises(ValueError):
            feature_map_overlays(*args, **kwargs)
    for args in [(good.cpu(), [(0, 0)], lut), (good, [(0, 0)], lut.cpu())]:
        with pytest.raises(RuntimeError):
            feature_map_overlays(*args, size=16)
    proto = good.permute(0, 2, 3, 1).contiguous()
    for bad_out in (K.MapOverlay(None, torch.empty((1, 16, 16), device=gpu, dtype=torch.float64), None, None, None),
                    K.MapOverlay(None, None, torch.empty((2, 16, 16), device=gpu, dtype=torch.uint8), None, None),
                    K.MapOverlay(None, None, None, None, torch.empty((1, 16, 16, 4), dtype=torch.float64))):
        with pytest.raises(RuntimeError):
            K.map_overlay(proto, [(0, 0)], lut, 16, out=bad_out)
    with pytest.raises(RuntimeError):
        K.map_overlay(proto, [(0, 0), (0, 5)], lut, 16)
    with pytest.raises(RuntimeError):
        K.map_overlay(good.permute(0, 2, 3, 1), [(0, 0)], lut, 16)                  # not dense NHWC
    torch.cuda.synchronize()


# ---- end to end -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """18 lossless PNG files, 40..90 pixels a side, two in each of 9 classes."""
    from PIL import Image
    root = tmp_path_factory.mktemp("overlay_folder")
    rng = np.random.default_rng(21)
    for i in range(18):
        d = root / f"class_{i // 2}"
        os.makedirs(d, exist_ok=True)
        h, w = (int(v) for v in rng.integers(40, 91, 2))
        Image.fromarray(synth_photo(h, w, 300 + i, "smooth" if i % 3 else "noise")).save(d / f"img_{i:02d}.png")
    return DecodedImageFolder(str(root))


def test_prototype_map_overlays_end_to_end_on_a_small_pipnet(gpu, folder, table):
    """The pass, then the overlays of its result: the entries are the reference's selection, every map is the one the
    pass scored (its maximum is the stored score -- the pooled value, which the pass clamps to 0 below the presence
    threshold of 0.1 -- and its first maximum lies at the stored location) and every picture is overlay_ref's."""
    net = build_model(load_golden("pipnet_mid_addon")[0]).to(gpu)
    loader = DeviceEvalLoader(folder, DeviceEvalTransform(64), gpu, batch_size=5, shuffle=False)
    res = prototype_topk(net, loader, 3, image_size=64).cpu()
    lut = torch.from_numpy(table).to(gpu)
    shown = R.map_selection(res)
    want_entry = [(p, g, j) for p in sorted(shown) for g, j in shown[p]]
    assert len(want_entry) >= 2 and any(len(e) >= 2 for e in shown.values())
    assert select_map_entries(res) == [shown.get(p, []) for p in range(res.scores.shape[0])]
    first = prototype_map_overlays(net, folder, res, lut, image_size=64, batch_size=4, keep_frames=True)
    assert first.maps.is_cuda and first.overlay.is_cuda and first.frames.is_cuda
    got = first.cpu()
    n = len(want_entry)
    assert got.entry.tolist() == [list(e) for e in want_entry]
    assert got.rank.tolist() == [i + 1 for p in sorted(shown) for i in range(len(shown[p]))]
    assert got.of.tolist() == [len(shown[p]) for p in sorted(shown) for _ in shown[p]]
    maps = got.maps.numpy()
    assert maps.shape == (n, 8, 8) and maps.dtype == np.float32
    for i, (p, g, j) in enumerate(want_entry):
        assert got.index[i] == res.index[p, g, j] and got.score[i] == res.scores[p, g, j]
        assert torch.equal(got.coords[i], res.coords[p, g, j])
        assert (got.h_idx[i], got.w_idx[i]) == (res.h_idx[p, g, j], res.w_idx[p, g, j])
        top = maps[i].max()
        score = res.scores[p, g, j].numpy()
        assert score == (top if top >= np.float32(0.1) else np.float32(0)), (i, float(top), float(score))
        col_max = maps[i].max(axis=0)                          # the reference's two-step torch.max: first maxima
        w_idx = int(col_max.argmax())
        assert (int(maps[i][:, w_idx].argmax()), w_idx) == (int(got.h_idx[i]), int(got.w_idx[i]))
        acc = np.float64(0)
        for v in maps[i].reshape(-1):
            acc = acc + np.float64(v)
        assert got.map_sum[i].numpy() == acc
    assert (got.score > 0).any()
    want = expected(maps, table, 64)
    assert_bits(got, want, FIELDS[1:])
    assert got.frame_index.tolist() == sorted({int(res.index[p, g, j]) for p, g, j in want_entry})
    assert tuple(got.frames.shape) == (len(got.frame_index), 64, 64, 3) and got.frames.dtype == torch.uint8
    again = prototype_map_overlays(net, folder, res, lut, image_size=64, batch_size=64, want_overlay=False).cpu()
    assert again.overlay is None and again.frames is None
    for f in ("entry", "rank", "of", "index", "score", "coords", "h_idx", "w_idx", "maps", "map_sum", "resized", "mask",
              "colour", "frame_index"):
        assert torch.equal(getattr(again, f), getattr(got, f)), f
    one = prototype_map_overlays(net, folder, res, lut, image_size=64, max_per_prototype=1).cpu()
    keep = [i for i, r in enumerate(got.rank.tolist()) if r == 1]
    assert torch.equal(one.entry, got.entry[keep]) and torch.equal(one.overlay, got.overlay[keep])
    assert (one.of == 1).all()
