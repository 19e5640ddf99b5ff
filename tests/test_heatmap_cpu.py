"""The arithmetic of the similarity heatmaps (count_pipnet_amd.gallery.explanation_heatmaps, csrc/heatmap_ops.hip)
against the statements the reference runs for heatmap_p{p}.png (util/visualize_prediction.py:92-100), on the CPU:

* ``kernels.bicubic_rows`` and the resize of tests/heatmap_ref.py against Pillow's ``resize(BICUBIC)``, bit for bit;
* the quantise, table, blend and byte steps of tests/heatmap_ref.py against torch, numpy and a ``plt.imsave`` PNG
  read back with Pillow, over all 65,536 (table byte, frame byte) pairs;
* what the public calls refuse before they need a device, and the entry point in the header and the library.

tests/test_gpu_heatmap.py then holds the kernel against tests/heatmap_ref.py.
"""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import heatmap_ref as R
from count_pipnet_amd import _lib, build
from count_pipnet_amd import kernels as K
from count_pipnet_amd.gallery import explanation_heatmaps, similarity_heatmaps
from count_pipnet_amd.local import LocalExplanation

SIZES = R.SIZES


def pillow_resize(q, s):
    return np.asarray(Image.fromarray(q, "L").resize((s, s), Image.BICUBIC))


# ---- resize -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,s", SIZES)
def test_bicubic_rows_and_the_reference_resize_match_pillow(h, w, s):
    rows_h, rows_v = R.table_rows(K.bicubic_rows(w, s)), R.table_rows(K.bicubic_rows(h, s))
    assert rows_h == [(x, list(k)) for x, k in R.coeff_rows(w, s)]         # the two restatements agree
    for seed in range(3):
        q = np.random.default_rng(100 * seed + h + w).integers(0, 256, (h, w), dtype=np.uint8)
        want = pillow_resize(q, s)
        assert np.array_equal(R.resize(q, s), want)
        assert np.array_equal(R.resize(q, s, rows_h, rows_v), want)


@pytest.mark.parametrize("h,w,s", SIZES)
def test_resize_of_sparse_maps_overshoots_and_matches_pillow(h, w, s):
    hit = {}
    for seed in range(4):
        q = R.sparse_map(h, w, 7 * seed + h * w)
        seen = {}
        got = R.resize(q, s, R.table_rows(K.bicubic_rows(w, s)), R.table_rows(K.bicubic_rows(h, s)), seen=seen)
        assert np.array_equal(got, pillow_resize(q, s))
        for axis, (lo, hi) in seen.items():
            hit[axis] = (min(lo, hit.get(axis, (0, 0))[0]), max(hi, hit.get(axis, (0, 0))[1]))
    assert set(hit) == {a for a, n in (("h", w), ("v", h)) if n != s}      # the skipped passes did not run
    for axis, n in (("h", w), ("v", h)):
        if n != s and n >= 5:             # a full row of taps: both clip8 bounds, the intermediate clamp included
            assert hit[axis][0] < 0 and hit[axis][1] > 255, (axis, hit[axis])


def test_bicubic_rows_shape_taps_and_refusals():
    t = K.bicubic_rows(26, 224)
    assert t.dtype == torch.int32 and tuple(t.shape) == (224, 7) and not t.is_cuda
    assert int(t[:, 1].max()) == 4 and int(t[:, 1].min()) == 2               # support 2 either side; cut at the edges
    n = t[:, 1].tolist()
    assert all(int(t[i, 2:2 + n[i]].sum()) in range((1 << 22) - 3, (1 << 22) + 4) for i in range(224))
    assert all((t[i, 2 + n[i]:] == 0).all() for i in range(224))
    assert K.bicubic_rows(16, 16)[:, 1].max() <= 5                            # the table of a skipped pass fits too
    for bad in ((17, 16), (0, 16), (300, 224)):
        with pytest.raises(ValueError):
            K.bicubic_rows(*bad)


# ---- quantise, table, blend, byte ---------------------------------------------------------------------------------
def test_quantise_at_the_byte_boundaries_matches_torch():
    m = np.asarray(R.boundary_values(), np.float32)
    want = torch.from_numpy(m).mul(255).byte().numpy()
    assert np.array_equal(R.quantise(m), want)
    assert want[0] == 0 and want[1] == 255 and want[3] == 255 and len(set(want.tolist())) >= 12


def library_heatmap(sim_map: torch.Tensor, frame_u8: np.ndarray, lut: np.ndarray, s: int) -> np.ndarray:
    """The picture the libraries themselves produce for one similarity map over one frame, as RGBA read back from
    the PNG: torch for the two conversions torchvision makes (a float map to an 8-bit "L" image is
    ``mul(255).byte()``, an 8-bit image to a float tensor is ``float().div(255)``), Pillow for the bicubic resize,
    numpy for the index, the lookup in the RGB table (in place of OpenCV's colour map and its BGR flip) and the
    blend -- a Python float times a float32 array, each product and the sum rounded to float32 -- and matplotlib's
    ``imsave`` with the range 0..1 for the bytes."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    as_bytes = sim_map.mul(255).byte().numpy()
    enlarged = Image.fromarray(as_bytes, "L").resize((s, s), Image.BICUBIC)
    unit = torch.from_numpy(np.array(enlarged)).float().div(255).numpy()
    index = (255 * unit).astype(np.uint8)
    colour = lut[index].astype(np.float32) / 255
    picture = torch.from_numpy(frame_u8).float().div(255).numpy()
    assert colour.dtype == picture.dtype == np.float32
    blended = 0.2 * colour + 0.6 * picture
    png = io.BytesIO()
    plt.imsave(png, blended, vmin=0.0, vmax=1.0, format="png")
    png.seek(0)
    return np.asarray(Image.open(png))


def test_blend_and_byte_steps_match_imsave_on_every_byte_pair():
    maps, frames, lut = R.exhaustive_case()
    differs_from_exact = 0
    for e in range(256):
        want = library_heatmap(torch.from_numpy(maps), frames[e], lut, 16)
        assert want.shape == (16, 16, 4) and want.dtype == np.uint8 and (want[..., 3] == 255).all()
        got, r = R.heatmap(maps, frames[e], lut)
        assert np.array_equal(r.reshape(-1), np.arange(256))
        assert np.array_equal(got, want[..., :3]), e
        differs_from_exact += int((got[..., 0].reshape(-1).astype(np.int64) != (2 * np.arange(256) + 6 * e) // 10).sum())
    assert differs_from_exact > 0        # float32 rounding is visible: exact arithmetic would not pass


def test_library_chain_with_a_resize_and_a_colour_table():
    rng = np.random.default_rng(3)
    lut = R.jet_like_lut()
    assert lut.shape == (256, 3) and len(np.unique(lut, axis=0)) > 200 and (lut[:, 0] != lut[:, 2]).any()
    for h, w, s in [(5, 7, 40), (8, 8, 64), (2, 3, 17)]:
        m = rng.random((h, w), dtype=np.float32)
        frame = rng.integers(0, 256, (s, s, 3), dtype=np.uint8)
        want = library_heatmap(torch.from_numpy(m), frame, lut, s)
        got, _ = R.heatmap(m, frame, lut)
        assert np.array_equal(got, want[..., :3]) and (want[..., 3] == 255).all()


# ---- what needs no device -----------------------------------------------------------------------------------------
def _operands(b=2, p=4, h=8, w=8, f=2, s=16):
    proto = torch.rand(b, h, w, p).permute(0, 3, 1, 2)                       # [B, P, h, w], NHWC-backed
    frames = torch.zeros(f, s, s, 3, dtype=torch.uint8)
    return proto, frames, torch.from_numpy(R.jet_like_lut())


def test_similarity_heatmaps_refuses_bad_arguments_without_a_device():
    proto, frames, lut = _operands()
    pairs = [(0, 1), (1, 3)]
    bad = [
        dict(lut=lut[:255]), dict(lut=lut.float()), dict(lut=torch.zeros(256, 4, dtype=torch.uint8)),
        dict(proto=_operands(h=17)[0]), dict(proto=_operands(w=32)[0]), dict(proto=proto.double()), dict(proto=proto[0]),
        dict(pairs=[(2, 0)]), dict(pairs=[(0, 4)]), dict(pairs=[(-1, 0)]), dict(pairs=[(0, 0, 2)]),
        dict(pairs=[(0.5, 0)]), dict(pairs=[(0, 1, 0, 0)]),
        dict(batch_size=0), dict(batch_size=-3),
        dict(frames=frames.float()), dict(frames=frames[..., :2]), dict(frames=frames[:, :, :8]), dict(frames=frames[0]),
        dict(weights=(0.5, 0.6)), dict(weights=(-0.1, 0.6)), dict(weights=(0.2,)),
    ]
    for kw in bad:
        args = dict(proto=proto, frames=frames, pairs=pairs, lut=lut)
        extra = {k: kw[k] for k in ("batch_size", "weights") if k in kw}
        args.update({k: v for k, v in kw.items() if k not in extra})
        with pytest.raises(ValueError):
            similarity_heatmaps(args["proto"], args["frames"], args["pairs"], args["lut"], **extra)
    with pytest.raises(RuntimeError, match="ROCm"):                          # all in order, but on the host
        similarity_heatmaps(proto, frames, pairs, lut)
    with pytest.raises(RuntimeError):
        K.heatmap_rgb8(proto.permute(0, 2, 3, 1), frames, [(0, 1, 0)], lut)
    with pytest.raises(ValueError):
        K.heatmap_rgb8(proto.permute(0, 2, 3, 1), frames, [(0, 1, 0)], lut[:255])


def _result(b, count, proto_ids):
    c, m = count.shape[1], proto_ids.shape[2]
    z = lambda *s: torch.zeros(*s, dtype=torch.int64)      # noqa: E731
    return LocalExplanation(classes=z(b, c), logits=torch.zeros(b, c), count=count, prototype=proto_ids,
                            similarity=torch.zeros(b, c, m), weight=torch.zeros(b, c, m),
                            simweight=torch.zeros(b, c, m), h_idx=z(b, c, m), w_idx=z(b, c, m),
                            coords=z(b, c, m, 4), rect=z(b, c, m, 4), proto_shape=(1, 4, 8, 8))


def test_explanation_heatmaps_refuses_bad_arguments_without_a_device():
    proto, frames, lut = _operands()
    res = _result(2, torch.tensor([[2, 0], [1, 5]]), torch.tensor([[[1, 3], [-1, -1]], [[0, -1], [2, 2]]]))
    with pytest.raises(ValueError):
        explanation_heatmaps(proto, frames, res, lut, batch_size=0)
    with pytest.raises(ValueError):
        explanation_heatmaps(proto, frames[:1], res, lut)                      # one frame per image of the result
    with pytest.raises(ValueError):
        explanation_heatmaps(proto[:1], frames, res, lut)
    with pytest.raises(ValueError):
        explanation_heatmaps(proto, frames, res, lut[:255])
    with pytest.raises(ValueError):
        explanation_heatmaps(proto[:, :2], frames, res, lut)                   # prototype 3 of a 2-prototype map
    with pytest.raises(RuntimeError, match="ROCm"):
        explanation_heatmaps(proto, frames, res, lut)


# ---- C ABI --------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_point():
    P, I32, F32 = _lib.P, _lib.I32, _lib.F32
    assert _lib.SIGNATURES["pipnet_heatmap_rgb8"] == [P, I32, I32, I32, I32, P, I32, I32, P, I32, P, P, P, F32, F32, P,
                                                      P, P]
    build.build()
    lib = _lib.load()
    assert hasattr(lib, "pipnet_heatmap_rgb8") and lib.pipnet_amd_abi_version() == 4
    # refused or passed over before any HIP call: a map larger than the frame, an LDS budget beyond 64 KiB, no items
    p = _lib.P(16)
    call = lambda h, w, s, n: lib.pipnet_heatmap_rgb8(p, 1, h, w, 4, p, 1, s, p, n, p, p, p, 0.2, 0.6, p, None, None)   # noqa: E731
    assert call(17, 8, 16, 1) == 1 and call(8, 17, 16, 1) == 1 and call(0, 8, 16, 1) == 1
    assert call(8, 8, 4096, 1) == 1 and call(8, 8, 4096, 0) == 1
    assert call(8, 8, 16, 0) == 0 and call(8, 8, 16, -1) == 1
    assert call(8, 8, 16, 1 << 24) == 1                                      # 2^24 workgroups: no grid holds them
    assert lib.pipnet_heatmap_rgb8(None, 1, 8, 8, 4, p, 1, 16, p, 1, p, p, p, 0.2, 0.6, p, None, None) == 1
