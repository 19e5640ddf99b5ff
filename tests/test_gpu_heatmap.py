"""Prototype similarity heatmaps on the GPU (count_pipnet_amd.gallery, csrc/heatmap_ops.hip): every byte against
tests/heatmap_ref.py, which tests/test_heatmap_cpu.py holds against torch, Pillow and matplotlib.

* pipnet_heatmap_rgb8 over the size list of the CPU test (both passes, one pass, none; 1 x 1 to 28 x 28 maps) at
  P = 1, 3, 16, 67 (the channel gather), items unsorted and repeated, ``out`` and ``resized`` inside sentinel
  padding, 4-byte aligned (four pixels per lane where S % 4 == 0) and off by one byte (one byte per lane);
* all 65,536 (table byte, frame byte) pairs (a contracted multiply-add or an approximate division shows here),
  0 / 255 maps that overshoot both clip8 bounds, the quantisation at the byte boundaries;
* ``explanation_heatmaps`` whatever the batch size, and end to end behind ``explain_predictions``, the net's own
  forward, ``DeviceEvalTransform`` and ``explanation_images``;
* the operand checks, which raise before anything is launched.
"""
import numpy as np
import pytest
import torch

import heatmap_ref as R
from count_pipnet_amd import _lib
from count_pipnet_amd import kernels as K
from count_pipnet_amd.data import DeviceEvalTransform, pack_images
from count_pipnet_amd.gallery import explanation_heatmaps, explanation_images, similarity_heatmaps
from count_pipnet_amd.local import LocalExplanation, explain_predictions
from golden_util import load_golden
from input_util import synth_photo
from model_util import build_model
from saliency_cases import same_bits
from test_gpu_saliency import Padded          # the sentinel-padded output views of the saliency tests (uint8: 0xA5)

pytestmark = pytest.mark.gpu

# the CPU list, a scale just below 1 (the widest window of map rows a band of output rows needs, several bands) and
# an S that is no multiple of 4 with more than one band
SIZES = R.SIZES + [(31, 30, 32), (9, 11, 33)]
WIDTHS = [1, 3, 16, 67]
SENTINEL = 0xA5


def _lut(gpu):
    return torch.from_numpy(R.jet_like_lut()).to(gpu)


def _want(maps, frames, items, lut, weights=R.WEIGHTS):
    """(out [N,S,S,3], resized [N,S,S]) of the reference; a repeated (b, p, frame) is computed once."""
    cache = {}
    for it in items:
        if it not in cache:
            cache[it] = R.heatmap(maps[it[0], :, :, it[1]], frames[it[2]], lut, weights)
    return np.stack([cache[it][0] for it in items]), np.stack([cache[it][1] for it in items])


def _run(gpu, maps, frames, items, lut, shift, weights=R.WEIGHTS):
    n, s = len(items), frames.shape[1]
    out, res = Padded((n, s, s, 3), torch.uint8, gpu, shift), Padded((n, s, s), torch.uint8, gpu, shift)
    got = K.heatmap_rgb8(torch.from_numpy(maps).to(gpu), torch.from_numpy(frames).to(gpu), items,
                         torch.from_numpy(lut).to(gpu), weights=weights, out=out.view, resized=res.view)
    assert got is out.view
    return out, res


# ---- kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", WIDTHS)
@pytest.mark.parametrize("h,w,s", SIZES)
def test_heatmap_kernel_matches_the_reference(gpu, h, w, s, p):
    rng = np.random.default_rng(1000 * p + 10 * h + w)
    maps = rng.random((3, h, w, p), dtype=np.float32)
    maps[0, 0, 0, :], maps[2, -1, -1, :] = 0.0, 1.0
    frames = rng.integers(0, 256, (2, s, s, 3), dtype=np.uint8)
    lut = R.jet_like_lut()
    items = [(2, p - 1, 1), (0, 0, 0), (1, p // 2, 1), (2, p - 1, 1), (0, p - 1, 0), (1, 0, 1), (2, 0, 0)]
    want_out, want_res = _want(maps, frames, items, lut)
    for shift in (0, 1):                   # 4-byte aligned: four pixels per lane where S % 4 == 0; else bytes
        out, res = _run(gpu, maps, frames, items, lut, shift)
        assert same_bits(res.view, want_res), (shift, "resized")
        assert same_bits(out.view, want_out), (shift, "out")
        assert out.untouched() and res.untouched(), shift
    # without the optional output, a fresh result, the items as an array: the same bytes
    got = K.heatmap_rgb8(torch.from_numpy(maps).to(gpu), torch.from_numpy(frames).to(gpu), np.asarray(items),
                         torch.from_numpy(lut).to(gpu))
    assert same_bits(got, want_out)


def test_every_table_byte_against_every_frame_byte(gpu):
    m, frames, lut = R.exhaustive_case()
    maps = m.reshape(1, 16, 16, 1)
    items = [(0, 0, e) for e in range(256)]
    r = np.arange(256, dtype=np.uint8).reshape(16, 16)
    want = np.stack([R.blend(r, frames[e], lut) for e in range(256)])
    exact = (2 * np.arange(256)[None, :] + 6 * np.arange(256)[:, None]) // 10          # floor(0.2 a + 0.6 c)
    assert (want[..., 0].reshape(256, 256) != exact).sum() > 0            # the float32 chain is not exact arithmetic
    for shift in (0, 1):
        out, res = _run(gpu, maps, frames, items, lut, shift)
        assert same_bits(res.view, np.broadcast_to(r, (256, 16, 16)).copy())
        assert same_bits(out.view, want), shift
        assert out.untouched() and res.untouched()
    # other weights take the same path: the two products are rounded one by one
    for weights in ((0.5, 0.5), (0.0, 1.0), (1.0, 0.0), (0.3, 0.45)):
        want_w = np.stack([R.blend(r, frames[e], lut, weights) for e in range(0, 256, 5)])
        got = K.heatmap_rgb8(torch.from_numpy(maps).to(gpu), torch.from_numpy(frames).to(gpu), items[::5],
                             torch.from_numpy(lut).to(gpu), weights=weights)
        assert same_bits(got, want_w), weights


@pytest.mark.parametrize("h,w,s", [(5, 7, 40), (13, 13, 104), (26, 26, 224), (9, 11, 33)])
def test_sparse_maps_overshoot_both_bounds(gpu, h, w, s):
    """Maps of exact 0 and 1 become 0 / 255 bytes: the bicubic lobes leave 0..255 in both passes, so the uint8
    intermediate and the result are clamped at both ends."""
    maps = np.stack([R.sparse_map(h, w, 50 + i).astype(np.float32) / np.float32(255) for i in range(3)], axis=-1)[None]
    assert set(np.unique(maps)) == {0.0, 1.0}
    frames = np.random.default_rng(s).integers(0, 256, (1, s, s, 3), dtype=np.uint8)
    lut = R.jet_like_lut()
    for i in range(3):
        seen = {}
        R.resize(R.quantise(maps[0, :, :, i]), s, seen=seen)
        assert all(lo < 0 and hi > 255 for lo, hi in seen.values()) and set(seen) == {"h", "v"}, seen
    items = [(0, 2, 0), (0, 0, 0), (0, 1, 0)]
    want_out, want_res = _want(maps, frames, items, lut)
    assert want_res.min() == 0 and want_res.max() == 255
    for shift in (0, 1):
        out, res = _run(gpu, maps, frames, items, lut, shift)
        assert same_bits(res.view, want_res) and same_bits(out.view, want_out), shift


def test_quantisation_at_the_byte_boundaries(gpu):
    """An 8 x 8 map at S = 8 (no resize): ``resized`` is the quantised map itself, against torch's mul(255).byte()."""
    vals = R.boundary_values()
    vals += [0.5] * (64 - len(vals))
    m = np.asarray(vals, np.float32).reshape(1, 8, 8, 1)
    want = torch.from_numpy(m).mul(255).byte().numpy().reshape(1, 8, 8)
    assert np.array_equal(R.quantise(m).reshape(1, 8, 8), want)
    frames = np.zeros((1, 8, 8, 3), np.uint8)
    for shift in (0, 1):
        _, res = _run(gpu, m, frames, [(0, 0, 0)], R.jet_like_lut(), shift)
        assert same_bits(res.view, want), shift
    # beyond the contract the kernel saturates instead of wrapping
    wild = np.asarray([-0.25, 1.5, 300.0, -1e30] + [0.25] * 60, np.float32).reshape(1, 8, 8, 1)
    _, res = _run(gpu, wild, frames, [(0, 0, 0)], R.jet_like_lut(), 0)
    assert res.view.reshape(-1)[:4].tolist() == [0, 255, 255, 0]


# ---- public calls -------------------------------------------------------------------------------------------------
def _result(count, proto_ids):
    b, c = count.shape
    m = proto_ids.shape[2]
    z = lambda *s: torch.zeros(*s, dtype=torch.int64)      # noqa: E731
    return LocalExplanation(classes=z(b, c), logits=torch.zeros(b, c), count=count, prototype=proto_ids,
                            similarity=torch.zeros(b, c, m), weight=torch.zeros(b, c, m),
                            simweight=torch.zeros(b, c, m), h_idx=z(b, c, m), w_idx=z(b, c, m),
                            coords=z(b, c, m, 4), rect=z(b, c, m, 4), proto_shape=(1, 6, 5, 7))


def test_explanation_heatmaps_do_not_depend_on_the_batch_size(gpu):
    rng = np.random.default_rng(8)
    b, p, h, w, s = 3, 6, 5, 7, 40
    maps = rng.random((b, h, w, p), dtype=np.float32)
    frames = rng.integers(0, 256, (b, s, s, 3), dtype=np.uint8)
    lut = R.jet_like_lut()
    count = torch.tensor([[3, 1], [0, 0], [5, 2]])                       # 5 kept, 3 stored: the list is truncated
    ids = torch.tensor([[[4, 0, 2], [4, -1, -1]], [[-1] * 3] * 2, [[5, 1, 3], [1, 5, -1]]])
    res = _result(count, ids)
    entry = [(0, 0, 0), (0, 0, 1), (0, 0, 2), (0, 1, 0), (2, 0, 0), (2, 0, 1), (2, 0, 2), (2, 1, 0), (2, 1, 1)]
    protos = [4, 0, 2, 4, 5, 1, 3, 1, 5]                                 # (0, 4) and (2, 1), (2, 5) occur twice
    want, _ = _want(maps, frames, [(e[0], q, e[0]) for e, q in zip(entry, protos)], lut)
    feats = torch.from_numpy(maps).to(gpu).permute(0, 3, 1, 2)           # [B, P, h, w], NHWC-backed as a forward's
    dev_frames, dev_lut = torch.from_numpy(frames).to(gpu), torch.from_numpy(lut).to(gpu)
    for bs in (1, 5, 64):
        got = explanation_heatmaps(feats, dev_frames, res, dev_lut, batch_size=bs)
        assert got.heatmaps.is_cuda and got.entry.tolist() == [list(e) for e in entry]
        assert got.prototype.tolist() == protos
        assert same_bits(got.heatmaps, want), bs
        host = got.cpu()
        assert not host.heatmaps.is_cuda and torch.equal(host.heatmaps, got.heatmaps.cpu())
    # an NCHW-contiguous map is copied to NHWC once: the same bytes; pairs with a frame of their own
    assert same_bits(explanation_heatmaps(feats.contiguous(), dev_frames, res, dev_lut).heatmaps, want)
    pairs = [(0, 4, 2), (2, 1, 0)]
    assert same_bits(similarity_heatmaps(feats, dev_frames, pairs, dev_lut), _want(maps, frames, pairs, lut)[0])
    res.count[:] = 0
    none = explanation_heatmaps(feats, dev_frames, res, dev_lut)
    assert tuple(none.heatmaps.shape) == (0, s, s, 3) and none.heatmaps.is_cuda
    assert tuple(none.entry.shape) == (0, 3) and tuple(none.prototype.shape) == (0,)
    assert tuple(similarity_heatmaps(feats, dev_frames, [], dev_lut).shape) == (0, s, s, 3)


@pytest.mark.parametrize("name", ["pipnet_mid_addon", "c1_count_identity"])
def test_heatmaps_end_to_end_behind_the_explanation_passes(gpu, name):
    """explain_predictions -> the net's forward -> the frames of the transform -> explanation_images and
    explanation_heatmaps: the entries align, and every heatmap is the reference applied to that forward's own map
    and that transform's own frame."""
    net = build_model(load_golden(name)[0]).to(gpu)
    photos = [synth_photo(40 + 7 * i, 90 - 5 * i, 700 + i, "smooth" if i % 2 else "noise") for i in range(5)]
    torch.manual_seed(5)
    xs, u8 = DeviceEvalTransform(64)(pack_images(photos), gpu, want_u8=True)
    res = explain_predictions(net, xs, 3, image_size=64, max_entries=4)
    with torch.no_grad():
        feats = net(xs, inference=True)[0]
    b, pn, h, w = feats.shape
    assert (h, w) == (8, 8) and b == 5 and feats.permute(0, 2, 3, 1).is_contiguous()
    lut = R.jet_like_lut()
    images = explanation_images(u8, res, image_size=64)
    heat = explanation_heatmaps(feats, u8, res, torch.from_numpy(lut).to(gpu), batch_size=3)
    n = int(res.count.clamp(max=4).sum())
    assert n >= 4 and tuple(heat.heatmaps.shape) == (n, 64, 64, 3)
    assert torch.equal(heat.entry, images.entry)
    host = res.cpu()
    assert heat.prototype.tolist() == [int(host.prototype[bi, r, j]) for bi, r, j in heat.entry.tolist()]
    maps, frames = feats.permute(0, 2, 3, 1).cpu().numpy(), u8.cpu().numpy()
    assert 0.0 <= maps.min() and maps.max() <= 1.0 + 2.0 ** -22
    want, _ = _want(maps, frames, [(e[0], q, e[0]) for e, q in zip(heat.entry.tolist(), heat.prototype.tolist())], lut)
    assert same_bits(heat.heatmaps, want)
    assert all(len(np.unique(x)) > 16 for x in want)                      # pictures, not constants


# ---- operand checks -----------------------------------------------------------------------------------------------
def test_operand_checks_raise_before_any_launch(gpu):
    maps = torch.rand(2, 8, 8, 4, device=gpu)
    frames = torch.zeros(2, 16, 16, 3, dtype=torch.uint8, device=gpu)
    lut = _lut(gpu)
    items = [(0, 1, 0), (1, 3, 1)]
    out = torch.full((2, 16, 16, 3), SENTINEL, dtype=torch.uint8, device=gpu)
    bad = [
        dict(maps=maps.cpu()), dict(frames=frames.cpu()), dict(lut=lut.cpu()),                      # CPU tensors
        dict(maps=maps.double()), dict(maps=maps.half()), dict(frames=frames.float()), dict(lut=lut.int()),
        dict(frames=frames.transpose(1, 2)), dict(maps=maps.permute(0, 2, 1, 3)), dict(maps=maps[..., ::2]),
        dict(lut=lut[:255]), dict(lut=torch.zeros(256, 4, dtype=torch.uint8, device=gpu)[:, :3]),
        dict(maps=torch.rand(2, 17, 8, 4, device=gpu)), dict(maps=torch.rand(2, 8, 17, 4, device=gpu)),      # h, w > S
        dict(frames=frames[:, :, :8]), dict(frames=frames[..., :2]),
        dict(items=[(2, 0, 0)]), dict(items=[(0, 4, 0)]), dict(items=[(0, 0, 2)]), dict(items=[(0, -1, 0)]),
        dict(items=[(0.5, 0, 0)]), dict(items=[(0, 0, 1 << 31)]),
        dict(out=out[:1]), dict(out=out.cpu()), dict(out=out.float()), dict(out=out.transpose(1, 2)),
        dict(resized=torch.zeros(2, 16, 16, 3, dtype=torch.uint8, device=gpu)),
        dict(weights=(0.7, 0.6)), dict(weights=(0.2, -0.6)),
    ]
    for kw in bad:
        args = dict(maps=maps, frames=frames, items=items, lut=lut, out=out, resized=None, weights=R.WEIGHTS)
        args.update(kw)
        with pytest.raises((ValueError, RuntimeError)):
            K.heatmap_rgb8(args["maps"], args["frames"], args["items"], args["lut"], weights=args["weights"],
                           out=args["out"], resized=args["resized"])
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()                                           # nothing was launched
    # the entry point itself: PIPNET_ERR_ARG for a map larger than the frame, whatever the caller checked
    lib = _lib.load()
    rows = K.bicubic_rows(8, 16).to(gpu)
    it = torch.tensor(items, dtype=torch.int32, device=gpu)
    stream = torch.cuda.current_stream(gpu).cuda_stream

    def call(h, w, n=2, resized=None):
        return lib.pipnet_heatmap_rgb8(maps.data_ptr(), 2, h, w, 4, frames.data_ptr(), 2, 16, it.data_ptr(), n,
                                       lut.data_ptr(), rows.data_ptr(), rows.data_ptr(), 0.2, 0.6, out.data_ptr(),
                                       resized, stream)

    assert call(17, 8) == _lib.CONSTANTS["ERR_ARG"] and call(8, 17) == _lib.CONSTANTS["ERR_ARG"]
    assert call(8, 8, n=-1) == _lib.CONSTANTS["ERR_ARG"] and call(8, 8, n=0) == 0
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    assert call(8, 8, resized=None) == 0                                     # a NULL ``resized`` is accepted
    torch.cuda.synchronize()
    want, _ = _want(maps.cpu().numpy(), frames.cpu().numpy(), items, R.jet_like_lut())
    assert same_bits(out, want)
    # a table already on the device is not read on the host: the kernel passes over its rows out of range
    table = torch.tensor([(1, 3, 1), (2, 0, 0), (0, 4, 0), (0, 0, -1), (0, 1, 0)], dtype=torch.int32, device=gpu)
    out5 = torch.full((5, 16, 16, 3), SENTINEL, dtype=torch.uint8, device=gpu)
    res5 = torch.full((5, 16, 16), SENTINEL, dtype=torch.uint8, device=gpu)
    assert K.heatmap_rgb8(maps, frames, table, lut, out=out5, resized=res5) is out5
    assert same_bits(out5[[4, 0]], want) and (out5[1:4] == SENTINEL).all() and (res5[1:4] == SENTINEL).all()
    for bad_table in (table.long(), table[:, :2], table.repeat(1, 2)[:, ::2]):
        with pytest.raises(RuntimeError):
            K.heatmap_rgb8(maps, frames, bad_table, lut)
