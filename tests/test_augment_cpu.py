"""The training augmentation off the GPU: (1) tests/augment_ref.py -- the numpy restatement the
GPU tests compare the kernels with -- against live Pillow, bit for bit, over every operation's
parameter range; (2) the host-side parameter sampler (count_pipnet_amd/augment.py): ranges,
operation spaces, frequencies, determinism and independence of the batch split."""
import math

import numpy as np
import pytest
import torch

import augment_ref as R
from count_pipnet_amd import augment as A
from input_util import synth_photo


@pytest.fixture(scope="module")
def pil():
    return pytest.importorskip("PIL.Image")


def _img(pil, a):
    return pil.fromarray(np.ascontiguousarray(a), "RGB")


def _np(im):
    return np.asarray(im.convert("RGB"), dtype=np.uint8)


PHOTO = synth_photo(56, 56, 21, "smooth")
NOISE = synth_photo(41, 56, 22, "noise")
BINS = list(range(A.NUM_BINS))


def _pil_affine(pil, a, m, fill):
    return _np(_img(pil, a).transform((a.shape[1], a.shape[0]), pil.Transform.AFFINE, m, pil.Resampling.NEAREST,
                                      fillcolor=(fill,) * 3))


# ---- (1) restatement vs Pillow ------------------------------------------------------------------

@pytest.mark.parametrize("op", ["ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate"])
def test_trivial_geometric_ops_all_magnitudes(pil, op):
    """All 31 magnitudes, both signs: shear and rotation take Pillow's fixed-point loop,
    translation its double loop."""
    for img in (PHOTO, NOISE[:41, :41]):
        size = img.shape[0]
        for k in BINS:
            for sign in (1.0, -1.0):
                mag = sign * A.GEOMETRIC_SPACE[op][0][k]
                m = A.geometric_matrix(op, mag, size)
                if op == "Rotate":
                    want = _np(_img(pil, img).rotate(mag, pil.Resampling.NEAREST, fillcolor=(0, 0, 0)))
                    assert (m is None) == (mag % 360 == 0)
                    assert m == R.rotate_matrix(mag, size, size)
                else:
                    want = _pil_affine(pil, img, m, 0)
                    assert R.warp_path(m) == (R.WARP_FIXED if op.startswith("Shear") and k else R.WARP_DOUBLE)
                row = A.warp_row(m, 0)
                got = R.affine_nearest(img, row[1:7], 0, path=int(row[0]))
                np.testing.assert_array_equal(got, want, err_msg=f"{op} {mag}")


def test_rotation_fill_255_and_non_square(pil):
    for angle in (10.0, -10.0, 3.7, -0.01, 359.0, 45.0):
        for img in (PHOTO, NOISE):
            h, w = img.shape[:2]
            want = _np(_img(pil, img).rotate(angle, pil.Resampling.NEAREST, fillcolor=(255,) * 3))
            got = R.affine_nearest(img, R.rotate_matrix(angle, w, h), 255)
            np.testing.assert_array_equal(got, want, err_msg=str(angle))


def test_random_affine_and_scale_only_matrices(pil):
    rng = np.random.default_rng(5)
    for _ in range(100):                    # RandomAffine(10, (.1, .1), (.9, 1.1)): fixed-point loop
        size = 56
        tx, ty = (int(round(v)) for v in rng.uniform(-5.6, 5.6, 2))
        m = A.affine_inverse_matrix([size / 2, size / 2], rng.uniform(-10, 10), [tx, ty], rng.uniform(0.9, 1.1),
                                    [0.0, 0.0])
        assert R.warp_path(m) == R.WARP_FIXED
        np.testing.assert_array_equal(R.affine_nearest(PHOTO, m, 255), _pil_affine(pil, PHOTO, m, 255))
    for _ in range(200):                    # scale / translate only: the double loop
        m = [rng.uniform(0.5, 2.0), 0.0, rng.uniform(-20, 20), 0.0, rng.uniform(0.5, 2.0), rng.uniform(-20, 20)]
        assert R.warp_path(m) == R.WARP_DOUBLE
        np.testing.assert_array_equal(R.affine_nearest(NOISE, m, 7), _pil_affine(pil, NOISE, m, 7), err_msg=str(m))
    ident = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    np.testing.assert_array_equal(R.affine_nearest(NOISE, ident, 0), NOISE)


@pytest.mark.parametrize("op", ["Brightness", "Color", "Contrast", "Sharpness"])
def test_enhance_ops_all_magnitudes(pil, op):
    """ImageEnhance.<op>(img).enhance(1 + mag) over both spaces' 31 magnitudes, both signs (so
    factors on both sides of the [0, 1] blend branch), and factor exactly 1."""
    from PIL import ImageEnhance
    mags = sorted({s * m for sp in (A.COLOUR_SPACE, A.COLOUR_SPACE_WITH_COLOR) for m in sp[op][0] for s in (1, -1)})
    code = A.OP_CODES[op]
    for img in (PHOTO, NOISE):
        enh = getattr(ImageEnhance, op)(_img(pil, img))
        for mag in mags + [0.0, 1.5, -1.0]:
            f = A.colour_param(op, mag)
            np.testing.assert_array_equal(R.colour_op(img, code, f), _np(enh.enhance(f)), err_msg=f"{op} {f}")
        np.testing.assert_array_equal(R.colour_op(img, code, 1.0), img)


def test_posterize_solarize(pil):
    from PIL import ImageOps
    assert sorted(set(A._POSTERIZE_BITS)) == [2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]
    for bits in range(2, 9):
        np.testing.assert_array_equal(R.posterize(NOISE, bits), _np(ImageOps.posterize(_img(pil, NOISE), bits)))
    for thr in [0.0, 255.0] + A.COLOUR_SPACE_WITH_COLOR["Solarize"][0]:
        np.testing.assert_array_equal(R.solarize(NOISE, thr), _np(ImageOps.solarize(_img(pil, NOISE), thr)),
                                      err_msg=str(thr))


def test_autocontrast_equalize_edges(pil):
    from PIL import ImageOps
    const_chan = PHOTO.copy()
    const_chan[..., 1] = 93                                   # a constant channel passes through
    narrow = (PHOTO // 4 + 60).astype(np.uint8)
    const = np.full((20, 20, 3), 17, np.uint8)                # a constant image
    small = NOISE[:12, :12]                                   # 144 pixels: Equalize's step is 0
    two = const.copy()
    two[:10] = 200
    for img in (PHOTO, NOISE, const_chan, narrow, const, small, two):
        np.testing.assert_array_equal(R.autocontrast(img), _np(ImageOps.autocontrast(_img(pil, img))))
        np.testing.assert_array_equal(R.equalize(img), _np(ImageOps.equalize(_img(pil, img))))
    np.testing.assert_array_equal(R.equalize(small), small)
    np.testing.assert_array_equal(R.autocontrast(const_chan)[..., 1], const_chan[..., 1])


def test_crop_then_resize_boxes(pil):
    """crop(box).resize: boxes at every edge, non-square, and the whole image -- and it is not
    Pillow's resize(box=...), which reads outside the box."""
    S1, S2 = 56, 29
    boxes = [(0, 0, 50, 50), (6, 6, 50, 50), (0, 6, 50, 44), (6, 0, 44, 50), (3, 2, 53, 41), (0, 0, 56, 56),
             (10, 12, 29, 29), (5, 5, 29, 40), (4, 4, 40, 29)]
    differs = 0
    for top, left, ch, cw in boxes:
        box = (left, top, left + cw, top + ch)
        want = _np(_img(pil, PHOTO).crop(box).resize((S2, S2), pil.Resampling.BILINEAR))
        np.testing.assert_array_equal(R.crop_resize(PHOTO, top, left, ch, cw, S2), want, err_msg=str(box))
        differs += int((_np(_img(pil, PHOTO).resize((S2, S2), pil.Resampling.BILINEAR, box=box)) != want).any())
    assert differs > 0
    np.testing.assert_array_equal(R.crop_resize(PHOTO[:29, :29], 0, 0, 29, 29, S2), PHOTO[:29, :29])


def test_hflip_grayscale_and_final_conversion(pil):
    np.testing.assert_array_equal(R.hflip(NOISE), _np(_img(pil, NOISE).transpose(pil.Transpose.FLIP_LEFT_RIGHT)))
    np.testing.assert_array_equal(R.luma(NOISE).astype(np.uint8), np.asarray(_img(pil, NOISE).convert("L")))
    from oracle import input_ref
    vp = [0, 0, 0, 0, 3, 5, 0, 0]
    got = R.view(NOISE[:40, :40], vp, 32, False, input_ref.IMAGENET_MEAN, input_ref.IMAGENET_STD)
    assert torch.equal(torch.from_numpy(got), input_ref.to_tensor_normalize(NOISE[3:35, 5:37]))


def test_composed_pipeline_vs_pillow_chain(pil):
    """transform1 + transform2 as the Pillow calls the reference makes, against R.pipeline."""
    from PIL import ImageEnhance, ImageOps
    from oracle import input_ref
    src = synth_photo(90, 50, 31, "smooth")
    S1, S2, s = 64, 40, 32
    m = A.geometric_matrix("ShearX", -0.3, S1)
    gp = A.warp_row(m, 0) + [1.0, 2.0, 3.0, 60.0, 57.0]
    vps = [[[R.OP_BRIGHTNESS, 1.07, R.OP_CONTRAST, 0.93, 1, 7, 0, 0]], [[R.OP_EQUALIZE, 0, 0, 0, 8, 0, 0, 0]]]
    u8, out = R.pipeline([src], [gp], vps, S1, S2, s)
    im = _img(pil, src).resize((S1, S1), pil.Resampling.BILINEAR)
    im = im.transform((S1, S1), pil.Transform.AFFINE, m, pil.Resampling.NEAREST, fillcolor=(0, 0, 0))
    im = im.transpose(pil.Transpose.FLIP_LEFT_RIGHT)
    im = im.crop((3, 2, 3 + 57, 2 + 60)).resize((S2, S2), pil.Resampling.BILINEAR)
    np.testing.assert_array_equal(u8[0], _np(im))
    v0 = ImageEnhance.Contrast(ImageEnhance.Brightness(im).enhance(1.07)).enhance(0.93).crop((7, 1, 39, 33))
    v1 = ImageOps.equalize(im).crop((0, 8, 32, 40))
    for k, v in enumerate((v0, v1)):
        assert torch.equal(torch.from_numpy(out[k, 0]), input_ref.to_tensor_normalize(_np(v)))


# ---- (2) the sampler ----------------------------------------------------------------------------

def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_operation_spaces_match_the_reference():
    """util/data.py:620-657, entry by entry."""
    lin = lambda a, b: [float(v) for v in torch.linspace(a, b, 31)]
    post = [float(v) for v in (8 - (torch.arange(31) / 5).round().int())]
    assert A.GEOMETRIC_SPACE == {"Identity": (None, False), "ShearX": (lin(0, 0.5), True),
                                 "ShearY": (lin(0, 0.5), True), "TranslateX": (lin(0, 16), True),
                                 "TranslateY": (lin(0, 16), True), "Rotate": (lin(0, 60), True)}
    assert list(A.GEOMETRIC_SPACE) == ["Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate"]
    assert A.COLOUR_SPACE == {"Identity": (None, False), "Brightness": (lin(0, 0.5), True),
                              "Color": (lin(0, 0.02), True), "Contrast": (lin(0, 0.5), True),
                              "Sharpness": (lin(0, 0.5), True), "Posterize": (post, False),
                              "AutoContrast": (None, False), "Equalize": (None, False)}
    assert A.COLOUR_SPACE_WITH_COLOR == {"Identity": (None, False), "Brightness": (lin(0, 0.5), True),
                                         "Color": (lin(0, 0.5), True), "Contrast": (lin(0, 0.5), True),
                                         "Sharpness": (lin(0, 0.5), True), "Posterize": (post, False),
                                         "Solarize": (lin(255, 0), False), "AutoContrast": (None, False),
                                         "Equalize": (None, False)}
    assert post[0] == 8 and post[-1] == 2


def test_policies_cover_every_dataset_family():
    want = {"pets": (48, 8), "partimagenet": (48, 8), "CUB-200-2011": (8, 4), "CUB-200-2011-pretrain": (32, 4),
            "CARS": (32, 4), "grayscale_example": (32, None), "geometric_shapes": (32, 8),
            "geometric_shapes_gaussian_noise": (32, 8), "geometric_shapes_224_gaussian_noise": (32, 8),
            "mnist_counting": (24, 8)}
    assert set(A.POLICIES) == set(want)
    for name, (p1, p2) in want.items():
        s1, s2 = A.POLICIES[name].sizes(192)
        assert s1 == 192 + p1 and s2 == (232 if p2 is None else 192 + p2)
    assert A.POLICIES["grayscale_example"].grayscale and A.POLICIES["grayscale_example"].sizes(128)[1] == 232
    assert [n for n, p in A.POLICIES.items() if p.noise] == ["geometric_shapes_gaussian_noise",
                                                              "geometric_shapes_224_gaussian_noise"]
    assert A.POLICIES["CARS"].colour == "trivial_color" and A.POLICIES["mnist_counting"].geometric == "affine"
    assert not A.POLICIES["geometric_shapes"].flip and A.POLICIES["pets"].flip
    with pytest.raises(ValueError):
        A.POLICIES["grayscale_example"].sizes(256)
    with pytest.raises(KeyError):
        A.get_policy("imagenet")


@pytest.mark.parametrize("name", sorted(A.POLICIES))
def test_every_parameter_within_its_range(name):
    size = 64
    p = A.POLICIES[name]
    s1, s2 = p.sizes(size)
    prm = A.sample_params(name, size, 300, _gen(11))
    g, v = prm.geom.numpy(), prm.view.numpy()
    assert g.shape == (300, 13) and v.shape == (2, 300, 8) and np.isfinite(g).all() and np.isfinite(v).all()
    assert set(np.unique(g[:, 0])) <= {0.0, 1.0, 2.0}
    fixed = g[:, 0] == 1
    assert ((g[fixed, 2] != 0) | (g[fixed, 4] != 0)).all()
    assert ((g[g[:, 0] == 2, 2] == 0) & (g[g[:, 0] == 2, 4] == 0)).all()
    assert (g[:, 7] == (0 if p.geometric == "trivial" else 255)).all()
    assert set(np.unique(g[:, 8])) == ({0.0, 1.0} if p.flip else {0.0})
    top, left, ch, cw = g[:, 9], g[:, 10], g[:, 11], g[:, 12]
    assert (g[:, 9:] == np.round(g[:, 9:])).all()
    assert (top >= 0).all() and (left >= 0).all() and (top + ch <= s1).all() and (left + cw <= s1).all()
    area, ratio = ch * cw / (s1 * s1), cw / ch
    assert (area > 0.93).all() and (area <= 1.0).all() and (ratio > 0.74).all() and (ratio < 1.35).all()
    if p.geometric != "trivial":                 # |angle| < 10, scale in (0.9, 1.1)
        det = g[:, 1] * g[:, 5] - g[:, 2] * g[:, 4]
        inv_scale = np.sqrt(det)
        lo, hi = (1 / 1.1, 1 / 0.9) if p.geometric == "affine" else (1 - 1e-9, 1 + 1e-9)
        assert (inv_scale > lo - 1e-9).all() and (inv_scale < hi + 1e-9).all()
        assert (np.abs(np.degrees(np.arctan2(g[:, 2], g[:, 1]))) < 10 + 1e-9).all()
    ops = v[:, :, [0, 2]]
    assert (v[:, :, 4:6] >= 0).all() and (v[:, :, 4:6] <= s2 - size).all()
    assert (v[:, :, 4:6] == np.round(v[:, :, 4:6])).all()
    assert set(np.unique(v[:, :, 6])) == ({0.0, 1.0} if p.noise else {0.0})
    assert (v[0, :, 7] == np.arange(300)).all() and (v[1, :, 7] == np.arange(300)).all()
    if p.colour == "jitter":
        assert {tuple(o) for o in ops.reshape(-1, 2)} == {(1.0, 3.0), (3.0, 1.0)}
        f = v[:, :, [1, 3]]
        assert (f > 0.9).all() and (f < 1.1).all()
    else:
        assert (ops[..., 1] == 0).all()
        allowed = {float(A.OP_CODES[n]) for n in (A.COLOUR_SPACE if p.colour == "trivial"
                                                  else A.COLOUR_SPACE_WITH_COLOR)}
        assert set(np.unique(ops[..., 0])) == allowed
        enh = np.isin(ops[..., 0], [1, 2, 3, 4])
        assert (v[:, :, 1][enh] >= 0.5 - 1e-6).all() and (v[:, :, 1][enh] <= 1.5 + 1e-6).all()
        post = ops[..., 0] == 5
        assert set(np.unique(v[:, :, 1][post])) <= {2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0}
        sol = ops[..., 0] == 6
        assert (v[:, :, 1][sol] >= 0).all() and (v[:, :, 1][sol] <= 255).all()


def test_trivial_augment_frequencies():
    """20,000 draws: every operation, magnitude bin and sign within 5 binomial standard
    deviations of uniform."""
    n = 20000
    for space in (A.GEOMETRIC_SPACE, A.COLOUR_SPACE, A.COLOUR_SPACE_WITH_COLOR):
        st = A._Stream(123, len(space))
        draws = [A.trivial_augment(space, st) for _ in range(n)]
        k = len(space)
        sd = math.sqrt(n * (1 / k) * (1 - 1 / k))
        for name in space:
            cnt = sum(1 for op, _ in draws if op == name)
            assert abs(cnt - n / k) < 5 * sd, (name, cnt)
        name = "Brightness" if "Brightness" in space else "Rotate"
        mags = [m for op, m in draws if op == name]
        vals = space[name][0]
        sdm = math.sqrt(len(mags) * (1 / 31) * (30 / 31))
        for b in range(31):
            cnt = sum(1 for m in mags if abs(m) == vals[b])
            assert abs(cnt - len(mags) / 31) < 5 * sdm, (name, b, cnt)
        nz = [m for m in mags if m != 0]
        neg = sum(1 for m in nz if m < 0)
        assert abs(neg - len(nz) / 2) < 5 * math.sqrt(len(nz) / 4)
    flips = A.sample_params("pets", 32, 2000, _gen(4)).geom[:, 8].sum().item()
    assert abs(flips - 1000) < 5 * math.sqrt(500)
    noisy = A.sample_params("geometric_shapes_gaussian_noise", 32, 2000, _gen(4)).view[:, :, 6].sum().item()
    assert abs(noisy - 2000) < 5 * math.sqrt(1000)


def test_same_seed_same_parameters_and_batch_split():
    for name in ("CUB-200-2011", "mnist_counting", "geometric_shapes_gaussian_noise"):
        a = A.sample_params(name, 64, 8, _gen(7))
        b = A.sample_params(name, 64, 8, _gen(7))
        c = A.sample_params(name, 64, 8, _gen(8))
        assert torch.equal(a.geom, b.geom) and torch.equal(a.view, b.view)
        assert not torch.equal(a.geom, c.geom) and not torch.equal(a.view, c.view)
        g = _gen(7)
        lo = A.sample_params(name, 64, 3, g, first_id=0)
        hi = A.sample_params(name, 64, 5, g, first_id=3)
        assert torch.equal(torch.cat([lo.geom, hi.geom]), a.geom)
        assert torch.equal(torch.cat([lo.view, hi.view], 1), a.view)
        later = A.sample_params(name, 64, 8, _gen(7), first_id=8)
        assert not torch.equal(later.geom, a.geom)


def test_random_resized_crop_fallback():
    st = A._Stream(1, 0)
    assert A.random_resized_crop_box(1, 400, st) == (0, 199, 1, 1)        # in_ratio > 4/3: central, h = height
    assert A.random_resized_crop_box(400, 1, st) == (199, 0, 1, 1)        # in_ratio < 3/4
    for _ in range(200):
        top, left, h, w = A.random_resized_crop_box(72, 72, st)
        assert 0 <= top <= 72 - h and 0 <= left <= 72 - w and 0.95 * 72 * 72 - 72 <= h * w <= 72 * 72


def test_transform_refuses_a_cpu_device():
    from count_pipnet_amd.data import DeviceTrainTransform, pack_images
    t = DeviceTrainTransform("CUB-200-2011", 32)
    assert (t.s1, t.s2) == (40, 36)
    with pytest.raises(RuntimeError):
        t(pack_images([NOISE]), "cpu")
