"""Two-view training augmentation on the GPU (pipnet_augment_geometry_rgb8 /
pipnet_augment_view_rgb8 through the C-ABI) against tests/augment_ref.py, which
tests/test_augment_cpu.py pins to Pillow: for explicit parameters the uint8 images and the
fp32 views are bit-exact -- integer resamples and index maps, IEEE fp32 blends and divisions."""
import math
import os

import numpy as np
import pytest
import torch

import augment_ref as R
from count_pipnet_amd import augment as A
from input_util import synth_photo
from oracle import input_ref

pytestmark = pytest.mark.gpu
MEAN, STD = input_ref.IMAGENET_MEAN, input_ref.IMAGENET_STD
S, S1, S2 = 32, 64, 40
SHAPES = [(37, 45), (64, 64), (50, 90), (90, 50), (33, 200)]
SOURCES = [synth_photo(h, w, 40 + i, "smooth" if i % 2 else "noise") for i, (h, w) in enumerate(SHAPES)]
BOXES = [(0, 0, 60, 60), (4, 4, 60, 60), (2, 11, 62, 53), (9, 0, 55, 64), (0, 0, 64, 64), (13, 7, 40, 40),
         (24, 20, 40, 44)]


def _geom_rows():
    """Every geometric operation at bins 0, 15, 30 with both signs, rotation +-10 with fill 255,
    RandomAffine, a scale-only matrix, identity; flip and crop box cycle through the rows."""
    warps = []
    for op in ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate"):
        for k in (0, 15, 30):
            for sign in (1.0, -1.0):
                warps.append(A.warp_row(A.geometric_matrix(op, sign * A.GEOMETRIC_SPACE[op][0][k], S1), 0))
    warps += [A.warp_row(A.rotate_matrix(a, S1, S1), 255) for a in (10.0, -10.0)]
    warps += [A.warp_row(A.affine_inverse_matrix([S1 / 2, S1 / 2], 7.3, [-5, 6], 0.93, [0.0, 0.0]), 255),
              A.warp_row(A.affine_inverse_matrix([S1 / 2, S1 / 2], -9.9, [6, -2], 1.08, [0.0, 0.0]), 255),
              A.warp_row([1.0 / 0.9, 0.0, -3.3, 0.0, 1.07, 2.6], 255),            # scale only: double loop
              A.warp_row([0.97, 0.0, 70.0, 0.0, 1.0, -70.0], 9),                  # entirely outside: all fill
              A.warp_row(None, 0), A.warp_row(None, 0), A.warp_row(None, 0)]
    return [w + [float(i % 2)] + [float(v) for v in BOXES[i % len(BOXES)]] for i, w in enumerate(warps)]


GEOM_ROWS = _geom_rows()
IDENTITY_G = A.warp_row(None, 0) + [0.0, 0.0, 0.0, float(S1), float(S1)]


def _geometry(gpu, images, gparams, s1, s2):
    from count_pipnet_amd import kernels as K
    from count_pipnet_amd.data import pack_images
    p = pack_images(images)
    out = K.augment_geometry_rgb8(p.pixels.to(gpu), p.offsets.to(gpu), p.sizes.to(gpu), p.sizes.numpy(),
                                  torch.tensor(gparams, dtype=torch.float64), s1, s2)
    torch.cuda.synchronize()
    return out


def _views(gpu, u8, vparams, s, gray=False, noise=None, seed=0):
    from count_pipnet_amd import kernels as K
    out = K.augment_view_rgb8(torch.as_tensor(u8).to(gpu), torch.tensor(vparams, dtype=torch.float64), s, MEAN, STD,
                              gray, A.NOISE_STD, seed, None if noise is None else noise.to(gpu))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def resized():
    """The first resize of the ragged sources, computed once and only read."""
    return [input_ref.pil_resize_bilinear(im, S1, S1) for im in SOURCES]


def _ref_geometry(resized_img, gp, s2):
    x = R.affine_nearest(resized_img, gp[1:7], int(gp[7]), path=int(gp[0]))
    x = R.hflip(x) if gp[8] else x
    return R.crop_resize(x, int(gp[9]), int(gp[10]), int(gp[11]), int(gp[12]), s2)


@pytest.mark.parametrize("batch", range(math.ceil(len(GEOM_ROWS) / 5)))
def test_geometry_every_operation(gpu, resized, batch):
    rows = [GEOM_ROWS[(5 * batch + b) % len(GEOM_ROWS)] for b in range(5)]
    got = _geometry(gpu, SOURCES, rows, S1, S2).cpu().numpy()
    assert got.shape == (5, S2, S2, 3) and got.dtype == np.uint8
    for b in range(5):
        np.testing.assert_array_equal(got[b], _ref_geometry(resized[b], rows[b], S2), err_msg=str(rows[b]))


def test_geometry_flip_and_boxes_on_one_warp(gpu, resized):
    """One shear, flip on and off, each crop box (origin, maximum offset, non-square, full size,
    S2-sized in one or both axes so a resample pass is skipped)."""
    warp = A.warp_row(A.geometric_matrix("ShearY", 0.25, S1), 0)
    for flip in (0.0, 1.0):
        for start in (0, 5):
            rows = [warp + [flip] + [float(v) for v in BOXES[(start + b) % len(BOXES)]] for b in range(5)]
            got = _geometry(gpu, SOURCES, rows, S1, S2).cpu().numpy()
            for b in range(5):
                np.testing.assert_array_equal(got[b], _ref_geometry(resized[b], rows[b], S2), err_msg=str(rows[b]))


# ---- views ------------------------------------------------------------------------------------

def _view_images(s2):
    a = synth_photo(s2, s2, 60, "noise")
    b = synth_photo(s2, s2, 61, "smooth")
    c = b.copy()
    c[..., 1] = 93                                      # constant channel
    d = (b // 4 + 60).astype(np.uint8)                  # narrow range
    e = np.full((s2, s2, 3), 17, np.uint8)              # constant image
    return np.stack([a, b, c, d, e])


VIEW_IMAGES = _view_images(S2)
COLOUR_CASES = ([(op, f) for op in (R.OP_BRIGHTNESS, R.OP_COLOR, R.OP_CONTRAST, R.OP_SHARPNESS) for f in (0.5, 1.5, 1.0)]
                + [(R.OP_COLOR, 0.98), (R.OP_COLOR, 1.02), (R.OP_POSTERIZE, 2.0), (R.OP_POSTERIZE, 8.0),
                   (R.OP_SOLARIZE, 0.0), (R.OP_SOLARIZE, 255.0), (R.OP_SOLARIZE, 127.5), (R.OP_AUTOCONTRAST, 0.0),
                   (R.OP_EQUALIZE, 0.0), (R.OP_IDENTITY, 0.0)])


def _check_views(gpu, imgs, vparams, s, gray=False):
    got = _views(gpu, imgs, vparams, s, gray)
    assert got.shape == (len(vparams), len(imgs), 3, s, s) and got.dtype == np.float32
    for v in range(len(vparams)):
        for b in range(len(imgs)):
            want = R.view(imgs[b], vparams[v][b], s, gray, MEAN, STD)
            np.testing.assert_array_equal(got[v, b], want, err_msg=f"view {v} image {b} {vparams[v][b]}")


@pytest.mark.parametrize("case", range(0, len(COLOUR_CASES), 2))
def test_view_every_colour_operation(gpu, case):
    """Two operations per launch, one per view (so the two views of an image differ); crop
    offsets at 0, the maximum and in between."""
    offs = [(0, 0), (8, 8), (3, 5), (8, 0), (0, 8)]
    vparams = [[[float(COLOUR_CASES[case + v][0]), COLOUR_CASES[case + v][1], 0.0, 0.0,
                 float(offs[(b + v) % 5][0]), float(offs[(b + v) % 5][1]), 0.0, float(b)] for b in range(5)]
               for v in range(2)]
    _check_views(gpu, VIEW_IMAGES, vparams, S)


def test_view_colour_jitter_both_orders_and_grayscale(gpu):
    """ColorJitter: brightness then contrast (Contrast's mean is that of the brightened image)
    and the other order, different factors per image and view; then Grayscale(3), V = 1."""
    f = [0.9, 1.1, 0.95, 1.04, 1.0999]
    vparams = [[[R.OP_BRIGHTNESS, f[b], R.OP_CONTRAST, f[4 - b], 2.0, 6.0, 0.0, 0.0] for b in range(5)],
               [[R.OP_CONTRAST, f[4 - b], R.OP_BRIGHTNESS, f[b], 7.0, 1.0, 0.0, 0.0] for b in range(5)]]
    _check_views(gpu, VIEW_IMAGES, vparams, S)
    chain = [[[R.OP_AUTOCONTRAST, 0.0, R.OP_EQUALIZE, 0.0, 1.0, 1.0, 0.0, 0.0] for b in range(5)]]
    _check_views(gpu, VIEW_IMAGES, chain, S)
    gray = [[[float(op), 1.3, 0.0, 0.0, 4.0, 4.0, 0.0, 0.0] for op in (0, 2, 3, 8, 4)]]
    _check_views(gpu, VIEW_IMAGES, gray, S, gray=True)


def test_view_equalize_step_zero(gpu):
    """144 pixels: Equalize's step is 0 and every channel passes through."""
    imgs = VIEW_IMAGES[:, :12, :12].copy()
    vparams = [[[R.OP_EQUALIZE, 0.0, 0.0, 0.0, 8.0, 3.0, 0.0, 0.0] for _ in range(5)]]
    _check_views(gpu, imgs, vparams, 4)
    got = _views(gpu, imgs, vparams, 4)
    assert torch.equal(torch.from_numpy(got[0, 0]), input_ref.to_tensor_normalize(imgs[0][8:12, 3:7]))


def test_full_pipeline_at_224(gpu):
    """CUB-200-2011 sizes (232 -> 228 -> 224) on two 500 x 375 photos through DeviceTrainTransform
    with explicit parameters."""
    from count_pipnet_amd.data import DeviceTrainTransform, pack_images
    imgs = [synth_photo(375, 500, 70, "smooth"), synth_photo(500, 375, 71, "noise")]
    t = DeviceTrainTransform("CUB-200-2011", 224)
    assert (t.s1, t.s2) == (232, 228)
    geom = [A.warp_row(A.geometric_matrix("Rotate", -38.0, 232), 0) + [1.0, 3.0, 1.0, 226.0, 229.0],
            A.warp_row(A.geometric_matrix("TranslateX", 16.0, 232), 0) + [0.0, 0.0, 0.0, 232.0, 232.0]]
    view = [[[R.OP_SHARPNESS, 1.5, 0.0, 0.0, 4.0, 0.0, 0.0, 0.0], [R.OP_EQUALIZE, 0.0, 0.0, 0.0, 0.0, 4.0, 0.0, 1.0]],
            [[R.OP_CONTRAST, 0.5, 0.0, 0.0, 1.0, 2.0, 0.0, 0.0], [R.OP_AUTOCONTRAST, 0.0, 0.0, 0.0, 2.0, 2.0, 0.0, 1.0]]]
    prm = A.AugmentParams(torch.tensor(geom, dtype=torch.float64), torch.tensor(view, dtype=torch.float64))
    xs1, xs2 = t(pack_images(imgs), gpu, params=prm)
    assert xs1.shape == xs2.shape == (2, 3, 224, 224) and xs1.is_cuda and xs1.dtype == torch.float32
    u8, want = R.pipeline(imgs, geom, view, 232, 228, 224)
    np.testing.assert_array_equal(_geometry(gpu, imgs, geom, 232, 228).cpu().numpy(), u8)
    np.testing.assert_array_equal(xs1.cpu().numpy(), want[0])
    np.testing.assert_array_equal(xs2.cpu().numpy(), want[1])


# ---- noise ------------------------------------------------------------------------------------

def _noise_params(flags, ids=None, op=R.OP_BRIGHTNESS):
    b = len(flags[0])
    return [[[float(op), 1.05, 0.0, 0.0, 3.0, 2.0, float(flags[v][k]), float(k if ids is None else ids[k])]
             for k in range(b)] for v in range(len(flags))]


def test_injected_noise_is_exact_and_flag_off_is_untouched(gpu):
    flags = [[1, 0, 1, 0, 1], [0, 1, 1, 0, 0]]
    vparams = _noise_params(flags)
    g = torch.Generator().manual_seed(3)
    noise = torch.randn(2, 5, 3, S, S, generator=g) * 0.1
    got = _views(gpu, VIEW_IMAGES, vparams, S, noise=noise)
    clean = _views(gpu, VIEW_IMAGES, _noise_params([[0] * 5, [0] * 5]), S)
    for v in range(2):
        for b in range(5):
            want = R.view(VIEW_IMAGES[b], vparams[v][b], S, False, MEAN, STD, noise[v, b].numpy())
            np.testing.assert_array_equal(got[v, b], want)
            assert (got[v, b] == clean[v, b]).all() == (not flags[v][b])
    philox = _views(gpu, VIEW_IMAGES, vparams, S, seed=5)           # flag off: bit-identical to no noise
    for v in range(2):
        for b in range(5):
            assert (philox[v, b] == clean[v, b]).all() == (not flags[v][b])


def test_philox_noise_is_seeded_split_invariant_and_gaussian(gpu):
    flags = [[1] * 5, [1] * 5]
    ids = [100, 101, 102, 103, 104]
    vparams = _noise_params(flags, ids, op=R.OP_IDENTITY)
    a = _views(gpu, VIEW_IMAGES, vparams, S, seed=11)
    b = _views(gpu, VIEW_IMAGES, vparams, S, seed=11)
    c = _views(gpu, VIEW_IMAGES, vparams, S, seed=12)
    np.testing.assert_array_equal(a, b)
    assert (a != c).mean() > 0.99
    lo = _views(gpu, VIEW_IMAGES[:2], [[r for r in v[:2]] for v in vparams], S, seed=11)
    hi = _views(gpu, VIEW_IMAGES[2:], [[r for r in v[2:]] for v in vparams], S, seed=11)
    np.testing.assert_array_equal(np.concatenate([lo, hi], 1), a)
    clean = _views(gpu, VIEW_IMAGES, _noise_params([[0] * 5, [0] * 5], ids, op=R.OP_IDENTITY), S)
    std = np.asarray(STD, np.float64)[None, None, :, None, None]
    z = ((a.astype(np.float64) - clean.astype(np.float64)) * std).reshape(-1)      # the added noise
    n = z.size
    assert n == 2 * 5 * 3 * S * S >= 24576
    assert abs(z.mean()) < 5 * 0.1 / math.sqrt(n), z.mean()
    assert abs(z.std() - 0.1) < 5 * 0.1 / math.sqrt(2 * n), z.std()
    assert (a[0] != a[1]).mean() > 0.99                 # the two views draw different noise
    assert abs(np.corrcoef(z[:S * S], z[S * S:2 * S * S])[0, 1]) < 5 / math.sqrt(S * S)   # channels R, G


# ---- errors, loader, training step ------------------------------------------------------------

def test_wrappers_reject_bad_arguments(gpu):
    from count_pipnet_amd import kernels as K
    u8 = torch.as_tensor(VIEW_IMAGES).to(gpu)
    ok = torch.tensor(_noise_params([[0] * 5]), dtype=torch.float64)
    for bad in ("float", "op", "sharp2", "crop"):
        vp = ok.clone()
        if bad == "float":
            vp = vp.float()
        elif bad == "op":
            vp[0, 0, 0] = 9
        elif bad == "sharp2":
            vp[0, 0, 2] = R.OP_SHARPNESS
        else:
            vp[0, 0, 4] = 9
        with pytest.raises(RuntimeError):
            K.augment_view_rgb8(u8, vp, S, MEAN, STD)
    with pytest.raises(RuntimeError):
        K.augment_view_rgb8(u8.cpu(), ok, S, MEAN, STD)
    with pytest.raises(RuntimeError):
        _geometry(gpu, SOURCES, [IDENTITY_G[:9] + [40.0, 0.0, 30.0, 30.0]] * 5, S1, S2)
    empty = _geometry(gpu, [], np.zeros((0, 13)), S1, S2)
    assert empty.shape == (0, S2, S2, 3)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("train")
    for c in range(3):
        os.makedirs(root / f"class_{c}")
        for j in range(4):
            im = synth_photo(70 + 9 * j, 80 + 11 * c, 10 * c + j, "smooth")
            Image.fromarray(im, "RGB").save(str(root / f"class_{c}" / f"img{j}.png"))
    return str(root)


def _epochs(loader, n):
    return [[(x1.cpu(), x2.cpu(), y.cpu()) for x1, x2, y in loader] for _ in range(n)]


def test_train_loader_two_epochs(gpu, folder):
    from count_pipnet_amd.data import get_train_loader
    mk = lambda seed: get_train_loader(folder, "geometric_shapes_gaussian_noise", 32, 5, gpu, num_workers=0, seed=seed)
    loader = mk(3)
    assert len(loader) == 2 and len(loader.dataset) == 12          # drop_last: 12 // 5
    first = None
    for xs1, xs2, ys in loader:
        assert xs1.shape == xs2.shape == (5, 3, 32, 32) and ys.shape == (5,)
        assert xs1.is_cuda and xs2.is_cuda and ys.is_cuda
        assert xs1.dtype == xs2.dtype == torch.float32 and ys.dtype == torch.int64
        assert bool(torch.isfinite(xs1).all()) and not torch.equal(xs1, xs2)
        first = first or (xs1.cpu(), xs2.cpu(), ys.cpu())
    a, b = _epochs(mk(7), 2), _epochs(mk(7), 2)
    assert [len(e) for e in a] == [2, 2]
    for ea, eb in zip(a, b):
        for ta, tb in zip(ea, eb):
            assert all(torch.equal(x, y) for x, y in zip(ta, tb))
    assert not torch.equal(a[0][0][0], a[1][0][0])                  # epochs differ
    assert not torch.equal(a[0][0][0], _epochs(mk(8), 1)[0][0][0])  # seeds differ
    # a Subset with a WeightedRandomSampler, one view (trainset_normal_augment)
    idx = list(range(0, 12, 2))
    sampler = torch.utils.data.WeightedRandomSampler(torch.ones(len(idx)), len(idx), replacement=True)
    one = get_train_loader(folder, "CARS", 32, 4, gpu, num_workers=0, sampler=sampler, indices=idx, seed=1, views=1)
    assert len(one) == 1 and len(one.dataset) == 6
    for xs, ys in one:
        assert xs.shape == (4, 3, 32, 32) and ys.shape == (4,) and int(ys.max()) <= 2


def test_finetune_step_fed_from_the_loader(gpu, folder):
    from count_pipnet_amd import train as T
    from count_pipnet_amd.data import get_train_loader
    from golden_util import load_train_golden
    from model_util import build_model
    meta, _, fwd_meta = load_train_golden("train_finetune_mid_addon")
    size = fwd_meta["case"]["size"]
    net = build_model(fwd_meta).to(gpu).train()
    for prm in net.parameters():
        prm.requires_grad = False
    cls = net._classification
    cls.weight.requires_grad = True
    opt = torch.optim.AdamW([{"params": [cls.weight], "lr": meta["lr"], "weight_decay": 0.0}], lr=meta["lr"])
    loader = get_train_loader(folder, "mnist_counting", size, 4, gpu, num_workers=0, seed=2)
    xs1, xs2, ys = next(iter(loader))
    w0 = cls.weight.detach().clone()
    stats = T.hip_finetune_step(net, xs1, xs2, ys, opt, True).cpu()
    assert bool(torch.isfinite(stats).all()) and float(stats[3]) > 0
    assert not torch.equal(cls.weight.detach(), w0)
