"""numpy restatement of the training augmentation's pixel arithmetic (Pillow 12.2.0's, which
torchvision's PIL transforms forward to) and of the composed two-stage pipeline that
``count_pipnet_amd/csrc/augment_ops.hip`` runs.  TEST INFRASTRUCTURE ONLY; does not import PIL --
``tests/test_augment_cpu.py`` pins every function here against live Pillow, bit for bit.

Parameter rows are the C-ABI's (include/pipnet_amd.h): ``gparams`` = (path, m0..m5, fill, flip,
top, left, height, width), ``vparams`` = (op1, p1, op2, p2, top, left, noise flag, image id).
"""
from __future__ import annotations

import math

import numpy as np

from oracle import input_ref

(OP_IDENTITY, OP_BRIGHTNESS, OP_COLOR, OP_CONTRAST, OP_SHARPNESS, OP_POSTERIZE, OP_SOLARIZE, OP_AUTOCONTRAST,
 OP_EQUALIZE) = range(9)
WARP_NONE, WARP_FIXED, WARP_DOUBLE = 0, 1, 2


# ---- geometry -------------------------------------------------------------------------------

def warp_path(m) -> int:
    """Which of Pillow's two affine loops a matrix takes (Geometry.c ImagingTransformAffine)."""
    return WARP_FIXED if (m[1] != 0 or m[3] != 0) else WARP_DOUBLE


def _fix(v: float) -> int:
    return int(math.floor(v * 65536.0 + 0.5))


def affine_nearest(img: np.ndarray, m, fill: int, path=None) -> np.ndarray:
    """``Image.transform(img.size, AFFINE, m, NEAREST, fillcolor=(fill,)*3)``."""
    h, w = img.shape[:2]
    m = [float(v) for v in m]
    path = warp_path(m) if path is None else path
    if path == WARP_NONE:
        return img.copy()
    if path == WARP_FIXED:
        a0, a1, a3, a4 = _fix(m[0]), _fix(m[1]), _fix(m[3]), _fix(m[4])
        a2 = _fix(m[2] + 0.5 * m[0] + 0.5 * m[1])
        a5 = _fix(m[5] + 0.5 * m[3] + 0.5 * m[4])
        y, x = np.mgrid[0:h, 0:w].astype(np.int64)
        xin = (a2 + x * a0 + y * a1) >> 16
        yin = (a5 + x * a3 + y * a4) >> 16
    else:
        def coords(n, o, step):
            out = np.empty(n, np.int64)
            for k in range(n):
                out[k] = -1 if o < 0 else int(o)
                o += step
            return out
        xin = np.broadcast_to(coords(w, m[2] + m[0] * 0.5, m[0])[None, :], (h, w))
        yin = np.broadcast_to(coords(h, m[5] + m[4] * 0.5, m[4])[:, None], (h, w))
    inside = (xin >= 0) & (xin < w) & (yin >= 0) & (yin < h)
    out = np.full_like(img, fill)
    out[inside] = img[yin[inside], xin[inside]]
    return out


def rotate_matrix(angle: float, w: int, h: int):
    """The matrix of ``Image.rotate(angle, NEAREST, expand=False, center=None)``; None when
    Pillow returns a copy (angle % 360 == 0)."""
    angle = angle % 360.0
    if angle == 0:
        return None
    r = -math.radians(angle)
    m = [round(math.cos(r), 15), round(math.sin(r), 15), 0.0, round(-math.sin(r), 15), round(math.cos(r), 15), 0.0]
    cx, cy = w / 2.0, h / 2.0
    m[2] = m[0] * (-cx) + m[1] * (-cy) + cx
    m[5] = m[3] * (-cx) + m[4] * (-cy) + cy
    return m


def hflip(img: np.ndarray) -> np.ndarray:
    return img[:, ::-1].copy()


def crop_resize(img: np.ndarray, top: int, left: int, ch: int, cw: int, out: int) -> np.ndarray:
    """``img.crop((left, top, left + cw, top + ch)).resize((out, out), BILINEAR)``: the
    coefficients are those of a ch x cw image and no tap leaves the crop."""
    return input_ref.pil_resize_bilinear(np.ascontiguousarray(img[top:top + ch, left:left + cw]), out, out)


# ---- colour ---------------------------------------------------------------------------------

def luma(img: np.ndarray) -> np.ndarray:
    x = img.astype(np.int64)
    return (x[..., 0] * 19595 + x[..., 1] * 38470 + x[..., 2] * 7471 + 0x8000) >> 16


def blend(degenerate: np.ndarray, img: np.ndarray, factor: float) -> np.ndarray:
    """``Image.blend(degenerate, img, factor)`` (every ImageEnhance operation)."""
    f = np.float32(factor)
    d = degenerate.astype(np.float32)
    t = d + f * (img.astype(np.float32) - d)           # fp32, no contraction
    if 0.0 <= float(f) <= 1.0:
        return t.astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.uint8))).astype(np.uint8)


def smooth(img: np.ndarray) -> np.ndarray:
    """``img.filter(ImageFilter.SMOOTH)``: 3x3 [[1,1,1],[1,5,1],[1,1,1]] / 13, border copied."""
    out = img.copy()
    h, w = img.shape[:2]
    if h < 3 or w < 3:
        return out
    x = img.astype(np.float32)
    ss = np.zeros((h - 2, w - 2, img.shape[2]), np.float32)
    for dy in range(3):
        row = x[dy:h - 2 + dy, 0:w - 2] + (np.float32(5.0) * x[dy:h - 2 + dy, 1:w - 1] if dy == 1
                                           else x[dy:h - 2 + dy, 1:w - 1]) + x[dy:h - 2 + dy, 2:w]
        ss = ss + row
    v = np.floor(ss / np.float32(13.0) + np.float32(0.5))
    out[1:h - 1, 1:w - 1] = np.clip(v, 0, 255).astype(np.uint8)
    return out


def _stack3(l: np.ndarray) -> np.ndarray:
    return np.repeat(l[..., None], 3, axis=2)


def brightness(img, f):
    return blend(np.zeros_like(img), img, f)


def color(img, f):
    return blend(_stack3(luma(img)), img, f)


def contrast(img, f):
    l = luma(img)
    hist = np.bincount(l.reshape(-1), minlength=256)
    mean = float((np.arange(256, dtype=np.float64) * hist).sum()) / l.size
    return blend(np.full_like(img, int(mean + 0.5)), img, f)


def sharpness(img, f):
    return blend(smooth(img), img, f)


def posterize(img, bits: int):
    return img & np.uint8(~((1 << (8 - int(bits))) - 1) & 255)


def solarize(img, thr: float):
    return np.where(img.astype(np.float64) < thr, img, 255 - img).astype(np.uint8)


def autocontrast(img):
    out = img.copy()
    for c in range(3):
        lo, hi = int(img[..., c].min()), int(img[..., c].max())
        if hi <= lo:
            continue
        scale = 255.0 / (hi - lo)
        off = -lo * scale
        lut = np.array([min(255, max(0, int(i * scale + off))) for i in range(256)], np.uint8)
        out[..., c] = lut[img[..., c]]
    return out


def equalize(img):
    out = img.copy()
    for c in range(3):
        h = np.bincount(img[..., c].reshape(-1), minlength=256).tolist()
        nz = [v for v in h if v]
        if len(nz) <= 1:
            continue
        step = (sum(nz) - nz[-1]) // 255
        if step == 0:
            continue
        n, lut = step // 2, []
        for i in range(256):
            lut.append(min(255, n // step))
            n += h[i]
        out[..., c] = np.array(lut, np.uint8)[img[..., c]]
    return out


def colour_op(img: np.ndarray, op: int, p: float) -> np.ndarray:
    op = int(op)
    if op == OP_IDENTITY:
        return img.copy()
    if op == OP_BRIGHTNESS:
        return brightness(img, p)
    if op == OP_COLOR:
        return color(img, p)
    if op == OP_CONTRAST:
        return contrast(img, p)
    if op == OP_SHARPNESS:
        return sharpness(img, p)
    if op == OP_POSTERIZE:
        return posterize(img, int(p))
    if op == OP_SOLARIZE:
        return solarize(img, p)
    if op == OP_AUTOCONTRAST:
        return autocontrast(img)
    if op == OP_EQUALIZE:
        return equalize(img)
    raise ValueError(op)


# ---- the composed pipeline --------------------------------------------------------------------

def geometry(img: np.ndarray, gp, S1: int, S2: int) -> np.ndarray:
    """transform1 of one decoded image under one ``gparams`` row -> S2 x S2 x 3 uint8."""
    gp = [float(v) for v in gp]
    x = input_ref.pil_resize_bilinear(img, S1, S1)
    x = affine_nearest(x, gp[1:7], int(gp[7]), path=int(gp[0]))
    if gp[8]:
        x = hflip(x)
    return crop_resize(x, int(gp[9]), int(gp[10]), int(gp[11]), int(gp[12]), S2)


def view(img: np.ndarray, vp, s: int, gray: bool, mean, std, noise=None) -> np.ndarray:
    """transform2 of one S2 x S2 image under one ``vparams`` row -> [3, s, s] float32.
    ``noise`` [3, s, s] is added after ToTensor when the row's flag is set."""
    vp = [float(v) for v in vp]
    x = colour_op(colour_op(img, vp[0], vp[1]), vp[2], vp[3])
    i, j = int(vp[4]), int(vp[5])
    x = x[i:i + s, j:j + s]
    if gray:
        x = _stack3(luma(x).astype(np.uint8))
    t = np.ascontiguousarray(x.transpose(2, 0, 1)).astype(np.float32) / np.float32(255.0)
    if vp[6] and noise is not None:
        t = t + noise.astype(np.float32)
    m = np.asarray(mean, np.float32)[:, None, None]
    sd = np.asarray(std, np.float32)[:, None, None]
    return (t - m) / sd


def pipeline(images, gparams, vparams, S1: int, S2: int, s: int, gray=False, mean=input_ref.IMAGENET_MEAN,
             std=input_ref.IMAGENET_STD, noise=None):
    """-> (u8 [B,S2,S2,3], views [V,B,3,s,s] float32)."""
    gparams, vparams = np.asarray(gparams, np.float64), np.asarray(vparams, np.float64)
    u8 = np.stack([geometry(im, gparams[b], S1, S2) for b, im in enumerate(images)])
    V = vparams.shape[0]
    out = np.stack([np.stack([view(u8[b], vparams[v, b], s, gray, mean, std,
                                   None if noise is None else np.asarray(noise)[v, b])
                              for b in range(len(images))]) for v in range(V)])
    return u8, out
