"""The heatmap_p{p}.png pixels of util/visualize_prediction.py:92-100, restated in numpy integers and float32 -- the
reference side of tests/test_gpu_heatmap.py.  tests/test_heatmap_cpu.py holds every step against the statements the
reference itself runs (torch's ``mul(255).byte()``, Pillow's ``resize(BICUBIC)``, ``plt.imsave``).

    q   = uint8(trunc(m * 255f))                              ToPILImage of a float map
    r   = Pillow's ImagingResample(BICUBIC) of q to S x S     horizontal pass, uint8 intermediate, vertical pass
    idx = uint8(255 * (r / 255f)) = r                         ToTensor, then the colour-table index
    v   = fl(fl(0.2f * fl(lut[r][c] / 255f)) + fl(0.6f * fl(frame[c] / 255f)))
    out = uint8(trunc(fl(v * 255f)))                          plt.imsave(vmin=0, vmax=1), without its alpha band
"""
import functools

import numpy as np

PREC = 22
WEIGHTS = (0.2, 0.6)


def quantise(m: np.ndarray) -> np.ndarray:
    """``m.mul(255).byte()`` for 0 <= m <= 1 + 2^-22, saturated beyond as the kernel saturates."""
    s = m.astype(np.float32) * np.float32(255)
    return np.clip(np.trunc(s), 0, 255).astype(np.uint8)


def _bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


@functools.lru_cache(maxsize=None)
def coeff_rows(in_size: int, out_size: int):
    """Per output coordinate (xmin, [k...]): precompute_coeffs + normalize_coeffs_8bpc, for in_size <= out_size."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    rows = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k, ww = [], 0.0
        for x in range(xmax):
            wt = _bicubic((x + xmin - center + 0.5) * (1.0 / filterscale))
            k.append(wt)
            ww += wt
        if ww != 0.0:
            k = [wt / ww for wt in k]
        rows.append((xmin, [int(-0.5 + wt * (1 << PREC)) if wt < 0 else int(0.5 + wt * (1 << PREC)) for wt in k]))
    return rows


def table_rows(table) -> list:
    """The rows of a ``kernels.bicubic_rows`` table [out, 2 + 5] in the form of ``coeff_rows``."""
    return [(int(r[0]), [int(v) for v in r[2:2 + int(r[1])]]) for r in np.asarray(table)]


def _pass(img: np.ndarray, rows, seen) -> np.ndarray:
    """One horizontal pass over the uint8 image ``img`` [rows, in] -> [rows, out]; ``seen`` collects the smallest
    and the largest value before clip8."""
    out = np.empty((img.shape[0], len(rows)), np.uint8)
    wide = img.astype(np.int64)
    for xx, (xmin, k) in enumerate(rows):
        acc = ((1 << (PREC - 1)) + wide[:, xmin:xmin + len(k)] @ np.asarray(k, np.int64).reshape(-1)) >> PREC
        if seen is not None:
            seen.append((int(acc.min()), int(acc.max())))
        out[:, xx] = np.clip(acc, 0, 255)
    return out


def resize(q: np.ndarray, size: int, rows_h=None, rows_v=None, seen=None) -> np.ndarray:
    """``Image.fromarray(q, "L").resize((size, size), Image.BICUBIC)`` of the uint8 map q [h, w], h, w <= size.
    ``rows_h`` / ``rows_v``: coefficient rows to use instead of ``coeff_rows`` (``table_rows`` of a table).
    ``seen``: a dict that receives, per pass that ran ("h", "v"), the (min, max) of the sums before clip8."""
    h, w = q.shape
    out = q
    for axis, n in (("h", w), ("v", h)):
        if n == size:                                # Pillow skips a pass whose axis keeps its size
            continue
        rows = {"h": rows_h, "v": rows_v}[axis]
        ranges = [] if seen is not None else None
        src = out if axis == "h" else np.ascontiguousarray(out.T)
        out = _pass(src, rows if rows is not None else coeff_rows(n, size), ranges)
        out = out if axis == "h" else out.T
        if seen is not None:
            seen[axis] = (min(r[0] for r in ranges), max(r[1] for r in ranges))
    return np.ascontiguousarray(out)


def blend(r: np.ndarray, frame: np.ndarray, lut: np.ndarray, weights=WEIGHTS) -> np.ndarray:
    """Steps 3-5: r [S, S] uint8, frame [S, S, 3] uint8, lut [256, 3] uint8 RGB -> [S, S, 3] uint8."""
    wh, wi = np.float32(weights[0]), np.float32(weights[1])
    heat = lut[r].astype(np.float32) / np.float32(255)
    img = frame.astype(np.float32) / np.float32(255)
    v = wh * heat + wi * img                     # numpy rounds each product and the sum to float32
    assert v.dtype == np.float32
    return np.clip(np.trunc(v * np.float32(255)), 0, 255).astype(np.uint8)


def heatmap(m: np.ndarray, frame: np.ndarray, lut: np.ndarray, weights=WEIGHTS):
    """(out [S, S, 3] uint8, resized [S, S] uint8) of the float32 map m [h, w] over ``frame`` [S, S, 3]."""
    r = resize(quantise(m), frame.shape[0])
    return blend(r, frame, lut, weights), r


def jet_like_lut() -> np.ndarray:
    """A [256, 3] uint8 RGB table shaped like JET (piecewise-linear ramps); every byte value occurs.  OpenCV's own
    table is the caller's to pass: any table checks the lookup."""
    x = np.arange(256) / 255.0
    rgb = np.stack([np.clip(1.5 - np.abs(4 * x - 3), 0, 1), np.clip(1.5 - np.abs(4 * x - 2), 0, 1),
                    np.clip(1.5 - np.abs(4 * x - 1), 0, 1)], axis=1)
    return np.round(rgb * 255).astype(np.uint8)


# ---- cases shared by tests/test_heatmap_cpu.py and tests/test_gpu_heatmap.py --------------------------------------
# (h, w, S): both passes from 1 x 1 up, none (16, 16, 16), vertical only, horizontal only, the C2 / C3 map sizes
SIZES = [(1, 1, 16), (2, 3, 17), (5, 7, 40), (8, 8, 64), (13, 13, 104), (16, 16, 16), (4, 16, 16), (16, 4, 16),
         (26, 26, 224), (28, 28, 224)]


def sparse_map(h, w, seed):
    """0 / 255 bytes, about one in three set: bicubic overshoot on both sides."""
    return ((np.random.default_rng(seed).random((h, w)) < 0.35) * 255).astype(np.uint8)


def boundary_values() -> list:
    """Map values at and one float32 ulp either side of the byte boundaries k / 255, and the ends of the domain."""
    vals = [0.0, 1.0, 1.0 + 2.0 ** -23, 1.0 + 2.0 ** -22]
    for k in (1, 2, 3, 51, 85, 127, 128, 170, 200, 254, 255):
        c = np.float32(k) / np.float32(255)
        vals += [np.nextafter(c, np.float32(0)), c, np.nextafter(c, np.float32(2))]
    return vals


def exhaustive_case():
    """256 entries of 16 x 16 at S = 16 (no resize): the map's byte is the pixel index, the table is the identity
    in every band and frame e is the constant e -- every (table byte, frame byte) pair once per band."""
    maps = ((np.arange(256, dtype=np.float32) + np.float32(0.5)) / np.float32(255)).reshape(16, 16)
    assert np.array_equal(quantise(maps).reshape(-1), np.arange(256))
    lut = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    frames = np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None, None, None], (256, 16, 16, 3)).copy()
    return maps, frames, lut
