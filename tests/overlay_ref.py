"""The ``*_overlay.png`` arrays of util/vis_pipnet.py:454-475 (PIP-Net) / :1000-1021 (CountPIPNet), restated in
numpy -- the reference side of tests/test_gpu_overlay.py.  tests/test_overlay_cpu.py holds every step against the
statements the reference itself runs (``scipy.ndimage.zoom``, ``cmap(value)`` of matplotlib's viridis).

    c       = spline_filter(m, order=3) in float64          mirror boundary, axis 0 first, then axis 1
    resized = float32(sum of 4 x 4 taps of c)               zoom(m, (S / h, S / w)): order 3, mode 'constant',
                                                            grid_mode False, so the step is (n - 1) / (S - 1)
    mask    = resized > 0.1f
    colour  = min(trunc(resized * 256f), 255), 0 off the mask
    overlay = (lut[colour], alpha) on the mask, zeros elsewhere, float64

Every operation is one IEEE operation on doubles (float32 for the last three lines) in a stated order; scalar
Python floats are doubles and never contracted.  Also the two rules that pick the entries a prototype's
``feature_maps/prototype_{p}`` folder shows (:362-391, :897-922), from the reference's statements.
"""
import math

import numpy as np

Z = math.sqrt(3.0) - 2.0                       # the pole of the cubic B-spline
GAIN = (1.0 - Z) * (1.0 - 1.0 / Z)
THRESHOLD = np.float32(0.1)
ALPHA = 0.7


# ---- prefilter ------------------------------------------------------------------------------------------------
def filter_lines(c: np.ndarray) -> None:
    """The order-3 prefilter along axis 0 of the float64 array ``c`` [n, lines], in place: every column is one
    line, all of them advanced together (elementwise numpy operations are one IEEE operation per element)."""
    n = c.shape[0]
    z = Z
    c *= GAIN
    zn = math.pow(z, n - 1)
    c[0] = c[0] + zn * c[n - 1]
    zi = z
    for i in range(1, n - 1):
        c[0] += zi * (c[i] + zn * c[n - 1 - i])
        zi *= z
    c[0] /= 1.0 - zn * zn
    for i in range(1, n):
        c[i] += z * c[i - 1]
    c[n - 1] = (z * c[n - 2] + c[n - 1]) * z / (z * z - 1.0)
    for i in range(n - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])


def prefilter(m: np.ndarray) -> np.ndarray:
    """``spline_filter(m, order=3, mode='mirror')`` of a float32 [h, w] map, float64: axis 0, then axis 1."""
    c = np.array(m, dtype=np.float64)
    assert c.ndim == 2 and min(c.shape) >= 3
    filter_lines(c)                             # axis 0: the columns
    ct = np.ascontiguousarray(c.T)
    filter_lines(ct)                            # axis 1: the rows
    return np.ascontiguousarray(ct.T)


# ---- zoom -----------------------------------------------------------------------------------------------------
def taps(n: int, s: int):
    """(index [s, 4] int64, weight [s, 4] float64) of the four taps of every output coordinate of an axis
    resized n -> s."""
    zoom = (n - 1) / (s - 1)
    x = np.arange(s, dtype=np.float64) * zoom
    f = np.floor(x)
    y = x - f
    t = 1.0 - y
    w0 = t * t * t / 6.0
    w1 = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0
    w2 = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0
    w3 = 1.0 - w0 - w1 - w2
    idx = f.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :]
    idx = np.where(idx < 0, -idx, idx)
    idx = np.where(idx >= n, 2 * (n - 1) - idx, idx)
    assert idx.min() >= 0 and idx.max() < n
    return idx, np.stack([w0, w1, w2, w3], axis=1)


def zoom(m: np.ndarray, size: int) -> np.ndarray:
    """``scipy.ndimage.zoom(m, (size / h, size / w))`` of a float32 [h, w] map: float32 [size, size]."""
    m = np.asarray(m)
    assert m.dtype == np.float32 and size >= 2
    h, w = m.shape
    c = prefilter(m)
    iy, wy = taps(h, size)
    ix, wx = taps(w, size)
    s = np.zeros((size, size), dtype=np.float64)
    for a in range(4):
        for b in range(4):
            v = c[iy[:, a][:, None], ix[:, b][None, :]]
            v = v * wy[:, a][:, None]
            v = v * wx[:, b][None, :]
            s = s + v
    return s.astype(np.float32)


# ---- threshold, colour, overlay -----------------------------------------------------------------------------------
def mask_of(resized: np.ndarray) -> np.ndarray:
    return np.asarray(resized, dtype=np.float32) > THRESHOLD


def colour_of(resized: np.ndarray) -> np.ndarray:
    """The row of matplotlib's 256-entry table ``cmap(value)`` reads for a float32 value above 0.1: the value
    times 256, truncated, 1.0 and everything above reading the last row; 0 off the mask."""
    r = np.asarray(resized, dtype=np.float32)
    scaled = np.minimum(r * np.float32(256), np.float32(255))
    idx = np.trunc(np.where(mask_of(r), scaled, np.float32(0))).astype(np.uint8)
    return idx


def overlay_of(resized: np.ndarray, lut: np.ndarray, alpha: float = ALPHA) -> np.ndarray:
    """float64 [..., 4]: ``(*cmap(v)[:3], alpha)`` on the mask, zeros elsewhere.  ``lut`` [256, 3] float64."""
    lut = np.asarray(lut, dtype=np.float64)
    assert lut.shape == (256, 3)
    mask, colour = mask_of(resized), colour_of(resized)
    out = np.zeros(mask.shape + (4,), dtype=np.float64)
    out[..., :3] = lut[colour]
    out[..., 3] = alpha
    out[~mask] = 0.0
    return out


def render(m: np.ndarray, lut: np.ndarray, size: int, alpha: float = ALPHA):
    """dict(resized, mask (uint8), colour, overlay) of one float32 map."""
    r = zoom(m, size)
    return dict(resized=r, mask=mask_of(r).astype(np.uint8), colour=colour_of(r), overlay=overlay_of(r, lut, alpha))


# ---- selection --------------------------------------------------------------------------------------------------
def pipnet_map_selection(scores, index, selected, unused, max_feature_maps_per_prototype=3):
    """vis_pipnet.py:362-391 over ``scores`` / ``index`` [P][1][k] lists: {p: [(group position, slot), ...]} in file
    order (``rank_{i+1}``).  ``prototype_storage`` holds the selected prototypes' stored images in slot order."""
    prototype_storage = {p: [dict(score=scores[p][0][j], slot=j) for j in range(len(index[p][0])) if index[p][0][j] >= 0]
                         for p in range(len(index)) if selected[p]}
    prototypes_not_used = [p for p in range(len(index)) if unused[p]]
    shown = {}
    for p, images in prototype_storage.items():
        if p in prototypes_not_used or len(images) == 0:
            continue
        selected_indices = []
        selected_indices.append(0)
        if len(images) > 2:
            selected_indices.append(len(images) // 2)
        if len(images) > 1:
            lowest_idx = len(images) - 1
            while lowest_idx > 0 and images[lowest_idx]['score'] < 0.1:
                lowest_idx -= 1
            if lowest_idx not in selected_indices:
                selected_indices.append(lowest_idx)
        selected_indices = selected_indices[:max_feature_maps_per_prototype]
        shown[p] = [(0, images[idx]['slot']) for idx in selected_indices]
    return shown


def count_map_selection(scores, index, groups, selected, max_feature_maps_per_prototype=3):
    """vis_pipnet.py:897-922 over ``scores`` / ``index`` [P][G][k] lists (``groups`` = the count of each group
    position, ascending): {p: [(group position, slot), ...]} in file order."""
    prototype_selected_images = {}
    for p in range(len(index)):
        if not selected[p]:
            continue
        prototype_selected_images[p] = []
        for g, count in enumerate(groups):
            prototype_selected_images[p].extend(
                [dict(count_group=count, model_count=scores[p][g][j], entry=(g, j))
                 for j in range(len(index[p][g])) if index[p][g][j] >= 0])
    prototypes_not_used = [p for p, images in prototype_selected_images.items() if len(images) == 0]
    shown = {}
    for p, images in prototype_selected_images.items():
        if p in prototypes_not_used or len(images) == 0:
            continue
        count_groups = {}
        for img_data in images:
            count = img_data['count_group']
            if count not in count_groups:
                count_groups[count] = []
            count_groups[count].append(img_data)
        selected_images = []
        for count, count_images in sorted(count_groups.items()):
            if len(count_images) > 0:
                sorted_images = sorted(count_images, key=lambda x: x['model_count'], reverse=True)
                selected_images.append(sorted_images[0])
        selected_images = selected_images[:max_feature_maps_per_prototype]
        shown[p] = [img_data['entry'] for img_data in selected_images]
    return shown


def map_selection(res, max_per_prototype=3):
    """{p: entries} of a host PrototypeTopK."""
    scores, index = res.scores.tolist(), res.index.tolist()
    if res.groups == [None]:
        return pipnet_map_selection(scores, index, res.selected.tolist(), res.unused.tolist(), max_per_prototype)
    return count_map_selection(scores, index, res.groups, res.selected.tolist(), max_per_prototype)
