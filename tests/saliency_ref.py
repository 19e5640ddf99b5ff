"""numpy restatement of the attribution-image steps of util/interpret_idg.py, the standard of
tests/test_saliency_cpu.py and tests/test_gpu_saliency.py.

Every function says in this project's own words what the reference's statements compute under numpy 2.2.6 and
torch; tests/test_saliency_cpu.py holds them bit for bit against tests/golden/saliency/*.npz, which the
reference's own statements wrote (tests/golden/gen_golden_saliency.py).  The percentile is written out --
``np.partition`` and the explicit interpolation -- and never delegates to ``np.percentile``, so the standard
does not move with the numpy of the machine that runs the tests.
"""
from __future__ import annotations

import numpy as np

PALETTE = ["#636EFA", "#EF553B", "#00CC96", "#AB63FA", "#FFA15A", "#19D3F3", "#FF6692", "#B6E880", "#FF97FF", "#FECB52"]
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
F32 = np.float32


def fold(maps: np.ndarray) -> np.ndarray:
    """[T,3,H,W] -> [T,H,W]: np.sum(np.abs(.), axis=2) of the [H,W,3] view, a three-term sum in channel order."""
    a = np.abs(maps.astype(F32))
    return (a[:, 0] + a[:, 1]) + a[:, 2]


def percentile_split(n: int, q: float):
    """(k, k + 1 clipped, gamma float32) of np.percentile's virtual index on a float32 array: numpy 2.2.6 divides
    q by float32(100) and multiplies by n - 1 in float32; at or past the last element both neighbours are the
    last element and gamma keeps index - (-1)."""
    index = F32(n - 1) * (F32(q) / F32(100))
    if index >= F32(n - 1):
        return n - 1, n - 1, F32(np.float64(index) + 1.0)
    k = int(np.floor(index))
    return k, k + 1, F32(np.float64(index) - k)


def lerp(lo: F32, hi: F32, gamma: F32) -> F32:
    """numpy's _lerp in float32: lo + (hi - lo) * gamma, replaced by hi - (hi - lo) * (1 - gamma) from gamma 0.5."""
    d = F32(hi - lo)
    if gamma >= 0.5:
        return F32(hi - F32(d * F32(F32(1) - gamma)))
    return F32(lo + F32(d * gamma))


def order_stats(folded: np.ndarray, q: float):
    """Per map (vmin, vtop, lo, hi, vq) float32 [T]: the extremes, the two order statistics around the q-th
    percentile (np.partition) and their interpolation."""
    t = folded.shape[0]
    n = folded.shape[1] * folded.shape[2]
    flat = folded.reshape(t, n).astype(F32)
    k, k1, gamma = percentile_split(n, q)
    out = np.zeros((5, t), dtype=F32)
    for i in range(t):
        part = np.partition(flat[i], sorted({0, k, k1, n - 1}))
        lo, hi = part[k], part[k1]
        out[:, i] = (part[0], part[n - 1], lo, hi, lerp(lo, hi, gamma))
    return tuple(out)


def normalize(folded: np.ndarray, vmin: np.ndarray, vq: np.ndarray, vtop: np.ndarray, fallback: bool = True):
    """(rule int32 [T], normalized float32 [T,H,W]) -- normalize_attribution_map (:183-204), or logit mode
    (:632-635) without ``fallback``; the two range tests compare float32 with float32."""
    t = folded.shape[0]
    rule = np.zeros(t, dtype=np.int32)
    norm = np.zeros(folded.shape, dtype=F32)
    for i in range(t):
        x = folded[i].astype(F32)
        den = F32(vq[i] - vmin[i])
        if fallback:
            if not den > F32(1e-3):
                den = F32(vtop[i] - vmin[i])
                rule[i] = 1 if den > F32(1e-5) else 2
        elif vq[i] == vmin[i]:
            rule[i] = 2                      # the reference divides by zero here; this project writes a zero map
        if rule[i] != 2:
            norm[i] = np.clip((x - F32(vmin[i])) / den, 0, 1)
    return rule, norm


def normalize_maps(maps: np.ndarray, q: float, fallback: bool = True):
    """dict of every field of saliency.SaliencyMaps for [T,3,H,W] or folded [T,H,W] maps."""
    folded = fold(maps) if maps.ndim == 4 else maps.astype(F32)
    if folded.shape[0] == 0:
        e = np.zeros(0, dtype=F32)
        return dict(folded=folded, vmin=e, vq=e, vtop=e, rule=np.zeros(0, dtype=np.int32), normalized=folded.copy())
    vmin, vtop, _, _, vq = order_stats(folded, q)
    rule, norm = normalize(folded, vmin, vq, vtop, fallback)
    return dict(folded=folded, vmin=vmin, vq=vq, vtop=vtop, rule=rule, normalized=norm)


def palette(count: int) -> np.ndarray:
    """[count,3] float64: the hex triples / 255.0, reused modulo ten (:420-421)."""
    table = np.zeros((count, 3), dtype=np.float64)
    for i in range(count):
        code = PALETTE[i % len(PALETTE)]
        table[i] = [int(code[k:k + 2], 16) / 255.0 for k in (1, 3, 5)]
    return table


def blend(normalized: np.ndarray, colours: np.ndarray = None) -> np.ndarray:
    """[H,W,4] float64: colour-weighted sum of the maps in order, clipped, with the running maximum as alpha."""
    t, h, w = normalized.shape
    colours = palette(t) if colours is None else colours
    rgb = np.zeros((h, w, 3), dtype=np.float64)
    alpha = np.zeros((h, w, 1), dtype=np.float64)
    for i in range(t):
        v = normalized[i].astype(np.float64)[..., None]
        rgb = rgb + colours[i] * v
        alpha = np.maximum(alpha, v)
    return np.concatenate((np.clip(rgb, 0, 1), alpha), axis=-1)


def unnormalize(x: np.ndarray, mean=MEAN, std=STD) -> np.ndarray:
    """[3,H,W] float32 -> [H,W,3] float32 clip(x * std + mean, 0, 1): two float32 roundings per value."""
    m = np.array(mean, dtype=np.float64).astype(F32).reshape(3, 1, 1)
    s = np.array(std, dtype=np.float64).astype(F32).reshape(3, 1, 1)
    prod = (x.astype(F32) * s).astype(F32)
    return np.clip(np.transpose((prod + m).astype(F32), (1, 2, 0)), 0, 1)


def colormap(normalized: np.ndarray, lut: np.ndarray) -> np.ndarray:
    """[...,4] uint8: byte-table entry min(int(v * 256), 255) of every v in [0, 1]."""
    idx = np.minimum((normalized.astype(F32) * F32(256)).astype(np.int64), 255)
    return lut[np.maximum(idx, 0)]


def active(contributions: np.ndarray, threshold: float):
    """Indices with contribution > threshold (float32 against float32, as torch compares), largest first, equal
    values in ascending index order."""
    keep = np.nonzero(contributions > F32(threshold))[0]
    return keep[np.argsort(-contributions[keep].astype(np.float64), kind="stable")].tolist()
