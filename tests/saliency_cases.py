"""Inputs shared by tests/test_saliency_cpu.py and tests/test_gpu_saliency.py: the size / T / percentile grids of
the attribution-image tests, seeded maps that meet all three normalisation rules, and the recorded fixtures."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from golden_util import GOLDEN_DIR

SALIENCY_DIR = os.path.join(GOLDEN_DIR, "saliency")
# 1 x 1 and 1 x 2: no upper neighbour / one; 8 x 8: one wave's worth; 5 x 13: one past it; 64 x 64: many blocks
SIZES = [(1, 1), (1, 2), (7, 9), (8, 8), (5, 13), (16, 16), (64, 64)]
COUNTS = [0, 1, 3, 12]                 # 12 wraps the ten-colour palette
PERCENTILES = [0, 50, 98, 99, 100]
END_TO_END = ("pipnet_mid_addon", "count_onehot")


def load_saliency(name: str):
    z = np.load(os.path.join(SALIENCY_DIR, name + ".npz"), allow_pickle=False)
    rec = {k: z[k] for k in z.files}
    return json.loads(str(rec.pop("meta"))), rec


def sample_maps(t: int, h: int, w: int, seed: int = 0) -> np.ndarray:
    """[t,3,h,w] float32 maps of mixed sign.  Map 1 (where there is one) has a range below 1e-3 but above 1e-5,
    map 2 is constant, the others have the scale of real attributions; between them the three rules."""
    g = np.random.default_rng(1000 * seed + 100 * t + 10 * h + w)
    maps = (g.standard_normal((t, 3, h, w)) * 0.02).astype(np.float32)
    if t > 1:
        maps[1] = (0.05 + g.standard_normal((3, h, w)) * 2e-5).astype(np.float32)
    if t > 2:
        maps[2] = np.float32(-0.125)
    return maps


def direct_contributions(net, x: torch.Tensor, noise) -> torch.Tensor:
    """interpret_idg.py:319-366 on a CPU module's own forward: [K, P] weighted activations of every class."""
    from count_pipnet_amd.attribution import _gumbel_module
    from count_pipnet_amd.backend import torch_backend
    from count_pipnet_amd.count_pipnet_utils import OneHotEncoder
    act = _gumbel_module(net)
    with torch.no_grad(), torch_backend():
        if not hasattr(net, "_max_count"):
            _, pooled, _ = net(x.unsqueeze(0))
            return pooled.squeeze(0) * net._classification.weight
        prev = act.exp_noise
        act.exp_noise = noise
        try:
            _, clamped, _ = net(x.unsqueeze(0), inference=True)
        finally:
            act.exp_noise = prev
        scalars = net._intermediate(clamped).squeeze(0) if isinstance(net._intermediate, OneHotEncoder) else None
        clamped = clamped.squeeze(0)
        weights = torch.zeros((net._num_classes, net._num_prototypes))
        for i in range(clamped.shape[0]):
            weights[:, i] = net.get_prototype_importance_per_class(i, scalars)
        return clamped * weights


def decisive_choice(contrib: torch.Tensor):
    """(class, threshold) with at least two kept prototypes and every contribution >= 2e-3 from the threshold."""
    for c in range(contrib.shape[0]):
        v = torch.sort(contrib[c]).values
        for j in range(len(v) - 2, 0, -1):              # at least two above the gap
            if float(v[j] - v[j - 1]) >= 4e-3 and float(v[j - 1]) >= 0:
                return c, float(v[j - 1] + v[j]) / 2
    raise AssertionError("no decisive (class, threshold) on this fixture")


def selection_noise(noise, steps: int = 8):
    """The Exp(1) draw for the selection forward of a Gumbel net: the one the attribution fixture used at the path's
    last step, which is the image itself -- its generator held every pixel's top-two gap of that forward >= 1e-3."""
    return None if noise is None else noise[steps - 1:steps]


def as_tensor(a: np.ndarray, device=None) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(device or "cpu")


def same_bits(got: torch.Tensor, want: np.ndarray) -> bool:
    """Equal dtype, shape and bit patterns (NaN-free data: array_equal, plus the sign of zeros)."""
    g = got.detach().cpu().numpy()
    if g.dtype != want.dtype or g.shape != want.shape or not np.array_equal(g, want):
        return False
    return g.dtype.kind != "f" or np.array_equal(np.signbit(g), np.signbit(want))
