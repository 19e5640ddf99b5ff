"""Training-augmentation policies and host-side parameter sampling (util/data.py:261-657).

The reference augments every training image in a DataLoader worker with torchvision /
kornia transforms.  Here the pixels are transformed on the device
(``csrc/augment_ops.hip``) and only the random *parameters* -- a few dozen numbers per image --
are drawn on the host, per batch, and shipped in two small float64 tables (layout:
include/pipnet_amd.h).

The distributions below are restated from torchvision >= 0.13 (``transforms.autoaugment.
TrivialAugmentWide``, ``transforms.RandomRotation / RandomAffine / RandomResizedCrop /
RandomCrop / RandomHorizontalFlip / ColorJitter`` and ``functional._get_inverse_affine_matrix``)
and kornia's ``RandomGaussianNoise``; neither library is a dependency, so the restatement could
not be run against them, and torchvision's RNG *stream* is not reproduced -- only its
distributions.  The operation spaces are the reference's own subclasses (util/data.py:620-657).

Every image draws from its own stream, seeded by (generator seed, image id), so the parameters
of an image do not depend on how the images are batched.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from ._lib import CONSTANTS

GEOM_PARAMS, VIEW_PARAMS = CONSTANTS["AUG_GEOM_PARAMS"], CONSTANTS["AUG_VIEW_PARAMS"]
WARP_NONE, WARP_FIXED, WARP_DOUBLE = 0, 1, 2
(OP_IDENTITY, OP_BRIGHTNESS, OP_COLOR, OP_CONTRAST, OP_SHARPNESS, OP_POSTERIZE, OP_SOLARIZE, OP_AUTOCONTRAST,
 OP_EQUALIZE) = range(9)
NUM_BINS = 31                                  # TrivialAugmentWide(num_magnitude_bins=31)
NOISE_STD = 0.1                                # RandomGaussianNoise(mean=0, std=0.1, p=0.5)


def _lin(lo: float, hi: float) -> List[float]:
    return [float(v) for v in torch.linspace(lo, hi, NUM_BINS)]


_POSTERIZE_BITS = [float(v) for v in (8 - (torch.arange(NUM_BINS) / ((NUM_BINS - 1) / 6)).round().int())]

# name -> (magnitudes or None for a parameterless operation, signed): util/data.py:620-657
GEOMETRIC_SPACE: Dict[str, Tuple[Optional[List[float]], bool]] = {      # TrivialAugmentWideNoColor
    "Identity": (None, False),
    "ShearX": (_lin(0.0, 0.5), True),
    "ShearY": (_lin(0.0, 0.5), True),
    "TranslateX": (_lin(0.0, 16.0), True),
    "TranslateY": (_lin(0.0, 16.0), True),
    "Rotate": (_lin(0.0, 60.0), True),
}
COLOUR_SPACE: Dict[str, Tuple[Optional[List[float]], bool]] = {         # TrivialAugmentWideNoShape
    "Identity": (None, False),
    "Brightness": (_lin(0.0, 0.5), True),
    "Color": (_lin(0.0, 0.02), True),
    "Contrast": (_lin(0.0, 0.5), True),
    "Sharpness": (_lin(0.0, 0.5), True),
    "Posterize": (_POSTERIZE_BITS, False),
    "AutoContrast": (None, False),
    "Equalize": (None, False),
}
COLOUR_SPACE_WITH_COLOR: Dict[str, Tuple[Optional[List[float]], bool]] = {   # ...NoShapeWithColor
    "Identity": (None, False),
    "Brightness": (_lin(0.0, 0.5), True),
    "Color": (_lin(0.0, 0.5), True),
    "Contrast": (_lin(0.0, 0.5), True),
    "Sharpness": (_lin(0.0, 0.5), True),
    "Posterize": (_POSTERIZE_BITS, False),
    "Solarize": (_lin(255.0, 0.0), False),
    "AutoContrast": (None, False),
    "Equalize": (None, False),
}
OP_CODES = {"Identity": OP_IDENTITY, "Brightness": OP_BRIGHTNESS, "Color": OP_COLOR, "Contrast": OP_CONTRAST,
            "Sharpness": OP_SHARPNESS, "Posterize": OP_POSTERIZE, "Solarize": OP_SOLARIZE,
            "AutoContrast": OP_AUTOCONTRAST, "Equalize": OP_EQUALIZE}


@dataclass(frozen=True)
class Policy:
    """One ``get_*`` of util/data.py: transform1 = Resize(size + pad1) -> ``geometric`` ->
    [flip] -> RandomResizedCrop(S2, scale=(0.95, 1)); transform2 = ``colour`` -> RandomCrop(size)
    -> [Grayscale(3)] -> ToTensor -> [noise] -> Normalize."""
    name: str
    pad1: int                      # S1 - size
    pad2: int                      # S2 - size (ignored when crop2 is set)
    geometric: str                 # "trivial" | "rotation" | "affine"
    colour: str                    # "trivial" | "trivial_color" | "jitter"
    flip: bool
    grayscale: bool = False
    noise: bool = False
    crop2: Optional[int] = None    # a fixed S2 whatever the image size

    def sizes(self, size: int) -> Tuple[int, int]:
        s1 = size + self.pad1
        s2 = self.crop2 if self.crop2 is not None else size + self.pad2
        if s2 < size:
            raise ValueError(f"policy {self.name}: RandomCrop({size}) does not fit the {s2}x{s2} image")
        return s1, s2


# keyed by get_data's dataset strings (util/data.py:32-107); '-pretrain' is get_birds' transform1p
POLICIES: Dict[str, Policy] = {p.name: p for p in (
    Policy("pets", 48, 8, "trivial", "trivial", True),
    Policy("partimagenet", 48, 8, "trivial", "trivial", True),
    Policy("CUB-200-2011", 8, 4, "trivial", "trivial", True),
    Policy("CUB-200-2011-pretrain", 32, 4, "trivial", "trivial", True),
    Policy("CARS", 32, 4, "trivial", "trivial_color", True),
    # the reference crops RandomResizedCrop(224 + 8) whatever img_size is (util/data.py:581)
    Policy("grayscale_example", 32, 8, "trivial", "trivial", True, grayscale=True, crop2=224 + 8),
    Policy("geometric_shapes", 32, 8, "rotation", "jitter", False),
    Policy("geometric_shapes_gaussian_noise", 32, 8, "rotation", "jitter", False, noise=True),
    Policy("geometric_shapes_224_gaussian_noise", 32, 8, "rotation", "jitter", False, noise=True),
    Policy("mnist_counting", 24, 8, "affine", "jitter", False),
)}


def get_policy(policy) -> Policy:
    if isinstance(policy, Policy):
        return policy
    if policy not in POLICIES:
        raise KeyError(f"unknown augmentation policy {policy!r}; known: {', '.join(POLICIES)}")
    return POLICIES[policy]


class AugmentParams(NamedTuple):
    geom: torch.Tensor     # [B, 13] float64 (host)
    view: torch.Tensor     # [V, B, 8] float64 (host)


# ---- matrices (host, Python doubles) ----------------------------------------------------------

def affine_inverse_matrix(center: Sequence[float], angle: float, translate: Sequence[float], scale: float,
                          shear: Sequence[float]) -> List[float]:
    """torchvision ``_get_inverse_affine_matrix``: the output -> input matrix that ``F.affine``
    hands to ``Image.transform(AFFINE)``."""
    rot, sx, sy = math.radians(angle), math.radians(shear[0]), math.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [d, -b, 0.0, -c, a, 0.0]
    m = [x / scale for x in m]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def rotate_matrix(angle: float, w: int, h: int) -> Optional[List[float]]:
    """Pillow ``Image.rotate(angle, expand=False, center=None)``'s matrix; None when Pillow
    returns a copy (angle % 360 == 0)."""
    angle = angle % 360.0
    if angle == 0:
        return None
    r = -math.radians(angle)
    m = [round(math.cos(r), 15), round(math.sin(r), 15), 0.0, round(-math.sin(r), 15), round(math.cos(r), 15), 0.0]
    cx, cy = w / 2.0, h / 2.0
    m[2] = m[0] * (-cx) + m[1] * (-cy) + cx
    m[5] = m[3] * (-cx) + m[4] * (-cy) + cy
    return m


def warp_row(m: Optional[Sequence[float]], fill: int) -> List[float]:
    """(path, m0..m5, fill) of a ``gparams`` row: Pillow's affine takes its fixed-point loop
    unless m1 == m3 == 0."""
    if m is None:
        return [float(WARP_NONE), 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, float(fill)]
    path = WARP_FIXED if (m[1] != 0 or m[3] != 0) else WARP_DOUBLE
    return [float(path)] + [float(v) for v in m] + [float(fill)]


def geometric_matrix(op: str, magnitude: float, size: int) -> Optional[List[float]]:
    """TrivialAugmentWide ``_apply_op`` for a geometric operation on a size x size PIL image."""
    c = [size * 0.5, size * 0.5]
    if op == "Identity":
        return None
    if op == "ShearX":
        return affine_inverse_matrix([0.0, 0.0], 0.0, [0, 0], 1.0, [math.degrees(math.atan(magnitude)), 0.0])
    if op == "ShearY":
        return affine_inverse_matrix([0.0, 0.0], 0.0, [0, 0], 1.0, [0.0, math.degrees(math.atan(magnitude))])
    if op == "TranslateX":
        return affine_inverse_matrix(c, 0.0, [int(magnitude), 0], 1.0, [0.0, 0.0])
    if op == "TranslateY":
        return affine_inverse_matrix(c, 0.0, [0, int(magnitude)], 1.0, [0.0, 0.0])
    if op == "Rotate":
        return rotate_matrix(magnitude, size, size)
    raise ValueError(op)


def colour_param(op: str, magnitude: float) -> float:
    """The kernel's parameter of a colour operation: the ImageEnhance factor 1 + magnitude,
    Posterize's bits, Solarize's threshold."""
    if op in ("Brightness", "Color", "Contrast", "Sharpness"):
        return 1.0 + magnitude
    if op == "Posterize":
        return float(int(magnitude))
    if op == "Solarize":
        return float(magnitude)
    return 0.0


# ---- sampling ---------------------------------------------------------------------------------

class _Stream:
    """Uniform draws of one image: its own generator, seeded by (seed, image id)."""

    def __init__(self, seed: int, image_id: int):
        z = (seed * 0x9E3779B97F4A7C15 + (image_id + 1) * 0xBF58476D1CE4E5B9) & ((1 << 64) - 1)
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & ((1 << 64) - 1)       # splitmix64 finaliser
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & ((1 << 64) - 1)
        z ^= z >> 31
        self.g = torch.Generator().manual_seed(z & ((1 << 63) - 1))
        self.buf: List[float] = []

    def rand(self) -> float:
        if not self.buf:
            self.buf = torch.rand(64, dtype=torch.float64, generator=self.g).tolist()[::-1]
        return self.buf.pop()

    def uniform(self, lo: float, hi: float) -> float:
        return lo + (hi - lo) * self.rand()

    def randint(self, n: int) -> int:
        """Uniform integer in [0, n)."""
        return min(int(self.rand() * n), n - 1)


def trivial_augment(space: Dict[str, Tuple[Optional[List[float]], bool]], st: _Stream) -> Tuple[str, float]:
    """TrivialAugmentWide.forward's draw: one operation uniformly, its magnitude uniformly from
    the 31 bins, negated with probability 1/2 when the operation is signed."""
    names = list(space)
    op = names[st.randint(len(names))]
    mags, signed = space[op]
    mag = mags[st.randint(len(mags))] if mags is not None else 0.0
    if signed and st.randint(2):
        mag *= -1.0
    return op, mag


def random_resized_crop_box(height: int, width: int, st: _Stream, scale=(0.95, 1.0),
                            ratio=(3.0 / 4.0, 4.0 / 3.0)) -> Tuple[int, int, int, int]:
    """RandomResizedCrop.get_params -> (top, left, height, width)."""
    area = height * width
    log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
    for _ in range(10):
        target = area * st.uniform(scale[0], scale[1])
        aspect = math.exp(st.uniform(log_ratio[0], log_ratio[1]))
        w = int(round(math.sqrt(target * aspect)))
        h = int(round(math.sqrt(target / aspect)))
        if 0 < w <= width and 0 < h <= height:
            return st.randint(height - h + 1), st.randint(width - w + 1), h, w
    in_ratio = float(width) / float(height)            # fallback: central crop
    if in_ratio < min(ratio):
        w = width
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = height
        w = int(round(h * max(ratio)))
    else:
        w, h = width, height
    return (height - h) // 2, (width - w) // 2, h, w


def _geom_row(p: Policy, s1: int, st: _Stream) -> List[float]:
    if p.geometric == "trivial":
        op, mag = trivial_augment(GEOMETRIC_SPACE, st)
        row = warp_row(geometric_matrix(op, mag, s1), 0)
    elif p.geometric == "rotation":                    # RandomRotation(10, fill=255)
        row = warp_row(rotate_matrix(st.uniform(-10.0, 10.0), s1, s1), 255)
    elif p.geometric == "affine":                      # RandomAffine(10, (.1, .1), (.9, 1.1), fill=255)
        angle = st.uniform(-10.0, 10.0)
        tx = int(round(st.uniform(-0.1 * s1, 0.1 * s1)))
        ty = int(round(st.uniform(-0.1 * s1, 0.1 * s1)))
        sc = st.uniform(0.9, 1.1)
        row = warp_row(affine_inverse_matrix([s1 * 0.5, s1 * 0.5], angle, [tx, ty], sc, [0.0, 0.0]), 255)
    else:
        raise ValueError(p.geometric)
    flip = 1.0 if (p.flip and st.rand() < 0.5) else 0.0
    return row + [flip] + [float(v) for v in random_resized_crop_box(s1, s1, st)]


def _view_row(p: Policy, s2: int, size: int, st: _Stream, image_id: int) -> List[float]:
    if p.colour == "jitter":                           # ColorJitter(brightness=.1, contrast=.1)
        order = torch.tensor([st.rand() for _ in range(4)]).argsort().tolist()    # randperm(4)
        fb, fc = st.uniform(0.9, 1.1), st.uniform(0.9, 1.1)
        ops = [(OP_BRIGHTNESS, fb) if k == 0 else (OP_CONTRAST, fc) for k in order if k in (0, 1)]
    else:
        op, mag = trivial_augment(COLOUR_SPACE if p.colour == "trivial" else COLOUR_SPACE_WITH_COLOR, st)
        ops = [(OP_CODES[op], colour_param(op, mag)), (OP_IDENTITY, 0.0)]
    top, left = st.randint(s2 - size + 1), st.randint(s2 - size + 1)
    noisy = 1.0 if (p.noise and st.rand() < 0.5) else 0.0
    return [float(ops[0][0]), ops[0][1], float(ops[1][0]), ops[1][1], float(top), float(left), noisy,
            float(image_id % (1 << 31))]


def sample_params(policy, size: int, n: int, generator: Optional[torch.Generator] = None, first_id: int = 0,
                  views: int = 2) -> AugmentParams:
    """Parameters of ``n`` images with ids first_id .. first_id + n - 1 under ``policy`` at image
    size ``size``.  The stream of an image depends on ``generator.initial_seed()`` and its id
    only: sampling 8 images at once or as 4 + 4 gives the same rows."""
    p = get_policy(policy)
    s1, s2 = p.sizes(int(size))
    seed = int(generator.initial_seed()) if generator is not None else int(torch.initial_seed())
    geom = torch.zeros((n, GEOM_PARAMS), dtype=torch.float64)
    view = torch.zeros((views, n, VIEW_PARAMS), dtype=torch.float64)
    for k in range(n):
        st = _Stream(seed, first_id + k)
        geom[k] = torch.tensor(_geom_row(p, s1, st), dtype=torch.float64)
        for v in range(views):
            view[v, k] = torch.tensor(_view_row(p, s2, int(size), st, first_id + k), dtype=torch.float64)
    return AugmentParams(geom, view)
