"""Helpers for the attribution fixtures recorded from the reference (tests/golden/gen_golden_attr.py)."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from count_pipnet_amd.synthetic import synth_exponential, synth_images
from golden_util import GOLDEN_DIR

ATTR_DIR = os.path.join(GOLDEN_DIR, "attr")
KINDS = ("prototype", "class")
METHODS = ("ig", "lig", "idg")


def attr_names():
    return sorted(f[:-4] for f in os.listdir(ATTR_DIR) if f.endswith(".npz"))


def load_attr(name: str):
    z = np.load(os.path.join(ATTR_DIR, name + ".npz"), allow_pickle=False)
    rec = {k: z[k] for k in z.files}
    meta = json.loads(str(rec.pop("meta")))
    return meta, rec


def attr_image(meta) -> torch.Tensor:
    c = meta["case"]
    x = synth_images(1, c["size"], seed=meta["image_seed"])[0]
    assert abs(float(x.double().sum()) - meta["input_sum"]) < 1e-6 * max(1.0, meta["input_abs"]), \
        "synthetic input generator drifted from the recorded fixture"
    return x


def attr_noise(meta):
    """The reference's Exp(1) draws of one attribution run, concatenated in call order
    ([passes * steps, P, h, w]; the ig / lig runs consume the first ``steps``); None for nets
    without Gumbel noise."""
    if not meta["noise_draws"]:
        return None
    return torch.cat([synth_exponential(tuple(meta["noise_shape"]), meta["noise_seed"] + k)
                      for k in range(meta["noise_draws"])])


def rel_err(a: torch.Tensor, ref64: np.ndarray) -> float:
    """max|A - R64| / max|R64|."""
    r = torch.from_numpy(ref64).double()
    return float((a.detach().cpu().double() - r).abs().max() / r.abs().max())
