"""Generate the attribution-image fixtures under tests/golden/saliency/ from the REFERENCE's own statements.

Runs only where the reference checkout exists (as gen_golden.py).  ``normalize_attribution_map`` is compiled from
the source of ``util/interpret_idg.py`` at run time (the module itself cannot be imported: it imports plotting
packages and looks for its checkout's directory name), the way gen_golden_attr.py takes ``ATTR_FUNC``; the inline
statements around it -- the fold (:413-415), the additive blend (:419-427, :454-457), the un-normalised image
(:442-446) and logit mode (:627-641, ``matplotlib.pyplot.imsave`` into a buffer) -- are restated here with numpy,
torch, plotly's palette and matplotlib as installed.  Nothing of the reference is written to this tree.

  steps.npz   seeded synthetic maps through every step: the three normalisation rules (a map with percentile
              range > 1e-3, one with percentile range <= 1e-3 but global range > 1e-5, a constant map), the blend
              of three maps, an un-normalised image, the ``Blues`` bytes of a logit map and the byte table itself;
  <case>.npz  for pipnet_mid_addon and count_onehot: the float64 reference maps of tests/golden/attr (``ref64``)
              through the reference's fold and normalisation -- prototype targets by
              ``normalize_attribution_map`` at the 98th percentile, class targets by logit mode at the 99th --
              with the denominator D it used.  A target is kept only where the rule cannot flip under the bound
              the device maps are held to: eps = MAP_BOUND * ref_err * max|ref64| (tests/test_gpu_attribution.py),
              |D_percentile - 1e-3| > 12 eps and D > 12 eps.  The margins found are printed.

The archives are written with fixed zip time stamps: two runs give the same bytes.

Usage:  python tests/golden/gen_golden_saliency.py
"""
from __future__ import annotations

import ast
import contextlib
import io
import json
import os
import sys
import zipfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gen_golden import REF  # noqa: E402
from count_pipnet_amd.synthetic import synth_images  # noqa: E402

OUT = os.path.join(HERE, "saliency")
ATTR = os.path.join(HERE, "attr")
CASES = ("pipnet_mid_addon", "count_onehot")
MAP_BOUND = 8                      # tests/test_gpu_attribution.py
SIZE = 32
PERCENTILES = (0, 50, 98, 99, 100)


def _reference_normalize():
    with open(os.path.join(REF, "util", "interpret_idg.py")) as f:
        lines = f.read().splitlines()
    body = []
    for i, line in enumerate(lines):
        if line.startswith("def normalize_attribution_map("):
            j = i + 1
            while j < len(lines) and (not lines[j].strip() or lines[j][0].isspace()):
                j += 1
            body += ast.parse("\n".join(lines[i:j])).body
    assert len(body) == 1
    ns = {"np": np}
    exec(compile(ast.Module(body=body, type_ignores=[]), "interpret_idg.py", "exec"), ns)
    fn = ns["normalize_attribution_map"]

    def quiet(image_2d, percentile):
        with contextlib.redirect_stdout(open(os.devnull, "w")):
            return fn(image_2d, percentile, 0)
    return quiet


def fold(one_map: torch.Tensor) -> np.ndarray:
    """interpret_idg.py:413-415 on one [3,H,W] map: channels last, absolute values, summed over the channels."""
    hwc = np.transpose(one_map.detach().cpu().numpy(), (1, 2, 0))
    return np.sum(np.abs(hwc), axis=2)


def plotly_palette():
    from plotly.colors import qualitative
    return list(qualitative.Plotly)


def blend(maps, h, w):
    """interpret_idg.py:397-398, :419-427, :454-457: float64 accumulators, colour i modulo the palette's length
    times map i added in place, alpha the running maximum, RGB clipped at the end, RGBA joined."""
    codes = plotly_palette()
    rgb, alpha = np.zeros((h, w, 3)), np.zeros((h, w, 1))
    for i, m in enumerate(maps):
        code = codes[i % len(codes)]
        colour = np.array([int(code[1:3], 16) / 255.0, int(code[3:5], 16) / 255.0, int(code[5:7], 16) / 255.0])
        rgb += colour * m[..., None]
        alpha = np.maximum(alpha, m[..., None])
    return np.concatenate((np.clip(rgb, 0, 1), alpha), axis=-1)


def unnormalize(batch: torch.Tensor) -> np.ndarray:
    """interpret_idg.py:442-446 on [1,3,H,W]: torch's x * std + mean, channels last, numpy's clip."""
    std = torch.tensor([0.229, 0.224, 0.225]).view(3, 1, 1)
    mean = torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1)
    hwc = (batch.squeeze(0) * std + mean).permute(1, 2, 0).detach().cpu().numpy()
    return np.clip(hwc, 0, 1)


def logit_clip(folded: np.ndarray, q=99):
    """interpret_idg.py:632-635: percentile range, no fallback."""
    top, low = np.percentile(folded, q), np.min(folded)
    return np.clip((folded - low) / (top - low), 0, 1), top, low


def imsave_bytes(clipped_map: np.ndarray, cmap: str) -> np.ndarray:
    """The RGBA pixels of plt.imsave(path, clipped_map, cmap=cmap) (:641), through a PNG in memory."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from PIL import Image
    buf = io.BytesIO()
    plt.imsave(buf, clipped_map, cmap=cmap, format="png")
    buf.seek(0)
    return np.asarray(Image.open(buf).convert("RGBA"), dtype=np.uint8).copy()


def byte_lut(cmap: str) -> np.ndarray:
    import matplotlib
    cm = matplotlib.colormaps[cmap]
    cm(0.5)                                    # initialises the table
    return (cm._lut[:256] * 255).astype(np.uint8)


def synthetic_maps():
    """Three [3,SIZE,SIZE] float32 maps, one per normalisation rule."""
    g = np.random.default_rng(20260)
    wide = (g.standard_normal((3, SIZE, SIZE)) * 0.01).astype(np.float32)
    narrow = (0.1 + g.standard_normal((3, SIZE, SIZE)) * 2e-5).astype(np.float32)
    flat = np.full((3, SIZE, SIZE), -0.25, dtype=np.float32)
    return np.stack([wide, narrow, flat])


def steps_fixture(normalize) -> dict:
    maps = synthetic_maps()
    folded = np.stack([fold(torch.from_numpy(m)) for m in maps])
    assert folded.dtype == np.float32
    rec = dict(maps=maps, folded=folded)
    norm = np.stack([normalize(f, 98) for f in folded])
    assert norm.dtype == np.float32
    rec["normalized_98"] = norm
    rec["vmin"] = np.array([np.min(f) for f in folded], dtype=np.float32)
    rec["vtop"] = np.array([np.max(f) for f in folded], dtype=np.float32)
    rec["percentiles"] = np.array(PERCENTILES, dtype=np.float64)
    vq = np.stack([[np.percentile(f, q) for q in PERCENTILES] for f in folded])
    assert vq.dtype == np.float32
    rec["vq"] = vq
    d98 = vq[:, PERCENTILES.index(98)] - rec["vmin"]
    dtop = rec["vtop"] - rec["vmin"]
    rules = [0 if a > 1e-3 else (1 if b > 1e-5 else 2) for a, b in zip(d98, dtop)]
    assert rules == [0, 1, 2], (rules, d98, dtop)
    rec["rule_98"] = np.array(rules, dtype=np.int32)
    # the blend of three maps: the rule-0 map at three percentiles
    three = np.stack([normalize(folded[0], q) for q in (98, 50, 99)])
    rec["blend_in"] = three
    rec["blend_rgba"] = blend(list(three), SIZE, SIZE)
    assert rec["blend_rgba"].dtype == np.float64
    x = synth_images(1, SIZE, seed=77)
    rec["image"] = x[0].numpy()
    rec["image_unnormalized"] = unnormalize(x)
    assert rec["image_unnormalized"].dtype == np.float32
    clipped, vmax, vmin = logit_clip(folded[0])
    assert clipped.dtype == np.float32 and float(clipped.min()) == 0.0 and float(clipped.max()) == 1.0
    rec["logit_normalized"] = clipped
    rec["logit_rgba"] = imsave_bytes(clipped, "Blues")
    rec["blues_lut"] = byte_lut("Blues")
    import matplotlib
    import plotly
    rec["meta"] = np.array(json.dumps(dict(numpy=np.__version__, matplotlib=matplotlib.__version__,
                                           plotly=plotly.__version__, torch=torch.__version__,
                                           palette=plotly_palette())))
    print(f"steps: rules {rules} percentile ranges {[float(v) for v in d98]} global ranges {[float(v) for v in dtop]}")
    return rec


def case_fixture(name: str, normalize) -> dict:
    z = np.load(os.path.join(ATTR, name + ".npz"), allow_pickle=False)
    rec = {}
    report = []
    for kind, q in (("prototype", 98), ("class", 99)):
        for method in ("ig", "lig", "idg"):
            key = f"{kind}_{method}"
            ref64, ref_err = z[key + "_ref64"], z[key + "_ref_err"]
            norms, dens, epss, rules, keeps = [], [], [], [], []
            for i in range(ref64.shape[0]):
                image_2d = fold(torch.from_numpy(ref64[i]))
                vmin, vtop = np.min(image_2d), np.max(image_2d)
                d_pct = float(np.percentile(image_2d, q) - vmin)
                d_top = float(vtop - vmin)
                eps = MAP_BOUND * float(ref_err[i]) * float(np.abs(ref64[i]).max())
                if kind == "prototype":
                    clipped = normalize(image_2d, q)
                    rule = 0 if np.float32(d_pct) > 1e-3 else (1 if np.float32(d_top) > 1e-5 else 2)
                    den = d_pct if rule == 0 else d_top
                    keep = abs(d_pct - 1e-3) > 12 * eps and den > 12 * eps and \
                        (rule == 0 or abs(d_top - 1e-5) > 12 * eps) and rule != 2
                else:
                    with np.errstate(all="ignore"):
                        clipped, _, _ = logit_clip(image_2d, q)
                    rule, den = 0, d_pct
                    keep = den > 12 * eps
                norms.append(clipped.astype(np.float32))
                dens.append(den)
                epss.append(eps)
                rules.append(rule)
                keeps.append(bool(keep))
                report.append(f"  {key}[{i}] rule {rule} D {den:.3e} eps {eps:.3e} D/12eps {den / (12 * eps):.1f} "
                              f"|Dpct-1e-3|/12eps {abs(d_pct - 1e-3) / (12 * eps):.1f} keep {bool(keep)}")
            rec[key + "_normalized"] = np.stack(norms)
            rec[key + "_den"] = np.array(dens, dtype=np.float64)
            rec[key + "_eps"] = np.array(epss, dtype=np.float64)
            rec[key + "_rule"] = np.array(rules, dtype=np.int32)
            rec[key + "_keep"] = np.array(keeps, dtype=bool)
    rec["meta"] = np.array(json.dumps(dict(name=name, map_bound=MAP_BOUND,
                                           percentiles=dict(prototype=98, **{"class": 99}))))
    print(f"{name}: kept {sum(int(v.sum()) for k, v in rec.items() if k.endswith('_keep'))} of "
          f"{sum(v.size for k, v in rec.items() if k.endswith('_keep'))} targets")
    print("\n".join(report))
    return rec


def save_npz(path: str, rec: dict) -> None:
    """np.savez_compressed with fixed zip time stamps, keys in sorted order."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(rec):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(rec[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    torch.set_num_threads(1)
    os.makedirs(OUT, exist_ok=True)
    normalize = _reference_normalize()
    todo = [("steps", steps_fixture(normalize))] + [(n, case_fixture(n, normalize)) for n in CASES]
    for name, rec in todo:
        path = os.path.join(OUT, name + ".npz")
        save_npz(path, rec)
        print(f"wrote {path} ({os.path.getsize(path) / 1e3:.1f} kB)")


if __name__ == "__main__":
    main()
