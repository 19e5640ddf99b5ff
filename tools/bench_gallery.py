"""Time count_pipnet_amd.gallery.prototype_gallery beside the reference's host procedure, on one GPU.

A synthetic ImageFolder of CUB-sized JPEG photos is written to a temporary directory, and a synthetic top-k result
(every prototype used, k entries each, images drawn uniformly, windows on the reference's patch lattice) stands in
for a pass.  Timed, each with a host clock ending in a device synchronise where a device is involved:

  gallery    prototype_gallery, whole call (decode + pack + H2D + resize + compose), after one warm-up call
  decode     only dataset[i] of the distinct images (what the gallery spends on the host before the device)
  device     resize + compose of already packed chunks (events around the launches)
  reference  vis_pipnet.py's procedure restated with Pillow: per shown entry Image.open -> Resize -> crop
             (ToTensor / make_grid / ToPILImage are copies of the same bytes and are left out)

Usage: python tools/bench_gallery.py [--prototypes 768] [--k 10] [--size 224] [--images 1024] [--out FILE]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from count_pipnet_amd import kernels as K                                               # noqa: E402
from count_pipnet_amd.data import DecodedImageFolder, DeviceEvalTransform, pack_images  # noqa: E402
from count_pipnet_amd.explain_forward import img_coordinates, patch_skip                # noqa: E402
from count_pipnet_amd.gallery import prototype_gallery                                  # noqa: E402
from count_pipnet_amd.topk import PrototypeTopK                                         # noqa: E402


def write_folder(root: str, n: int, classes: int = 16) -> None:
    from PIL import Image
    rng = np.random.default_rng(1)
    yy, xx = np.meshgrid(np.linspace(0, 1, 375), np.linspace(0, 1, 500), indexing="ij")
    for i in range(n):
        d = os.path.join(root, f"class_{i % classes:03d}")
        os.makedirs(d, exist_ok=True)
        img = np.stack([128 + 90 * np.sin(2 * np.pi * (f * 3 * xx + g * 3 * yy) + ph)
                        for f, g, ph in rng.uniform(-1, 1, (3, 3))], axis=-1) + rng.normal(0, 12, (375, 500, 3))
        img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
        Image.fromarray(img if i % 2 else img.transpose(1, 0, 2).copy()).save(os.path.join(d, f"{i:05d}.jpg"), quality=90)


def synthetic_topk(pn: int, k: int, n_images: int, size: int, hw: int = 26) -> PrototypeTopK:
    g = torch.Generator().manual_seed(2)
    index = torch.randint(0, n_images, (pn, 1, k), generator=g)
    scores = torch.rand(pn, 1, k, generator=g).sort(dim=2, descending=True).values * 0.8 + 0.2
    h_idx, w_idx = torch.randint(0, hw, (pn, 1, k), generator=g), torch.randint(0, hw, (pn, 1, k), generator=g)
    shape = (1, pn, hw, hw)
    coords = torch.stack(img_coordinates(size, shape, 32, patch_skip(size, hw), h_idx, w_idx), dim=-1)
    sel = torch.ones(pn, dtype=torch.bool)
    return PrototypeTopK(scores=scores, index=index, h_idx=h_idx, w_idx=w_idx, coords=coords,
                         abstained=torch.zeros((), dtype=torch.int64), selected=sel, unused=~sel, groups=[None],
                         proto_shape=shape)


def reference_procedure(ds, res: PrototypeTopK, size: int) -> int:
    from PIL import Image
    done = 0
    for p in range(res.index.shape[0]):
        for j in range(res.index.shape[2]):
            h0, h1, w0, w1 = res.coords[p, 0, j].tolist()
            image = Image.open(ds.samples[int(res.index[p, 0, j])][0]).resize((size, size), Image.BILINEAR)
            done += int(np.asarray(image)[h0:h1, w0:w1].size > 0)
    return done


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--prototypes", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gallery: no ROCm GPU visible (there is no CPU fallback)")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        write_folder(root, a.images)
        ds = DecodedImageFolder(root)
        res = synthetic_topk(a.prototypes, a.k, len(ds), a.size)
        distinct = sorted(set(res.index.flatten().tolist()))
        say(f"{a.prototypes} prototypes x k = {a.k} = {a.prototypes * a.k} entries at {a.size}^2, {len(distinct)} distinct of "
            f"{len(ds)} JPEG files (375 x 500 / 500 x 375), batch_size {a.batch_size}; folder written in "
            f"{time.perf_counter() - t0:.1f} s")
        prototype_gallery(None, ds, res, image_size=a.size, device=dev, batch_size=a.batch_size)       # warm-up
        torch.cuda.synchronize()
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            g = prototype_gallery(None, ds, res, image_size=a.size, device=dev, batch_size=a.batch_size)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        say(f"gallery    prototype_gallery, whole call           {min(times) * 1e3:9.1f} ms   (3 runs: "
            + ", ".join(f"{t * 1e3:.1f}" for t in times) + ")")
        assert int(g.cells.sum()) == a.prototypes * a.k and bool(g.ok.all())
        t0 = time.perf_counter()
        decoded = [ds[i][0] for i in distinct]
        t_dec = time.perf_counter() - t0
        say(f"decode     dataset[i] of the {len(distinct)} distinct images      {t_dec * 1e3:9.1f} ms   "
            f"({t_dec / len(distinct) * 1e3:.2f} ms per image)")
        tf = DeviceEvalTransform(a.size)
        chunks = [pack_images(decoded[i:i + a.batch_size]) for i in range(0, len(decoded), a.batch_size)]
        grids = torch.full_like(g.grids, 40)
        reps = min(max(a.prototypes * a.k // len(distinct), 1), a.k)       # as many items per frame as the gallery has
        items = [[(f, 0, 32, 0, 32, (c * a.batch_size + f) % a.prototypes, 0, j * 33 + 1) for f in range(len(ch.offsets))
                  for j in range(reps)] for c, ch in enumerate(chunks)]
        for timed in (False, True):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            start.record()
            for ch, it in zip(chunks, items):
                K.patch_compose_rgb8(tf(ch, dev, want_u8=True)[1], it, grids)
            end.record()
            torch.cuda.synchronize()
            t_dev = time.perf_counter() - t0
        say(f"device     H2D + resize + compose of packed chunks    {t_dev * 1e3:9.1f} ms   (events: {start.elapsed_time(end):.1f} ms)")
        t0 = time.perf_counter()
        done = reference_procedure(ds, res, a.size)
        t_ref = time.perf_counter() - t0
        say(f"reference  Pillow open -> resize -> crop per entry    {t_ref * 1e3:9.1f} ms   ({done} entries, "
            f"{t_ref / done * 1e3:.2f} ms per entry)")
        say(f"reference / gallery = {t_ref / min(times):.1f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
