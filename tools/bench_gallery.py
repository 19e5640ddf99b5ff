"""Time count_pipnet_amd.gallery.prototype_gallery beside the reference's host procedure, on one GPU.

A synthetic ImageFolder of CUB-sized JPEG photos is written to a temporary directory, and a synthetic top-k result
(every prototype used, k entries each, images drawn uniformly, windows on the reference's patch lattice) stands in
for a pass.  Timed, each with a host clock ending in a device synchronise where a device is involved:

  gallery    prototype_gallery, whole call (decode + pack + H2D + resize + compose), after one warm-up call
  decode     only dataset[i] of the distinct images (what the gallery spends on the host before the device)
  device     resize + compose of already packed chunks (events around the launches)
  reference  vis_pipnet.py's procedure restated with Pillow: per shown entry Image.open -> Resize -> crop
             (ToTensor / make_grid / ToPILImage are copies of the same bytes and are left out)

``--heatmaps`` times the similarity heatmaps instead (gallery.explanation_heatmaps, pipnet_heatmap_rgb8) at C2
dimensions: 64 images, a 26 x 26 x 768 map, 224^2 frames, a LocalExplanation of 3 classes with ``--entries`` kept
prototypes each.  Random maps and frames stand in for a forward (the kernel's work does not depend on the values):

  heatmaps   explanation_heatmaps, whole call, device events around it
  launches   the pipnet_heatmap_rgb8 launches alone into a preallocated result (events), and the bytes the
             algorithm moves per second: per entry one h x w float32 channel and one frame in, one picture out;
             both at ``--batch-size`` entries per launch and with every entry in one launch
  reference  the reference's heatmap chain (visualize_prediction.py:92-99) per entry on the host CPU with torch,
             Pillow and numpy, the copy of the [B, P, h, w] maps to the host included (a table lookup stands in for
             cv2.applyColorMap)

``--overlays`` times the prototype feature-map overlays (gallery.feature_map_overlays, pipnet_map_overlay) at C2
dimensions: ``--count`` (1,536) pairs drawn from a 26 x 26 x 768 map of 64 images, rendered to 224^2.  Random maps
stand in for a forward and three ramps for viridis (the kernel's work does not depend on the values: a pixel off the
mask is stored as zeros):

  overlays   feature_map_overlays, whole call, device events around it (the results are allocated inside)
  launches   the pipnet_map_overlay launches alone into preallocated results (events), and the bytes the algorithm
             moves per second: per entry the h x w float32 map in and out, and 38 bytes out per pixel (resized 4,
             mask 1, colour 1, overlay 32); both at ``--batch-size`` entries per launch and with every entry in one
  reference  the reference's chain (vis_pipnet.py:459-475) on the host CPU for ``--host-entries`` overlays: scipy's
             ``zoom``, the mask and the Python loop calling matplotlib's ``cmap`` once per pixel; skipped where
             scipy or matplotlib cannot be imported

Usage: python tools/bench_gallery.py [--prototypes 768] [--k 10] [--size 224] [--images 1024] [--out FILE]
       python tools/bench_gallery.py --heatmaps [--entries 8] [--size 224] [--batch-size 64] [--out FILE]
       python tools/bench_gallery.py --overlays [--count 1536] [--host-entries 3] [--size 224] [--batch-size 64] [--out FILE]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from count_pipnet_amd import kernels as K                                               # noqa: E402
from count_pipnet_amd.data import DecodedImageFolder, DeviceEvalTransform, pack_images  # noqa: E402
from count_pipnet_amd.explain_forward import img_coordinates, patch_skip                # noqa: E402
from count_pipnet_amd.gallery import explanation_heatmaps, feature_map_overlays, prototype_gallery    # noqa: E402
from count_pipnet_amd.local import LocalExplanation                                     # noqa: E402
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


HBM_ACHIEVABLE = 6.3e12         # bytes / s a streaming kernel reaches on an MI355X (8 TB/s peak)


def jet_like_lut() -> np.ndarray:
    """[256, 3] uint8 RGB ramps shaped like JET; the arithmetic does not depend on the table's values."""
    x = np.arange(256) / 255.0
    rgb = [np.clip(1.5 - np.abs(4 * x - c), 0, 1) for c in (3, 2, 1)]
    return np.round(np.stack(rgb, axis=1) * 255).astype(np.uint8)


def synthetic_explanation(b: int, classes: int, entries: int, pn: int) -> LocalExplanation:
    g = torch.Generator().manual_seed(3)
    z = lambda *s: torch.zeros(*s, dtype=torch.int64)      # noqa: E731
    zf = lambda *s: torch.zeros(*s)                        # noqa: E731
    return LocalExplanation(classes=z(b, classes), logits=zf(b, classes),
                            count=torch.full((b, classes), entries, dtype=torch.int64),
                            prototype=torch.randint(0, pn, (b, classes, entries), generator=g),
                            similarity=zf(b, classes, entries), weight=zf(b, classes, entries),
                            simweight=zf(b, classes, entries), h_idx=z(b, classes, entries), w_idx=z(b, classes, entries),
                            coords=z(b, classes, entries, 4), rect=z(b, classes, entries, 4), proto_shape=(1, pn, 26, 26))


def host_heatmaps(feats: torch.Tensor, frames: torch.Tensor, res: LocalExplanation, lut: np.ndarray, size: int) -> int:
    """The baseline: what the reference's vis_pred does per stored entry for its heatmap, with the same libraries, on
    the host -- both device-to-host copies, then per entry the map as an 8-bit image (torch), Pillow's bicubic resize,
    back to float32 in 0..1, the table lookup on ``uint8(255 * .)`` and the float32 blend 0.2 * colour + 0.6 * image.
    Writing the PNG is left out on both sides."""
    maps_host, frames_host = feats.cpu(), frames.cpu()
    made = 0
    for bi in range(res.prototype.shape[0]):
        picture = frames_host[bi].float().div(255).numpy()                 # one float image per frame
        for p in res.prototype[bi].flatten().tolist():
            small = Image.fromarray(maps_host[bi, p].mul(255).byte().numpy(), "L")
            unit = torch.from_numpy(np.array(small.resize((size, size), Image.BICUBIC))).float().div(255).numpy()
            colour = lut[(255 * unit).astype(np.uint8)].astype(np.float32) / 255
            blended = 0.2 * colour + 0.6 * picture
            made += int(blended.shape == (size, size, 3) and blended.dtype == np.float32)
    return made


def time_heatmaps(say, nhwc, feats, frames, res, lut, batch_size: int) -> float:
    """Times ``explanation_heatmaps`` and its launches alone at ``batch_size``; the whole call's best time in ms."""
    n, s = res.prototype.numel(), frames.shape[1]
    per_entry = nhwc.shape[1] * nhwc.shape[2] * 4 + 2 * s * s * 3
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    whole = []
    for i in range(6):                                                     # the first call is the warm-up
        torch.cuda.synchronize()
        start.record()
        out = explanation_heatmaps(feats, frames, res, lut, batch_size=batch_size)
        end.record()
        torch.cuda.synchronize()
        whole.append(start.elapsed_time(end))
    assert tuple(out.heatmaps.shape) == (n, s, s, 3)
    say(f"batch_size {batch_size}:")
    say(f"heatmaps   explanation_heatmaps, whole call (events)   {min(whole[1:]):9.3f} ms   (5 runs: "
        + ", ".join(f"{t:.3f}" for t in whole[1:]) + ")")
    items = [(int(e[0]), int(q), int(e[0])) for e, q in zip(out.entry.tolist(), out.prototype.tolist())]
    table = torch.tensor(items, dtype=torch.int32, device=frames.device)   # sent once, as the call above does
    chunks = [table[i:i + batch_size] for i in range(0, n, batch_size)]
    dst = torch.empty_like(out.heatmaps)
    reps, alone = 20, []
    for i in range(4):
        torch.cuda.synchronize()
        start.record()
        for _ in range(reps):
            for c, it in enumerate(chunks):
                K.heatmap_rgb8(nhwc, frames, it, lut, out=dst[c * batch_size:c * batch_size + len(it)])
        end.record()
        torch.cuda.synchronize()
        alone.append(start.elapsed_time(end) / reps)
    assert torch.equal(dst, out.heatmaps)
    rate = n * per_entry / (min(alone[1:]) * 1e-3)
    say(f"launches   {len(chunks)} pipnet_heatmap_rgb8 launch(es) (events)      {min(alone[1:]):9.3f} ms   (3 x {reps} runs: "
        + ", ".join(f"{t:.3f}" for t in alone[1:]) + f"), {min(alone[1:]) / len(chunks) * 1e3:.1f} us per launch")
    say(f"           {rate / 1e12:.3f} TB/s of algorithmic bytes = {100 * rate / HBM_ACHIEVABLE:.1f} % of the "
        f"{HBM_ACHIEVABLE / 1e12:.1f} TB/s a streaming kernel reaches from HBM (8 TB/s peak)")
    return min(whole[1:])


def heatmaps_main(a, dev, say) -> None:
    b, pn, hw, classes, s = 64, 768, 26, 3, a.size
    g = torch.Generator().manual_seed(4)
    nhwc = torch.rand((b, hw, hw, pn), generator=g).to(dev)
    feats = nhwc.permute(0, 3, 1, 2)                                       # [B, P, h, w], NHWC-backed as a forward's
    frames = torch.randint(0, 256, (b, s, s, 3), generator=g, dtype=torch.uint8).to(dev)
    lut_np = jet_like_lut()
    lut = torch.from_numpy(lut_np).to(dev)
    res = synthetic_explanation(b, classes, a.entries, pn)
    n = b * classes * a.entries
    per_entry = hw * hw * 4 + 2 * s * s * 3
    say("python tools/bench_gallery.py " + " ".join(sys.argv[1:]))
    say(f"{b} images x {classes} classes x {a.entries} prototypes = {n} heatmaps at {s}^2 from a {hw} x {hw} x {pn} map; "
        f"{per_entry} bytes per entry (one channel and one frame in, one picture out), {n * per_entry / 1e6:.1f} MB in "
        f"all, the {b * s * s * 3 / 1e6:.1f} MB of frames re-read from cache; the maps are {nhwc.numel() * 4 / 1e6:.0f} MB")
    best = time_heatmaps(say, nhwc, feats, frames, res, lut, a.batch_size)
    if n != a.batch_size:
        time_heatmaps(say, nhwc, feats, frames, res, lut, n)               # every entry in one launch
    t0 = time.perf_counter()
    done = host_heatmaps(feats, frames, res, lut_np, s)
    t_ref = time.perf_counter() - t0
    t0 = time.perf_counter()
    feats.cpu()
    t_copy = time.perf_counter() - t0
    say(f"reference  the reference's chain per entry on the host {t_ref * 1e3:9.1f} ms   ({done} entries, "
        f"{t_ref / done * 1e3:.2f} ms per entry; {t_copy * 1e3:.1f} ms of it the copy of the maps to the host, "
        f"torch {torch.get_num_threads()} threads)")
    say(f"reference / heatmaps at batch_size {a.batch_size} = {t_ref * 1e3 / best:.0f}")


def time_overlays(say, nhwc, feats, pairs, lut, s: int, batch_size: int) -> float:
    """Times ``feature_map_overlays`` and its launches alone at ``batch_size``; the whole call's best time in ms."""
    n, hw = len(pairs), nhwc.shape[1] * nhwc.shape[2]
    per_entry = 2 * hw * 4 + s * s * 38
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    whole = []
    for i in range(6):                                                     # the first call is the warm-up
        out = None                                                         # the allocator hands the blocks back
        torch.cuda.synchronize()
        start.record()
        out = feature_map_overlays(feats, pairs, lut, size=s, batch_size=batch_size)
        end.record()
        torch.cuda.synchronize()
        whole.append(start.elapsed_time(end))
    assert tuple(out.overlay.shape) == (n, s, s, 4)
    say(f"batch_size {batch_size}:")
    say(f"overlays   feature_map_overlays, whole call (events)   {min(whole[1:]):9.3f} ms   (5 runs: "
        + ", ".join(f"{t:.3f}" for t in whole[1:]) + ")")
    table = torch.tensor(pairs, dtype=torch.int32, device=nhwc.device)     # sent once, as the call above does
    dst = K.MapOverlay(*(torch.empty_like(t) for t in out))
    chunks = [(table[i:i + batch_size], K.MapOverlay(*(t[i:i + batch_size] for t in dst))) for i in range(0, n, batch_size)]
    reps, alone = 10, []
    for i in range(4):
        torch.cuda.synchronize()
        start.record()
        for _ in range(reps):
            for it, part in chunks:
                K.map_overlay(nhwc, it, lut, s, out=part)
        end.record()
        torch.cuda.synchronize()
        alone.append(start.elapsed_time(end) / reps)
    assert all(torch.equal(a, b) for a, b in zip(dst, out))
    rate = n * per_entry / (min(alone[1:]) * 1e-3)
    say(f"launches   {len(chunks)} pipnet_map_overlay launch(es) (events)       {min(alone[1:]):9.3f} ms   (3 x {reps} runs: "
        + ", ".join(f"{t:.3f}" for t in alone[1:]) + f"), {min(alone[1:]) / len(chunks) * 1e3:.1f} us per launch")
    say(f"           {rate / 1e12:.3f} TB/s of algorithmic bytes = {100 * rate / HBM_ACHIEVABLE:.1f} % of the "
        f"{HBM_ACHIEVABLE / 1e12:.1f} TB/s a streaming kernel reaches from HBM (8 TB/s peak)")
    return min(whole[1:])


def host_overlays(maps: np.ndarray, s: int) -> int:
    """The baseline: vis_pipnet.py:459-475 per overlay with the reference's libraries, or -1 without them."""
    try:
        import matplotlib
        from scipy.ndimage import zoom
    except ImportError:
        return -1
    cmap = matplotlib.colormaps["viridis"]
    made = 0
    for feature_map_np in maps:
        resized_feature_map = zoom(feature_map_np, (s / feature_map_np.shape[0], s / feature_map_np.shape[1]))
        mask = resized_feature_map > 0.1
        overlay = np.zeros((*resized_feature_map.shape, 4))
        for y in range(resized_feature_map.shape[0]):
            for x in range(resized_feature_map.shape[1]):
                if mask[y, x]:
                    color = cmap(resized_feature_map[y, x])
                    overlay[y, x] = (*color[:3], 0.7)
        made += int(overlay.shape == (s, s, 4))
    return made


def overlays_main(a, dev, say) -> None:
    b, pn, hw, s, n = 64, 768, 26, a.size, a.count
    g = torch.Generator().manual_seed(6)
    nhwc = (torch.rand((b, hw, hw, pn), generator=g) ** 3).to(dev)         # x^3 > 0.1 for about half of the pixels
    feats = nhwc.permute(0, 3, 1, 2)                                       # [B, P, h, w], NHWC-backed as a forward's
    x = np.arange(256) / 255.0
    lut = torch.from_numpy(np.stack([x, 1 - x, 0.5 + 0.5 * x], axis=1)).to(dev)
    pairs = torch.stack([torch.randint(0, b, (n,), generator=g), torch.randint(0, pn, (n,), generator=g)], dim=1).tolist()
    per_entry = 2 * hw * hw * 4 + s * s * 38
    say("python tools/bench_gallery.py " + " ".join(sys.argv[1:]))
    say(f"{n} overlays at {s}^2 from a {hw} x {hw} x {pn} map of {b} images; {per_entry} bytes per entry (the map in "
        f"and out, 38 bytes per pixel out: resized 4, mask 1, colour 1, overlay 32), {n * per_entry / 1e6:.1f} MB in all; "
        f"the maps are {nhwc.numel() * 4 / 1e6:.0f} MB")
    best = time_overlays(say, nhwc, feats, pairs, lut, s, a.batch_size)
    if n != a.batch_size:
        time_overlays(say, nhwc, feats, pairs, lut, s, n)                  # every entry in one launch
    maps = np.stack([feats[bi, p].cpu().numpy() for bi, p in pairs[:a.host_entries]])
    t0 = time.perf_counter()
    done = host_overlays(maps, s)
    t_ref = time.perf_counter() - t0
    if done < 0:
        say("reference  scipy or matplotlib cannot be imported here: the host chain was not timed")
        return
    say(f"reference  zoom + mask + cmap per pixel on the host    {t_ref * 1e3:9.1f} ms   ({done} entries, "
        f"{t_ref / done * 1e3:.1f} ms per entry, {t_ref / done * n:.0f} s for {n})")
    say(f"reference per entry / overlays per entry at batch_size {a.batch_size} = {t_ref / done * 1e3 / (best / n):.0f}")


def write_out(path, lines) -> None:
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--heatmaps", action="store_true", help="time the similarity heatmaps instead of the gallery")
    ap.add_argument("--entries", type=int, default=8, help="--heatmaps: kept prototypes per (image, class)")
    ap.add_argument("--overlays", action="store_true", help="time the feature-map overlays instead of the gallery")
    ap.add_argument("--count", type=int, default=1536, help="--overlays: how many (image, prototype) pairs")
    ap.add_argument("--host-entries", type=int, default=3, help="--overlays: overlays the host chain is timed on")
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

    if a.heatmaps or a.overlays:
        (heatmaps_main if a.heatmaps else overlays_main)(a, dev, say)
        write_out(a.out, lines)
        return
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
    write_out(a.out, lines)


if __name__ == "__main__":
    main()
