"""Training-augmentation cost on one GPU against the same work in Pillow on the host.

(a) device: event-timed ms per batch of ``pipnet_augment_geometry_rgb8`` and
    ``pipnet_augment_view_rgb8`` (through their kernels.py wrappers, parameters sampled once) at
    B images of 500x375 -> size, and each entry's achieved bytes/s against the HBM peak.  The
    bytes are what the algorithm has to move, computed from the shapes:
      geometry: the decoded pixels + the S1 x S1 intermediate written and read + the output;
      view:     V reads of the S2 x S2 image per pass over it (one pass, plus one per
                operation that needs whole-image statistics) + the fp32 views.
    Also the wall time of the whole transform call (sampling, checks, copies; synchronised).
(b) host: the Pillow calls the reference's workers make for the same parameters (the calls of
    tests/test_augment_cpu.py) in a thread pool of 16.
(c) the joint-phase ``hip_train_step`` of the C2 network (tools/bench_train.py) at the same batch,
    so the augmentation's share of a training step is on record.

Prints one JSON line per measurement."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from count_pipnet_amd import augment as A  # noqa: E402
from count_pipnet_amd.data import IMAGENET_MEAN, IMAGENET_STD, DeviceTrainTransform, pack_images  # noqa: E402

HBM_PEAK = 8.0e12        # bytes/s, MI355X specification


def photos(n):
    rng = np.random.default_rng(0)
    out = []
    for i in range(n):
        h, w = (375, 500) if i % 2 == 0 else (500, 375)
        yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
        img = np.stack([128 + 90 * np.sin(6.3 * (rng.uniform(-3, 3) * xx + rng.uniform(-3, 3) * yy)) for _ in range(3)], -1)
        out.append(np.clip(np.rint(img + rng.normal(0, 12, img.shape)), 0, 255).astype(np.uint8))
    return out


def event_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


def pillow_image(img, gp, vps, s1, s2, size):
    """transform1 + transform2 (per view) of one image in Pillow / numpy, as a reference worker."""
    from PIL import Image, ImageEnhance, ImageOps
    im = Image.fromarray(img, "RGB").resize((s1, s1), Image.Resampling.BILINEAR)
    if gp[0]:
        im = im.transform((s1, s1), Image.Transform.AFFINE, gp[1:7], Image.Resampling.NEAREST,
                          fillcolor=(int(gp[7]),) * 3)
    if gp[8]:
        im = im.transpose(Image.Transpose.FLIP_LEFT_RIGHT)
    top, left, ch, cw = (int(v) for v in gp[9:13])
    im = im.crop((left, top, left + cw, top + ch)).resize((s2, s2), Image.Resampling.BILINEAR)
    mean = np.asarray(IMAGENET_MEAN, np.float32)[:, None, None]
    std = np.asarray(IMAGENET_STD, np.float32)[:, None, None]
    views = []
    for vp in vps:
        v = im
        for op, p in ((int(vp[0]), vp[1]), (int(vp[2]), vp[3])):
            if op in (A.OP_BRIGHTNESS, A.OP_COLOR, A.OP_CONTRAST, A.OP_SHARPNESS):
                enh = {A.OP_BRIGHTNESS: ImageEnhance.Brightness, A.OP_COLOR: ImageEnhance.Color,
                       A.OP_CONTRAST: ImageEnhance.Contrast, A.OP_SHARPNESS: ImageEnhance.Sharpness}[op]
                v = enh(v).enhance(p)
            elif op == A.OP_POSTERIZE:
                v = ImageOps.posterize(v, int(p))
            elif op == A.OP_SOLARIZE:
                v = ImageOps.solarize(v, p)
            elif op == A.OP_AUTOCONTRAST:
                v = ImageOps.autocontrast(v)
            elif op == A.OP_EQUALIZE:
                v = ImageOps.equalize(v)
        i, j = int(vp[4]), int(vp[5])
        t = np.asarray(v.crop((j, i, j + size, i + size)), np.uint8).transpose(2, 0, 1).astype(np.float32) / 255.0
        if vp[6]:
            t = t + np.random.default_rng(int(vp[7])).normal(0, 0.1, t.shape).astype(np.float32)
        views.append((t - mean) / std)
    return views


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--policies", default="CUB-200-2011,geometric_shapes_gaussian_noise")
    ap.add_argument("--train-steps", type=int, default=10, help="0 skips (c)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment needs a ROCm GPU (no fallback)")
    from count_pipnet_amd import kernels as K
    dev = torch.device("cuda:0")
    imgs = photos(a.batch)
    packed = pack_images(imgs)
    src_bytes = int(packed.pixels.numel())
    for name in a.policies.split(","):
        t = DeviceTrainTransform(name, a.size)
        prm = A.sample_params(name, a.size, a.batch, torch.Generator().manual_seed(0))
        pixels, offsets, sizes = (x.to(dev) for x in (packed.pixels, packed.offsets, packed.sizes))
        sizes_host = packed.sizes.numpy()
        geo = lambda: K.augment_geometry_rgb8(pixels, offsets, sizes, sizes_host, prm.geom, t.s1, t.s2)
        u8 = geo()
        view = lambda: K.augment_view_rgb8(u8, prm.view, a.size, t.mean, t.std, t.policy.grayscale, A.NOISE_STD, 1)
        g_ms = event_ms(geo, a.steps, a.warmup)
        v_ms = event_ms(view, a.steps, a.warmup)
        both = event_ms(lambda: t(packed, dev, params=prm), a.steps, a.warmup)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            t(packed, dev, generator=torch.Generator().manual_seed(0))
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / a.steps * 1e3
        b, v = a.batch, 2
        g_bytes = src_bytes + 2 * b * t.s1 * t.s1 * 3 + b * t.s2 * t.s2 * 3
        ops = prm.view[:, :, [0, 2]]
        passes = 1.0 + float(((ops == 3) | (ops == 7) | (ops == 8)).double().sum(-1).mean())
        v_bytes = v * b * (t.s2 * t.s2 * 3 * passes + 3 * a.size * a.size * 4)
        print(json.dumps({
            "metric": "device augmentation, ms per batch (event-timed, median of steps)", "policy": name,
            "batch": a.batch, "size": a.size, "s1": t.s1, "s2": t.s2, "steps": a.steps,
            "geometry_ms": g_ms[0], "geometry_ms_min_max": g_ms[1:], "geometry_bytes": g_bytes,
            "geometry_bytes_per_s": g_bytes / (g_ms[0] * 1e-3), "geometry_share_of_hbm_peak": g_bytes / (g_ms[0] * 1e-3) / HBM_PEAK,
            "view_ms": v_ms[0], "view_ms_min_max": v_ms[1:], "view_bytes": v_bytes, "view_image_passes": passes,
            "view_bytes_per_s": v_bytes / (v_ms[0] * 1e-3), "view_share_of_hbm_peak": v_bytes / (v_ms[0] * 1e-3) / HBM_PEAK,
            "transform_ms_with_copies": both[0], "transform_ms_min_max": both[1:],
            "transform_wall_ms_with_sampling": wall}), flush=True)
        gp, vp = prm.geom.numpy(), prm.view.numpy()
        work = lambda k: pillow_image(imgs[k], gp[k], [vp[0, k], vp[1, k]], t.s1, t.s2, a.size)
        with ThreadPoolExecutor(a.threads) as pool:
            list(pool.map(work, range(a.batch)))
            host = []
            for _ in range(5):
                t0 = time.perf_counter()
                list(pool.map(work, range(a.batch)))
                host.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        for k in range(8):
            work(k)
        one = (time.perf_counter() - t0) / 8 * 1e3
        print(json.dumps({"metric": "host Pillow chain, ms per batch", "policy": name, "threads": a.threads,
                          "batch": a.batch, "pillow_ms": statistics.median(host), "pillow_ms_min_max": [min(host), max(host)],
                          "pillow_ms_per_image_one_thread": one,
                          "device_over_host": both[0] / statistics.median(host)}), flush=True)
    if a.train_steps:
        from bench_train import build, timed
        from count_pipnet_amd import train as T
        g = torch.Generator().manual_seed(0)
        xs1 = torch.randn(a.batch, 3, a.size, a.size, generator=g).to(dev)
        xs2 = torch.randn(a.batch, 3, a.size, a.size, generator=g).to(dev)
        ys = torch.randint(0, 200, (a.batch,), generator=g).to(dev)
        sdg = torch.Generator().manual_seed(1)
        net, opt = build(dev)
        fine = timed(lambda: T.hip_finetune_step(net, xs1, xs2, ys, opt, True, generator=sdg), a.train_steps, 3)
        del net, opt
        net_j, opt_j, opt_jn = build(dev, joint=True)
        joint = timed(lambda: T.hip_train_step(net_j, xs1, xs2, ys, opt_jn, opt_j, False, 1, 1, True, generator=sdg),
                      a.train_steps, 3)
        print(json.dumps({"metric": "training iteration of the C2 network, ms per batch (host clock, synchronised)",
                          "batch_per_view": a.batch, "hip_train_step_joint_ms": joint * 1e3,
                          "hip_finetune_step_ms": fine * 1e3}), flush=True)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
