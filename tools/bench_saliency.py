"""Time count_pipnet_amd.saliency.interpret_prototypes beside the host post-processing, on one GPU.

Workload: the C2 model (ConvNeXt-tiny-26 PIP-Net, 224^2) on one synthetic image; the classifier row of the
predicted class is scaled so that about ``--active`` prototypes pass the 0.1 contribution threshold.  Two routes
from the same ``attribute`` call to the overlay and the un-normalised image:

  device  normalize_maps + blend_maps + unnormalize_image on the HIP kernels, nothing copied
  host    maps.cpu() (the copy waits for the device) and tests/saliency_ref.py in numpy, as a caller of
          ``attribute`` had to write it: fold, np.partition percentile, normalise, float64 blend, un-normalise

Each part is timed by a host clock around work that ends in a device synchronise, after one warm-up of every
part; the attribution part is repeated ``--repeats`` times, the post-processing parts ``--post-repeats`` times,
alternating the two routes.  The least and the median are printed.

Usage: python tools/bench_saliency.py [--active 16] [--steps 192] [--batch-size 16] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import bench                                                    # noqa: E402
import saliency_ref as R                                        # noqa: E402
from count_pipnet_amd import saliency as S                      # noqa: E402
from count_pipnet_amd.attribution import attribute              # noqa: E402
from count_pipnet_amd.synthetic import synth_images             # noqa: E402

THRESHOLD = 0.1


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def scale_row(net, x, want: int) -> int:
    """Scale the predicted class's classifier row so that ``want`` contributions exceed THRESHOLD."""
    with torch.no_grad():
        _, pooled, out = net(x.unsqueeze(0))
        c = int(out[0].argmax())
        contrib = torch.sort(pooled[0] * net._classification.weight[c], descending=True).values
        want = min(want, int((contrib > 0).sum()) - 1)
        mid = float(contrib[want - 1] + contrib[want]) / 2
        net._classification.weight[c] *= THRESHOLD / mid
    return c


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--active", type=int, default=16)
    ap.add_argument("--steps", type=int, default=192)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--post-repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_saliency: no ROCm GPU visible (there is no CPU fallback)")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def row(name, what, ts):
        say(f"{name:<10} {what:<58} least {min(ts):9.2f} ms   median {statistics.median(ts):9.2f} ms   "
            f"({len(ts)} runs)")

    net, _ = bench.make_net(dev)
    net.eval()
    x = synth_images(1, 224, seed=21)[0].to(dev)
    c = scale_row(net, x, a.active)
    active = S.active_prototypes(net, x, c, THRESHOLD)
    t = len(active.indices)
    kw = dict(kind="prototype", method="ig", steps=a.steps, batch_size=a.batch_size)
    say(f"ConvNeXt-tiny-26 PIP-Net, 224^2, class {c}, {t} active prototypes (threshold {THRESHOLD}), ig, "
        f"{a.steps} steps in chunks of {a.batch_size}; {torch.cuda.get_device_name(0)}")

    def device_post(maps):
        sal = S.normalize_maps(maps, 98.0)
        return sal, S.blend_maps(sal.normalized), S.unnormalize_image(x)

    def host_post(maps):
        m = maps.cpu().numpy()
        sal = R.normalize_maps(m, 98.0)
        return sal, R.blend(sal["normalized"]), R.unnormalize(x.cpu().numpy())

    _, attr = clock(lambda: attribute(net, x, active.indices, **kw))                    # warm-up of every part
    device_post(attr.maps), host_post(attr.maps), S.active_prototypes(net, x, c, THRESHOLD)
    t_sel = [clock(lambda: S.active_prototypes(net, x, c, THRESHOLD))[0] for _ in range(a.post_repeats)]
    t_attr = [clock(lambda: attribute(net, x, active.indices, **kw))[0] for _ in range(a.repeats)]
    t_dev, t_host = [], []
    for _ in range(a.post_repeats):                                                      # alternated
        t_dev.append(clock(lambda: device_post(attr.maps))[0])
        t_host.append(clock(lambda: host_post(attr.maps))[0])
    t_copy = [clock(lambda: attr.maps.cpu())[0] for _ in range(a.post_repeats)]
    t_whole = [clock(lambda: S.interpret_prototypes(net, x, c, steps=a.steps, batch_size=a.batch_size))[0]
               for _ in range(a.repeats)]
    row("select", "active_prototypes (forward + one index read)", t_sel)
    row("attribute", f"attribute(kind='prototype'), {t} targets", t_attr)
    row("device", "normalize_maps + blend_maps + unnormalize_image (HIP)", t_dev)
    row("host", "maps.cpu() + saliency_ref fold/percentile/normalise/blend", t_host)
    row("copy", f"of which maps.cpu(), {attr.maps.numel() * 4 / 1e6:.1f} MB", t_copy)
    row("whole", "interpret_prototypes, one call", t_whole)
    sal, overlay, image = device_post(attr.maps)
    ref, ref_overlay, ref_image = host_post(attr.maps)
    same = (bool((sal.normalized.cpu().numpy() == ref["normalized"]).all()) and
            bool((overlay.cpu().numpy() == ref_overlay).all()) and bool((image.cpu().numpy() == ref_image).all()))
    say(f"device results equal the host results bit for bit: {same}; rules {sal.rule.tolist()}")
    say(f"post-processing host / device = {min(t_host) / min(t_dev):.1f}; post-processing share of the whole call: "
        f"device {min(t_dev) / min(t_whole) * 100:.3f} %, host {min(t_host) / (min(t_attr) + min(t_host)) * 100:.3f} %")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
