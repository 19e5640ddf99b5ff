"""Device and host-enqueue time of the soft Gumbel head's entry point (``kernels.count_gumbel_soft``), which takes
and returns a stream-ordered scratch for its workgroups' partial sums on every call.  A host wait
separates the calls, as one separates training steps, so a pool that gives memory back at a wait shows its cost.

    python tools/time_soft_gumbel.py
"""
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from count_pipnet_amd import kernels as K  # noqa: E402

dev = torch.device("cuda:0")
for b, h, w, p in [(128, 28, 28, 768), (12, 8, 8, 16)]:
    logits = torch.randn(b, h, w, p, device=dev)
    for _ in range(3):
        K.count_gumbel_soft(logits, 0.8, None, 5)
    torch.cuda.synchronize()
    dev_ms, host_ms = [], []
    for _ in range(15):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        K.count_gumbel_soft(logits, 0.8, None, 5)
        e1.record()
        host_ms.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        dev_ms.append(e0.elapsed_time(e1))
    print(f"{(b, h, w, p)}: device median {statistics.median(dev_ms):.3f} ms (min {min(dev_ms):.3f}, "
          f"max {max(dev_ms):.3f}); host enqueue median {statistics.median(host_ms):.3f} ms "
          f"(max {max(host_ms):.3f})", flush=True)
