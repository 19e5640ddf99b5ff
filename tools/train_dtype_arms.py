"""The --train-dtype arms of tools/bench_train.py and tools/bench_train_count.py: one training step timed with its
frozen layers in each requested arithmetic (pipnet.set_hip_train_dtype), the arms alternating in one process on one
net, so clock and thermal drift fall on every arm alike.

Every arm's shapes are warmed up first; then each repeat runs the arms in turn, each for at least ``min_seconds`` of
back-to-back steps between two device events (no host synchronisation inside).  Reported per arm: the median ms per
iteration over the repeats with the fastest and slowest repeat, and images per second at the median.
"""
from __future__ import annotations

import math
import statistics

import torch

from count_pipnet_amd.pipnet import set_hip_train_dtype


def _event_ms(step, n: int) -> float:
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(n):
        step()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def timed_at_least(step, min_seconds: float) -> float:
    """ms per step over one run of >= ``min_seconds`` between device events (the step count from a 3-step probe)."""
    n = max(3, math.ceil(min_seconds * 1e3 / (_event_ms(step, 3) / 3.0)) + 1)
    while True:
        ms = _event_ms(step, n)
        if ms >= min_seconds * 1e3:
            return ms / n
        n = math.ceil(n * 1.5 * min_seconds * 1e3 / ms)


def compare(net, step, arms, images: int, repeats: int, warmup: int, min_seconds: float) -> dict:
    """``step()`` is one iteration on ``net``; returns {arm: ms_per_iter (median), ms_min, ms_max, images_per_sec,
    repeats: [ms, ...]} with the arms alternated ``repeats`` times."""
    for arm in arms:                              # every shape of every arm: weight packs, workspaces, code objects
        set_hip_train_dtype(net, arm)
        for _ in range(warmup):
            step()
    torch.cuda.synchronize()
    runs = {arm: [] for arm in arms}
    for _ in range(repeats):
        for arm in arms:
            set_hip_train_dtype(net, arm)
            runs[arm].append(timed_at_least(step, min_seconds))
    set_hip_train_dtype(net, "fp32")
    out = {}
    for arm, ms in runs.items():
        med = statistics.median(ms)
        out[arm] = {"ms_per_iter": med, "ms_min": min(ms), "ms_max": max(ms), "images_per_sec": images / med * 1e3,
                    "repeats": ms}
    return out
