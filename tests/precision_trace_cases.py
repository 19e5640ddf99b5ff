"""The forward-only ConvNeXt executor in each of its precisions, as the library sees it.

``CASES`` maps a name to a function ``(gpu) -> (calls, digest)``: ``convnext_features_hip(net._net.features, xs, {},
sd_keep, precision)`` on a fresh net under ``train_trace_cases.record_calls()``.  A launch hook (``K.set_launch_hook``)
set for the length of the case adds ``[kernel name, flops.hex()]`` of every hooked launch to the same list, in call
order, so the labels and the flop counts the wrappers report are part of the trace.  ``digest`` is a sha256 over dtype,
shape and bytes of the returned NHWC features.

Twelve cases, two models x ``PRECISIONS`` x two modes:

* ``pipnet_mid_addon`` on 4 images of 64^2: 96 and 192 channels on 16 x 16 and 8 x 8 maps, below the fused-MLP
  thresholds (the fp32 arm runs the unfused pair), tiles 0, 4 and 7 of the low-precision GEMMs;
* ``c2_pipnet_convnext26`` on 2 images of 224^2: all four widths, the fused MLP, tile 5, stride-1 downsamples;
* eval (``sd_keep`` None) and train: ``forced_masks`` of tests/test_train_lowp_cpu.py, one dropped and one kept sample
  in every block with p > 0, so one forward runs the rowscale arm and (block 0, p = 0) the plain arm.

tests/golden/gen_precision_call_trace.py records both on the parent commit into
tests/golden/precision_call_trace.json; tests/test_gpu_precision_trace.py holds the tree to it.
"""
import hashlib

import torch

from count_pipnet_amd import kernels as K
from count_pipnet_amd.convnext_features import PRECISIONS, convnext_features_hip
from count_pipnet_amd.synthetic import synth_images
from golden_util import golden_args, load_golden
from model_util import build_model
from test_train_lowp_cpu import forced_masks
from train_trace_cases import record_calls

# (kernel name, argument position) pairs that differ between two runs of the parent and are left out
MASKED = ()
# model -> (images, image size, image seed, mask seed)
MODELS = {"pipnet_mid_addon": (4, 64, 640, 64), "c2_pipnet_convnext26": (2, 224, 224, 2)}


def features_digest(h):
    h = h.detach().cpu().contiguous()
    return hashlib.sha256(f"{h.dtype}|{tuple(h.shape)}|".encode() + h.numpy().tobytes()).hexdigest()


def forward(model, precision, train):
    def case(gpu):
        images, size, seed, mask_seed = MODELS[model]
        meta, _ = load_golden(model)
        net = build_model(meta).to(gpu)
        xs = synth_images(images, size, seed=seed).to(gpu)
        sd_keep = forced_masks(golden_args(meta), images, torch.Generator().manual_seed(mask_seed)) if train else None
        with record_calls(MASKED) as calls:
            K.set_launch_hook(lambda kname, flops, fn: (calls.append([kname, float(flops).hex()]), fn()))
            try:
                with torch.no_grad():
                    h = convnext_features_hip(net._net.features, xs, {}, sd_keep, precision)
            finally:
                K.set_launch_hook(None)
        return calls, features_digest(h)
    return case


CASES = {f"{model}_{precision}_{'train' if train else 'eval'}": forward(model, precision, train)
         for model in MODELS for precision in PRECISIONS for train in (False, True)}
