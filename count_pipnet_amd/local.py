"""Local explanations, on the device -- the per-image pass of ``util/visualize_prediction.py``.

For one prediction the reference asks which prototypes were found in the image, where, and how
much each adds to each top class (``vis_pred`` :63-88: the 3 best classes; ``vis_pred_experiments``
:138-168: every class).  It runs at batch size 1 and does, per (class, prototype) pair, two
``.item()`` reads and a Python multiply, and per kept pair the two-step ``torch.max`` on a map.
``explain_predictions`` computes the same lists for a whole batch with no host synchronisation:

  PIP-Net      backbone + add-on logits -> fused softmax + max-pool + arg-location (the proto map
               is never written) -> threshold + NonNegLinear -> per-image selection kernel
  CountPIPNet  the existing forward -> arg-location on its 0/1 map -> per-image selection kernel

The selection (pipnet_local_explain_f32) ranks the classes, orders the prototypes and compacts, for
each top class, the prototypes whose contribution passes the reference's test.  Decoding the image,
cropping, drawing the rectangle, PNG writing and file names stay with the caller.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import kernels as K
from .explain_forward import (PATCH_SIZE, HostCopy, is_count, located_forward, map_is_small, note_map, patch_geometry,
                              patch_skip, unwrap)

MIN_SIMWEIGHT = 0.01            # visualize_prediction.py:75: abs(simweight) > 0.01


@dataclass
class LocalExplanation(HostCopy):
    """Result of ``explain_predictions``; tensors stay on the device until ``.cpu()`` is asked for.
    C = class ranks (rank 0 = the largest logit), M = ``max_entries`` slots per (image, class) in
    prototype order (pooled score descending, lower index first among equals).  Empty slots hold
    -1 in every index, coordinate and rectangle field and 0 in the float fields."""
    classes: Tensor       # [B, C] int64 class index by rank
    logits: Tensor        # [B, C] float32 logit of each ranked class
    count: Tensor         # [B, C] int64 kept prototypes of the class; > max_entries: the list is truncated
    prototype: Tensor     # [B, C, M] int64
    similarity: Tensor    # [B, C, M] float32 pooled score (count) of the kept prototype
    weight: Tensor        # [B, C, M] float32 weight entry used
    simweight: Tensor     # [B, C, M] float32 their product
    h_idx: Tensor         # [B, C, M] int64 latent row of the prototype's maximum
    w_idx: Tensor         # [B, C, M] int64 latent column
    coords: Tensor        # [B, C, M, 4] int64 (h_min, h_max, w_min, w_max): the patch the reference crops
    rect: Tensor          # [B, C, M, 4] int64 (x0, y0, x1, y1): the rectangle the reference draws (:87)
    proto_shape: Tuple[int, int, int, int]   # (1, P, H, W) handed to img_coordinates


def count_importance_matrix(net, classifier_input_scalars: Optional[Tensor] = None) -> Tensor:
    """[K, P] with column p = ``net.get_prototype_importance_per_class(p, classifier_input_scalars)``:
    what one unit of prototype p's classifier inputs adds to each class.  ``vis_pred`` indexes
    ``_classification.weight[c, p]``, which means that only while the classifier's input width is
    P; for the identity intermediate layer the two are equal.  With scalars (the dataset's mean
    intermediate features) it is the virtual classification matrix of count_pipnet.py:312-321."""
    if classifier_input_scalars is not None:      # the layer builds its input weights where it likes (one-hot: host)
        classifier_input_scalars = classifier_input_scalars.to(
            net._intermediate.prototype_to_classifier_input_weights(0).device)
    return torch.stack([net.get_prototype_importance_per_class(p, classifier_input_scalars)
                        for p in range(net._num_prototypes)], dim=1)


def explain_predictions(net, xs: Tensor, top_classes: Optional[int] = 3, *, image_size: int,
                        min_simweight: float = MIN_SIMWEIGHT, max_entries: int = 64,
                        weight: Optional[Tensor] = None) -> LocalExplanation:
    """For every image of the batch ``xs`` the ``top_classes`` best classes (None: all, as
    ``vis_pred_experiments``; 3: ``vis_pred``) and, for each, the prototypes p with
    ``abs(pooled[p] * weight[c, p]) > min_simweight`` in the reference's order, with their scores,
    weights, products, latent locations, image patches and rectangles -- the lists of
    visualize_prediction.py:63-88 / :138-168 at any batch size.

    ``net``: a PIPNet / CountPIPNet on a ROCm device, bare, under a ``.module`` wrapper, or in a
    world-size-1 ShardedInference; it is put in eval mode, as the reference does.  Every image gets
    the bits of its own batch-1 forward, so the result does not depend on the batching.  Ties are
    decided by the lower index (classes and prototypes alike) and the keep test is evaluated on the
    fp64 product, as the reference's Python floats are.  ``weight`` [K, P] replaces the default:
    ``_classification.weight`` for PIP-Net, the per-class prototype importance for CountPIPNet
    (``count_importance_matrix``).  ``count`` holds the true number of kept prototypes; only the
    first ``max_entries`` are stored.  Nothing in the call waits for the device."""
    net = unwrap(net, "explain_predictions")
    net.eval()
    count = is_count(net)
    pn = net._num_prototypes
    kc = net._classification.weight.shape[0]
    c = kc if top_classes is None else int(top_classes)
    if not 1 <= c <= kc:
        raise ValueError(f"explain_predictions: top_classes must be in 1..{kc} (or None), got {top_classes}")
    if max_entries < 1:
        raise ValueError(f"explain_predictions: max_entries must be at least 1, got {max_entries}")
    if not min_simweight >= 0:
        raise ValueError(f"explain_predictions: min_simweight must be >= 0, got {min_simweight}")
    K.require_device(xs, "input images")
    dev = xs.device
    with torch.no_grad():
        if weight is not None:
            if tuple(weight.shape) != (kc, pn):
                raise ValueError(f"explain_predictions: weight {tuple(weight.shape)} must be "
                                 f"[classes, prototypes] = {(kc, pn)}")
            w = weight.detach().to(device=dev, dtype=torch.float32)
            if w.stride(1) != 1:
                w = w.contiguous()
        elif count:
            w = count_importance_matrix(net).to(device=dev, dtype=torch.float32)
        else:
            w = net._classification.weight.detach()
        fwd = located_forward(net, xs, map_is_small(net, xs))
        note_map(net, xs, fwd.hw)
        cls, cls_logit, n, e_proto, e_sim, e_w, e_simw, e_loc = K.local_explain(
            fwd.scores, fwd.loc, fwd.out, w, c, max_entries, min_simweight)
        empty = e_proto < 0
        h_idx, w_idx, coords, shape = patch_geometry(e_loc, empty, pn, fwd.hw[0], fwd.hw[1], image_size)
        skip = patch_skip(image_size, fwd.hw[1])
        rect = torch.stack((w_idx * skip, h_idx * skip, torch.clamp(w_idx * skip + PATCH_SIZE, max=image_size),
                            torch.clamp(h_idx * skip + PATCH_SIZE, max=image_size)), dim=-1)      # empty slots: masked below
        return LocalExplanation(
            classes=cls.long(), logits=cls_logit, count=n.long(), prototype=e_proto.long(), similarity=e_sim,
            weight=e_w, simweight=e_simw, h_idx=h_idx, w_idx=w_idx, coords=coords,
            rect=rect.masked_fill(empty.unsqueeze(-1), -1), proto_shape=shape)
