"""The local-explanation loop of util/visualize_prediction.py (:63-88 vis_pred, :138-168
vis_pred_experiments) restated on CPU tensors of ONE image, for the tests of
count_pipnet_amd.local / pipnet_local_explain_f32.

As in the reference: both orders come from a descending torch.sort (made stable, which fixes the
tie order the reference leaves to the sort), the keep test multiplies two Python floats
(``.item()`` values, read here through ``tolist()``), and the location is the two-step torch.max
on the prototype's map."""
import numpy as np
import torch


def reference_lists(proto, pooled, out, weight, top_classes=3, min_abs=0.01):
    """proto [1,P,H,W], pooled [1,P], out [1,K], weight [K,P] (CPU float32); ``top_classes`` None =
    all.  -> [(class, logit, [(prototype, sim, w, simweight, h_idx, w_idx), ...]), ...] by rank."""
    sorted_out_indices = torch.sort(out.squeeze(0), descending=True, stable=True).indices
    sorted_pooled_indices = torch.sort(pooled.squeeze(0), descending=True, stable=True).indices.tolist()
    pooled_f, out_f, weight_f = pooled[0].tolist(), out[0].tolist(), weight.tolist()      # .item() of each entry
    ranks = []
    for pred_class_idx in (sorted_out_indices if top_classes is None else sorted_out_indices[:top_classes]).tolist():
        entries = []
        for prototype_idx in sorted_pooled_indices:
            simweight = pooled_f[prototype_idx] * weight_f[pred_class_idx][prototype_idx]
            if abs(simweight) > min_abs:
                max_h, max_idx_h = torch.max(proto[0, prototype_idx, :, :], dim=0)
                max_w, max_idx_w = torch.max(max_h, dim=0)
                max_idx_h = max_idx_h[max_idx_w].item()
                max_idx_w = max_idx_w.item()
                entries.append((prototype_idx, pooled_f[prototype_idx], weight_f[pred_class_idx][prototype_idx],
                                simweight, max_idx_h, max_idx_w))
        ranks.append((pred_class_idx, out_f[pred_class_idx], entries))
    return ranks


def pack(images, max_entries):
    """[reference_lists(...) per image] -> the arrays of the kernel's layout: classes, logits, count
    [B,C]; prototype, similarity, weight, simweight, h_idx, w_idx [B,C,M], the lists cut at
    ``max_entries``, empty slots (-1, 0, 0, 0, -1, -1), the product rounded to float32."""
    b, c, m = len(images), len(images[0]), max_entries
    res = {"classes": -np.ones((b, c), np.int64), "logits": np.zeros((b, c), np.float32),
           "count": np.zeros((b, c), np.int64), "prototype": -np.ones((b, c, m), np.int64),
           "similarity": np.zeros((b, c, m), np.float32), "weight": np.zeros((b, c, m), np.float32),
           "simweight": np.zeros((b, c, m), np.float32), "h_idx": -np.ones((b, c, m), np.int64),
           "w_idx": -np.ones((b, c, m), np.int64)}
    for i, ranks in enumerate(images):
        assert len(ranks) == c
        for r, (cls, logit, entries) in enumerate(ranks):
            res["classes"][i, r], res["logits"][i, r], res["count"][i, r] = cls, logit, len(entries)
            for j, (p, sim, w, simweight, h_idx, w_idx) in enumerate(entries[:m]):
                res["prototype"][i, r, j], res["h_idx"][i, r, j], res["w_idx"][i, r, j] = p, h_idx, w_idx
                res["similarity"][i, r, j], res["weight"][i, r, j] = sim, w
                res["simweight"][i, r, j] = np.float32(simweight)
    return res
