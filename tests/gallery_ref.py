"""Plain restatements of what count_pipnet_amd.gallery must reproduce, written from the reference's statements
and from torchvision's published ``make_grid`` rather than from the module under test:

* the PIP-Net (util/vis_pipnet.py:278-313) and CountPIPNet (:758-838) selection of the entries a prototype's
  grid shows, over plain lists, statement by statement;
* ``make_grid(patches, nrow, padding=1, pad_value=40/255.)[:, 1:-1, :]`` in numpy on uint8 HWC patches (the
  uint8 round trip through ToTensor / ToPILImage is the identity: tests/test_gallery_cpu.py), its single-image
  branch included;
* the outline rule of ``ImageDraw.rectangle(outline=, width=)`` (held against Pillow in test_gallery_cpu.py);
* the frame: Pillow's resize as the project's own oracle restates it (oracle/input_ref.py).
"""
import math

import numpy as np

from oracle import input_ref

PATCH = 32
PAD = 40


# ---- selection ------------------------------------------------------------------------------------------
def pipnet_selection(scores, index, selected, unused):
    """vis_pipnet.py:278-313 over ``scores`` / ``index`` [P][1][k] lists: {p: [(group position, slot), ...]} of
    the prototypes that get a grid.  ``selected`` = the prototypes of ``prototype_storage``; ``unused`` is
    recomputed here (:279-288) and must agree with the pass's flag."""
    prototype_storage = {p: [dict(score=scores[p][0][j], slot=j) for j in range(len(index[p][0])) if index[p][0][j] >= 0]
                         for p in range(len(index)) if selected[p]}
    prototypes_not_used = []
    for p, images in prototype_storage.items():
        found_significant = False
        for img_data in images:
            if img_data['score'] > 0.1:
                found_significant = True
                break
        if not found_significant:
            prototypes_not_used.append(p)
    assert prototypes_not_used == [p for p in range(len(index)) if unused[p]]
    shown = {}
    for p, images in prototype_storage.items():
        if p in prototypes_not_used:
            continue
        if len(images) > 0:
            shown[p] = [(0, img_data['slot']) for img_data in images]
    return shown


def count_selection(scores, index, groups, selected, k):
    """vis_pipnet.py:758-838 over ``scores`` / ``index`` [P][G][k] lists (``groups`` = the count of each group
    position, ``available_counts``): {p: [(group position, slot), ...]} of the prototypes that get a grid."""
    available_counts = groups
    topk_storage = {p: {count: [(scores[p][g][j], dict(count_group=count, model_count=scores[p][g][j], entry=(g, j)))
                                for j in range(len(index[p][g])) if index[p][g][j] >= 0]
                        for g, count in enumerate(available_counts)}
                    for p in range(len(index)) if selected[p]}
    prototype_selected_images = {}
    for p in topk_storage.keys():
        prototype_selected_images[p] = []
        for count in available_counts:
            prototype_selected_images[p].extend([item[1] for item in topk_storage[p][count]])
    prototypes_not_used = []
    for p, images in prototype_selected_images.items():
        if len(images) == 0:
            prototypes_not_used.append(p)
    shown = {}
    for p, images in prototype_selected_images.items():
        if p in prototypes_not_used:
            continue
        count_groups = {}
        for img_data in images:
            count = img_data['count_group']
            if count not in count_groups:
                count_groups[count] = []
            count_groups[count].append(img_data)
        uniform_samples = []
        if len(count_groups) > 0:
            samples_per_group = k // len(count_groups)
            extra_samples = k % len(count_groups)
            for count, count_images in sorted(count_groups.items()):
                sorted_images = sorted(count_images, key=lambda x: x['model_count'], reverse=True)
                samples_to_take = samples_per_group + (1 if extra_samples > 0 else 0)
                extra_samples -= 1 if extra_samples > 0 else 0
                uniform_samples.extend(sorted_images[:min(samples_to_take, len(sorted_images))])
        if len(uniform_samples) < k:
            unused_images = []
            for count, count_images in count_groups.items():
                sorted_images = sorted(count_images, key=lambda x: x['model_count'], reverse=True)
                samples_to_take = samples_per_group + (1 if count in list(sorted(count_groups.keys()))[:extra_samples] else 0)
                if len(sorted_images) > samples_to_take:
                    unused_images.extend(sorted_images[samples_to_take:])
            unused_images.sort(key=lambda x: x['model_count'], reverse=True)
            uniform_samples.extend(unused_images[:min(k - len(uniform_samples), len(unused_images))])
        uniform_samples = uniform_samples[:k]
        uniform_samples.sort(key=lambda x: x['model_count'], reverse=True)
        if len(images) > 0:
            shown[p] = [img_data['entry'] for img_data in uniform_samples]
    return shown


def selection(res):
    """{p: entries} of a host PrototypeTopK."""
    scores, index = res.scores.tolist(), res.index.tolist()
    if res.groups == [None]:
        return pipnet_selection(scores, index, res.selected.tolist(), res.unused.tolist())
    return count_selection(scores, index, res.groups, res.selected.tolist(), res.scores.shape[2])


# ---- make_grid ----------------------------------------------------------------------------------------------
def make_grid(patches, nrow, padding=1, pad_value=PAD):
    """torchvision.utils.make_grid on a list of HxWx3 uint8 arrays (HWC here, CHW there)."""
    tensor = np.stack(patches, axis=0)                  # torch.stack: raises when the shapes differ
    if tensor.shape[0] == 1:
        return tensor[0]
    nmaps = tensor.shape[0]
    xmaps = min(nrow, nmaps)
    ymaps = int(math.ceil(float(nmaps) / xmaps))
    height, width = int(tensor.shape[1] + padding), int(tensor.shape[2] + padding)
    grid = np.full((height * ymaps + padding, width * xmaps + padding, 3), pad_value, np.uint8)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= nmaps:
                break
            grid[y * height + padding:y * height + height, x * width + padding:x * width + width] = tensor[k]
            k = k + 1
    return grid


def patch_grid(patches, k, pad_value=PAD):
    """``make_grid(patches, nrow=k, padding=1, pad_value)[:, 1:-1, :]``, or None where it raises."""
    try:
        grid = make_grid(patches, k, 1, pad_value)
    except ValueError:
        return None
    return grid[1:-1]


# ---- rectangle --------------------------------------------------------------------------------------------------
def draw_rect(frame, rect, width, colour=(255, 255, 0)):
    """``frame`` (HxWx3 uint8) with the outline of (x0, y0, x1, y1), both corners inclusive."""
    x0, y0, x1, y1 = rect
    yy, xx = np.mgrid[0:frame.shape[0], 0:frame.shape[1]]
    line = (xx >= x0) & (xx <= x1) & (yy >= y0) & (yy <= y1) & \
        ((xx < x0 + width) | (xx > x1 - width) | (yy < y0 + width) | (yy > y1 - width))
    out = frame.copy()
    out[line] = colour
    return out


# ---- hand-built pass results ------------------------------------------------------------------------------------
def build_topk(pn, groups, k, lists, selected=None, window=(0, 32, 0, 32)):
    """A host PrototypeTopK from ``lists[(p, group position)] = [(score, dataset index[, (h0, h1, w0, w1)]), ...]``
    in slot order; empty slots as prototype_topk leaves them.  ``unused`` by its definition."""
    import torch
    from count_pipnet_amd.topk import PrototypeTopK
    g = len(groups)
    scores = torch.zeros(pn, g, k)
    index = torch.full((pn, g, k), -1, dtype=torch.int64)
    coords = torch.full((pn, g, k, 4), -1, dtype=torch.int64)
    for (p, gi), items in lists.items():
        for j, item in enumerate(items):
            scores[p, gi, j], index[p, gi, j] = item[0], item[1]
            coords[p, gi, j] = torch.tensor(item[2] if len(item) > 2 else window)
    sel = torch.ones(pn, dtype=torch.bool) if selected is None else torch.tensor(selected, dtype=torch.bool)
    loc = torch.where(index >= 0, torch.zeros_like(index), index)
    return PrototypeTopK(scores=scores, index=index, h_idx=loc, w_idx=loc.clone(), coords=coords,
                         abstained=torch.zeros((), dtype=torch.int64), selected=sel,
                         unused=sel & ~(scores > 0.1).flatten(1).any(dim=1), groups=list(groups),
                         proto_shape=(1, pn, 8, 8))


# ---- frames and the two results ---------------------------------------------------------------------------------
def frame(img, size):
    return input_ref.eval_transform(img, (size, size))[1]


def expected_gallery(res, frame_of, image_size, pad_value=PAD):
    """What prototype_gallery must return for the host PrototypeTopK ``res``; ``frame_of(i)`` is the resized
    frame of dataset index i.  Arrays under the field names of PrototypeGallery (``frames`` always)."""
    pn, _, k = res.scores.shape
    shown = selection(res)
    out = dict(grids=np.full((pn, PATCH, k * (PATCH + 1) + 1, 3), pad_value, np.uint8),
               height=np.zeros(pn, np.int64), width=np.zeros(pn, np.int64), cells=np.zeros(pn, np.int64),
               ok=np.ones(pn, bool), entry_index=-np.ones((pn, k), np.int64), entry_group=-np.ones((pn, k), np.int64),
               entry_slot=-np.ones((pn, k), np.int64), entry_score=np.zeros((pn, k), np.float32),
               entry_coords=-np.ones((pn, k, 4), np.int64))
    drawn = set()
    for p, entries in shown.items():
        patches = []
        for c, (g, j) in enumerate(entries):
            i = int(res.index[p, g, j])
            h0, h1, w0, w1 = res.coords[p, g, j].tolist()
            out["entry_index"][p, c], out["entry_group"][p, c], out["entry_slot"][p, c] = i, g, j
            out["entry_score"][p, c], out["entry_coords"][p, c] = float(res.scores[p, g, j]), (h0, h1, w0, w1)
            patches.append(frame_of(i)[h0:h1, w0:w1])
        grid = patch_grid(patches, k, pad_value)
        if grid is None:
            out["ok"][p] = False
            continue
        out["height"][p], out["width"][p], out["cells"][p] = grid.shape[0], grid.shape[1], len(entries)
        out["grids"][p, :grid.shape[0], :grid.shape[1]] = grid
        drawn |= {int(res.index[p, g, j]) for g, j in entries}
    out["frame_index"] = np.array(sorted(drawn), np.int64)
    out["frames"] = np.stack([frame_of(i) for i in sorted(drawn)]) if drawn else \
        np.zeros((0, image_size, image_size, 3), np.uint8)
    return out


def expected_explanations(res, frames, width=2):
    """What explanation_images must return for the host LocalExplanation ``res`` and the resized ``frames``
    [B,S,S,3] (numpy): arrays under the field names of ExplanationImages."""
    b, c, m = res.prototype.shape
    entry, patches, hw, rects = [], [], [], []
    for bi in range(b):
        for r in range(c):
            for j in range(min(int(res.count[bi, r]), m)):
                h0, h1, w0, w1 = res.coords[bi, r, j].tolist()
                cut = frames[bi][h0:h1, w0:w1]
                pad = np.zeros((PATCH, PATCH, 3), np.uint8)
                pad[:cut.shape[0], :cut.shape[1]] = cut
                entry.append((bi, r, j))
                patches.append(pad)
                hw.append(cut.shape[:2])
                rects.append(draw_rect(frames[bi], res.rect[bi, r, j].tolist(), width))
    s = frames.shape[1]
    return dict(entry=np.array(entry, np.int64).reshape(-1, 3),
                patches=np.stack(patches) if patches else np.zeros((0, PATCH, PATCH, 3), np.uint8),
                patch_hw=np.array(hw, np.int64).reshape(-1, 2),
                rects=np.stack(rects) if rects else np.zeros((0, s, s, 3), np.uint8))
