"""Prototype galleries and explanation patches, on the device -- the pixel half of ``util/vis_pipnet.py`` and
``util/visualize_prediction.py``.

``topk.prototype_topk`` and ``local.explain_predictions`` stop at dataset indices and patch coordinates.  The
reference goes on, per entry and on the host: open the file, Pillow resize, ``ToTensor``, crop the window,
``torchvision.utils.make_grid(..., nrow=k, padding=1, pad_value=40/255.)[:, 1:-1, :]``, ``ToPILImage``
(vis_pipnet.py:298-319, :758-849), or crop and ``ImageDraw.rectangle`` (visualize_prediction.py:80-88).
``ToTensor`` followed by ``mul(255).byte()`` returns every uint8 value unchanged and ``40/255.`` comes back as
40, so all of it is integer copying of the resized uint8 frame, which ``pipnet_resize_normalize_rgb8`` writes
bit-identically to Pillow:

  prototype_gallery    selection of the shown entries (host, the tables are P * G * k small) -> the distinct
                       images decoded once each, ``batch_size`` at a time -> resized on the device -> one
                       ``pipnet_patch_compose_rgb8`` launch per chunk lays the windows into the grids
  explanation_images   per stored entry the patch (same kernel) and the frame with the rectangle
                       outlined (``pipnet_draw_rects_rgb8``)
  explanation_heatmaps / similarity_heatmaps
                       per entry ``heatmap_p{p}.png`` (visualize_prediction.py:92-100): the prototype's
                       similarity map as bytes, Pillow's bicubic resize to the frame, the colour table and
                       the float32 blend ``0.2 * colour + 0.6 * image`` that ``plt.imsave`` turns into bytes,
                       bit for bit and in one ``pipnet_heatmap_rgb8`` launch per ``batch_size`` entries; the
                       map is read from the forward's own NHWC tensor
  prototype_map_overlays / feature_map_overlays
                       per entry the arrays behind ``feature_maps/prototype_{p}/*_overlay.png``
                       (vis_pipnet.py:454-475, :1000-1021): the prototype's similarity map, its
                       ``scipy.ndimage.zoom`` to the image (a cubic B-spline in float64), ``mask = resized > 0.1``
                       and the RGBA overlay ``(*cmap(resized[y, x])[:3], 0.7)`` the reference fills in a Python
                       loop over the pixels, bit for bit and in one ``pipnet_map_overlay`` launch per
                       ``batch_size`` entries; ``select_map_entries`` is the rule that picks up to three stored
                       images per prototype (:362-391, :897-922)

Only ``prototype_map_overlays`` runs a model forward (the pass keeps no maps, so the selected images go through
the located forward once more).  The reference opens the files without ``.convert("RGB")``; for RGB and 8-bit
grey files the pixels it crops are those of the loader's ``convert("RGB")`` (a grey file gives a grey grid in
three equal bands instead of one), and that is the contract: palette and alpha files follow the loader's
``convert("RGB")``, where the reference would resize palette indices or keep the alpha band.  The label strip,
its text, ``grid_topk_all.png``, file names and PNG encoding stay with the caller; so do, for the heatmaps, the
colour table itself (OpenCV's JET is an argument, not shipped) and the alpha band of 255 that ``plt.imsave`` adds,
and for the overlays the viridis table (an argument: ``matplotlib.colormaps['viridis'](np.arange(256))[:, :3]``)
and the matplotlib figures themselves: titles, the rectangle, the colour bar, ``*_original.png`` and
``*_feature_map.png``.

``make_grid``'s rule is restated from torchvision's published source (the package is not a dependency).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import kernels as K
from .convnext_features import as_nhwc
from .data import DeviceEvalTransform, pack_images
from .explain_forward import PATCH_SIZE, HostCopy, located_forward_maps, map_is_small, note_map, unwrap
from .local import LocalExplanation
from .topk import PrototypeTopK

GRID_PADDING = 1                # make_grid(padding=1)
GRID_PAD_VALUE = 40             # pad_value=40/255. after ToPILImage


@dataclass
class PrototypeGallery(HostCopy):
    """Result of ``prototype_gallery``.  ``Image.fromarray(g.grids[p, :g.height[p], :g.width[p]].cpu().numpy())``
    is the patch part of the reference's ``grid_topk_{p}.png``.  The pixel tensors stay on the device until
    ``.cpu()`` is asked for; the small tables are built on the host and stay there."""
    grids: Tensor          # [P, 32, k * 33 + 1, 3] uint8 (device); outside [:height, :width]: pad_value
    height: Tensor         # [P] int64 rows of the grid (32; 30 for a single patch; 0: no grid)
    width: Tensor          # [P] int64 columns: cells * 33 + 1 (32 for a single patch; 0: no grid)
    cells: Tensor          # [P] int64 patches in the grid; 0: the reference writes no file for p
    ok: Tensor             # [P] bool; False: the windows differ in size, the reference's make_grid raises
    entry_index: Tensor    # [P, k] int64 dataset index of the cell's image, in grid order; -1: empty
    entry_group: Tensor    # [P, k] int64 group (position in res.groups) the entry comes from
    entry_slot: Tensor     # [P, k] int64 its slot there: res.scores[p, entry_group, entry_slot]
    entry_score: Tensor    # [P, k] float32
    entry_coords: Tensor   # [P, k, 4] int64 (h_min, h_max, w_min, w_max)
    frame_index: Tensor    # [F] int64 the distinct dataset indices of the drawn entries, ascending
    frames: Optional[Tensor]      # [F, S, S, 3] uint8 (device) resized images of frame_index; None unless keep_frames


@dataclass
class ExplanationImages(HostCopy):
    """Result of ``explanation_images``: one row per stored entry of a ``LocalExplanation``, in (b, r, j) order."""
    entry: Tensor          # [N, 3] int64 (image b, class rank r, slot j)
    patches: Tensor        # [N, 32, 32, 3] uint8 (device): the window coords[b, r, j] at the top left, 0 beyond patch_hw
    patch_hw: Tensor       # [N, 2] int64 (rows, columns) of the window
    rects: Tensor          # [N, S, S, 3] uint8 (device): the frame of image b with rect[b, r, j] outlined


@dataclass
class ExplanationHeatmaps(HostCopy):
    """Result of ``explanation_heatmaps``: one row per stored entry of a ``LocalExplanation``, in (b, r, j) order,
    the rows of ``ExplanationImages``.  ``plt.imsave`` adds an alpha band of 255 to these pixels."""
    entry: Tensor          # [N, 3] int64 (image b, class rank r, slot j)
    prototype: Tensor      # [N] int64 the entry's prototype p: the file is heatmap_p{p}.png
    heatmaps: Tensor       # [N, S, S, 3] uint8 (device): the similarity map of p over the frame of image b


@dataclass
class PrototypeMapOverlays(HostCopy):
    """Result of ``prototype_map_overlays``: one row per shown entry, prototypes ascending and within a prototype
    in file order.  PIP-Net names the files ``proto_{p}_rank_{rank}_of_{of}_score_{score:.3f}``, CountPIPNet
    ``proto_{p}_count_{groups[g]}_model_count_{score:.1f}_class_{label}``.  The pixel tensors stay on the device
    until ``.cpu()`` is asked for; the small tables are built on the host and stay there."""
    entry: Tensor          # [N, 3] int64 (prototype p, group position g, slot j): res.scores[p, g, j]
    rank: Tensor           # [N] int64 i + 1 of the entry among its prototype's
    of: Tensor             # [N] int64 how many entries its prototype has
    index: Tensor          # [N] int64 dataset index of the image
    score: Tensor          # [N] float32
    coords: Tensor         # [N, 4] int64 (h_min, h_max, w_min, w_max): the rectangle
    h_idx: Tensor          # [N] int64 latent row of the maximum: the red cross of *_feature_map.png
    w_idx: Tensor          # [N] int64 latent column
    maps: Tensor           # [N, h, w] float32 (device): feature_map_np
    map_sum: Tensor        # [N] float64: the map summed in float64, row-major from the first element on
    resized: Tensor        # [N, S, S] float32 (device): zoom(feature_map_np, (S / h, S / w))
    mask: Tensor           # [N, S, S] uint8 (device): resized > 0.1
    colour: Tensor         # [N, S, S] uint8 (device): the row of the colour table, 0 off the mask
    overlay: Optional[Tensor]     # [N, S, S, 4] float64 (device): what plt.imshow(overlay, alpha=0.7) is given; None unless wanted
    frame_index: Tensor    # [F] int64 the distinct dataset indices of the entries, ascending
    frames: Optional[Tensor]      # [F, S, S, 3] uint8 (device) resized images of frame_index; None unless keep_frames


# ---- selection (host) -------------------------------------------------------------------------------

def _pipnet_selection(index, selected, unused, p: int) -> List[Tuple[int, int]]:
    """vis_pipnet.py:298-313: a used prototype shows its stored images in list order."""
    if not selected[p] or unused[p]:
        return []
    return [(0, j) for j, i in enumerate(index[p][0]) if i >= 0]


def _count_selection(scores, index, groups, selected, p: int, k: int) -> List[Tuple[int, int]]:
    """vis_pipnet.py:758-838 over the per-group lists of prototype p; an entry is (group position, slot).
    The statements are the reference's, its fill step included: by then ``extra_samples`` has been counted down
    to 0, so a group that took ``samples_per_group + 1`` offers its last taken entry again."""
    if not selected[p]:                                         # :656-661: no storage for the prototype
        return []
    images = [(g, j) for g in range(len(groups)) for j, i in enumerate(index[p][g]) if i >= 0]      # :760-764
    if len(images) == 0:                                        # :768-770, :781
        return []

    def score(e):
        return scores[p][e[0]][e[1]]

    count_groups = {}
    for e in images:                                            # :785-791
        count_groups.setdefault(groups[e[0]], []).append(e)
    samples_per_group = k // len(count_groups)                  # :797-798
    extra_samples = k % len(count_groups)
    uniform_samples = []
    for _, count_images in sorted(count_groups.items()):        # :801-809
        sorted_images = sorted(count_images, key=score, reverse=True)
        samples_to_take = samples_per_group + (1 if extra_samples > 0 else 0)
        extra_samples -= 1 if extra_samples > 0 else 0
        uniform_samples.extend(sorted_images[:min(samples_to_take, len(sorted_images))])
    if len(uniform_samples) < k:                                # :812-827
        unused_images = []
        for count, count_images in count_groups.items():
            sorted_images = sorted(count_images, key=score, reverse=True)
            samples_to_take = samples_per_group + (1 if count in list(sorted(count_groups.keys()))[:extra_samples] else 0)
            if len(sorted_images) > samples_to_take:
                unused_images.extend(sorted_images[samples_to_take:])
        unused_images.sort(key=score, reverse=True)
        uniform_samples.extend(unused_images[:min(k - len(uniform_samples), len(unused_images))])
    uniform_samples = uniform_samples[:k]                       # :830
    uniform_samples.sort(key=score, reverse=True)               # :833, stable: ties keep their order
    return uniform_samples


def select_entries(res: PrototypeTopK) -> List[List[Tuple[int, int]]]:
    """Per prototype the (group position, slot) entries the reference's grid shows, in grid order; an empty list
    where it writes no grid.  ``res`` on the host."""
    k = int(res.scores.shape[2])
    scores, index = res.scores.tolist(), res.index.tolist()
    selected, unused = res.selected.tolist(), res.unused.tolist()
    if res.groups == [None]:
        return [_pipnet_selection(index, selected, unused, p) for p in range(len(index))]
    return [_count_selection(scores, index, res.groups, selected, p, k) for p in range(len(index))]


def _pipnet_map_selection(scores, index, selected, unused, p: int, most: int) -> List[Tuple[int, int]]:
    """vis_pipnet.py:362-391: the highest, the middle and the lowest stored image that still exceeds 0.1."""
    if not selected[p] or unused[p]:
        return []
    slots = [j for j, i in enumerate(index[p][0]) if i >= 0]
    n = len(slots)
    if n == 0:
        return []
    picked = [0]
    if n > 2:
        picked.append(n // 2)
    if n > 1:
        lowest = n - 1
        while lowest > 0 and scores[p][0][slots[lowest]] < 0.1:
            lowest -= 1
        if lowest not in picked:
            picked.append(lowest)
    return [(0, slots[i]) for i in picked[:most]]


def _count_map_selection(index, groups, selected, p: int, most: int) -> List[Tuple[int, int]]:
    """vis_pipnet.py:897-922: per non-empty count group, counts ascending, the image with the largest model count.
    A group's list is sorted by it and ``sorted`` is stable, so that is the group's first stored slot."""
    if not selected[p]:
        return []
    order = sorted(range(len(groups)), key=lambda g: groups[g])
    first = [(g, next((j for j, i in enumerate(index[p][g]) if i >= 0), None)) for g in order]
    return [(g, j) for g, j in first if j is not None][:most]


def select_map_entries(res: PrototypeTopK, max_per_prototype: int = 3) -> List[List[Tuple[int, int]]]:
    """Per prototype the (group position, slot) entries whose feature maps the reference draws
    (``max_feature_maps_per_prototype``), in file order; an empty list where it draws none.  ``res`` on the host."""
    if isinstance(max_per_prototype, bool) or not isinstance(max_per_prototype, int) or max_per_prototype < 1:
        raise ValueError(f"select_map_entries: max_per_prototype must be an integer >= 1, got {max_per_prototype!r}")
    scores, index = res.scores.tolist(), res.index.tolist()
    selected, unused = res.selected.tolist(), res.unused.tolist()
    if res.groups == [None]:
        return [_pipnet_map_selection(scores, index, selected, unused, p, max_per_prototype) for p in range(len(index))]
    return [_count_map_selection(index, res.groups, selected, p, max_per_prototype) for p in range(len(index))]


# ---- geometry -----------------------------------------------------------------------------------------

def _window(coords: Sequence[int], size: int) -> Tuple[int, int, int, int]:
    """(h0, h1, w0, w1) of ``img[:, h_min:h_max, w_min:w_max]`` on a size x size image, as Python slices it."""
    h0, h1, _ = slice(coords[0], coords[1]).indices(size)
    w0, w1, _ = slice(coords[2], coords[3]).indices(size)
    return h0, max(h1, h0), w0, max(w1, w0)


def grid_layout(windows: Sequence[Tuple[int, int, int, int]]):
    """``make_grid(patches, nrow=k, padding=1)[:, 1:-1, :]`` of n <= k patches as copies: (height, width,
    [(h0, h1, w0, w1, y, x) per patch]), or None where ``make_grid`` raises (the windows differ in size) or
    nothing is left to show.  n >= 2: one row of cells, the canvas ``ph`` by ``n * (pw + 1) + 1``, patch j at
    column ``j * (pw + 1) + 1``; n == 1: ``make_grid`` returns the image unpadded, so the crop takes the patch's
    own first and last row."""
    ph, pw = windows[0][1] - windows[0][0], windows[0][3] - windows[0][2]
    if any((h1 - h0, w1 - w0) != (ph, pw) for h0, h1, w0, w1 in windows) or not (0 < ph <= PATCH_SIZE and
                                                                              0 < pw <= PATCH_SIZE):
        return None
    if len(windows) == 1:
        h0, h1, w0, w1 = windows[0]
        return (ph - 2, pw, [(h0 + 1, h1 - 1, w0, w1, 0, 0)]) if ph > 2 else None
    step = pw + GRID_PADDING
    return ph, len(windows) * step + GRID_PADDING, [(h0, h1, w0, w1, 0, j * step + GRID_PADDING)
                                                    for j, (h0, h1, w0, w1) in enumerate(windows)]


# ---- frames ---------------------------------------------------------------------------------------------

def _device(net, device) -> torch.device:
    if device is not None:
        dev = torch.device(device)
    elif net is not None:
        dev = next(unwrap(net, "prototype_gallery").parameters()).device
    else:
        dev = torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise RuntimeError(f"count_pipnet_amd.gallery runs on a ROCm device only (got {dev}); there is no CPU fallback")
    return dev


def _load_frames(dataset, indices: Sequence[int], image_size: int, dev) -> Tensor:
    """[n, S, S, 3] uint8 on ``dev``: ``Resize((S, S))`` of ``dataset[i]`` for every i, Pillow's pixels."""
    for i in indices:
        if not 0 <= i < len(dataset):
            raise ValueError(f"dataset index {i} lies outside the dataset of {len(dataset)} images")
    packed = pack_images([dataset[i][0] for i in indices])
    return DeviceEvalTransform(image_size)(packed, dev, want_u8=True)[1]


# ---- public calls -----------------------------------------------------------------------------------------

def prototype_gallery(net_or_none, dataset, res: PrototypeTopK, *, image_size: int, device=None, batch_size: int = 64,
                      keep_frames: bool = False, pad_value: int = GRID_PAD_VALUE) -> PrototypeGallery:
    """The patch grids of ``vizualize_network`` (the patch part of every ``grid_topk_{p}.png``) from a
    ``prototype_topk`` result.

    ``dataset``: the ``DecodedImageFolder`` the pass ran over (``dataset[i] -> (HxWx3 uint8, target)``, i the
    index the pass recorded).  ``net_or_none`` only names the device (``device`` overrides it; neither: the
    current ROCm device); no forward runs and the net is not touched.

    Selection is the reference's: PIP-Net (vis_pipnet.py:278-313) shows, for every prototype with
    ``selected & ~unused``, its stored images in slot order; CountPIPNet (:758-838) samples the count groups
    uniformly, fills up from the rest by score and sorts by score (stable), a repeated image included where the
    reference repeats one.  The distinct images are decoded once each, ``batch_size`` at a time, resized on the
    device and their windows laid into the grids by one launch per chunk; the frames are dropped after their
    chunk unless ``keep_frames``.  Pixels: see the module docstring (palette and alpha files follow the
    loader's ``convert("RGB")``)."""
    if batch_size < 1:
        raise ValueError(f"prototype_gallery: batch_size must be at least 1, got {batch_size}")
    if not 0 <= int(pad_value) <= 255:
        raise ValueError(f"prototype_gallery: pad_value must be in 0..255, got {pad_value}")
    dev = _device(net_or_none, device)
    res = res.cpu()
    pn, _, k = res.scores.shape
    selection = select_entries(res)
    coords = res.coords.tolist()
    height, width, cells = (torch.zeros(pn, dtype=torch.int64) for _ in range(3))
    ok = torch.ones(pn, dtype=torch.bool)
    entry_index, entry_group, entry_slot = (torch.full((pn, k), -1, dtype=torch.int64) for _ in range(3))
    entry_score = torch.zeros((pn, k), dtype=torch.float32)
    entry_coords = torch.full((pn, k, 4), -1, dtype=torch.int64)
    by_image = {}                 # dataset index -> [(h0, h1, w0, w1, canvas, y, x)]
    for p, entries in enumerate(selection):
        if not entries:
            continue
        for c, (g, j) in enumerate(entries):
            entry_index[p, c], entry_group[p, c], entry_slot[p, c] = res.index[p, g, j], g, j
            entry_score[p, c], entry_coords[p, c] = res.scores[p, g, j], res.coords[p, g, j]
        layout = grid_layout([_window(coords[p][g][j], image_size) for g, j in entries])
        if layout is None:
            ok[p] = False
            continue
        height[p], width[p], cells[p] = layout[0], layout[1], len(entries)
        for (g, j), (h0, h1, w0, w1, y, x) in zip(entries, layout[2]):
            by_image.setdefault(int(res.index[p, g, j]), []).append((h0, h1, w0, w1, p, y, x))
    distinct = sorted(by_image)
    grids = torch.full((pn, PATCH_SIZE, k * (PATCH_SIZE + GRID_PADDING) + GRID_PADDING, 3), int(pad_value),
                       dtype=torch.uint8, device=dev)
    kept = []
    for c0 in range(0, len(distinct), batch_size):
        chunk = distinct[c0:c0 + batch_size]
        frames = _load_frames(dataset, chunk, image_size, dev)
        K.patch_compose_rgb8(frames, [(f,) + item for f, i in enumerate(chunk) for item in by_image[i]], grids)
        if keep_frames:
            kept.append(frames)
    frames = None
    if keep_frames:
        frames = torch.cat(kept) if kept else torch.empty((0, image_size, image_size, 3), dtype=torch.uint8, device=dev)
    return PrototypeGallery(grids=grids, height=height, width=width, cells=cells, ok=ok, entry_index=entry_index,
                            entry_group=entry_group, entry_slot=entry_slot, entry_score=entry_score,
                            entry_coords=entry_coords, frame_index=torch.tensor(distinct, dtype=torch.int64),
                            frames=frames)


def explanation_images(dataset_or_frames, res: LocalExplanation, *, image_size: int, indices=None,
                       batch_size: int = 64, rect_width: int = 2) -> ExplanationImages:
    """The ``*_patch.png`` and ``*_rect.png`` pixels of ``vis_pred`` (visualize_prediction.py:80-88) for every
    stored entry of an ``explain_predictions`` result: ``j < min(count, max_entries)`` of every (image b, class
    rank r), in that order.

    ``dataset_or_frames``: either the resized uint8 frames [B, S, S, 3] of the batch on the device (S =
    ``image_size``; ``DeviceEvalTransform(S)(packed, device, want_u8=True)[1]``), or a ``DecodedImageFolder``
    with ``indices`` = the dataset index of each of ``res``'s B rows, which are then decoded and resized
    ``batch_size`` at a time on ``res``'s device.  ``patches[n]`` holds the window ``coords[b, r, j]`` of the
    frame (Python slice semantics), zero-padded to 32 x 32 only where the window was cut, ``patch_hw[n]`` its true
    size; ``rects[n]`` is the frame with ``rect[b, r, j]`` outlined in yellow, ``rect_width`` wide, as
    ``ImageDraw.rectangle`` draws it (one rectangle per image, as the reference reopens the file per entry),
    produced ``batch_size`` entries at a time.  A rectangle narrower than ``2 * rect_width + 1`` raises
    ValueError.  Pixels: see the module docstring.  File names stay with the caller; the third picture of an
    entry, its heatmap, comes from ``explanation_heatmaps``."""
    if batch_size < 1:
        raise ValueError(f"explanation_images: batch_size must be at least 1, got {batch_size}")
    dev_res = res.classes.device
    res = res.cpu()
    b = res.prototype.shape[0]
    if torch.is_tensor(dataset_or_frames):
        frames = dataset_or_frames
        if indices is not None:
            raise ValueError("explanation_images: indices go with a dataset, not with frames")
        if tuple(frames.shape) != (b, image_size, image_size, 3) or frames.dtype != torch.uint8:
            raise ValueError(f"explanation_images: frames must be uint8 {(b, image_size, image_size, 3)}, got "
                             f"{frames.dtype} {tuple(frames.shape)}")
        if not frames.is_cuda:
            raise RuntimeError("explanation_images: frames must be on a ROCm device; there is no CPU fallback")
    else:
        idx = [int(i) for i in (indices if indices is not None else [])]
        if indices is None or len(idx) != b:
            raise ValueError(f"explanation_images: a dataset needs indices, one per image of the result ({b})")
        dev = _device(None, dev_res if dev_res.type == "cuda" else None)
        chunks = [_load_frames(dataset_or_frames, idx[i:i + batch_size], image_size, dev)
                  for i in range(0, b, batch_size)]
        frames = torch.cat(chunks) if chunks else torch.empty((0, image_size, image_size, 3), dtype=torch.uint8,
                                                              device=dev)
    dev = frames.device
    entry = _stored_entries(res)
    n = len(entry)
    coords, rect = res.coords.tolist(), res.rect.tolist()
    windows = [_window(coords[bi][r][j], image_size) for bi, r, j in entry]
    boxes = np.asarray([rect[bi][r][j] for bi, r, j in entry], dtype=np.int64).reshape(-1, 4)
    K.rect_outline_check(boxes, rect_width)
    patches = torch.zeros((n, PATCH_SIZE, PATCH_SIZE, 3), dtype=torch.uint8, device=dev)
    K.patch_compose_rgb8(frames, [(e[0],) + w + (i, 0, 0) for i, (e, w) in enumerate(zip(entry, windows))], patches)
    src = [e[0] for e in entry]
    parts = [K.draw_rects_rgb8(frames, src[i:i + batch_size], boxes[i:i + batch_size], rect_width)
             for i in range(0, n, batch_size)]
    rects = torch.cat(parts) if parts else torch.empty((0, image_size, image_size, 3), dtype=torch.uint8, device=dev)
    return ExplanationImages(entry=torch.tensor(entry, dtype=torch.int64).reshape(-1, 3), patches=patches,
                             patch_hw=torch.tensor([(w[1] - w[0], w[3] - w[2]) for w in windows],
                                                   dtype=torch.int64).reshape(-1, 2), rects=rects)


def _stored_entries(res: LocalExplanation) -> List[Tuple[int, int, int]]:
    """The stored entries (b, r, j) of ``res`` (on the host), j < min(count, max_entries), in (b, r, j) order."""
    b, c, m = res.prototype.shape
    stored = torch.clamp(res.count, max=m).tolist()
    return [(bi, r, j) for bi in range(b) for r in range(c) for j in range(stored[bi][r])]


def similarity_heatmaps(proto_features: Tensor, frames: Tensor, pairs, lut: Tensor, *, batch_size: int = 64,
                        weights=K.HEATMAP_WEIGHTS) -> Tensor:
    """[N, S, S, 3] uint8 on the device: per pair the RGB pixels of the reference's ``heatmap_p{p}.png``
    (visualize_prediction.py:92-100), see the module docstring.

    ``proto_features``: the [B, P, h, w] float32 similarity maps a forward returned (``net(xs, inference=True)[0]``);
    our forward's output is NHWC-backed and is read in place, any other layout is copied once.  ``frames``
    [F, S, S, 3] uint8: the resized images (``DeviceEvalTransform(S)(packed, device, want_u8=True)[1]``), h, w <= S.
    ``pairs``: a list (or integer array) of (b, p), the frame being ``frames[b]``, or of (b, p, frame).  ``lut``
    [256, 3] uint8 RGB on the device: the colour table; the reference's is
    ``cv2.applyColorMap(np.arange(256, dtype=np.uint8), cv2.COLORMAP_JET)[:, 0, ::-1]``.  ``weights``: the factors
    of the colour and of the image (>= 0, sum <= 1).  ``batch_size`` pairs are rendered per launch.  A wrong shape,
    dtype, pair or ``batch_size`` raises ValueError, an operand off the ROCm device RuntimeError, before anything is
    launched.  Nothing in the call waits for the device."""
    if batch_size < 1:
        raise ValueError(f"similarity_heatmaps: batch_size must be at least 1, got {batch_size}")
    if not torch.is_tensor(proto_features) or proto_features.dim() != 4:
        raise ValueError("similarity_heatmaps: proto_features must be the [B, P, h, w] tensor of a forward")
    K.heatmap_shapes(proto_features.permute(0, 2, 3, 1), frames, lut)
    K.heatmap_weights(weights)
    b, p = proto_features.shape[:2]
    f, s = frames.shape[:2]
    items = np.asarray(pairs if len(pairs) else np.zeros((0, 2)), dtype=np.float64)
    if items.ndim != 2 or items.shape[1] not in (2, 3) or (items != np.floor(items)).any():
        raise ValueError("similarity_heatmaps: pairs must be rows of integers (b, p) or (b, p, frame)")
    items = items.astype(np.int64)
    if items.shape[1] == 2:
        items = np.concatenate([items, items[:, :1]], axis=1)
    bad = (items < 0).any(axis=1) | (items[:, 0] >= b) | (items[:, 1] >= p) | (items[:, 2] >= f)
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError(f"similarity_heatmaps: pair {i} {tuple(int(v) for v in items[i])} lies outside the {b} "
                         f"images, {p} prototypes or {f} frames")
    if not (proto_features.is_cuda and frames.is_cuda and lut.is_cuda):
        raise RuntimeError("similarity_heatmaps: proto_features, frames and lut must be on a ROCm device; there is "
                           "no CPU fallback")
    proto = as_nhwc(proto_features)
    n = items.shape[0]
    out = torch.empty((n, s, s, 3), dtype=torch.uint8, device=frames.device)
    table = torch.from_numpy(items.astype(np.int32)).to(frames.device, non_blocking=True)      # checked above, sent once
    for i in range(0, n, batch_size):
        K.heatmap_rgb8(proto, frames, table[i:i + batch_size], lut, weights=weights, out=out[i:i + batch_size])
    return out


def explanation_heatmaps(proto_features: Tensor, frames: Tensor, res: LocalExplanation, lut: Tensor, *,
                         batch_size: int = 64) -> ExplanationHeatmaps:
    """The ``heatmap_p{p}.png`` pixels of ``vis_pred`` (visualize_prediction.py:92-100) for every stored entry of an
    ``explain_predictions`` result, in the (b, r, j) order of ``explanation_images``: ``heatmaps[n]`` belongs to
    that call's ``patches[n]`` and ``rects[n]``.

    ``proto_features`` [B, P, h, w] and ``frames`` [B, S, S, 3] are those of the batch ``res`` explains: the maps of
    ``net(xs, inference=True)`` and the uint8 frames of the transform that made ``xs``.  A prototype kept under
    several classes of an image is rendered once per occurrence, as the reference does.  ``lut``, the arithmetic
    and the errors: ``similarity_heatmaps`` (the reference's weights 0.2 / 0.6).  But for the copy of ``res`` to the
    host, nothing in the call waits for the device."""
    if batch_size < 1:
        raise ValueError(f"explanation_heatmaps: batch_size must be at least 1, got {batch_size}")
    res = res.cpu()
    b = res.prototype.shape[0]
    if not torch.is_tensor(proto_features) or proto_features.dim() != 4 or proto_features.shape[0] != b or \
            not torch.is_tensor(frames) or frames.dim() != 4 or frames.shape[0] != b:
        raise ValueError(f"explanation_heatmaps: proto_features [B, P, h, w] and frames [B, S, S, 3] must hold the "
                         f"{b} images of the result")
    entry = _stored_entries(res)
    proto = res.prototype.tolist()
    ids = [proto[bi][r][j] for bi, r, j in entry]
    heatmaps = similarity_heatmaps(proto_features, frames, [(e[0], p) for e, p in zip(entry, ids)], lut,
                                   batch_size=batch_size)
    return ExplanationHeatmaps(entry=torch.tensor(entry, dtype=torch.int64).reshape(-1, 3),
                               prototype=torch.tensor(ids, dtype=torch.int64), heatmaps=heatmaps)


def _pairs(fn: str, pairs, cols, limits, names: str) -> np.ndarray:
    """``pairs`` as an int64 [N, cols] table with every column inside its limit, or ValueError."""
    items = np.asarray(pairs if len(pairs) else np.zeros((0, cols)), dtype=np.float64)
    if items.ndim != 2 or items.shape[1] != cols or (items != np.floor(items)).any():
        raise ValueError(f"{fn}: pairs must be rows of {cols} integers")
    items = items.astype(np.int64)
    bad = (items < 0).any(axis=1) | (items >= np.asarray(limits, dtype=np.int64)[None, :]).any(axis=1)
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError(f"{fn}: pair {i} {tuple(int(v) for v in items[i])} lies outside the {names}")
    return items


def feature_map_overlays(proto_features: Tensor, pairs, lut: Tensor, *, size: int, alpha: float = K.OVERLAY_ALPHA,
                         batch_size: int = 64, want_overlay: bool = True) -> K.MapOverlay:
    """Per pair (b, p) the arrays behind the reference's ``*_overlay.png`` (vis_pipnet.py:454-475), see the module
    docstring: ``MapOverlay(maps [N, h, w] float32, resized [N, S, S] float32, mask [N, S, S] uint8, colour [N, S, S]
    uint8, overlay [N, S, S, 4] float64 or None)`` on the device, S = ``size``.

    ``proto_features``: the [B, P, h, w] float32 similarity maps a forward returned (``net(xs, inference=True)[0]``),
    h, w >= 3; our forward's output is NHWC-backed and is read in place, any other layout is copied once.  ``pairs``:
    a list (or integer array) of (b, p); a pair may repeat.  ``lut`` [256, 3] float64 on the device: the colour table,
    the reference's is ``matplotlib.colormaps['viridis'](np.arange(256))[:, :3]``.  ``alpha``: the fourth band on the
    mask.  ``batch_size`` pairs are rendered per launch; without ``want_overlay`` the 32 bytes per pixel of the
    overlay are neither computed nor allocated.  A wrong shape, dtype, pair, ``size`` or ``batch_size`` raises
    ValueError, an operand off the ROCm device RuntimeError, before anything is launched.  Nothing in the call waits
    for the device."""
    fn = "feature_map_overlays"
    if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
        raise ValueError(f"{fn}: batch_size must be an integer >= 1, got {batch_size!r}")
    if not torch.is_tensor(proto_features) or proto_features.dim() != 4:
        raise ValueError(f"{fn}: proto_features must be the [B, P, h, w] tensor of a forward")
    b, h, w, p, s = K.overlay_shapes(proto_features.permute(0, 2, 3, 1), lut, size, alpha)
    items = _pairs(fn, pairs, 2, (b, p), f"{b} images or {p} prototypes")
    if not (proto_features.is_cuda and lut.is_cuda):
        raise RuntimeError(f"{fn}: proto_features and lut must be on a ROCm device; there is no CPU fallback")
    dev = proto_features.device
    proto = as_nhwc(proto_features)
    n = items.shape[0]
    out = K.MapOverlay(maps=torch.empty((n, h, w), dtype=torch.float32, device=dev),
                       resized=torch.empty((n, s, s), dtype=torch.float32, device=dev),
                       mask=torch.empty((n, s, s), dtype=torch.uint8, device=dev),
                       colour=torch.empty((n, s, s), dtype=torch.uint8, device=dev),
                       overlay=torch.empty((n, s, s, 4), dtype=torch.float64, device=dev) if want_overlay else None)
    table = torch.from_numpy(items.astype(np.int32)).to(dev, non_blocking=True)                # checked above, sent once
    for i in range(0, n, batch_size):
        K.map_overlay(proto, table[i:i + batch_size], lut, s, alpha=alpha,
                      out=K.MapOverlay(*(None if t is None else t[i:i + batch_size] for t in out)))
    return out


def _load_inputs(dataset, indices: Sequence[int], image_size: int, dev) -> Tuple[Tensor, Tensor]:
    """(normalised float32 inputs [n, 3, S, S], resized uint8 frames [n, S, S, 3]) of ``dataset[i]`` on ``dev``."""
    for i in indices:
        if not 0 <= i < len(dataset):
            raise ValueError(f"dataset index {i} lies outside the dataset of {len(dataset)} images")
    packed = pack_images([dataset[i][0] for i in indices])
    return DeviceEvalTransform(image_size)(packed, dev, want_u8=True)


def prototype_map_overlays(net, dataset, res: PrototypeTopK, lut: Tensor, *, image_size: int, batch_size: int = 64,
                           max_per_prototype: int = 3, want_overlay: bool = True,
                           keep_frames: bool = False) -> PrototypeMapOverlays:
    """The feature maps and overlays ``vizualize_network`` draws with ``visualize_prototype_maps`` (vis_pipnet.py
    :354-486 PIP-Net, :889-1032 CountPIPNet) from a ``prototype_topk`` result: per shown entry the map, its sum, the
    spline-resized map, the mask, the colour index and the RGBA overlay, see the module docstring.

    ``net``: the PIPNet / CountPIPNet the pass ran (bare, under ``.module`` or in a world-size-1 ShardedInference);
    it is put in eval mode, as the reference has it.  ``dataset``: the ``DecodedImageFolder`` the pass ran over.
    ``lut`` [256, 3] float64 on the net's device: the colour table (``feature_map_overlays``).

    The entries are ``select_map_entries(res, max_per_prototype)``.  The pass keeps no maps, so their distinct images
    are decoded once each, ``batch_size`` at a time, and run through the located forward with the map written
    (``explain_forward.located_forward_maps``: the bits of the pass, so ``maps[n].max()`` is the pooled value the
    pass scored and its first maximum lies at ``(h_idx, w_idx)``); then one ``pipnet_map_overlay`` launch renders
    ``batch_size`` entries.  A Gumbel CountPIPNet draws fresh noise in that forward: its maps are a new draw, not
    the pass's -- a caller who kept the maps of its own forward renders them with ``feature_map_overlays``.
    ``map_sum`` is computed on the host from a copy of the maps, which waits for the device once, after the last
    launch.  The frames are dropped after their chunk unless ``keep_frames``.  Errors: ``feature_map_overlays``."""
    fn = "prototype_map_overlays"
    if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
        raise ValueError(f"{fn}: batch_size must be an integer >= 1, got {batch_size!r}")
    res = res.cpu()
    selection = select_map_entries(res, max_per_prototype)
    pn = res.scores.shape[0]
    _, _, h, w = res.proto_shape
    fake = torch.empty((0, h, w, pn), dtype=torch.float32, device="meta")
    s = K.overlay_shapes(fake, lut, image_size)[4]
    net = unwrap(net, fn)
    if getattr(net, "_num_prototypes", pn) != pn:
        raise ValueError(f"{fn}: the result holds {pn} prototypes, the net {net._num_prototypes}")
    dev = _device(net, None)
    if not lut.is_cuda:
        raise RuntimeError(f"{fn}: lut must be on a ROCm device; there is no CPU fallback")
    entry = [(p, g, j) for p, entries in enumerate(selection) for g, j in entries]
    n = len(entry)
    rank = [i + 1 for entries in selection for i in range(len(entries))]
    of = [len(entries) for entries in selection for _ in entries]
    pick = tuple(torch.tensor(col, dtype=torch.int64) for col in zip(*entry)) if n else None

    def column(t: Tensor) -> Tensor:
        return t[pick].clone() if n else t.new_empty((0,) + tuple(t.shape[3:]))

    index = column(res.index)
    by_image = {}                 # dataset index -> [(row n, prototype)]
    for row, (i, (p, _, _)) in enumerate(zip(index.tolist(), entry)):
        by_image.setdefault(i, []).append((row, p))
    distinct = sorted(by_image)
    maps = torch.empty((n, h, w), dtype=torch.float32, device=dev)
    kept = []
    net.eval()
    with torch.no_grad():
        for c0 in range(0, len(distinct), batch_size):
            chunk = distinct[c0:c0 + batch_size]
            xs, frames = _load_inputs(dataset, chunk, s, dev)
            fwd, proto = located_forward_maps(net, xs, map_is_small(net, xs))
            note_map(net, xs, fwd.hw)
            if tuple(fwd.hw) != (h, w):
                raise ValueError(f"{fn}: the net gives a {fwd.hw[0]} x {fwd.hw[1]} map at image_size {s}, the result "
                                 f"was made with {h} x {w}")
            rows = [row for i in chunk for row, _ in by_image[i]]
            got = K.map_overlay(as_nhwc(proto), [(f, p) for f, i in enumerate(chunk) for _, p in by_image[i]], lut, s,
                                out=K.MapOverlay(torch.empty((len(rows), h, w), dtype=torch.float32, device=dev),
                                                 None, None, None, None)).maps          # a gather: nothing is resized
            maps.index_copy_(0, torch.tensor(rows, dtype=torch.int64).to(dev, non_blocking=True), got)
            if keep_frames:
                kept.append(frames)
    pictures = feature_map_overlays(maps.view(n, 1, h, w), [(i, 0) for i in range(n)], lut, size=s,
                                    batch_size=batch_size, want_overlay=want_overlay)
    frames = None
    if keep_frames:
        frames = torch.cat(kept) if kept else torch.empty((0, s, s, 3), dtype=torch.uint8, device=dev)
    host = maps.cpu().numpy().astype(np.float64).reshape(n, h * w)
    map_sum = torch.from_numpy(np.cumsum(host, axis=1)[:, -1].copy())        # a sequential sum in the stored order
    return PrototypeMapOverlays(
        entry=torch.tensor(entry, dtype=torch.int64).reshape(-1, 3), rank=torch.tensor(rank, dtype=torch.int64),
        of=torch.tensor(of, dtype=torch.int64), index=index, score=column(res.scores), coords=column(res.coords),
        h_idx=column(res.h_idx), w_idx=column(res.w_idx), maps=maps, map_sum=map_sum, resized=pictures.resized,
        mask=pictures.mask, colour=pictures.colour, overlay=pictures.overlay,
        frame_index=torch.tensor(distinct, dtype=torch.int64), frames=frames)
