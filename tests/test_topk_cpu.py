"""Prototype top-k pass, the parts that need no GPU: the latent-location -> image-patch arithmetic
of util/vis_pipnet.py:1162-1193 / util/func.py:3-15 as restated in count_pipnet_amd.topk, and the
argument checks of the three C entry points (status before any HIP call)."""
import argparse
import ctypes

import pytest
import torch

from count_pipnet_amd import _lib, build
from count_pipnet_amd.topk import img_coordinates, patch_size

# (image size, shape handed over = (1, P, H, W), skip, (h, w), expected (h_min, h_max, w_min, w_max));
# patchsize 32.  Derived by hand from the reference text, which indexes the 4-D shape as if it were
# 3-D: shape[1] / shape[2] are P and H.
COORD_CASES = [
    (224, (1, 768, 26, 26), 8, (0, 0), (0, 32, 0, 32)),
    (224, (1, 768, 26, 26), 8, (1, 25), (8, 40, 192, 224)),
    (224, (1, 768, 26, 26), 8, (25, 3), (192, 224, 24, 56)),
    (224, (1, 26, 26, 26), 8, (1, 25), (4, 36, 192, 224)),        # P == 26: the small-stride branch
    (224, (1, 768, 13, 13), 16, (5, 12), (80, 112, 192, 224)),
    (64, (1, 32, 8, 8), 5, (7, 2), (32, 64, 10, 42)),
]


@pytest.mark.parametrize("size,shape,skip,hw,want", COORD_CASES)
def test_img_coordinates_known_answers(size, shape, skip, hw, want):
    assert img_coordinates(size, shape, 32, skip, *hw) == want
    # tensor form, as the pass calls it
    got = img_coordinates(size, shape, 32, skip, torch.tensor([hw[0]]), torch.tensor([hw[1]]))
    assert tuple(int(t[0]) for t in got) == want


def test_img_coordinates_row_clamp_looks_at_prototype_count():
    """h_idx == shape[1] - 1 compares with P - 1 of the 4-D shape: with 4 prototypes, row 3 of an
    8-row map is treated as the last row."""
    h0, h1, _, _ = img_coordinates(64, (1, 4, 8, 8), 32, 5, 3, 2)
    assert (h0, h1) == (32, 64)
    h0, h1, _, _ = img_coordinates(64, (1, 32, 8, 8), 32, 5, 3, 2)
    assert (h0, h1) == (15, 47)


def test_img_coordinates_tensor_form_matches_scalar_form():
    for size, shape, skip in [(224, (1, 768, 26, 26), 8), (224, (1, 26, 26, 26), 8), (64, (1, 4, 8, 8), 5)]:
        n = shape[-1]
        hh, ww = torch.meshgrid(torch.arange(n), torch.arange(n), indexing="ij")
        got = torch.stack(img_coordinates(size, shape, 32, skip, hh, ww), dim=-1)
        for h in range(n):
            for w in range(n):
                assert tuple(got[h, w].tolist()) == img_coordinates(size, shape, 32, skip, h, w)


@pytest.mark.parametrize("wshape,size,skip", [(26, 224, 8), (13, 224, 16), (8, 64, 5)])
def test_patch_size(wshape, size, skip):
    assert patch_size(argparse.Namespace(image_size=size, wshape=wshape, use_mid_layers=False)) == (32, skip)


def _lib_loaded():
    build.build()
    return _lib.load()


PTR = ctypes.c_void_p(64)     # never dereferenced: every call below returns before a HIP call


def _topk(lib, b=1, p=4, g=1, k=3, score=PTR, st_score=PTR, st_index=PTR, st_loc=PTR, st_fill=PTR, out=None,
          kc=0, abst=PTR):
    return lib.pipnet_topk_update(score, PTR, b, p, 0, None, g, 0, 0.0, out, kc, k, st_score, st_index, st_loc,
                                  st_fill, abst, None)


def test_topk_update_rejects_bad_arguments_without_gpu():
    lib = _lib_loaded()
    assert _topk(lib, k=0) == 1 and _topk(lib, k=33) == 1 and _topk(lib, k=-1) == 1
    assert _topk(lib, p=0) == 1 and _topk(lib, p=-3) == 1 and _topk(lib, g=0) == 1 and _topk(lib, b=-1) == 1
    for null in ("score", "st_score", "st_index", "st_loc", "st_fill"):
        assert _topk(lib, **{null: None}) == 1, null
    assert _topk(lib, out=PTR, kc=0) == 1 and _topk(lib, out=PTR, kc=5, abst=None) == 1
    assert _topk(lib, b=0) == 0 and _topk(lib, b=0, k=32) == 0 and _topk(lib, b=0, k=1, out=PTR, kc=5) == 0


def test_argmax_entry_points_reject_bad_arguments_without_gpu():
    lib = _lib_loaded()
    spa, ma = lib.pipnet_softmax_pool_argmax_f32, lib.pipnet_map_argmax_f32
    assert spa(PTR, 1, 8, 8, 0, None, PTR, PTR, PTR, None) == 1            # P <= 0
    assert spa(PTR, 1, 8, 8, -5, None, PTR, PTR, PTR, None) == 1
    assert spa(PTR, 1, 8, 8, 4096, None, PTR, PTR, PTR, None) == 1         # more channels than a wave row holds
    assert spa(PTR, 1, 0, 8, 32, None, PTR, PTR, PTR, None) == 1 and spa(PTR, 1, 8, 0, 32, None, PTR, PTR, PTR, None) == 1
    assert spa(PTR, -1, 8, 8, 32, None, PTR, PTR, PTR, None) == 1
    assert spa(None, 1, 8, 8, 32, None, PTR, PTR, PTR, None) == 1
    assert spa(PTR, 1, 8, 8, 32, None, None, PTR, PTR, None) == 1          # null pooled
    assert spa(PTR, 1, 8, 8, 32, None, PTR, None, PTR, None) == 1          # null loc
    assert spa(PTR, 1, 8, 8, 32, None, PTR, PTR, None, None) == 1          # null workspace
    assert spa(PTR, 1, 8, 8, 32, None, PTR, PTR, ctypes.c_void_p(68), None) == 2   # workspace not 8-B aligned
    assert spa(PTR, 0, 8, 8, 32, None, PTR, PTR, PTR, None) == 0           # empty batch, proto optional
    assert ma(PTR, 1, 8, 8, 0, PTR, PTR, None) == 1 and ma(PTR, 1, 8, 0, 16, PTR, PTR, None) == 1
    assert ma(None, 1, 8, 8, 16, PTR, PTR, None) == 1 and ma(PTR, 1, 8, 8, 16, None, PTR, None) == 1
    assert ma(PTR, 1, 8, 8, 16, PTR, None, None) == 1 and ma(PTR, -2, 8, 8, 16, PTR, PTR, None) == 1
    assert ma(PTR, 0, 8, 8, 16, PTR, PTR, None) == 0


def test_per_image_gemm_plan_is_scoped_and_off_by_default():
    """The split-K planning rows are the call's own rows unless a caller asks for the per-image plan."""
    from count_pipnet_amd import kernels as K
    assert K._plan_rows(768) == 768
    with K.per_image_gemm_plan(12):
        assert K._plan_rows(768) == 64 and K._plan_rows(770) == 770
        with K.per_image_gemm_plan(1):
            assert K._plan_rows(768) == 768
        assert K._plan_rows(768) == 64
    assert K._plan_rows(768) == 768
    assert K.splitk_factor(768, 384, 1536) == 1 and K.splitk_factor(64, 384, 1536) > 1
