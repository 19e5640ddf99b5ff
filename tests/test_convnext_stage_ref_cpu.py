"""CPU checks of the ConvNeXt stage matrix (tests/convnext_stage_ref.py): the float64 references against
torch's float64 library ops, the condition that fixes F_BOUND (torch float32 stays within F_BOUND * bound on
every case of every grid), the shape of the grids, and the mutants the grids and the bound were sized against.

The mutants are float32 torch evaluations on the CPU with one thing wrong; no kernel is changed.  Each must
exceed F_BOUND * bound by at least 4x on at least one element of the case it names -- the same assertion, on
the same case, that tests/test_gpu_convnext_stages.py makes of the HIP kernels.
"""
import pytest
import torch
import torch.nn.functional as F

import convnext_stage_ref as R

MUTANT_MARGIN = 4.0


def _dw_case(c, h, w, kind=R.NORMAL):
    found = [case for case in R.DW_CASES if (case[0], case[2], case[3], case[4]) == (c, h, w, kind)]
    assert len(found) == 1, (c, h, w, kind, found)
    return found[0]


# ---------------------------------------------------------------------------------------------------
# the references (1e-12, times 1e3 on the offset cases: there y ~ 1000 carries a float64 rounding of
# 1000 * 2^-53 ~ 1e-13 in either evaluation, which r g ~ 1 passes on to the output)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,h,w,kind", [(96, 9, 16, R.NORMAL), (96, 2, 57, R.NORMAL), (192, 7, 29, R.OFFSET),
                                        (384, 8, 15, "impulse_edge"), (768, 7, 14, R.FLAT), (768, 7, 1, R.NORMAL)])
def test_dwconv7_ln_ref_is_torch_float64(c, h, w, kind):
    case = _dw_case(c, h, w, kind)
    d = {k: v.double() for k, v in R.dw_data(case).items()}
    y = F.conv2d(d["x"].permute(0, 3, 1, 2), R.w49c_to_torch(d["w"]), d["bias"], padding=3, groups=c)
    y = y.permute(0, 2, 3, 1)
    want = F.layer_norm(y, (c,), d["ln_w"], d["ln_b"], R.EPS)
    f = R.dw_data(case)
    ref = R.dwconv7_ln_ref(f["x"], f["w"], f["bias"], f["ln_w"], f["ln_b"])
    scale = max(1.0, float(y.abs().max()))
    assert float((ref.y - y).abs().max()) <= 1e-12 * scale
    assert float((ref.out - want).abs().max()) <= 1e-12 * (1e3 if kind == R.OFFSET else max(1.0, float(want.abs().max())))
    assert torch.equal(ref.out, R.dw_expect(case)[0])
    # the intermediates are what the names say
    assert float((ref.d - (y - y.mean(-1, keepdim=True))).abs().max()) <= 1e-12 * scale
    rstd = torch.rsqrt(y.var(-1, unbiased=False, keepdim=True) + R.EPS)
    assert float((ref.r - rstd).abs().max() / ref.r.max()) <= 1e-9
    assert bool((ref.A >= ref.y.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("case", [(1, 5, R.NORMAL), (65, 4, R.NORMAL), (193, 3, R.OFFSET), (2048, 5, R.FLAT),
                                  (1000, 517, R.NORMAL)])
def test_layernorm_ref_is_torch_float64(case):
    assert case in R.LN_CASES
    d = R.ln_data(case)
    want = F.layer_norm(d["x"].double(), (case[0],), d["ln_w"].double(), d["ln_b"].double(), R.EPS)
    ref = R.layernorm_ref(d["x"], d["ln_w"], d["ln_b"])
    assert float((ref.out - want).abs().max()) <= 1e-12 * (1e3 if case[2] == R.OFFSET else 1)
    assert torch.equal(ref.y, d["x"].double()) and torch.equal(ref.A, d["x"].double().abs())


@pytest.mark.parametrize("case", [(3, 36, 20, R.NORMAL), (1, 4, 4, R.NORMAL), (1, 4, 8, R.NORMAL), (3, 36, 20, R.OFFSET)])
def test_stem_ref_is_torch_float64(case):
    assert case in R.STEM_CASES
    d = {k: v.double() for k, v in R.stem_data(case).items()}
    y = F.conv2d(d["x"], d["w"], d["bias"], stride=4).permute(0, 2, 3, 1)
    want = F.layer_norm(y, (96,), d["ln_w"], d["ln_b"], R.EPS)
    f = R.stem_data(case)
    ref = R.stem_ref(f["x"], f["w"], f["bias"], f["ln_w"], f["ln_b"])
    assert ref.out.shape == (case[0], case[1] // 4, case[2] // 4, 96)
    assert float((ref.y - y).abs().max()) <= 1e-12 * max(1.0, float(y.abs().max()))
    assert float((ref.out - want).abs().max()) <= 1e-12 * (1e3 if case[3] == R.OFFSET else 1)


def test_data_is_fp32_and_deterministic():
    for data, case in ((R.dw_data, R.DW_CASES[0]), (R.ln_data, R.LN_CASES[0]), (R.stem_data, R.STEM_CASES[4])):
        first = {k: v.clone() for k, v in data(case).items()}
        data.cache_clear()
        for k, v in data(case).items():
            assert v.dtype == torch.float32 and torch.equal(v, first[k])


def test_flat_and_impulse_data():
    case = _dw_case(96, 9, 31, R.FLAT)
    d = R.dw_data(case)
    assert not d["x"].any() and d["bias"].unique().numel() == 1
    out, _ = R.dw_expect(case)
    assert float((out - d["ln_b"].double()).abs().max()) <= 1e-9       # variance 0: the output is ln_b
    d = R.ln_data((65, 5, R.FLAT))
    assert bool((d["x"] == d["x"][:, :1]).all()) and d["x"][:, 0].unique().numel() == 5
    for kind in R.IMPULSES:
        case = _dw_case(192, 7, 15, kind)
        x = R.dw_data(case)["x"]
        for i, (py, px) in enumerate(R.impulse_positions(case)):
            nz = x[i].abs().sum(-1).nonzero().tolist()
            assert nz == [[py, px]], (kind, nz)
    assert R.impulse_positions(_dw_case(192, 7, 15, "impulse_edge"))[0] == (5, 13)


# ---------------------------------------------------------------------------------------------------
# the grids
# ---------------------------------------------------------------------------------------------------
def _rule(c, w):
    """The dispatch rule as the issue of this matrix states it (TX, TY)."""
    if c == 96:
        return (7, 1) if w <= 16 else (4, 4) if w <= 32 else (7, 2)
    if c == 192:
        return (7, 1) if w <= 8 else (4, 2) if w <= 16 else (7, 2)
    return {384: (7, 3), 768: (13, 1)}[c]


def test_dw_grid_covers_every_variant_and_edge():
    assert 100 <= len(R.DW_CASES) <= 200 and len(set(R.DW_CASES)) == len(R.DW_CASES)
    for c, tile, npix, ws, h_all, w_pair, hs, special in R.DW_VARIANTS:
        assert npix == (192 // (c // 4)) * tile[0]
        assert all(_rule(c, w) == tile == R.dw_variant(c, w) for w in ws)
        mine = [case for case in R.DW_NORMAL_CASES if case[0] == c and case[3] in ws]
        assert h_all >= 7 and {case[3] for case in mine if case[2] == h_all} == set(ws)
        for w in w_pair:
            assert {case[2] for case in mine if case[3] == w} >= set(hs)
        exact, ragged = w_pair
        assert exact % npix == 0 or (max(ws) < npix and exact % tile[0] == 0)
        assert ragged % npix and ragged % tile[0]
        assert {case[1] for case in mine} == {1, 3}
        kinds = [case[4] for case in R.DW_SPECIAL_CASES if (case[0], case[2], case[3]) == (c,) + special]
        assert kinds == [R.OFFSET, R.FLAT, R.RIPPLE] + list(R.IMPULSES)
        assert special[0] >= 7 and special[1] >= 7 and special[0] != special[1] and special[1] % tile[0]
    # both sides of every W threshold, and three column tiles at the largest W of every C
    ws = {c: {case[3] for case in R.DW_CASES if case[0] == c} for c in (96, 192, 384, 768)}
    assert {16, 17, 32, 33} <= ws[96] and {8, 9, 16, 17} <= ws[192]
    for c, npix in ((96, 56), (192, 28), (384, 14), (768, 13)):
        assert -(-max(ws[c]) // npix) == 3 and max(ws[c]) % npix == 1


def test_ln_and_stem_grids():
    assert len(R.LN_CASES) == 14 * 5 * 3
    for edge in (64, 128, 192, 384, 768):                # nj thresholds 2 / 3 / 6 / 12 of the launcher
        assert edge in R.LN_CHANNELS and edge + 1 in R.LN_CHANNELS
    assert 2048 in R.LN_CHANNELS and 1 in R.LN_CHANNELS
    bsz, h, w, _ = R.STEM_BIG
    pixels = bsz * (h // 4) * (w // 4)
    tiles = -(-pixels // 32)
    assert (pixels, tiles, tiles - 2048, pixels % 32) == (88592, 2769, 721, 16)
    assert (1, 4, 4, R.NORMAL) in R.STEM_CASES and (3, 36, 20, R.OFFSET) in R.STEM_CASES


# ---------------------------------------------------------------------------------------------------
# what fixes F_BOUND: torch float32 on every case
# ---------------------------------------------------------------------------------------------------
def test_f_bound_is_a_fraction():
    assert 0 < R.F_BOUND < 1


@pytest.mark.parametrize("family", list(R.FAMILIES))
def test_torch_float32_within_f_bound(family):
    cases, f32, expect, fmt = R.FAMILIES[family]
    worst = max((R.worst_ratio(f32(case), expect(case)), fmt % case) for case in cases)
    print(f"{family}: torch float32 max err / bound = {worst[0]:.5f} at {worst[1]} (F_BOUND {R.F_BOUND})")
    assert worst[0] <= R.F_BOUND, worst
    # F_BOUND is 8 x the largest of these ratios: none may come near it
    assert worst[0] <= R.F_BOUND / 4, worst


# ---------------------------------------------------------------------------------------------------
# mutants (float32 torch, CPU)
# ---------------------------------------------------------------------------------------------------
def _ln_f32(y, g, b, one_pass=False, eps_outside=False, mean_div=None):
    c = y.shape[-1]
    mean = y.sum(-1, keepdim=True) / (mean_div or c)
    if one_pass:
        var = (y * y).sum(-1, keepdim=True) / c - mean * mean
    else:
        var = ((y - mean) ** 2).sum(-1, keepdim=True) / c
    r = 1.0 / (torch.sqrt(var) + R.EPS) if eps_outside else 1.0 / torch.sqrt(var + R.EPS)
    return (y - mean) * r * g + b


def _dw_y_f32(case, w49c=None):
    d = R.dw_data(case)
    w49c = d["w"] if w49c is None else w49c
    return F.conv2d(d["x"].permute(0, 3, 1, 2), R.w49c_to_torch(w49c), d["bias"], padding=3,
                    groups=case[0]).permute(0, 2, 3, 1)


def _dw_mutant(case, w49c=None, **wrong):
    d = R.dw_data(case)
    out = _ln_f32(_dw_y_f32(case, w49c), d["ln_w"], d["ln_b"], **wrong)
    return R.worst_ratio(out, R.dw_expect(case)) / R.F_BOUND


def _ln_mutant(case, **wrong):
    d = R.ln_data(case)
    return R.worst_ratio(_ln_f32(d["x"], d["ln_w"], d["ln_b"], **wrong), R.ln_expect(case)) / R.F_BOUND


def test_unmutated_float32_passes():
    """The mutant harness itself, with nothing wrong, is inside the tolerance on the cases the mutants use."""
    for c, h, w, kind in ((96, 9, 16, R.OFFSET), (768, 7, 14, R.OFFSET), (96, 9, 31, R.FLAT), (96, 9, 31, R.RIPPLE), (384, 8, 15, R.NORMAL),
                          (192, 7, 15, "impulse_interior")):
        assert _dw_mutant(_dw_case(c, h, w, kind)) <= 1
    for case in ((192, 517, R.OFFSET), (65, 5, R.FLAT), (65, 4, R.NORMAL)):
        assert _ln_mutant(case) <= 1


@pytest.mark.parametrize("c,h,w", [(96, 9, 16), (96, 9, 57), (192, 7, 29), (384, 8, 15), (768, 7, 14)])
def test_mutant_one_pass_variance_dw(c, h, w):
    assert _dw_mutant(_dw_case(c, h, w, R.OFFSET), one_pass=True) >= MUTANT_MARGIN


@pytest.mark.parametrize("case", [(65, 517, R.OFFSET), (192, 517, R.OFFSET), (2048, 5, R.OFFSET)])
def test_mutant_one_pass_variance_ln(case):
    assert _ln_mutant(case, one_pass=True) >= MUTANT_MARGIN


def test_mutant_one_pass_variance_stem():
    case = (3, 36, 20, R.OFFSET)
    d = R.stem_data(case)
    y = F.conv2d(d["x"], d["w"], d["bias"], stride=4).permute(0, 2, 3, 1)
    out = _ln_f32(y, d["ln_w"], d["ln_b"], one_pass=True)
    assert R.worst_ratio(out, R.stem_expect(case)) / R.F_BOUND >= MUTANT_MARGIN


# On a flat case eps outside the square root shows only where the float32 mean of the constant is inexact
# (d != 0 times r = 1e6): in this evaluation at six of the eight variants -- at (96, 9, 57) and (192, 7, 29) the
# mean is exact and the mutant invisible.  The ripple cases do not depend on that luck: all of them catch it.
@pytest.mark.parametrize("c,h,w", [(96, 9, 16), (96, 9, 31), (192, 7, 8), (192, 7, 15), (384, 8, 15), (768, 7, 14)])
def test_mutant_eps_outside_sqrt_dw_flat(c, h, w):
    assert _dw_mutant(_dw_case(c, h, w, R.FLAT), eps_outside=True) >= MUTANT_MARGIN


@pytest.mark.parametrize("c,h,w", [(v[0],) + v[7] for v in R.DW_VARIANTS])
def test_mutant_eps_outside_sqrt_dw_ripple(c, h, w):
    assert _dw_mutant(_dw_case(c, h, w, R.RIPPLE), eps_outside=True) >= MUTANT_MARGIN


# every row of a flat row-LayerNorm case has a constant of its own: some row's mean is always inexact
@pytest.mark.parametrize("case", [(65, 5, R.FLAT), (769, 517, R.FLAT), (2048, 3, R.FLAT)])
def test_mutant_eps_outside_sqrt_ln_flat(case):
    assert _ln_mutant(case, eps_outside=True) >= MUTANT_MARGIN




@pytest.mark.parametrize("tap", [(0, 0), (6, 6)])
@pytest.mark.parametrize("c,h,w", [(v[0],) + v[7] for v in R.DW_VARIANTS])
def test_mutant_tap_zeroed(c, h, w, tap):
    case = _dw_case(c, h, w)
    w49c = R.dw_data(case)["w"].clone()
    w49c[7 * tap[0] + tap[1]] = 0
    assert _dw_mutant(case, w49c) >= MUTANT_MARGIN


def test_tap_zeroed_needs_seven_rows():
    """Why every variant has an H >= 7 case: at H = 3 no output row reaches ky = 0 or ky = 6, so a missing tap
    there changes nothing."""
    case = _dw_case(96, 3, 16)
    w49c = R.dw_data(case)["w"].clone()
    w49c[0] = 0
    w49c[48] = 0
    assert torch.equal(_dw_y_f32(case, w49c), _dw_y_f32(case))


@pytest.mark.parametrize("kind", R.IMPULSES)
@pytest.mark.parametrize("c,h,w", [(v[0],) + v[7] for v in R.DW_VARIANTS])
def test_mutant_taps_transposed(c, h, w, kind):
    case = _dw_case(c, h, w, kind)
    assert h != w
    w49c = R.dw_data(case)["w"].reshape(7, 7, c).transpose(0, 1).reshape(49, c)
    assert _dw_mutant(case, w49c) >= MUTANT_MARGIN


@pytest.mark.parametrize("rows", R.LN_ROWS)
def test_mutant_mean_over_lane_slots(rows):
    """mean = sum / (64 NJ): 128 at C = 65."""
    assert _ln_mutant((65, rows, R.NORMAL), mean_div=128) >= MUTANT_MARGIN
