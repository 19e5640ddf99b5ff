"""tests/explain_ref.py against what it restates (CPU), and the conditions the GPU grid of
tests/test_gpu_explain_matrix.py relies on, checked on the grid's own seeded inputs: the share of
(image, prototype) pairs whose location has a single candidate pixel, and that every planted fact
does occur."""
import numpy as np
import pytest
import torch

import explain_ref as R


def _nchw(m):
    return m.permute(0, 3, 1, 2)


def _two_step(m_nhwc):
    h_idx, w_idx = R.two_step_loc(_nchw(m_nhwc))
    return h_idx * m_nhwc.shape[2] + w_idx


# ---- the references ------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 1, 1, 5), (2, 1, 6, 7), (2, 6, 1, 7), (3, 5, 7, 9), (2, 7, 5, 9), (2, 13, 13, 4)])
def test_first_rank_loc_is_the_two_step_max(shape):
    g = torch.Generator().manual_seed(sum(shape))
    rand = torch.randn(*shape, generator=g)
    tied = torch.randint(0, 3, shape, generator=g).float()             # three levels: many pixels hold the maximum
    const = torch.full(shape, -2.5)
    inf = tied.clone()
    inf[tied == 2] = float("inf")
    for m in (rand, tied, const, inf, torch.full(shape, -float("inf"))):
        assert torch.equal(R.first_rank_loc(m), _two_step(m))
        assert torch.equal(R.first_rank_loc(m, skip_nan=True), _two_step(m))
        assert torch.equal(R.max_skip_nan(m), m.double().amax(dim=(1, 2)))
    if shape[1] > 1 and shape[2] > 1:                                  # the rule is not the flat argmax
        flat = tied.reshape(shape[0], -1, shape[3]).argmax(dim=1)
        assert not torch.equal(R.first_rank_loc(tied), flat)


def test_first_rank_loc_on_nan_maps():
    nan, inf = float("nan"), float("inf")
    m = torch.tensor([[1.0, nan, 5.0], [5.0, 2.0, nan]]).view(1, 2, 3, 1)          # maxima at (0,2) and (1,0)
    assert R.first_rank_loc(m).tolist() == [[0]]                        # amax is NaN: no pixel equals it
    assert R.first_rank_loc(m, skip_nan=True).tolist() == [[3]]         # (1,0): the smaller w
    assert R.max_skip_nan(m).tolist() == [[5.0]]
    m = torch.full((1, 2, 3, 1), nan)
    assert R.first_rank_loc(m, skip_nan=True).tolist() == [[0]] and R.max_skip_nan(m).tolist() == [[-inf]]
    m = torch.full((1, 2, 3, 1), -inf)
    m[0, 0, 0, 0] = nan
    assert R.first_rank_loc(m, skip_nan=True).tolist() == [[3]]         # the first -inf by rank: (1,0)


def _replay_inputs(n, p, h, w, seed, kind):
    score, _, _ = R.topk_inputs(n, p, kind, 0)
    g = torch.Generator().manual_seed(seed)
    loc = torch.randint(0, h * w, (n, p), generator=g, dtype=torch.int32)
    outputs = []
    for i in range(n):
        fmap = torch.zeros(1, p, h * w)
        fmap.scatter_(2, loc[i].long().view(1, p, 1), 1.0)
        outputs.append((fmap.view(1, p, h, w), score[i:i + 1], torch.ones(1, 3)))
    return score, loc, outputs


@pytest.mark.parametrize("kind", R.TOPK_KINDS)
@pytest.mark.parametrize("k", [1, 4, 32])
def test_topk_expected_is_the_reference_loop(kind, k):
    n, p, h, w, i0 = 23, 6, 3, 4, 2 ** 31 - 3
    score, loc, outputs = _replay_inputs(n, p, h, w, k, kind)
    groups = [int(v) for v in torch.randint(-1, 3, (n,), generator=torch.Generator().manual_seed(k))]
    for min_score in (None, R.MIN_AT, R.MIN_BELOW):
        for grp in (None, groups):
            lists, _ = R.reference_lists(outputs, k, range(p), min_score=min_score, groups=grp)
            for gi in ([0] if grp is None else [0, 1, 2]):             # 2 is never drawn: an empty list
                s, idx, l = R.topk_expected(score.numpy(), loc.numpy(), k, None if grp is None else np.array(grp), gi,
                                            min_score, i0)
                assert s.dtype == np.float32 and idx.dtype == np.int64 and l.dtype == np.int32
                for pp in range(p):
                    lst = lists.get((pp, None if grp is None else gi), [])
                    want = [(sc, i + i0, hh * w + ww) for sc, i, hh, ww in lst]
                    got = [(float(s[pp, j]), int(idx[pp, j]), int(l[pp, j])) for j in range(len(lst))]
                    assert got == want, (kind, k, min_score, gi, pp)
                    assert (s[pp, len(lst):] == 0).all() and (idx[pp, len(lst):] == -1).all()
                    assert (l[pp, len(lst):] == -1).all()
    assert (R.topk_expected(score.numpy(), loc.numpy(), k, None, 1)[1] == -1).all()       # no ids: all in group 0


def test_min_score_levels():
    at, below = np.float32(R.MIN_AT), np.float32(R.MIN_BELOW)
    assert at in np.float32(R.LEVELS) and below < at and np.nextafter(below, np.float32(1)) == at
    score = np.float32([[0.25], [R.MIN_BELOW], [0.5]])
    loc = np.zeros((3, 1), np.int32)
    assert R.topk_expected(score, loc, 3, min_score=R.MIN_AT)[1].tolist() == [[2, 0, -1]]      # equal: kept
    assert R.topk_expected(score, loc, 3, min_score=R.MIN_BELOW)[1].tolist() == [[2, 0, 1]]


def test_abstained_is_amax_equal_zero():
    nan = float("nan")
    out = torch.tensor([[0.0, -1.0, -2.0], [-0.0, -1.0, -1.0], [R.SUBNORMAL, 0.0, -1.0], [-1.0, -2.0, -3.0],
                        [nan, 0.0, 0.0], [0.0, 0.5, 0.0]])
    assert R.abstained(out).tolist() == [True, True, False, False, False, False]
    for k in R.ABSTAIN_K:
        out = R.abstain_case(17, k, 0)
        kinds = [R.ABSTAIN_KINDS[r % 6] for r in range(17)]
        assert R.abstained(out).tolist() == [kd in ("zero", "neg_zero") for kd in kinds]
        sub = out[kinds.index("subnormal")]
        assert float(sub.max()) == R.SUBNORMAL and 0 < R.SUBNORMAL < 1.5e-45          # kept by torch on the CPU
        assert bool(torch.isnan(out[kinds.index("nan")]).any())
        if k > 1:
            assert float(out[kinds.index("nan")].nan_to_num(-1.0).max()) == 0.0       # NaN beside zeros


# ---- (a) the pool_argmax grid ----------------------------------------------------------------
def test_pool_rows_sit_at_both_edges_of_every_bucket():
    edges = {1: (1, 64), 2: (65, 128), 4: (129, 256), 8: (257, 512), 12: (513, 768), 16: (769, 1024), 32: (1025, 2048)}
    ps = [p for p, _, _ in R.POOL_ROWS]
    for nj, (lo, hi) in edges.items():
        assert lo in ps and hi in ps, nj
    assert max(R.POOL_B * h * w * p for p, h, w in R.POOL_ROWS) <= 2 * 13 * 13 * 2048


@pytest.mark.parametrize("p,h,w", R.POOL_ROWS)
def test_pool_row_has_single_candidates(p, h, w):
    """At least 99 % of the (image, prototype) pairs judged by candidates leave exactly one candidate
    pixel, so the candidate test cannot hide a wrong location; torch's float32 softmax lands inside the
    candidates and inside the pooled tolerance."""
    c = R.pool_case(p, h, w)
    free = c["free"]
    n_cand = c["cand"].sum(dim=(1, 2))[:, free]
    share = float((n_cand == 1).double().mean())
    print(f"P = {p} ({h} x {w}): single-candidate pairs {int((n_cand == 1).sum())} / {n_cand.numel()} = {share:.4f}")
    assert share >= 0.99
    assert bool((n_cand >= 1).all())
    f32 = torch.softmax(c["x"], dim=-1)
    loc = R.first_rank_loc(f32)
    at = c["cand"].reshape(R.POOL_B, h * w, p).gather(1, loc[:, None, :])[:, 0]
    assert bool(at.all())
    err = (f32.amax(dim=(1, 2)).double() - c["pooled"]).abs()
    assert bool((err <= R.POOL_ATOL + R.POOL_RTOL * c["pooled"]).all())
    assert torch.equal(R.first_rank_loc(c["proto"])[:, free][n_cand == 1], loc[:, free][n_cand == 1])


@pytest.mark.parametrize("p,h,w", [r for r in R.POOL_ROWS if r[1] * r[2] >= 4])
def test_pool_row_planted_facts(p, h, w):
    c = R.pool_case(p, h, w)
    x = c["x"]
    pix = R.planted_pixels(h, w)
    flat = [hh * w + ww for hh, ww in pix]
    rank = [ww * h + hh for hh, ww in pix]
    assert len(set(flat)) == 3
    for hh, ww in pix[1:]:                                              # one vector in three pixels
        assert torch.equal(x[:, hh, ww], x[:, pix[0][0], pix[0][1]])
    winner = flat[rank.index(min(rank))]
    if h > 1 and w > 1:
        assert winner != min(flat)                                      # the flat argmax would be wrong
    else:
        assert winner == min(flat)                                      # one row or column: the two orders agree
    if h * w > R.PIX_PER_BLOCK:                                         # the cross-workgroup atomicMax decides
        assert winner // R.PIX_PER_BLOCK != max(flat) // R.PIX_PER_BLOCK
        assert max(flat) - min(flat) >= 32 or h * w == 33               # 33 pixels: only 0 and 32 are 32 apart,
    else:                                                               # and pixel 0 wins under either order
        assert len({f % R.WAVES for f in flat}) == 3                    # three waves of the one workgroup
    sat, dead = p - 1, p // 2
    assert c["planted"] == {sat: (1.0, winner), dead: (0.0, 0)} and sat != dead
    f32 = torch.softmax(x, dim=-1)
    for hh, ww in pix:
        assert bool((f32[:, hh, ww, sat] == 1.0).all())                 # exactly 1.0f
    assert bool((f32[..., dead] == 0.0).all())                          # exactly 0.0f
    hit = (f32[..., sat] == 1.0).reshape(R.POOL_B, -1).sum(dim=1)
    assert hit.tolist() == [3] * R.POOL_B                               # nowhere else
    assert (R.first_rank_loc(f32)[:, sat] == winner).all() and (R.first_rank_loc(f32)[:, dead] == 0).all()
    assert bool((1.0 - c["pooled"][:, sat] < 2.0 ** -30).all())         # float64: far inside the rounding to 1.0f
    assert bool((c["pooled"][:, dead] < 1e-80).all())


def test_ones_case_is_exactly_one():
    x = R.ones_case()
    assert x.shape == (R.POOL_B, 5, 7, 1) and bool((torch.softmax(x, dim=-1) == 1.0).all())


# ---- (b), (c): the other grids -----------------------------------------------------------------
def test_map_cases_hold_what_they_name():
    assert sorted(p for p, _, _ in R.MAP_ROWS) == sorted(R.MAP_P) and len(R.MAP_ROWS) == 7
    assert (2048, 2, 9) in R.MAP_ROWS and R.map_case(2048, 2, 9, "random").shape[0] == 3
    for p, h, w in R.MAP_ROWS:
        for kind in R.MAP_KINDS + ["nan"]:
            m = R.map_case(p, h, w, kind)
            assert m.shape[1:] == (h, w, p) and m.dtype == torch.float32 and m.is_contiguous()
        assert bool((R.map_case(p, h, w, "negative") < 0).all())
        sp = R.map_case(p, h, w, "sparse")
        assert set(sp.unique().tolist()) <= {0.0, 1.0} and float(sp[0, :, :, 0].max()) == 0.0
        assert float(sp[1, :, :, p - 1].sum()) == 1.0 and float(sp[1, h - 1, w - 1, p - 1]) == 1.0
        assert bool(torch.isinf(R.map_case(p, h, w, "pos_inf")).any())
        nan = R.map_case(p, h, w, "nan")
        assert bool(torch.isnan(nan[0, :, :, 0]).all())
        assert bool((R.max_skip_nan(nan)[0, 0] == -float("inf")).all())
    nan = R.map_case(65, 5, 7, "nan")
    part = torch.isnan(nan).reshape(2, 35, 65).sum(dim=1)
    assert bool(((part > 0) & (part < 35)).any())                      # maps that are partly NaN
    assert int(R.first_rank_loc(nan, skip_nan=True)[1, 1]) == 7         # NaN first, then -inf: pixel (1, 0)


def test_topk_rows_cover_every_axis():
    rows = R.TOPK_ROWS
    assert {r[0] for r in rows} == {1, 63, 64, 65, 768, 2048} and {r[1] for r in rows} == {1, 3, 5}
    assert {r[2] for r in rows} == {1, 2, 10, 31, 32} and {r[3] for r in rows} == set(R.TOPK_KINDS)
    assert {r[4] for r in rows} == set(R.I0S) and {r[5] for r in rows} == {None, R.MIN_AT, R.MIN_BELOW}
    assert (2048, 3, 32) in {r[:3] for r in rows}
    mult = {(r[0] * r[1]) % 64 == 0 for r in rows}
    assert mult == {True, False}
    assert all(sum(s) == R.TOPK_N for s in R.TOPK_SPLITS.values())
    for p, g, k, kind, i0, ms in rows:
        if p > 65:
            continue
        c = R.topk_case(p, g, k, kind, i0, ms)
        if c["group"] is not None:
            ids = set(c["group"].tolist())
            assert -1 in ids and g in ids and ids <= set(range(-1, g + 1))
        if ms is not None:
            assert bool((c["score"] == ms).any() if ms == R.MIN_AT else (c["score"] < ms).any())
        if i0 == 2 ** 31 - 3:
            idx = np.concatenate([e[1].ravel() for e in c["expected"]])
            assert (idx >= 2 ** 31).any() and ((idx >= 0) & (idx < 2 ** 31)).any()
    z = R.topk_inputs(R.TOPK_N, 65, "zeros", 5)[0]
    assert bool((torch.signbit(z) & (z == 0)).any()) and bool((~torch.signbit(z) & (z == 0)).any())
    assert bool(torch.isinf(R.topk_inputs(R.TOPK_N, 65, "inf", 3)[0]).any())
