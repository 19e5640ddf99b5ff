"""tests/backbone_bwd_ref.py checked without a GPU: every grid row reaches the slab count it names through the
library's own host functions (pipnet_wgrad_workspace_bytes, pipnet_bn_slabs), the exact cases are exact
(float32 on the CPU gives the float64 reference's bits, every partial sum is below 2^24), the same graphs in
torch float32 stay inside the tolerances of the inexact outputs (the share they use is printed), the tie
fixtures hold exact float32 ties, the width grid reaches every PIPNET_BY_NJ4 branch, and the operand checks
of the wrappers raise before the library is touched."""
import pytest
import torch

import backbone_bwd_ref as R
from count_pipnet_amd import _lib
from count_pipnet_amd import kernels as K


@pytest.fixture(scope="module")
def lib():
    from count_pipnet_amd import build
    build.build()
    return _lib.load()


def _slabs(lib, m, n1, n2):
    return lib.pipnet_wgrad_workspace_bytes(m, n1, n2) // (4 * n1 * n2)


# ---- the plans ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n1,n2,slabs,ktiles", R.WGRAD_ROWS)
def test_wgrad_rows_reach_their_slabs(lib, m, n1, n2, slabs, ktiles):
    assert _slabs(lib, m, n1, n2) == slabs
    assert R.slab_ktiles(m, slabs) == ktiles and sum(ktiles) == -(-m // R.WBK)
    if slabs > 1:
        assert ktiles[0] >= 8                                    # a split only with >= 8 K-tiles per full slab
    assert 16 * m + 3 < 2 ** 24


def test_wgrad_grid_reaches_what_it_names():
    rows = {r[:3]: r for r in R.WGRAD_ROWS}
    assert rows[(4100, 128, 128)][4][-2:] == [3, 0] and rows[(2081, 4, 4)][4][-1] == 3
    assert rows[(65570, 128, 128)][4].count(0) == 21 and len(rows[(65570, 128, 128)][4]) == 249
    assert rows[(9000, 768, 768)][3] == 14 < (-(-9000 // 32)) // 8            # fewer than the 35 slabs allowed
    cases = R.WGRAD_CASES
    assert {c[:3] for c in cases} == set(rows)                                # every row runs
    direct = [c for c in cases if rows[c[:3]][3] <= 1]
    split = [c for c in cases if rows[c[:3]][3] > 1]
    assert sum(c[3] for c in direct) >= 5 and sum(c[3] for c in split) >= 2   # accumulate on both kinds
    assert (5, 4, 8, True, False, 0) in cases                                 # one slab through the workspace
    assert (0, 8, 8, True, False, 0) in cases and (0, 8, 8, False, False, 0) in cases
    assert sum(c[4] for c in cases) == 2                                      # strided A and B
    ld = [c for c in cases if c[5]]
    assert len(ld) == 2 and {rows[c[:3]][3] > 1 for c in ld} == {True, False}
    assert all(c[5] % 4 == 0 for c in ld)


@pytest.mark.parametrize("b,h,w,cin,cout,k,s,p,acc,slabs", R.WGRAD_CONV_ROWS)
def test_conv_rows(lib, b, h, w, cin, cout, k, s, p, acc, slabs):
    oh, ow = R.conv_out_hw(h, w, k, s, p)
    assert h != w and oh != ow
    assert cin in (4, 132) and cout in (4, 132)
    assert _slabs(lib, b * oh * ow, cout, k * k * cin) == slabs
    if slabs > 1:
        assert b * oh * ow >= 544


def test_conv_grid():
    forms = {(k, s, p) for _, _, _, _, _, k, s, p, _, _ in R.WGRAD_CONV_ROWS}
    assert forms == {(3, 1, 1), (3, 2, 1), (1, 2, 0), (7, 2, 3), (4, 4, 0)}
    assert any(r[9] > 1 for r in R.WGRAD_CONV_ROWS) and any(r[8] for r in R.WGRAD_CONV_ROWS)
    assert any(r[3] == 132 and (r[5] * r[5] * 132) % 128 for r in R.WGRAD_CONV_ROWS)    # a tap ends inside a tile
    stem = [r for r in R.WGRAD_CONV_ROWS if r[5:8] == (4, 4, 0)][0]
    assert stem[1] % 4 and stem[2] % 4                                        # leftover rows and columns
    assert {r[5] for r in R.WGRAD_CONV2X2_ROWS} == {1, 2} and any(r[6] for r in R.WGRAD_CONV2X2_ROWS)
    for b, h, w, cin, cout, s, acc in R.WGRAD_CONV2X2_ROWS:
        oh, ow = R.conv_out_hw(h, w, 2, s, 0)
        assert h != w and oh != ow and h % 2 == 1


@pytest.mark.parametrize("m,c,g,res,relu,running,want_dx,want_masked", R.BN_ROWS)
def test_bn_rows_reach_their_slabs(lib, m, c, g, res, relu, running, want_dx, want_masked):
    assert lib.pipnet_bn_slabs(m, c) == g


def test_bn_grid(lib):
    gs = {r[2] for r in R.BN_ROWS}
    assert 1 in gs and any(16 < g <= 64 for g in gs) and any(64 < g < 1024 for g in gs) and 1024 in gs
    assert lib.pipnet_bn_slabs(65600, 256) == 1024 and 65600 // (4 * 16) == 1025        # clamped, not reached
    assert any((c // 4) % 64 for _, c, *_ in R.BN_ROWS if c // 4 > 64)                  # ragged quads
    assert {(r[3], r[4]) for r in R.BN_ROWS} == {(False, False), (False, True), (True, False), (True, True)}
    assert {r[5] for r in R.BN_ROWS} == {True, False} and {r[6] for r in R.BN_ROWS} == {True, False}
    assert {r[7] for r in R.BN_ROWS} == {True, False}
    assert any(m * c // 4 > R.BN_ELEM_SWEEP for m, c, *_ in R.BN_ROWS)
    assert lib.pipnet_bn_slabs(*R.BN_LARGE_MEAN[:2]) == R.BN_LARGE_MEAN[2]
    assert lib.pipnet_bn_slabs(16, 24) == 0 and lib.pipnet_bn_slabs(0, 64) == 0         # rejected shapes


def test_width_and_row_grids():
    seen = {(R.nj4(c), c % 256 != 0) for c in R.WIDTHS}
    assert seen == {(n, r) for n in (1, 2, 3, 4, 8) for r in (True, False)}
    assert R.nj4(2052) is None
    assert {R.nj4(p) for p in R.HEAD_WIDTHS} == {1, 2, 3, 4, 8}
    assert any(m <= R.SWEEP_ROWS for m in R.ROW_COUNTS) and R.SWEEP_ROWS in R.ROW_COUNTS
    assert R.SWEEP_ROWS + 1 in R.ROW_COUNTS and any(m > 2 * R.SWEEP_ROWS for m in R.ROW_COUNTS)
    bh, h, w, p = R.HEAD_SWEEP
    assert bh * h * w > 4096
    assert any(m % rps for m, _, rps, _, _ in R.LS_CASES)
    assert {c[3] for c in R.LS_CASES} == {True, False} and {c[4] for c in R.LS_CASES} == {True, False}
    assert {c[2] for c in R.LN_CASES} == {True, False} and {c[3] for c in R.LN_CASES} == {True, False}
    assert R.GELU_N % 4 == 0 and R.GELU_N // 4 > 8192 * 256
    ms = [m for m, _, _ in R.COLSUM_ROWS]
    assert 0 in ms and any(0 < m < 64 for m in ms) and 64 in ms and 65 in ms and any(s for _, _, s in R.COLSUM_ROWS)
    assert any(h < 7 and w < 7 for _, h, w, _ in R.DWCONV_ROWS) and any(h >= 7 and w >= 7 for _, h, w, _ in R.DWCONV_ROWS)


# ---- exact cases are exact ------------------------------------------------------------------------------
def _exact(ref64, ref32):
    assert ref64.dtype == torch.float64 and ref32.dtype == torch.float32
    assert torch.equal(ref64, ref64.round()) and (ref64.numel() == 0 or float(ref64.abs().max()) < 2 ** 24)
    assert torch.equal(ref64.float(), ref32)


@pytest.mark.parametrize("m,n1,n2,acc,strided,ldx", R.WGRAD_CASES)
def test_wgrad_cases_exact(m, n1, n2, acc, strided, ldx):
    _exact(R.wgrad_ref(m, n1, n2, acc, strided), R.wgrad_ref(m, n1, n2, acc, strided, torch.float32))
    c = R.wgrad_case(m, n1, n2, strided)
    if m:
        assert float((c["a"].abs().t() @ c["b"].abs()).max()) + 3 < 2 ** 24      # every partial sum, any order


@pytest.mark.parametrize("row", R.WGRAD_CONV_ROWS)
def test_conv_cases_exact(row):
    _exact(R.conv_wgrad_ref(*row[:9]), R.conv_wgrad_ref(*row[:9], dtype=torch.float32))


@pytest.mark.parametrize("b,h,w,cin,cout,s,acc", R.WGRAD_CONV2X2_ROWS)
def test_conv2x2_cases_exact(b, h, w, cin, cout, s, acc):
    _exact(R.conv_wgrad_ref(b, h, w, cin, cout, 2, s, 0, acc),
           R.conv_wgrad_ref(b, h, w, cin, cout, 2, s, 0, acc, dtype=torch.float32))


@pytest.mark.parametrize("m,n,strided", R.COLSUM_ROWS)
def test_colsum_cases_exact(m, n, strided):
    for acc in (False, True):
        _exact(R.colsum_ref(m, n, strided, acc), R.colsum_ref(m, n, strided, acc, torch.float32))


@pytest.mark.parametrize("m,c,rps,with_rs,acc", R.LS_CASES)
def test_ls_cases_exact(m, c, rps, with_rs, acc):
    a, b = R.ls_ref(m, c, rps, with_rs, acc), R.ls_ref(m, c, rps, with_rs, acc, torch.float32)
    for k in ("out", "dy2", "d_ls", "d_b2"):
        _exact(a[k], b[k])
    k = R.ls_case(m, c, rps, with_rs)
    assert float((k["dy"].abs() * 2 * k["y2"].abs()).sum(0).max()) + 3 < 2 ** 24


@pytest.mark.parametrize("b,h,w,c", R.DWCONV_ROWS)
def test_dwconv_cases_exact(b, h, w, c):
    x, y = R.dw_ref(b, h, w, c), R.dw_ref(b, h, w, c, torch.float32)
    for k in x:
        _exact(x[k], y[k])


@pytest.mark.parametrize("m,c,want_dz,acc", R.LN_CASES)
def test_ln_d_beta_exact_and_float32_inside_tolerance(m, c, want_dz, acc):
    a, b = R.ln_ref(m, c, acc), R.ln_ref(m, c, acc, torch.float32)
    _exact(a["d_beta"], b["d_beta"])
    s_dz = R.share(b["dz"], a["dz"], *R.TOL["ln_dz"])
    s_dg = R.share(b["d_gamma"], a["d_gamma"], R.TOL["colsum_rtol"], R.colsum_atol(m))
    print(f"ln float32 share M={m} C={c}: dz {s_dz:.3f} d_gamma {s_dg:.3f}")
    assert s_dz <= 1 and s_dg <= 1


@pytest.mark.parametrize("row", R.BN_ROWS)
def test_bn_float32_inside_tolerance(row):
    m, c, _, res, relu, _, want_dx = row[:7]
    a = R.bn_ref(m, c, res, relu)
    b = R.bn_ref(m, c, res, relu, dtype=torch.float32, mask=a["y"] > 0)
    _exact(a["d_beta"], b["d_beta"])
    _exact(a["masked"], b["masked"])
    assert torch.equal(a["y"] > 0, a["y"].float() > 0)         # the float32 output the kernel is given has the mask
    scale = float(a["dx"].abs().max())
    shares = dict(y=R.share(b["y"], a["y"], *R.TOL["bn_apply"]),
                  dx=R.share(b["dx"], a["dx"], R.TOL["bn_dx"][0], R.TOL["bn_dx"][1] * scale) if want_dx else 0.0,
                  d_gamma=R.share(b["d_gamma"], a["d_gamma"], R.TOL["colsum_rtol"], R.colsum_atol(m)),
                  invstd=R.share(b["invstd"], a["invstd"], *R.TOL["bn_stats"]),
                  running_var=R.share(b["running_var"], a["running_var"], *R.TOL["bn_stats"]))
    print(f"bn float32 share M={m} C={c}: " + " ".join(f"{k} {v:.3f}" for k, v in shares.items()))
    assert max(shares.values()) <= 1


def test_bn_large_mean_separates_one_pass_from_welford():
    m, c, _ = R.BN_LARGE_MEAN
    x = R.bn_case(m, c, True)["x"]
    var = x.var(0, unbiased=False)
    x32 = x.float()
    two_pass = x32.var(0, unbiased=False).double()
    one_pass = ((x32 * x32).mean(0) - x32.mean(0) ** 2).double()
    e2, e1 = float(((two_pass - var) / var).abs().max()), float(((one_pass - var) / var).abs().max())
    print(f"large-mean variance, relative error: float32 two-pass {e2:.2e}, one-pass E[x^2]-E[x]^2 {e1:.2e}")
    assert e2 < R.TOL["large_mean"] / 100 and e1 > R.TOL["large_mean"] * 10


def _head_cases():
    bh = 2
    out = [(bh, *R.HEAD_MAP, p, "all", None) for p in R.HEAD_WIDTHS]
    out += [(bh, *R.HEAD_MAP, 260, mode, None) for mode in R.HEAD_MODES if mode != "all"]
    out += [(*R.TIE_SHAPE, "all", tie) for tie in R.TIE_KINDS]
    return out


@pytest.mark.parametrize("bh,h,w,p,mode,tie", _head_cases())
def test_head_float32_inside_tolerance(bh, h, w, p, mode, tie):
    a, b = R.head_ref(bh, h, w, p, mode, tie), R.head_ref(bh, h, w, p, mode, tie, torch.float32)
    s = R.share(b["d_logits"], a["d_logits"], *R.TOL["head"])
    print(f"head float32 share P={p} {mode} {tie}: {s:.3f}")
    assert s <= 1


def test_gelu_float32_inside_tolerance():
    x = R.randn((1 << 16,), 11, 3.0)
    s = R.share(R.gelu_ref(x.float()), R.gelu_ref(x), *R.TOL["gelu"])
    print(f"gelu float32 share: {s:.3f}")
    assert s <= 1


# ---- the tie fixtures ---------------------------------------------------------------------------------
@pytest.mark.parametrize("tie", R.TIE_KINDS)
def test_tie_fixtures_hold_exact_ties(tie):
    bh, h, w, p = R.TIE_SHAPE
    proto = R.head_proto(bh, h, w, p, tie)
    assert proto.dtype == torch.float32
    cols = proto.view(2 * bh, h * w, p)
    top = cols.max(dim=1, keepdim=True).values
    hits = cols == top                                                   # exact float32 equality
    if tie == "first_last":
        assert bool(hits[:, 0].all()) and bool(hits[:, -1].all())
    elif tie == "middle":
        i, j = R.TIE_MIDDLE
        assert bool(hits[:, i].all()) and bool(hits[:, j].all()) and not bool(hits[:, :i].any())
    elif tie == "constant":
        assert bool(hits[:, :, 0::2].all())
    else:
        assert bool((top == 1.0).any()) and int((hits.sum(1) >= 2).sum()) >= 3      # several columns tie at 1.0f
    # the reference routes the pooled gradient to the first maximum: with the tanh term alone every
    # (image, prototype) has a non-zero pooled gradient, and it lands on the first hit only
    ref = R.head_ref(bh, h, w, p, "tanh", tie)
    g = ref["g"].reshape(2 * bh, h * w, p)
    first = hits.int().argmax(dim=1)                                     # first index of the maximum
    want = torch.zeros_like(hits).scatter_(1, first.unsqueeze(1), True)
    assert torch.equal(g != 0, want)


# ---- the wrappers' operand checks raise before the library is touched ------------------------------------
BAD_CALL_NAMES = [n for n, _ in R.bad_calls(K, lambda *s: None)]


def test_wrappers_reject_cpu_tensors_without_the_library(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", touched)
    monkeypatch.setattr(_lib, "call", touched)
    for name, call in R.bad_calls(K, lambda *s: torch.zeros(*s)):
        with pytest.raises(RuntimeError):
            call()
    x = torch.zeros(6, 8)
    with pytest.raises(RuntimeError, match="float32 ROCm device tensor"):
        K.ln_backward(x, x, torch.zeros(8), torch.zeros(8), torch.zeros(8))
    with pytest.raises(RuntimeError, match="float32 ROCm device tensor"):
        K.bn_stats(x.double(), 1e-5, 0.1)


@pytest.mark.parametrize("name", BAD_CALL_NAMES)
def test_wrappers_reject_wrong_shapes_without_the_library(monkeypatch, name):
    """The device test switched off, every bad operand must still stop at its own shape check -- the message
    names the function -- before the library is loaded or called."""
    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", touched)
    monkeypatch.setattr(_lib, "call", touched)
    monkeypatch.setattr(K, "require_device", lambda t, what="input": None)
    call = dict(R.bad_calls(K, lambda *s: torch.zeros(*s)))[name]
    with pytest.raises(RuntimeError, match=name.split()[0].rstrip("_") + "|contiguous"):
        call()
