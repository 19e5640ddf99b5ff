"""The backbone backward (csrc/backward_ops.hip) and BatchNorm (csrc/bn_ops.hip) kernels over their full launch
plans, against the float64 references of tests/backbone_bwd_ref.py (grids, data and tolerances there; checked
without a GPU by tests/test_backbone_bwd_cpu.py).

* exact rows (integer data, every sum below 2^24): ``torch.equal`` with the float64 reference, and the
  sentinel frame around every caller-allocated output intact;
* every reduction is called twice and must repeat its bits (fixed slabs, fixed order, no atomics);
* inexact outputs inside the sibling tests' tolerances; the share of the tolerance used is printed.
"""
import pytest
import torch

import backbone_bwd_ref as R
from count_pipnet_amd import _lib
from count_pipnet_amd import kernels as K

pytestmark = pytest.mark.gpu


def _f(t, gpu):
    return None if t is None else t.float().contiguous().to(gpu)


def _same(got, ref64):
    """Bit-equal to the float64 reference (an exact row)."""
    return torch.equal(got.cpu(), ref64.float())


def _close(name, got, ref64, rtol, atol):
    print(f"  {name}: share of tolerance {R.share(got.cpu(), ref64, rtol, atol):.3f}")
    torch.testing.assert_close(got.cpu().double(), ref64, rtol=rtol, atol=atol, msg=lambda m: f"{name}: {m}")


# ---- wgrad ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n1,n2,acc,strided,ldx", R.WGRAD_CASES)
def test_wgrad(gpu, m, n1, n2, acc, strided, ldx):
    c = R.wgrad_case(m, n1, n2, strided)
    if strided:
        big = _f(c["big"], gpu)
        a, b = big[:, c["a_cols"][0]:c["a_cols"][1]], big[:, c["b_cols"][0]:c["b_cols"][1]]
        assert a.stride(0) == n1 + n2 + 8 and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
    else:
        a, b = _f(c["a"], gpu), _f(c["b"], gpu)
    ref = R.wgrad_ref(m, n1, n2, acc, strided)
    outs = []
    for _ in range(2):
        fr = R.Framed((n1, n2), gpu, base=c["base"] if acc else None, ld=n2 + ldx if ldx else None)
        assert K.wgrad(a, b, out=fr.view, accumulate=acc) is fr.view
        assert _same(fr.view, ref)
        assert fr.intact()
        outs.append(fr.view.clone())
    assert torch.equal(outs[0], outs[1])
    if not acc and not ldx:
        assert _same(K.wgrad(a, b), ref)


def test_wgrad_no_rows_leaves_the_workspace_alone(gpu):
    """M = 0 through the C entry point with a framed one-float workspace (what kernels.wgrad passes): the
    accumulate call changes neither C nor the workspace, the plain call stores zeros."""
    n1 = n2 = 8
    base = R.wgrad_case(0, n1, n2, False)["base"]
    stream = torch.cuda.current_stream(gpu).cuda_stream
    for acc in (1, 0):
        out, ws = R.Framed((n1, n2), gpu, base=base), R.Framed((1,), gpu)
        _lib.call("pipnet_wgrad_f32", None, n1, None, n2, 0, n1, n2, out.view.data_ptr(), n2, acc, ws.view.data_ptr(),
                  stream)
        torch.cuda.synchronize()
        assert ws.untouched() and out.intact()
        assert _same(out.view, base if acc else torch.zeros(n1, n2, dtype=torch.float64))


@pytest.mark.parametrize("b,h,w,cin,cout,k,s,p,acc,slabs", R.WGRAD_CONV_ROWS)
def test_wgrad_conv(gpu, b, h, w, cin, cout, k, s, p, acc, slabs):
    c = R.conv_case(b, h, w, cin, cout, k, s, p)
    x, dy = _f(c["x"], gpu), _f(c["dy"], gpu)
    ref = R.conv_wgrad_ref(b, h, w, cin, cout, k, s, p, acc)
    outs = []
    for _ in range(2):
        fr = R.Framed((cout, k * k * cin), gpu, base=c["base"] if acc else None)
        K.wgrad_conv(dy, x, k, k, s, fr.view, accumulate=acc, pad=p)
        assert _same(fr.view, ref)
        assert fr.intact()
        outs.append(fr.view.clone())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("b,h,w,cin,cout,s,acc", R.WGRAD_CONV2X2_ROWS)
def test_wgrad_conv2x2(gpu, b, h, w, cin, cout, s, acc):
    c = R.conv_case(b, h, w, cin, cout, 2, s, 0)
    x, dy = _f(c["x"], gpu), _f(c["dy"], gpu)
    ref = R.conv_wgrad_ref(b, h, w, cin, cout, 2, s, 0, acc)
    outs = []
    for _ in range(2):
        fr = R.Framed((cout, 4 * cin), gpu, base=c["base"] if acc else None)
        K.wgrad_conv2x2(dy, x, s, fr.view, accumulate=acc)
        assert _same(fr.view, ref)
        assert fr.intact()
        outs.append(fr.view.clone())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("m,n,strided", R.COLSUM_ROWS)
def test_colsum(gpu, m, n, strided):
    c = R.colsum_case(m, n, strided)
    big = _f(c["big"], gpu)
    a = big[:, 4:4 + n] if strided else big
    for acc in (False, True):
        ref = R.colsum_ref(m, n, strided, acc)
        outs = []
        for _ in range(2):
            fr = R.Framed((n,), gpu, base=c["base"] if acc else None)
            K.colsum(a, out=fr.view, accumulate=acc)
            assert _same(fr.view, ref)
            assert fr.intact()
            outs.append(fr.view.clone())
        assert torch.equal(outs[0], outs[1])
    assert _same(K.colsum(a), R.colsum_ref(m, n, strided, False))


# ---- layer scale, residual, LayerNorm -------------------------------------------------------------------
@pytest.mark.parametrize("m,c,rps,with_rs,acc", R.LS_CASES)
def test_resid_scale_and_ls_backward(gpu, m, c, rps, with_rs, acc):
    k = R.ls_case(m, c, rps, with_rs)
    ref = R.ls_ref(m, c, rps, with_rs, acc)
    x, y2, dy, ls, rs = (_f(k[n], gpu) for n in ("x", "y2", "dy", "ls", "rs"))
    fo = R.Framed((m, c), gpu)
    K.resid_scale(x, y2, ls, rs, rps, out=fo.view)
    assert _same(fo.view, ref["out"]) and fo.intact()
    assert _same(K.resid_scale(x, y2, ls, rs, rps), ref["out"])
    outs = []
    for _ in range(2):
        fl = R.Framed((c,), gpu, base=k["base_ls"] if acc else None)
        fb = R.Framed((c,), gpu, base=k["base_b2"] if acc else None)
        dy2 = K.ls_backward(dy, y2, ls, rs, rps, fl.view, fb.view, accumulate=acc)
        assert _same(dy2, ref["dy2"])
        assert _same(fl.view, ref["d_ls"]) and _same(fb.view, ref["d_b2"])
        assert fl.intact() and fb.intact()
        outs.append((dy2, fl.view.clone(), fb.view.clone()))
    assert all(torch.equal(p, q) for p, q in zip(*outs))


@pytest.mark.parametrize("m,c,want_dz,acc", R.LN_CASES)
def test_ln_backward(gpu, m, c, want_dz, acc):
    k = R.ln_case(m, c)
    ref = R.ln_ref(m, c, acc)
    z, dt, gamma = _f(k["z"], gpu), _f(k["dt"], gpu), _f(k["gamma"], gpu)
    outs = []
    for _ in range(2):
        fg = R.Framed((c,), gpu, base=k["base_g"] if acc else None)
        fb = R.Framed((c,), gpu, base=k["base_b"] if acc else None)
        dz = K.ln_backward(z, dt, gamma, fg.view, fb.view, want_dz=want_dz, accumulate=acc)
        assert fg.intact() and fb.intact()
        assert (dz is not None) == want_dz
        outs.append((fg.view.clone(), fb.view.clone()) + ((dz,) if want_dz else ()))
    assert all(torch.equal(p, q) for p, q in zip(*outs))
    dg, db = outs[0][:2]
    assert _same(db, ref["d_beta"])                                        # dt is integer: an exact column sum
    _close(f"ln d_gamma M={m} C={c}", dg, ref["d_gamma"], R.TOL["colsum_rtol"], R.colsum_atol(m))
    if want_dz:
        _close(f"ln dz M={m} C={c}", outs[0][2], ref["dz"], *R.TOL["ln_dz"])


def test_widths_above_2048_are_rejected_untouched(gpu):
    m, c = 4, 2052
    z = torch.ones(m, c, device=gpu)
    v = torch.ones(c, device=gpu)
    f1, f2 = R.Framed((c,), gpu), R.Framed((c,), gpu)
    with pytest.raises(RuntimeError):
        K.ls_backward(z, z, v, None, 1, f1.view, f2.view)
    with pytest.raises(RuntimeError):
        K.ln_backward(z, z, v, f1.view, f2.view)
    torch.cuda.synchronize()
    assert f1.untouched() and f2.untouched()
    assert _same(K.colsum(z), torch.full((c,), float(m), dtype=torch.float64))          # the stream still works


# ---- depthwise 7x7 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,h,w,c", R.DWCONV_ROWS)
def test_dwconv7(gpu, b, h, w, c):
    k = R.dw_case(b, h, w, c)
    ref = R.dw_ref(b, h, w, c)
    x, dz = _f(k["x"], gpu), _f(k["dz"], gpu)
    wp, wflip = _f(R.pack_dw(k["wt"]), gpu), _f(R.pack_dw(k["wt"].flip(2, 3)), gpu)
    assert _same(K.dwconv7_plain(x, wp, _f(k["bias"], gpu)), ref["y"])                  # forward with bias
    fx = R.Framed((b, h, w, c), gpu, base=k["base_x"])
    K.dwconv7_plain(dz, wflip, None, out=fx.view, accumulate=True)                     # input gradient, added
    assert _same(fx.view, ref["dx"]) and fx.intact()
    for acc in (False, True):
        outs = []
        for _ in range(2):
            fw = R.Framed((49, c), gpu, base=k["base_w"] if acc else None)
            fb = R.Framed((c,), gpu, base=k["base_b"] if acc else None)
            K.dwconv7_wgrad(dz, x, fw.view, fb.view, accumulate=acc)
            assert _same(fw.view, ref["dw_acc" if acc else "dw"]) and _same(fb.view, ref["db_acc" if acc else "db"])
            assert fw.intact() and fb.intact()
            outs.append((fw.view.clone(), fb.view.clone()))
        assert all(torch.equal(p, q) for p, q in zip(*outs))


# ---- max-pool head ------------------------------------------------------------------------------------------
def _head(gpu, bh, h, w, p, mode, tie=None):
    ref = R.head_ref(bh, h, w, p, mode, tie)
    w_align, w_tanh, _ = R.HEAD_MODES[mode]
    got = K.head_backward(ref["proto"].to(gpu), ref["pooled"].to(gpu), _f(ref["d_out"], gpu), ref["w"].to(gpu),
                          w_align, w_tanh)
    _close(f"head d_logits P={p} {mode} {tie}", got, ref["d_logits"], *R.TOL["head"])
    again = K.head_backward(ref["proto"].to(gpu), ref["pooled"].to(gpu), _f(ref["d_out"], gpu), ref["w"].to(gpu),
                            w_align, w_tanh)
    assert torch.equal(got, again)


@pytest.mark.parametrize("p", R.HEAD_WIDTHS)
def test_head_backward_every_width(gpu, p):
    _head(gpu, 2, *R.HEAD_MAP, p, "all")


@pytest.mark.parametrize("mode", sorted(R.HEAD_MODES))
def test_head_backward_each_term(gpu, mode):
    _head(gpu, 2, *R.HEAD_MAP, 260, mode)


def test_head_backward_second_sweep(gpu):
    _head(gpu, *R.HEAD_SWEEP, "all")


@pytest.mark.parametrize("tie", R.TIE_KINDS)
def test_head_backward_ties_go_to_the_first_maximum(gpu, tie):
    """Exact float32 ties of a column's maximum: the pooled gradient goes to the first one, as AdaptiveMaxPool2d's.
    (An argmax that takes the last maximum fails first_last, middle and constant.  It cannot fail saturated: a
    pixel whose softmax is exactly 1.0f has a zero softmax Jacobian, so d logits there is 0 wherever the pooled
    gradient lands -- that row pins the values at saturation, not the tie rule.)"""
    _head(gpu, *R.TIE_SHAPE, "all", tie)
    _head(gpu, *R.TIE_SHAPE, "tanh", tie)


# ---- BatchNorm --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,c,g,res,relu,running,want_dx,want_masked", R.BN_ROWS)
def test_batchnorm(gpu, m, c, g, res, relu, running, want_dx, want_masked):
    k = R.bn_case(m, c)
    ref = R.bn_ref(m, c, res, relu)
    x, gamma, beta, dy = (_f(k[n], gpu) for n in ("x", "gamma", "beta", "dy"))
    stats = []
    for _ in range(2):
        rm, rv = (_f(k["rm"], gpu), _f(k["rv"], gpu)) if running else (None, None)
        stats.append(K.bn_stats(x, R.BN_EPS, R.BN_MOMENTUM, rm, rv) + ((rm, rv) if running else ()))
    assert all(torch.equal(p, q) for p, q in zip(*stats))
    mean, invstd = stats[0][:2]
    tag = f"bn M={m} C={c}"
    _close(f"{tag} mean", mean, ref["mean"], *R.TOL["bn_stats"])
    _close(f"{tag} invstd", invstd, ref["invstd"], *R.TOL["bn_stats"])
    if running:
        _close(f"{tag} running_mean", stats[0][2], ref["running_mean"], *R.TOL["bn_stats"])
        _close(f"{tag} running_var", stats[0][3], ref["running_var"], *R.TOL["bn_stats"])
    y = K.bn_apply(x, mean, invstd, gamma, beta, _f(k["res"], gpu) if res else None, relu)
    _close(f"{tag} y", y, ref["y"], *R.TOL["bn_apply"])
    # the ReLU mask is the reference output's (same signs in float32): masked dy and d_beta are exact
    relu_out = _f(ref["y"], gpu) if relu else None
    outs = [K.bn_backward(x, dy, mean, invstd, gamma, relu_out=relu_out, want_dx=want_dx, want_masked=want_masked)
            for _ in range(2)]
    for p, q in zip(*outs):
        assert (p is None and q is None) or torch.equal(p, q)
    dx, dm, dg, db = outs[0]
    assert (dx is not None) == want_dx and (dm is not None) == want_masked
    assert _same(db, ref["d_beta"])
    if want_masked:
        assert _same(dm, ref["masked"])
    _close(f"{tag} d_gamma", dg, ref["d_gamma"], R.TOL["colsum_rtol"], R.colsum_atol(m))
    if want_dx:
        _close(f"{tag} dx", dx, ref["dx"], R.TOL["bn_dx"][0], R.TOL["bn_dx"][1] * float(ref["dx"].abs().max()))


def test_batchnorm_large_mean(gpu):
    """x = 1000 + randn: the variance must come from centred sums (Welford / Chan), not E[x^2] - E[x]^2."""
    m, c, _ = R.BN_LARGE_MEAN
    k = R.bn_case(m, c, True)
    ref = R.bn_ref(m, c, False, False, large_mean=True)
    rm, rv = _f(k["rm"], gpu), _f(k["rv"], gpu)
    mean, invstd = K.bn_stats(_f(k["x"], gpu), R.BN_EPS, R.BN_MOMENTUM, rm, rv)
    rel = lambda got, want: float(((got.cpu().double() - want) / want).abs().max())          # noqa: E731
    print(f"  large mean: invstd rel. error {rel(invstd, ref['invstd']):.2e}, running_var {rel(rv, ref['running_var']):.2e},"
          f" mean abs. error {float((mean.cpu().double() - ref['mean']).abs().max()):.2e}")
    torch.testing.assert_close(invstd.cpu().double(), ref["invstd"], rtol=R.TOL["large_mean"], atol=0)
    torch.testing.assert_close(rv.cpu().double(), ref["running_var"], rtol=R.TOL["large_mean"], atol=0)
    # the mean as on every other row (a running float32 mean near 1000 rounds to 6e-5 at each of its steps, so no
    # bound of an ulp or two can be asked of it)
    torch.testing.assert_close(mean.cpu().double(), ref["mean"], rtol=R.TOL["bn_stats"][0], atol=R.TOL["bn_stats"][1])


def test_batchnorm_rejections(gpu):
    for shape in ((8, 24), (1, 16)):                       # 6 channel quads do not divide the workgroup; one row
        with pytest.raises(RuntimeError):
            K.bn_stats(torch.ones(*shape, device=gpu), R.BN_EPS, R.BN_MOMENTUM)
    torch.cuda.synchronize()
    mean, invstd = K.bn_stats(torch.ones(8, 16, device=gpu), R.BN_EPS, R.BN_MOMENTUM)
    assert torch.equal(mean.cpu(), torch.ones(16))


# ---- the rest ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,oh,ow,c,h,w,s,acc", R.SCATTER_ROWS)
def test_stride_scatter(gpu, b, oh, ow, c, h, w, s, acc):
    ref = R.scatter_ref(b, oh, ow, c, h, w, s, acc)
    fr = R.Framed((b, h, w, c), gpu, base=ref["base"] if acc else None)
    K.stride_scatter(_f(ref["x"], gpu), h, w, s, out=fr.view, accumulate=acc)
    assert _same(fr.view, ref["out"]) and fr.intact()


def test_stride_scatter_rejects_a_lattice_outside_the_image(gpu):
    fr = R.Framed((1, 4, 7, 4), gpu)
    with pytest.raises(RuntimeError):
        K.stride_scatter(torch.ones(1, 3, 3, 4, device=gpu), 4, 7, 2, out=fr.view)     # (OH - 1) * 2 = 4 >= H
    torch.cuda.synchronize()
    assert fr.untouched()


def test_gelu_forward_second_sweep(gpu):
    x = R.randn((R.GELU_N,), 12, 3.0)
    got = K.gelu_fwd(_f(x, gpu))
    _close("gelu_fwd", got, R.gelu_ref(x), *R.TOL["gelu"])


@pytest.mark.parametrize("n", R.CLAMP_SIZES)
def test_clamp_min(gpu, n):
    base = R.ints((n,), -4, 4, 13 + n)
    for lo in (0.0, 1.0):
        fr = R.Framed((n,), gpu, base=base)
        assert K.clamp_min_(fr.view, lo) is fr.view
        assert _same(fr.view, base.clamp(min=lo)) and fr.intact()


def test_rejected_operands(gpu):
    """One wrong operand per check of the wrappers: each raises before anything is enqueued, and the stream
    stays usable."""
    for name, call in R.bad_calls(K, lambda *s: torch.zeros(*s, device=gpu)):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(RuntimeError):                                   # an operand on the host
        K.ln_backward(torch.zeros(6, 8, device=gpu), torch.zeros(6, 8, device=gpu), torch.zeros(8),
                      torch.zeros(8, device=gpu), torch.zeros(8, device=gpu))
    torch.cuda.synchronize()
    a = torch.ones(5, 8, device=gpu)
    assert _same(K.colsum(a), torch.full((8,), 5.0, dtype=torch.float64))
