"""The inference-head kernels of csrc/head.hip called directly, at every width and edge their
launchers and loops branch on, against the float64 references of tests/head_ref.py (pinned to the
module paths by tests/test_head_ref_cpu.py).  Instantiation -> the row that reaches it:

  softmax_pool_kernel<NJ, MODE, float>          test_softmax_pool_f32: every P row runs MODE 0 and 1
      NJ = 1   P = 1, 63, 64          NJ = 2   P = 65, 128         NJ = 4   P = 129, 256
      NJ = 8   P = 257, 512           NJ = 12  P = 513, 768        NJ = 16  P = 769, 1024
      NJ = 32  P = 1025, 2048         HW 1 / 31 / 32 / 33 / 65 in rotation: one wave busy, a short
      pixel block, a full one, a second and a third block of one pixel
  softmax_pool_kernel<NJ, MODE, __bf16>         test_softmax_pool_bf16, P = 20 (NJ 1) and 1004 (NJ 16): P % 8 != 0
  softmax_pool_bf16q_kernel<NV, MODE>           test_softmax_pool_bf16, both modes:
      NV = 1   P = 8, 504, 512        NV = 2   P = 520, 1024       NV = 4   P = 1032, 2048
  softmax_pool_kernel<NJ, 0, float, LIN>        test_fused_head f32: NJ 1 (P 64), 2 (100), 8 (512), 32 (1032)
  softmax_pool_kernel<2, 0, __bf16, LIN>        test_fused_head bf16, P = 100 (100 % 8 != 0)
  softmax_pool_bf16q_kernel<NV, 0, LIN>         test_fused_head bf16: NV 1 (P 64, 512), NV 4 (P 1032)
  nonneg_linear_wave<4, 4>, vector path         test_nonneg_linear: nk < NC at K = 1, 3, 5, 17, 33, 9; a partly
      empty class block at K = 3, 5, 17, 33, 9; D < 256 (lanes without a slice) at D = 4; slice counts 1, 3, 5
      (not multiples of the unroll) at D = 256, 768, 1280, a ragged last slice at D = 260, 1028; D = 6144 / K = 9
      (C5) and D = 2048 / K = 200
  nonneg_linear_wave<4, 4>, scalar path         test_nonneg_linear: D = 130 / K = 37 and D = 37 / K = 2 (D % 4 != 0)
  nonneg_linear_wave<4, 1> / <8, 1> (LDS row)   test_fused_head f32 / bf16 quads: K = 1, 5, 17, 9, all with nk < NC
  count_gumbel_kernel<NJ, false, true>          test_count_gumbel_injected_noise (and test_count_gumbel_ties)
  count_gumbel_kernel<NJ, false, false> (FAST)  test_count_gumbel_philox_noise
      NJ = 1   P = 4, 16              NJ = 2   P = 100, 128        NJ = 4   P = 132, 256 (test_count_gumbel_bucket_4)
      NJ = 8   P = 260, 512           NJ = 12  P = 768             NJ = 16  P = 1000      NJ = 32  P = 1028, 2048
      (the launcher buckets by ceil(P / 64), so P = 260 is bucket 8 with NJ4 = 2 and no row of the grid
      falls into bucket 4, P in 129..256: two rows are added for it, in both noise forms)
  count_finish_kernel, count_encode_kernel      test_count_finish / test_count_encode, past the 2048 x 256 thread cap

Tolerances.  proto rtol 1e-5 / atol 1e-7, pooled the same (max) or rtol 1e-5 / atol 1e-6 (sum): the
bounds of test_softmax_pool; torch float32 on the CPU stays below 0.06 of them on these rows, the
kernels below 0.03.
NonNegLinear: |out - ref| <= (D / 64 + 7) 2^-24 |x'| relu(w)^T + 2^-23 |ref|, the worst case of the
kernel's own summation (D / 64 serial fmas per lane, six butterfly adds, the bias add) -- derived,
not tuned.  The hard head is judged by candidates (head_ref.hard_head): a channel may win where its
z + tol reaches the top's z - tol; tests/test_head_ref_cpu.py asserts that this leaves one candidate
at >= 99 % of the grid's pixels.  Every comparison prints its worst error / tolerance ratio before
it asserts (pytest -s).

No NaN or +-inf logits are fed to the hard head: a lane whose first channel is -inf forms
-inf - (-inf) in the running-sum update of count_gumbel_kernel, and the add-on convolution cannot
produce one; the hot loop carries no guard for it."""
import functools

import pytest
import torch

import head_ref as R
from count_pipnet_amd import kernels as K

pytestmark = pytest.mark.gpu

PROTO_TOL = dict(rtol=1e-5, atol=1e-7)
POOLED_TOL = {0: dict(rtol=1e-5, atol=1e-7), 1: dict(rtol=1e-5, atol=1e-6)}


def _close(what, got, want, rtol, atol):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got - want).abs()
    ratio = float((err / (atol + rtol * want.abs())).max()) if err.numel() else 0.0
    print(f"{what}: max |err| {float(err.max()) if err.numel() else 0.0:.3e}, worst err / tolerance {ratio:.3f}")
    torch.testing.assert_close(got, want, rtol=rtol, atol=atol, msg=lambda m: f"{what}: {m}")


# ---- a / b. softmax + pool -------------------------------------------------------------------
POOL_HW = [1, 31, 32, 33, 65]
POOL_P = [1, 63, 64, 65, 128, 129, 256, 257, 512, 513, 768, 769, 1024, 1025, 2048]
POOL_ROWS = [(p, POOL_HW[i % 5]) for i, p in enumerate(POOL_P)]
BF16_HW = [1, 33, 65]
BF16_P = [8, 504, 512, 520, 1024, 1032, 2048, 20, 1004]
BF16_ROWS = [(p, BF16_HW[i % 3]) for i, p in enumerate(BF16_P)]


def _check_pool(fn, gpu, x, proto, pooled, mode):
    xd = x.to(gpu)
    pr, po = fn(xd, mode)
    assert pr.shape == x.shape and po.shape == pooled.shape and pr.dtype == po.dtype == torch.float32
    _close("proto", pr, proto, **PROTO_TOL)
    _close("pooled", po, pooled, **POOLED_TOL[mode])
    if mode == 1:
        _close("pooled vs the spatial sum of the returned proto", po, pr.double().sum(dim=(1, 2)), **POOLED_TOL[1])
    out = (torch.full_like(pr, 7.0), torch.full_like(po, 7.0))
    pr2, po2 = fn(xd, mode, out=out)
    assert pr2 is out[0] and po2 is out[1] and torch.equal(pr2, pr)
    if mode == 0:
        assert torch.equal(po2, po)                                       # zeroed per call, a max of the same bits
    else:                                                                 # (the order of the float atomics is free)
        _close("pooled, second call into buffers holding 7.0", po2, pooled, **POOLED_TOL[1])


@pytest.mark.parametrize("mode", [0, 1], ids=["max", "sum"])
@pytest.mark.parametrize("p,hw", POOL_ROWS)
def test_softmax_pool_f32(gpu, p, hw, mode):
    x, proto, pmax, psum = R.pool_case(2, hw, p)
    _check_pool(K.softmax_pool, gpu, x, proto, psum if mode else pmax, mode)


@pytest.mark.parametrize("mode", [0, 1], ids=["max", "sum"])
@pytest.mark.parametrize("p,hw", BF16_ROWS)
def test_softmax_pool_bf16(gpu, p, hw, mode):
    x, proto, pmax, psum = R.pool_case(2, hw, p, True)
    assert x.dtype == torch.bfloat16
    _check_pool(K.softmax_pool_bf16, gpu, x, proto, psum if mode else pmax, mode)


def test_softmax_pool_arguments(gpu):
    """A width without an instantiation and an unknown pool mode raise; an empty batch, whose tensors
    have null data pointers, is a no-op (the launchers used to reject the null pointers first)."""
    for fn, dt in ((K.softmax_pool, torch.float32), (K.softmax_pool_bf16, torch.bfloat16)):
        with pytest.raises(RuntimeError):
            fn(torch.zeros(1, 1, 2, 2049 if dt == torch.float32 else 2056, device=gpu, dtype=dt), 0)
        with pytest.raises(RuntimeError):
            fn(torch.zeros(1, 1, 2, 16, device=gpu, dtype=dt), 2)          # no such pool mode
        pr, po = fn(torch.zeros(0, 1, 5, 16, device=gpu, dtype=dt), 0)     # B = 0: nothing to launch
        assert pr.shape == (0, 1, 5, 16) and po.shape == (0, 16)
    torch.cuda.synchronize()
    _, po = K.softmax_pool(torch.zeros(1, 1, 3, 16, device=gpu), 1)        # the stream stays usable
    assert torch.equal(po.cpu(), torch.full((1, 16), 3.0 / 16))


# ---- c. NonNegLinear -------------------------------------------------------------------------
LINEAR_ROWS = [
    (1, 4, 1),             # one lane holds the one slice, K < 4
    (2, 768, 3),           # C2's width, 3 slices per lane, nk = 3 < NC
    (3, 256, 5),           # exactly one slice per lane; the second wave has nk = 1
    (2, 260, 17),          # a second slice in lane 0 only; two class blocks, the second with one class
    (2, 1028, 16),         # a full class block, a fifth slice in lane 0 only
    (2, 1280, 33),         # 5 slices (one past the unroll), three class blocks
    (2, 6144, 9),          # C5: 24 slices, K = 9
    (2, 130, 37),          # D % 4 != 0: the scalar path, lanes 0 and 1 hold a third element
    (3, 37, 2),            # scalar path with idle lanes, K < 4
    (2, 2048, 200),        # 8 slices, K = 200: thirteen class blocks, the last half empty
]


def _check_linear(what, out, want, abs_sum, d):
    """|out - want| <= (d / 64 + 7) 2^-24 abs_sum + 2^-23 |want| (module docstring)."""
    bound = (d / 64 + 7) * R.F32_EPS * abs_sum + 2 * R.F32_EPS * want.abs()
    err = (out.double().cpu() - want).abs()
    ratio = float(torch.where(bound > 0, err / bound.clamp_min(1e-300), (err > 0).double() * 1e9).max())
    print(f"{what}: max |err| {float(err.max()):.3e}, worst err / bound {ratio:.3f}")
    assert bool((err <= bound).all()), f"{what}: worst err / bound {ratio}"


@pytest.mark.parametrize("thresh", [None, R.THRESH], ids=["nothresh", "thresh"])
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("b,d,k", LINEAR_ROWS)
def test_nonneg_linear(gpu, b, d, k, with_bias, thresh):
    x, w, bias = R.linear_case(b, d, k)
    bias = bias if with_bias else None
    want_x, want, abs_sum = R.nonneg_linear(x, w, bias, thresh)
    xd, wd, bd = x.to(gpu), w.to(gpu), None if bias is None else bias.to(gpu)
    xo, out = K.nonneg_linear(xd, wd, bd, thresh)
    assert xo.shape == (b, d) and out.shape == (b, k)
    assert torch.equal(xo.cpu().double(), want_x)                          # bit for bit
    if thresh is not None:
        kept, cut = x == R.AT_THRESH, x == R.BELOW_THRESH
        assert bool(kept.any()) and bool(cut.any())
        assert bool((xo.cpu()[kept] == R.AT_THRESH).all()) and bool((xo.cpu()[cut] == 0).all())
    _check_linear("out", out, want, abs_sum, d)
    for row in range(b):                                                   # batch-invariant: a row alone, same bits
        xo1, out1 = K.nonneg_linear(xd[row:row + 1].clone(), wd, bd, thresh)
        assert torch.equal(out1[0], out[row]) and torch.equal(xo1[0], xo[row])


# ---- d. hard Gumbel head ---------------------------------------------------------------------
def _check_hard(proto, hist, j):
    """proto [B, hw, 1, P], hist [B, P] of the device against a judged case (head_ref.judge):
    -> (device argmax [B, hw, 1], #single-candidate pixels, #pixels)."""
    proto, hist = proto.cpu(), hist.cpu()
    b, _, _, p = proto.shape
    nz = proto != 0
    assert bool((nz.sum(-1) == 1).all()), "not exactly one non-zero per pixel"
    idx = nz.int().argmax(-1)
    val = torch.gather(proto, -1, idx[..., None])[..., 0].double()
    print(f"one-hot value: max |v - 1| {float((val - 1).abs().max()):.3e} (allowed {2.0 ** -23:.3e})")
    assert bool(((val - 1).abs() <= 2.0 ** -23).all())
    single = j["single"]
    assert torch.equal(idx[single], j["top"][single]), "argmax differs at a single-candidate pixel"
    assert bool(torch.gather(j["cand"], -1, idx[..., None]).all()), "a pixel picked a channel outside its candidates"

    def bincount(i):
        return torch.stack([torch.bincount(i[n].reshape(-1), minlength=p) for n in range(b)])
    assert hist.dtype == torch.int32 and torch.equal(hist.long(), bincount(idx))
    assert int((hist.long() - bincount(j["top"])).abs().sum()) <= 2 * int((~single).sum())
    print(f"single-candidate pixels {int(single.sum())} / {single.numel()}")
    return idx, int(single.sum()), single.numel()


@pytest.mark.parametrize("b,hw,p,tau", R.GUMBEL_GRID)
def test_count_gumbel_injected_noise(gpu, b, hw, p, tau):
    c = R.gumbel_case(b, hw, p, tau)
    xd, ed = c["x"].to(gpu), c["e"].to(gpu)
    proto, hist = K.count_gumbel(xd, tau, ed, seed=0)
    _check_hard(proto, hist, c)
    out = (torch.full_like(proto, 7.0), torch.full_like(hist, 7))          # reused buffers: hist is zeroed per call
    proto2, hist2 = K.count_gumbel(xd, tau, ed, seed=0, out=out)
    assert torch.equal(proto2, proto) and torch.equal(hist2, hist)


PHILOX_SEED, PHILOX_OFFSET = (1 << 40) + 12345, 123457


@functools.lru_cache(maxsize=None)
def _philox_case(b, hw, p, tau):
    """The grid row judged on the kernel's own log E: element i of the NHWC [B, HW, P] map draws
    word i % 4 of Philox block offset + i / 4, which philox_exp1(log_e=True) returns in the
    hardware-log form the FAST instantiation computes."""
    x = R.gumbel_logits(b, hw, p)
    log_e = K.philox_exp1(PHILOX_SEED, PHILOX_OFFSET, b * hw * p, "cuda", log_e=True).view(b, hw, 1, p)
    return x, R.judge(x, log_e.cpu().double(), tau)


@pytest.mark.parametrize("b,hw,p,tau", R.GUMBEL_GRID)
def test_count_gumbel_philox_noise(gpu, b, hw, p, tau):
    x, j = _philox_case(b, hw, p, tau)
    xd = x.to(gpu)
    proto, hist = K.count_gumbel(xd, tau, None, PHILOX_SEED, PHILOX_OFFSET)
    _, single, total = _check_hard(proto, hist, j)
    assert single >= 0.9 * total                                            # the draw is the device's: fail loudly
    if b > 1:                                                               # images [b0:] alone repeat their bits
        b0 = b - 1
        proto_b, hist_b = K.count_gumbel(xd[b0:], tau, None, PHILOX_SEED, PHILOX_OFFSET + b0 * hw * p // 4)
        assert torch.equal(proto_b, proto[b0:]) and torch.equal(hist_b, hist[b0:])
    if b * hw >= 16:                                                        # (2 pixels could agree by chance)
        proto_o, _ = K.count_gumbel(xd, tau, None, PHILOX_SEED, PHILOX_OFFSET + 1)
        assert not torch.equal(proto_o, proto)                              # the offset is not ignored


def test_count_gumbel_philox_grid_is_decisive(gpu):
    single = total = 0
    for row in R.GUMBEL_GRID:
        s = _philox_case(*row)[1]["single"]
        single, total = single + int(s.sum()), total + s.numel()
    print(f"single-candidate pixels over the grid: {single} / {total}")
    assert single >= 0.99 * total


@pytest.mark.parametrize("noise", ["injected", "philox"])
@pytest.mark.parametrize("b,hw,p,tau", R.GUMBEL_EXTRA)
def test_count_gumbel_bucket_4(gpu, b, hw, p, tau, noise):
    """ceil(P / 64) in 3..4 -> count_gumbel_kernel<4, ...> (NJ4 = 1), which no row of the grid reaches."""
    if noise == "injected":
        c = R.gumbel_case(b, hw, p, tau)
        proto, hist = K.count_gumbel(c["x"].to(gpu), tau, c["e"].to(gpu), seed=0)
        _, single, total = _check_hard(proto, hist, c)
    else:
        x, j = _philox_case(b, hw, p, tau)
        proto, hist = K.count_gumbel(x.to(gpu), tau, None, PHILOX_SEED, PHILOX_OFFSET)
        _, single, total = _check_hard(proto, hist, j)
    assert single >= 0.9 * total


@pytest.mark.parametrize("p,tau", R.TIE_ROWS)
def test_count_gumbel_ties(gpu, p, tau):
    """E = 1 (log E = 0 exactly) and integer logits: every z is exact, the maximum is planted at two or
    more channels of every pixel (head_ref.tie_case), and the lowest index must win -- the per-lane
    scan's strict > and the wave reduction's (om == m && oi < mi)."""
    x, first = R.tie_case(p, tau)
    b, hw = x.shape[:2]
    proto, hist = K.count_gumbel(x.to(gpu), tau, torch.ones(b, p, hw, 1, device=gpu), seed=0)
    proto, hist = proto.cpu(), hist.cpu()
    nz = proto != 0
    assert bool((nz.sum(-1) == 1).all())
    idx = nz.int().argmax(-1)
    wrong = idx != first
    assert not bool(wrong.any()), (idx[wrong][:8].tolist(), first[wrong][:8].tolist())
    want = torch.stack([torch.bincount(first[n].reshape(-1), minlength=p) for n in range(b)])
    assert torch.equal(hist.long(), want)


def test_count_gumbel_arguments(gpu):
    def z(*shape):
        return torch.zeros(*shape, device=gpu)

    for p, tau in ((30, 1.0), (2052, 1.0), (16, 0.0), (16, -1.0)):
        with pytest.raises(RuntimeError):
            K.count_gumbel(z(1, 2, 1, p), tau, None, seed=1)
    proto, hist = K.count_gumbel(z(0, 2, 1, 16), 1.0, None, seed=1)         # B = 0: a no-op
    assert proto.shape == (0, 2, 1, 16) and hist.shape == (0, 16)
    torch.cuda.synchronize()
    proto, hist = K.count_gumbel(z(1, 3, 1, 8), 1.0, torch.ones(1, 8, 3, 1, device=gpu), seed=1)
    assert torch.equal(hist.cpu(), torch.tensor([[3, 0, 0, 0, 0, 0, 0, 0]], dtype=torch.int32))   # all tied: channel 0


# ---- e. count_finish, count_encode -----------------------------------------------------------
FINISH_SHAPE = (300, 2048)        # 614,400 elements: past the 2048 x 256 = 524,288 threads of the capped grid


@pytest.mark.parametrize("max_count", [0, 3, 7])
@pytest.mark.parametrize("do_round", [True, False], ids=["round", "noround"])
@pytest.mark.parametrize("source", ["hist", "sums"])
def test_count_finish(gpu, source, do_round, max_count):
    if source == "hist":
        values = torch.randint(0, 12, FINISH_SHAPE, generator=torch.Generator().manual_seed(4), dtype=torch.int32)
        values[-1, -5:] = torch.tensor([0, 1, 7, 8, 11], dtype=torch.int32)           # the tail of the strided loop
        raw, clamped = K.count_finish(values.to(gpu), None, max_count, do_round)
    else:
        values = R.finish_values(*FINISH_SHAPE)
        raw, clamped = K.count_finish(None, values.to(gpu), max_count, do_round)
    want_raw, want = R.count_finish(values, max_count, do_round)
    assert torch.equal(raw.cpu(), values.float()) and torch.equal(raw.cpu().double(), want_raw)
    assert torch.equal(clamped.cpu().double(), want)


ENCODE_ROWS = [(3, 37, 1), (3, 37, 3), (3, 37, 5), (64, 2048, 5)]      # the last: 655,360 outputs, past the cap


@pytest.mark.parametrize("b,p,c", ENCODE_ROWS)
def test_count_encode(gpu, b, p, c):
    from count_pipnet_amd.count_pipnet_utils import create_modified_encoding
    x = R.encode_counts(c, b, p)
    xd = x.to(gpu)
    for do_round in (False, True):
        got = K.count_encode(xd, c, 0, do_round).cpu()
        assert got.shape == (b, p * c)
        assert torch.equal(got.double(), R.count_encode(x, c, 0, do_round))
        assert torch.equal(got, create_modified_encoding(x.round() if do_round else x, c).view(b, -1))
    w = torch.randn(c, generator=torch.Generator().manual_seed(c))
    got = K.count_encode(xd, c, 1, False, w.to(gpu)).cpu()
    assert torch.equal(got, R.count_encode(x, c, 1, False, w).float())       # one float32 product
    assert torch.equal(got, (x[..., None] * w).view(b, -1))


# ---- f. fused head ---------------------------------------------------------------------------
FUSED_ROWS = [(2, 1, 64, 1), (2, 32, 100, 5), (1, 33, 512, 17), (2, 65, 1032, 9)]      # (B, HW, P, K)


@pytest.mark.parametrize("thresh", [None, R.THRESH], ids=["nothresh", "thresh"])
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("b,hw,p,k", FUSED_ROWS)
def test_fused_head(gpu, b, hw, p, k, dtype, with_bias, thresh):
    """softmax_pool_linear against the float64 references (not only the two-kernel path): proto and
    pooled within the bounds of (a); x' and the logits judged on the device's own pooled row -- x'
    bit for bit, the logits within the bound of (c) at D = P."""
    x, proto, pmax, _ = R.pool_case(b, hw, p, dtype == "bf16")
    _, w, bias = R.linear_case(b, p, k)
    bias = bias if with_bias else None
    xd, wd, bd = x.to(gpu), w.to(gpu), None if bias is None else bias.to(gpu)
    pr, po, xo, out = K.softmax_pool_linear(xd, wd, bd, thresh)
    pr2, po2 = (K.softmax_pool_bf16 if dtype == "bf16" else K.softmax_pool)(xd, 0)
    xo2, out2 = K.nonneg_linear(po2, wd, bd, thresh)
    torch.cuda.synchronize()
    assert torch.equal(pr, pr2) and torch.equal(po, po2) and torch.equal(xo, xo2) and torch.equal(out, out2)
    _close("proto", pr, proto, **PROTO_TOL)
    _close("pooled", po, pmax, **POOLED_TOL[0])
    want_x, want, abs_sum = R.nonneg_linear(po.cpu(), w, bias, thresh)
    assert torch.equal(xo.cpu().double(), want_x)
    if thresh is not None:
        assert bool((want_x == 0).any())                                       # the threshold cuts
    _check_linear("logits", out, want, abs_sum, p)
    part, tickets = K._HEAD_WS[(xd.device.index, torch.cuda.current_stream(xd.device).cuda_stream)]
    assert int(tickets.abs().sum()) == 0 and float(part.abs().sum()) == 0.0      # reset by the launch
