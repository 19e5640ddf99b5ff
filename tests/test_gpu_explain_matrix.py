"""The location and streaming top-k kernels of csrc/explain.hip (the fourth, local_explain_kernel, has
tests/test_gpu_local_explain.py) at every width and edge their launchers and loops branch on, against
the float64 / exact references of tests/explain_ref.py (pinned by tests/test_explain_ref_cpu.py).
Instantiation -> the row that reaches it:

  pool_argmax_kernel<NJ, false> / <NJ, true>    test_pool_argmax: every row runs both WRITE forms, through
      K.softmax_pool_argmax and once more through pipnet_softmax_pool_argmax_f32 on framed buffers
      NJ = 1   P = 1 (1x1), 63 (1x9), 64 (9x1); test_pool_argmax_one_channel (P = 1, 5x7, two workgroups)
      NJ = 2   P = 65 (5x7), 128 (7x5)            NJ = 4   P = 129 (6x6), 256 (4x8)
      NJ = 8   P = 257 (8x4), 512 (13x13)         NJ = 12  P = 513 (3x11), 768 (11x3)
      NJ = 16  P = 769 (8x9), 1024 (2x17)         NJ = 32  P = 1025 (17x2), 2048 (7x7: 64 KiB of LDS)
      HW = 1 (one wave busy), H = 1, W = 1, H > W, 32 pixels (one full block), 33 (a second block of one
      pixel), 169 (six workgroups)
  argmax_unpack_kernel                          every row of test_pool_argmax
  map_argmax_kernel                             test_map_argmax / _nan / _framed: P = 1, 63, 64 (one channel
      block, partly and exactly full), 65, 128, 129 (2 and 3 blocks), 2048 (32 blocks, B = 3) on maps 1x1, 1x3,
      3x1 (waves without a pixel), 5x7, 7x5, 16x16, 2x9
  topk_update_kernel, state blocks              test_topk_update: P = 1 .. 2048, G = 1, 3, 5, k = 1 .. 32, five
      batchings of 70 images, i0 = 0, 2^31 - 3, 2^40; test_topk_update_one_call_of_300 (38 chunks, k = 32);
      test_topk_update_nothing_qualifies (the !changed return); test_topk_update_corrupt_fill (the clamps)
  topk_update_kernel, abstain blocks            test_abstain_counter: K = 1, 9, 64 (one trip of the column
      loop), 65, 200, 1000 (2, 4, 16 trips), B = 1, 7, 8, 9, 17 (1 .. 3 blocks of 8 rows)

Judging.  pooled against float64 within POOLED_TOL[0] of tests/test_gpu_head_matrix.py (rtol 1e-5 / atol
1e-7), the only inexact comparison; it prints its worst error / tolerance before it asserts (pytest -s).
A location is judged three ways: inside the float64 candidates (explain_ref.located_pool; tests/
test_explain_ref_cpu.py asserts that >= 99 % of the pairs of every row leave a single candidate), equal to
first_rank_loc of the kernel's own proto map (the tie rule on the kernel's bits), and exactly on the planted
ties.  Everything about map_argmax and topk_update is exact.  Caller-allocated outputs of the direct-entry
rows lie in frames of 0xA5 bytes as wide as the output itself (explain_ref.Framed), so a mis-indexed store
stays inside the allocation and is seen.

No NaN or +-inf logits are fed to pool_argmax: the add-on convolution cannot produce them, and a -inf
pixel maximum forms -inf - (-inf) in softmax_pixel.  No NaN scores are fed to topk_update: the reference's
own sort is undefined on them."""
import numpy as np
import pytest
import torch

import explain_ref as R
from count_pipnet_amd import _lib
from count_pipnet_amd import kernels as K
from test_gpu_head_matrix import POOLED_TOL

pytestmark = pytest.mark.gpu


def _share(what, got, want, rtol, atol):
    got, want = got.detach().double().cpu(), want.double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got - want).abs()
    ratio = float((err / (atol + rtol * want.abs())).max())
    print(f"{what}: max |err| {float(err.max()):.3e}, worst err / tolerance {ratio:.3f}")
    torch.testing.assert_close(got, want, rtol=rtol, atol=atol, msg=lambda m: f"{what}: {m}")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


# ---- (a) pool_argmax_kernel --------------------------------------------------------------------
def _pool_argmax_direct(xd, write, frames=None):
    """pipnet_softmax_pool_argmax_f32 on framed pooled / loc / proto and a workspace of exactly B * P
    int64 that holds 0xFF bytes on entry (a second call: whatever the first left)."""
    b, h, w, p = xd.shape
    if frames is None:
        frames = dict(pooled=R.Framed((b, p), torch.float32, xd.device, frame=max(64, b * p)),
                      loc=R.Framed((b, p), torch.int32, xd.device, frame=max(64, b * p)),
                      ws=R.Framed((b * p,), torch.int64, xd.device, frame=max(64, b * p)).fill_bytes(0xFF),
                      proto=R.Framed(xd.shape, torch.float32, xd.device, frame=max(64, xd.numel())) if write else None)
    proto = frames["proto"]
    _lib.call("pipnet_softmax_pool_argmax_f32", xd.data_ptr(), b, h, w, p, proto.view.data_ptr() if write else None,
              frames["pooled"].view.data_ptr(), frames["loc"].view.data_ptr(), frames["ws"].view.data_ptr(),
              K._stream(xd))
    torch.cuda.synchronize()
    return frames


@pytest.mark.parametrize("p,h,w", R.POOL_ROWS)
def test_pool_argmax(gpu, p, h, w):
    c = R.pool_case(p, h, w)
    xd = c["x"].to(gpu)
    b = xd.shape[0]
    proto0, pooled0 = K.softmax_pool(xd, 0)
    none, pooled1, loc1 = K.softmax_pool_argmax(xd)
    proto2, pooled2, loc2 = K.softmax_pool_argmax(xd, write_proto=True)
    torch.cuda.synchronize()
    # 1. the existing contract: the bits of softmax_pool, one location for both WRITE forms
    assert none is None and loc1.dtype == torch.int32 and loc1.shape == (b, p)
    assert torch.equal(pooled1, pooled0) and torch.equal(pooled2, pooled0) and torch.equal(proto2, proto0)
    assert torch.equal(loc1, loc2)
    loc = loc1.cpu().long()
    assert bool(((loc >= 0) & (loc < h * w)).all())
    # 2. float64: pooled within the head matrix's bound, the location among the candidates
    _share(f"pooled P={p} {h}x{w}", pooled1, c["pooled"], **POOLED_TOL[0])
    at = c["cand"].reshape(b, h * w, p).gather(1, loc[:, None, :])[:, 0]
    assert bool(at.all()), f"{int((~at).sum())} locations outside their candidates"
    # 3. the tie rule on the kernel's own bits
    own = R.first_rank_loc(proto2.cpu())
    assert torch.equal(loc, own), (loc[loc != own][:8].tolist(), own[loc != own][:8].tolist())
    assert torch.equal(pooled1.cpu(), proto2.cpu().amax(dim=(1, 2)))
    # 4. planted exact ties, the saturated and the dead channel
    for ch, (val, where) in c["planted"].items():
        assert bool((pooled1[:, ch] == val).all()), (ch, pooled1[:, ch].tolist())
        assert bool((loc[:, ch] == where).all()), (ch, loc[:, ch].tolist(), where)
    assert (h * w >= 4) == bool(c["planted"])
    # 5. the C entry on framed buffers, 6. and again into the same buffers
    for write in (False, True):
        fr = _pool_argmax_direct(xd, write)
        for again in (False, True):
            if again:
                fr = _pool_argmax_direct(xd, write, fr)
            assert torch.equal(fr["pooled"].view, pooled0) and torch.equal(fr["loc"].view, loc1)
            if write:
                assert torch.equal(fr["proto"].view, proto0)
            for name, f in fr.items():
                assert f is None or f.intact(), f"{name}: a store outside the buffer (write={write}, again={again})"
        key = fr["ws"].view.cpu()                              # every key was zeroed, then raised: none is 0xFF.. still
        assert torch.equal((key >> 32).int(), _bits(pooled0).cpu().view(-1))


def test_pool_argmax_one_channel(gpu):
    """P = 1 on a 5 x 7 map: every pixel of both workgroups is exactly 1.0, the first by rank is (0, 0)."""
    xd = R.ones_case().to(gpu)
    for write in (False, True):
        proto, pooled, loc = K.softmax_pool_argmax(xd, write_proto=write)
        assert bool((pooled == 1.0).all()) and bool((loc == 0).all())
        assert proto is None or bool((proto == 1.0).all())


def test_empty_batch_is_a_no_op(gpu):
    """B = 0: an empty torch tensor's data pointer is null, and the entry points used to test for null
    pointers before they returned for the empty batch."""
    x = torch.zeros(0, 5, 7, 16, device=gpu)
    proto, pooled, loc = K.softmax_pool_argmax(x, write_proto=True)
    assert proto.shape == (0, 5, 7, 16) and pooled.shape == (0, 16) and loc.shape == (0, 16)
    val, loc = K.map_argmax(x)
    assert val.shape == (0, 16) and loc.shape == (0, 16)
    with pytest.raises(RuntimeError):
        K.softmax_pool_argmax(torch.zeros(0, 5, 7, 2049, device=gpu))          # the width is still checked
    torch.cuda.synchronize()


# ---- (b) map_argmax_kernel ---------------------------------------------------------------------
def _check_map(m, val, loc, skip_nan=False):
    h, w = m.shape[1:3]
    want_val = R.max_skip_nan(m) if skip_nan else m.double().amax(dim=(1, 2))
    want_loc = R.first_rank_loc(m, skip_nan=skip_nan)
    assert val.dtype == torch.float32 and loc.dtype == torch.int32
    assert torch.equal(val.cpu().double(), want_val)                # a maximum: no arithmetic
    got = loc.cpu().long()
    assert torch.equal(got, want_loc), (got[got != want_loc][:8].tolist(), want_loc[got != want_loc][:8].tolist())
    if not skip_nan and not bool(torch.isnan(m).any()):
        h_ref, w_ref = R.two_step_loc(m.permute(0, 3, 1, 2))
        assert torch.equal(got, h_ref * w + w_ref)


@pytest.mark.parametrize("kind", R.MAP_KINDS)
@pytest.mark.parametrize("p,h,w", R.MAP_ROWS)
def test_map_argmax(gpu, p, h, w, kind):
    m = R.map_case(p, h, w, kind)
    val, loc = K.map_argmax(m.to(gpu))
    _check_map(m, val, loc)
    if kind == "sparse":
        assert val[0, 0] == 0 and loc[0, 0] == 0 and val[1, p - 1] == 1 and loc[1, p - 1] == h * w - 1
    if kind in ("constant", "neg_inf"):
        assert bool((loc == 0).all())


@pytest.mark.parametrize("p,h,w", [(65, 5, 7), (2048, 2, 9), (1, 1, 3)])
def test_map_argmax_nan(gpu, p, h, w):
    """What explain.hip documents: NaN entries never compare greater and are passed over -- the maximum of
    the other entries at its column-first location; an all-NaN map gives (-inf, 0)."""
    m = R.map_case(p, h, w, "nan")
    val, loc = K.map_argmax(m.to(gpu))
    _check_map(m, val, loc, skip_nan=True)
    assert val[0, 0] == -R.INF and loc[0, 0] == 0
    assert not bool(torch.isnan(val).any())


@pytest.mark.parametrize("p,h,w", [(129, 16, 16), (2048, 2, 9)])
def test_map_argmax_framed(gpu, p, h, w):
    m = R.map_case(p, h, w, "random")
    md = m.to(gpu)
    b = m.shape[0]
    fv = R.Framed((b, p), torch.float32, gpu, frame=b * p)
    fl = R.Framed((b, p), torch.int32, gpu, frame=b * p)
    _lib.call("pipnet_map_argmax_f32", md.data_ptr(), b, h, w, p, fv.view.data_ptr(), fl.view.data_ptr(), K._stream(md))
    torch.cuda.synchronize()
    _check_map(m, fv.view, fl.view)
    assert fv.intact() and fl.intact()


# ---- (c) topk_update_kernel --------------------------------------------------------------------
def _framed_state(n_groups, p, k, gpu, frame=None):
    """A K.TopkState whose tensors lie in sentinel frames (at least 64 elements = two lists of k <= 32 wide)."""
    st = K.TopkState(n_groups, p, k, gpu)
    frames = {}
    for name in ("score", "index", "loc", "fill", "abstained"):
        t = getattr(st, name)
        frames[name] = R.Framed(t.shape, t.dtype, gpu, frame=frame or 64, base=t)
        setattr(st, name, frames[name].view)
    return st, frames


def _feed(st, c, splits, i0, min_score, gpu, dev=None):
    score, loc, group = dev or (c["score"].to(gpu), c["loc"].to(gpu), None if c["group"] is None else c["group"].to(gpu))
    at = 0
    for nb in splits:
        sl = slice(at, at + nb)
        K.topk_update(st, score[sl], loc[sl], i0 + at, group=None if group is None else group[sl], min_score=min_score)
        at += nb
    assert at == score.shape[0]
    return score, loc, group


def _assert_state(st, c, frames, what):
    for gi, (s, i, l) in enumerate(c["expected"]):
        assert np.array_equal(st.score[gi].cpu().numpy(), s), (what, gi, "score")
        assert np.array_equal(st.index[gi].cpu().numpy(), i), (what, gi, "index")
        assert np.array_equal(st.loc[gi].cpu().numpy(), l), (what, gi, "loc")
    assert np.array_equal(st.fill.cpu().numpy(), c["fill"]), (what, "fill")
    for name, f in frames.items():
        assert f.intact(), (what, name)


@pytest.mark.parametrize("p,n_groups,k,kind,i0,min_score", R.TOPK_ROWS)
def test_topk_update(gpu, p, n_groups, k, kind, i0, min_score):
    """Whatever the batching, every list is the k best by (score descending, dataset index ascending)."""
    c = R.topk_case(p, n_groups, k, kind, i0, min_score)
    dev = None
    for name, splits in R.TOPK_SPLITS.items():
        st, frames = _framed_state(n_groups, p, k, gpu)
        dev = _feed(st, c, splits, i0, min_score, gpu, dev)
        _assert_state(st, c, frames, name)
        assert int(st.abstained) == 0


def test_topk_update_one_call_of_300(gpu):
    """One call of B = 300 at k = 32: 38 chunks of TOPK_CHUNK images, the in-batch markers -2 - b run to
    -301 and every one is replaced by its location at write-back."""
    p, k, i0 = 65, 32, 2 ** 31 - 3
    c = R.topk_case(p, 3, k, "levels", i0, None, n=300)
    st, frames = _framed_state(3, p, k, gpu)
    _feed(st, c, [300], i0, None, gpu)
    _assert_state(st, c, frames, "one call")
    assert bool((st.loc >= -1).all()) and bool((st.fill == k).any())
    st2, frames2 = _framed_state(3, p, k, gpu)
    _feed(st2, c, [150, 1, 149], i0, None, gpu)
    _assert_state(st2, c, frames2, "three calls")


@pytest.mark.parametrize("p,n_groups,k", [(65, 3, 10), (2048, 3, 32)])
def test_topk_update_nothing_qualifies(gpu, p, n_groups, k):
    """A call in which no image qualifies -- scores below min_score, ids without a list, scores that do not
    beat a full list's last entry -- leaves the state bit for bit as it was."""
    c = R.topk_case(p, n_groups, k, "levels", 0, R.MIN_AT)
    st, frames = _framed_state(n_groups, p, k, gpu)
    _feed(st, c, [R.TOPK_N], 0, R.MIN_AT, gpu)
    before = [_bits(getattr(st, f)).clone() for f in ("score", "index", "loc", "fill")]
    low = torch.full((9, p), 0.1, device=gpu)
    loc = torch.full((9, p), 5, device=gpu, dtype=torch.int32)
    K.topk_update(st, low, loc, 1000, group=torch.zeros(9, device=gpu, dtype=torch.int32), min_score=R.MIN_AT)
    K.topk_update(st, low + 5.0, loc, 1000, group=torch.tensor([-1, n_groups] * 4 + [-1], device=gpu, dtype=torch.int32))
    K.topk_update(st, torch.empty(0, p, device=gpu), loc[:0], 1000)                 # B = 0: an empty last batch
    for f, was in zip(("score", "index", "loc", "fill"), before):
        assert torch.equal(_bits(getattr(st, f)), was), f
    _assert_state(st, c, frames, "after the empty calls")


def test_topk_update_equal_to_the_last_entry_stays_out(gpu):
    """Full lists (k = 2 of 70 images), then for every prototype its own last score again, later in the
    dataset: an equal score does not beat the last entry, nothing changes."""
    p, k = 65, 2
    c = R.topk_case(p, 1, k, "levels", 0, None)
    st, frames = _framed_state(1, p, k, gpu)
    _feed(st, c, [R.TOPK_N], 0, None, gpu)
    assert bool((st.fill == k).all())
    before = [_bits(getattr(st, f)).clone() for f in ("score", "index", "loc", "fill")]
    again = st.score[0, :, -1].clone().expand(9, p).contiguous()
    K.topk_update(st, again, torch.full((9, p), 5, device=gpu, dtype=torch.int32), 1000)
    for f, was in zip(("score", "index", "loc", "fill"), before):
        assert torch.equal(_bits(getattr(st, f)), was), f
    _assert_state(st, c, frames, "after the equal scores")


def test_topk_update_corrupt_fill(gpu):
    """The documented clamps: a negative fill count is read as 0, one above k as k, a stored location
    below -1 as -1.  Every state tensor lies in a frame 64 >= 2 k slots wide, and an unclamped count of
    k + 1 or -1 would index one slot beyond / before a list of k: inside the allocation either way."""
    p, k, n1 = 65, 10, 40
    score, loc, _ = R.topk_inputs(R.TOPK_N, p, "continuous", 0)
    sd, ld = score.to(gpu), loc.to(gpu)
    st, frames = _framed_state(1, p, k, gpu)
    K.topk_update(st, sd[:n1], ld[:n1], 0)
    s_all, i_all, l_all = R.topk_expected(score.numpy(), loc.numpy(), k)
    s_new, i_new, l_new = R.topk_expected(score[n1:].numpy(), loc[n1:].numpy(), k, i0=n1)
    assert (i_new >= 0).all()                                   # 30 new images fill a list of 10: nothing stale shows
    changed = (i_all >= n1).any(axis=1)
    old_top = np.flatnonzero(changed & (i_all[:, 0] < n1) & (np.arange(p) >= 20) & (np.arange(p) < 50))
    assert len(old_top) >= 2
    lost, over = list(range(0, 10)), list(range(10, 20))
    st.fill[0, lost] = -1
    st.fill[0, over] = k + 1
    st.loc[0, old_top[0], 0] = -2                               # would pass for the marker of image 0 of the batch
    st.loc[0, old_top[1], 0] = -7
    K.topk_update(st, sd[n1:], ld[n1:], n1)
    torch.cuda.synchronize()
    for name, f in frames.items():
        assert f.intact(), name
    got_s, got_i, got_l = (t[0].cpu().numpy() for t in (st.score, st.index, st.loc))
    assert np.array_equal(got_s[lost], s_new[lost]) and np.array_equal(got_i[lost], i_new[lost])
    assert np.array_equal(got_l[lost], l_new[lost])             # as if the lists had been empty
    rest = np.arange(10, p)
    l_all[old_top[:2], 0] = -1
    assert np.array_equal(got_s[rest], s_all[rest]) and np.array_equal(got_i[rest], i_all[rest])
    assert np.array_equal(got_l[rest], l_all[rest])             # fill k + 1 as k; locations below -1 read back as -1
    assert bool((st.fill == k).all())


@pytest.mark.parametrize("k_logits", R.ABSTAIN_K)
def test_abstain_counter(gpu, k_logits):
    """The count is the reference's torch.amax(out, dim=1) == 0. per row: +0.0 and -0.0 abstain, the
    smallest subnormal, an all-negative row and a row holding a NaN beside zeros do not."""
    st, frames = _framed_state(1, 1, 1, gpu)
    total = 0
    for b, shift in list(zip(R.ABSTAIN_B, range(5))) + [(1, s) for s in range(1, 6)]:      # B = 1: every kind alone
        out = R.abstain_case(b, k_logits, shift)
        want = R.abstained(out)
        K.topk_update(st, torch.zeros(b, 1, device=gpu), torch.zeros(b, 1, device=gpu, dtype=torch.int32), 0,
                      out=out.to(gpu))
        got = int(st.abstained) - total
        kinds = [R.ABSTAIN_KINDS[(r + shift) % 6] for r in range(b)]
        assert got == int(want.sum()), (b, k_logits, kinds, got, want.tolist())
        total += got
    assert total > 0 and all(f.intact() for f in frames.values())
