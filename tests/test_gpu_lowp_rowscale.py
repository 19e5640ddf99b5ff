"""The CNBlock Linear2 under train-mode stochastic depth on the low-precision operands, through the C ABI:
K.linear_bf16_mix_rowscale (plain bf16 rows) and K.linear_s3_rowscale (split planes),

    y = R + row_scale[m // rows_per_scale] * (scale * (x W^T + bias)),   fp32 y and R, R may be y.

Held to an fp64 evaluation over the same bf16-valued (or split: hi.hi + lo.hi + hi.lo) operands at 2e-6 of
max |ref|, the fp32-output bar of tests/test_gpu_convnext_bf16.py and tests/test_gpu_split.py; a dropped sample's
rows are the residual's bits; in place and out of place give the same bits; a sample's rows do not depend on the
batch they are in.  The shapes are the smallest that can still go wrong: M = 189 = 3 samples x 63 rows, so every
64 / 128 / 256-row tile straddles samples and ends ragged; N = 200 / 520 ragged in every tile width; K = 96
zero-padded to 128 for the plain bf16 operand.
"""
import functools

import pytest
import torch

from count_pipnet_amd import kernels as K

pytestmark = pytest.mark.gpu

TILES = (0, 4, 5, 7)                     # every tile the entries accept (-1 = the automatic choice)
P_DROP = 0.1 * 5 / 17                    # block 5 of ConvNeXt-tiny
KEEP = 1.0 / (1.0 - P_DROP)
FORMATS = ("bf16", "s3")


def _split(x):
    hi = x.to(torch.bfloat16)
    return hi, (x - hi.float()).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _operands(fmt, m, cin, cout, seed):
    """Host operands of one product and the fp64 value of scale * (x W^T + bias) over what the kernel multiplies:
    (x as the entry takes it, fp32 weight [cout, cin], bias, scale, residual, that fp64 branch) -- computed once."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(m, cin, generator=g)
    w = torch.randn(cout, cin, generator=g) * cin ** -0.5
    bias = torch.randn(cout, generator=g) * 0.1
    scale = torch.rand(cout, generator=g) + 0.5
    r = torch.randn(m, cout, generator=g)
    if fmt == "bf16":
        xa = x.to(torch.bfloat16)
        prod = xa.double() @ w.to(torch.bfloat16).double().t()
    else:
        (xh, xl), (wh, wl) = _split(x), _split(w)
        xa = torch.cat([xh, xl], dim=-1).contiguous()
        prod = xh.double() @ wh.double().t() + xl.double() @ wh.double().t() + xh.double() @ wl.double().t()
    return xa, w, bias, scale, r, scale.double() * (prod + bias.double())


def _pack(fmt, w, gpu):
    w4 = w.to(gpu).view(w.shape[0], 1, 1, w.shape[1])
    return K.pack_conv_weight_bf16(w4) if fmt == "bf16" else K.split_planes_weight(w4)


def _launch(fmt, *args, **kw):
    return (K.linear_bf16_mix_rowscale if fmt == "bf16" else K.linear_s3_rowscale)(*args, **kw)


def _run(gpu, fmt, m, cin, cout, rs, rows_per_scale, tile, seed):
    """(in-place result, out-of-place result, residual, fp64 reference) of one launch pair."""
    xa, w, bias, scale, r, branch = _operands(fmt, m, cin, cout, seed)
    rs = torch.tensor(rs, dtype=torch.float32)
    ref = r.double() + rs.double().repeat_interleave(rows_per_scale)[:m, None] * branch
    wp, xd, bd, sd_, rsd = _pack(fmt, w, gpu), xa.to(gpu), bias.to(gpu), scale.to(gpu), rs.to(gpu)
    r_in = r.to(gpu)
    y = _launch(fmt, xd, wp, bd, sd_, r_in, rsd, rows_per_scale, tile=tile)
    assert y.data_ptr() == r_in.data_ptr()                     # in place on the residual stream
    r_keep, out = r.to(gpu), torch.full((m, cout), float("nan"), device=gpu)
    y2 = _launch(fmt, xd, wp, bd, sd_, r_keep, rsd, rows_per_scale, out=out, tile=tile)
    torch.cuda.synchronize()
    assert y2.data_ptr() == out.data_ptr() and torch.equal(r_keep.cpu(), r)     # the residual is only read
    return y.cpu(), y2.cpu(), r, ref


def _check(y, y2, r, ref, rs, rows_per_scale):
    assert y.dtype == torch.float32 and torch.equal(y, y2)     # in place == out of place, bit for bit
    err = (y.double() - ref).abs().max().item()
    assert err <= 2e-6 * ref.abs().max().item(), (err, ref.abs().max().item())
    for b, f in enumerate(rs):
        rows = slice(b * rows_per_scale, min((b + 1) * rows_per_scale, y.shape[0]))
        if f == 0.0:
            assert torch.equal(y[rows], r[rows]), f"dropped sample {b} moved"
        else:
            assert not torch.equal(y[rows], r[rows])


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("cin,cout", [(96, 200), (128, 520), (96, 520), (128, 200), (128, 256)])
@pytest.mark.parametrize("tile", TILES)
def test_rowscale_every_tile_ragged(gpu, tile, cin, cout, fmt):
    """N = 256 besides the issue's ragged widths: the only width here at which tile 4 runs its full-width form."""
    rs = (KEEP, 0.0, KEEP)
    _check(*_run(gpu, fmt, 189, cin, cout, rs, 63, tile, seed=cin + cout), rs, 63)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("rs", [(0.0, 0.0, 0.0), (KEEP, KEEP, KEEP)], ids=["all_dropped", "all_kept"])
def test_rowscale_all_dropped_and_all_kept(gpu, rs, fmt):
    y, y2, r, ref = _run(gpu, fmt, 189, 128, 200, rs, 63, 4, seed=328)
    _check(y, y2, r, ref, rs, 63)
    if rs[0] == 0.0:
        assert torch.equal(y, r)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("b,h,cin,cout", [(3, 9, 384, 96), (2, 11, 768, 192), (2, 13, 1536, 384), (1, 7, 3072, 768)])
def test_rowscale_automatic_tile_at_the_linear2_shapes(gpu, b, h, cin, cout, fmt):
    """The four Linear2 shapes of ConvNeXt-tiny, reduced: rows_per_scale = h^2, kept and dropped samples mixed
    (a batch of one has nothing to mix: kept)."""
    rs = ((KEEP, 0.0, KEEP), (KEEP, 0.0), (KEEP,))[3 - b]
    _check(*_run(gpu, fmt, b * h * h, cin, cout, rs, h * h, -1, seed=b * 1000 + h), rs, h * h)


@pytest.mark.parametrize("fmt", FORMATS)
def test_rowscale_batch_invariant(gpu, fmt):
    """Samples 2..4 of a 40 x 28^2 batch equal the 3-sample launch bit for bit (384 -> 96), each with its factor."""
    g = torch.Generator().manual_seed(9)
    hw, cin, cout = 28 * 28, 384, 96
    x = torch.randn(40 * hw, cin, generator=g)
    xa = x.to(torch.bfloat16) if fmt == "bf16" else torch.cat(_split(x), dim=-1).contiguous()
    xa = xa.to(gpu)
    wp = _pack(fmt, torch.randn(cout, cin, generator=g) * cin ** -0.5, gpu)
    bias, scale = torch.randn(cout, generator=g).to(gpu), (torch.rand(cout, generator=g) + 0.5).to(gpu)
    r = torch.randn(40 * hw, cout, generator=g).to(gpu)
    rs = torch.where(torch.rand(40, generator=g) < 0.3, 0.0, KEEP).float()
    rs[2:5] = torch.tensor([KEEP, 0.0, KEEP])
    rs = rs.to(gpu)
    full = _launch(fmt, xa, wp, bias, scale, r.clone(), rs, hw)
    part = _launch(fmt, xa[2 * hw:5 * hw].contiguous(), wp, bias, scale, r[2 * hw:5 * hw].clone(),
                   rs[2:5].contiguous(), hw)
    assert torch.equal(full[2 * hw:5 * hw], part)
    assert torch.equal(part[hw:2 * hw], r[3 * hw:4 * hw]) and not torch.equal(part[:hw], r[2 * hw:3 * hw])


@pytest.mark.parametrize("fmt", FORMATS)
def test_rowscale_operand_errors(gpu, fmt):
    m, cin, cout = 189, 128, 200
    xa, w, bias, scale, r, _ = _operands(fmt, m, cin, cout, 328)
    xd, wp, bd, sd_, rd = xa.to(gpu), _pack(fmt, w, gpu), bias.to(gpu), scale.to(gpu), r.to(gpu)
    rs = torch.tensor([KEEP, 0.0, KEEP], device=gpu)
    _launch(fmt, xd, wp, bd, sd_, rd, rs, 63)                                    # the well-formed call
    bad = [
        dict(row_scale=None), dict(row_scale=rs[:2].contiguous()),               # missing / short row_scale
        dict(rows_per_scale=0), dict(rows_per_scale=-63), dict(rows_per_scale=62),
        dict(row_scale=rs.cpu()), dict(x=xd.cpu()), dict(w=wp.cpu()), dict(r=rd.cpu()), dict(scale=sd_.cpu()),
        dict(bias=bd.cpu()), dict(scale=None), dict(r=None),                     # host tensors, missing operands
        dict(x=xd.float()), dict(row_scale=rs.double()), dict(r=rd[:-1].contiguous()),
        dict(w=wp[:, :-32].contiguous()),                                        # wrong packed K
        dict(out=torch.empty(m, cout - 8, device=gpu)),
    ] + [dict(tile=t) for t in (1, 2, 3, 6, 8, 9, 10, 11, 12)]                   # refused tiles, the persistent one too
    for kw in bad:
        a = dict(x=xd, w=wp, bias=bd, scale=sd_, r=rd, row_scale=rs, rows_per_scale=63, tile=-1, out=None)
        a.update(kw)
        with pytest.raises(RuntimeError):
            _launch(fmt, a["x"], a["w"], a["bias"], a["scale"], a["r"], a["row_scale"], a["rows_per_scale"],
                    out=a["out"], tile=a["tile"])
    torch.cuda.synchronize()
    odd = torch.zeros(4, 40 if fmt == "bf16" else 80, device=gpu, dtype=torch.bfloat16)   # Cin = 40: not % 32
    w40 = _pack(fmt, torch.zeros(64, 40), gpu)
    with pytest.raises(RuntimeError):
        _launch(fmt, odd, w40, None, torch.ones(64, device=gpu), torch.zeros(4, 64, device=gpu),
                torch.ones(1, device=gpu), 4)
