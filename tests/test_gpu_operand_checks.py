"""Every tensor operand of a wrapper is checked before the library sees its pointer: a float64, CPU,
one-element-short or strided stand-in for any operand raises RuntimeError, nothing is launched and the
caller's outputs stay bit for bit what they were.  No kernel ever runs on a bad argument here."""
import pytest
import torch

from count_pipnet_amd import _lib
from count_pipnet_amd import kernels as K

pytestmark = pytest.mark.gpu
SENTINEL = -7.25


def _z(gpu, *shape):
    return torch.full(shape, 0.5, device=gpu)


# name -> (wrapper, operands by keyword, other arguments, the operands the call writes); the smallest shapes the
# kernel tests use: one image, the narrowest supported channel count, a map of a few pixels
def _cases(gpu):
    z = lambda *s: _z(gpu, *s)  # noqa: E731
    bf = lambda *s: _z(gpu, *s).bfloat16()  # noqa: E731
    lowp = dict(bias=z(64), scale=z(64), r=z(1, 4, 4, 64), out=z(1, 4, 4, 64))      # 1 x 4 x 4 x 64 -> 64, 1x1
    lowp_rest = dict(kh=1, kw=1, stride=1, pad=0, epilogue=_lib.EPI_F32_RESID)
    return {
        "convnext_stem": (K.convnext_stem, dict(x_nchw=z(1, 3, 4, 8), w=z(96, 3, 4, 4), b=z(96), ln_w=z(96),
                                                ln_b=z(96)), {}, ()),
        "dwconv7_ln": (K.dwconv7_ln, dict(x_nhwc=z(1, 4, 5, 96), w_packed=z(49, 96), bias=z(96), ln_w=z(96),
                                          ln_b=z(96), out=z(1, 4, 5, 96)), {}, ("out",)),
        "dwconv7_ln_s3": (K.dwconv7_ln_s3, dict(x_nhwc=z(1, 4, 5, 96), w_packed=z(49, 96), bias=z(96), ln_w=z(96),
                                                ln_b=z(96)), {}, ()),
        "dwconv7_ln_bf16": (K.dwconv7_ln_bf16, dict(x_nhwc=z(1, 4, 5, 96), w_packed=z(49, 96), bias=z(96), ln_w=z(96),
                                                    ln_b=z(96)), {}, ()),
        "layernorm": (K.layernorm, dict(x=z(3, 96), w=z(96), b=z(96), out=z(3, 96)), {}, ("out",)),
        "layernorm_s3": (K.layernorm_s3, dict(x=z(3, 96), w=z(96), b=z(96)), {}, ()),
        "layernorm_bf16": (K.layernorm_bf16, dict(x=z(3, 96), w=z(96), b=z(96)), {}, ()),
        "conv_s3": (K.conv_s3, dict(x2=bf(1, 4, 4, 128), w_packed=K.split_planes_weight(z(64, 1, 1, 64)), **lowp),
                    dict(cout=64, **lowp_rest), ("out",)),
        "conv_bf16_mix": (K.conv_bf16_mix, dict(x=bf(1, 4, 4, 64), w_packed=K.pack_conv_weight_bf16(z(64, 1, 1, 64)),
                                                **lowp), lowp_rest, ("out",)),
        "conv2x2": (K.conv2x2, dict(x_nhwc=z(1, 4, 4, 96), w_packed=z(192, 2, 2, 96), bias=z(192)), dict(stride=2), ()),
        "conv2d_nhwc": (K.conv2d_nhwc, dict(x=z(1, 5, 5, 64), w_packed=z(64, 3, 3, 64), bias=z(64), r=z(1, 5, 5, 64)),
                        dict(stride=1, pad=1, epilogue=_lib.EPI_BIAS_RESID_RELU), ()),
        "wgrad": (K.wgrad, dict(a=z(5, 4), b=z(5, 8), out=z(4, 8)), {}, ("out",)),
        "ln_backward": (K.ln_backward, dict(z=z(7, 96), dt=z(7, 96), gamma=z(96), d_gamma=z(96), d_beta=z(96)), {},
                        ("d_gamma", "d_beta")),
    }


def _bad_variants(t):
    strided = torch.as_strided(torch.zeros(2 * t.numel(), device=t.device, dtype=t.dtype), t.shape,
                               [2 * s for s in t.stride()])             # t's dtype: only the layout is wrong
    return {"float64": t.double(), "cpu": t.cpu(), "one short": t.flatten()[:-1], "strided": strided.copy_(t)}


@pytest.mark.parametrize("name", ["convnext_stem", "dwconv7_ln", "dwconv7_ln_s3", "dwconv7_ln_bf16", "layernorm",
                                  "layernorm_s3", "layernorm_bf16", "conv_s3", "conv_bf16_mix", "conv2x2",
                                  "conv2d_nhwc", "wgrad", "ln_backward"])
def test_bad_operands_raise_before_any_launch(gpu, monkeypatch, name):
    fn, tensors, rest, written = _cases(gpu)[name]
    fn(**tensors, **rest)                                    # the valid call runs
    torch.cuda.synchronize()
    for w in written:
        tensors[w].fill_(SENTINEL)
    variants = {(what, kind): bad for what, t in tensors.items() for kind, bad in _bad_variants(t).items()}
    before = {key: bad.clone() for key, bad in variants.items()}

    def touched(*a, **k):
        raise AssertionError("a rejected call reached the library")
    monkeypatch.setattr(_lib, "call", touched)
    monkeypatch.setattr(_lib, "load", touched)
    for (what, kind), bad in variants.items():
        with pytest.raises(RuntimeError):
            fn(**{**tensors, what: bad}, **rest)
            pytest.fail(f"{name}: a {kind} {what} was accepted")
    torch.cuda.synchronize()
    for w in written:
        assert torch.equal(tensors[w], torch.full_like(tensors[w], SENTINEL)), f"{name}: {w} was written"
    for key, bad in variants.items():
        assert torch.equal(bad, before[key]), f"{name}: the rejected {key} was written"
