"""The profiling labels are the library's own (pipnet_*_label: the selection that launches a kernel also
names it) and are, byte for byte, the ones recorded in tests/golden/kernel_labels.json from the commit
before the Python label functions were replaced by those queries."""
import json
import os
import re

import pytest

import kernel_label_cases as C
from count_pipnet_amd import _lib, build, kernels as K
from test_capi_symbols import _nm_demangled

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "kernel_labels.json")))


def label_of(family, args):
    """The label through the function the launch wrappers of count_pipnet_amd.kernels call."""
    if family == "gemm":
        return K.gemm_kernel_name(*args)
    if family in ("conv", "s3"):
        return K.bf16_conv_kernel_name(*args, s3=family == "s3")
    if family == "dual":
        return K.conv1x1_bf16_dual_kernel_name(*args)
    m, c, hw = args
    return K.cnblock_mlp_kernel_name(c, m, hw)


def label_or_none(family, args):
    try:
        return label_of(family, args)
    except RuntimeError:
        return None


def test_fixture_holds_the_cases():
    assert [(r["family"], tuple(r["args"])) for r in GOLDEN["rows"]] == C.explicit_cases()
    assert re.fullmatch(r"[0-9a-f]{40}", GOLDEN["parent"])
    assert set(GOLDEN["sweeps"]) == set(C.FAMILIES)


def test_explicit_rows_are_the_recorded_labels():
    build.build()
    bad = [(r, got) for r in GOLDEN["rows"] if (got := label_or_none(r["family"], tuple(r["args"]))) != r["label"]]
    assert not bad, bad[:5]


@pytest.mark.parametrize("family", C.FAMILIES)
def test_sweep_reproduces_the_recorded_digest(family):
    build.build()
    assert C.sweep_digest(family, label_of) == GOLDEN["sweeps"][family]


def test_every_label_is_a_symbol_of_the_library():
    """Explicit rows and sweeps: each distinct label is the demangled name of a kernel in the built library
    (the fused MLP kernel lives in an anonymous namespace, which the label has never carried)."""
    build.build()
    syms = set(re.findall(r"void ((?:pipnet_\w+::|\(anonymous namespace\)::)\w+<.*>)\(", _nm_demangled()))
    syms = {s.replace("(anonymous namespace)::", "") for s in syms}
    labels = set()
    for cases in [C.explicit_cases()] + [C.sweep_cases(f) for f in C.FAMILIES]:
        labels |= {label_or_none(f, a) for f, a in cases}
    labels.discard(None)
    assert len(labels) > 100 and labels <= syms, sorted(labels - syms)


def test_traffic_profile_keys_are_still_produced():
    """profiles/traffic_kernels.json is keyed on these labels: every templated pipnet_*:: key is the label of
    some recorded row (the fused stem's kernel is no template; its label is a literal of kernels.stem_pool_bf16)."""
    keys = json.load(open(os.path.join(os.path.dirname(HERE), "profiles", "traffic_kernels.json")))
    want = {k for k in keys if re.match(r"(pipnet_\w+::)?\w+<", k)}
    assert len(want) > 10 and want <= {r["label"] for r in GOLDEN["rows"]}


def test_refused_launches_have_no_label():
    build.build()
    with pytest.raises(RuntimeError):
        K.bf16_conv_kernel_name(64, 56, 56, 256, 512, 1, 1, 2, 0, _lib.EPI_BIAS, 8)       # no halo shape
    with pytest.raises(RuntimeError):
        K.bf16_conv_kernel_name(1, 28, 28, 256, 256, 3, 3, 1, 1, _lib.EPI_BIAS, 7)         # tile 7: split epilogues only
    with pytest.raises(RuntimeError):
        K.cnblock_mlp_kernel_name(384, 1024)
    buf = __import__("ctypes").create_string_buffer(8)                                      # too small a buffer
    assert _lib.load().pipnet_cnblock_mlp_label(1024, 96, 0, buf, 8) == -1


# One launch per select branch, at the smallest recorded shape that reaches it.
HOOKED_GEMMS = [(70, 37, 20), (129, 132, 48), (70, 128, 64), (65, 36, 64), (130, 388, 224), (19205, 384, 768),
                (3, 8, 544)]        # K-tail, BK16, 64-row, 64-row NPAD, 128-row, wide, split-K (2 slabs)
# one image of a C3 layer (H, Cin, Cout, k, stride, pad, epilogue, requested tile): tiles 0, 4, 5, 6, 8, 9, 11
HOOKED_CONVS = [(56, 64, 256, 1, 1, 0, _lib.EPI_BIAS, -1), (56, 64, 256, 1, 1, 0, _lib.EPI_BIAS, 4),
                (56, 256, 512, 1, 2, 0, _lib.EPI_BIAS, -1), (56, 64, 64, 1, 1, 0, _lib.EPI_BIAS_RELU, -1),
                (28, 256, 256, 3, 1, 1, _lib.EPI_BIAS_RELU, -1), (28, 512, 256, 1, 1, 0, _lib.EPI_BIAS_RELU, -1),
                (56, 64, 64, 3, 1, 1, _lib.EPI_BIAS_RELU, -1)]
HOOKED_S3 = [(96, 0), (384, 4), (96, 4), (768, 5), (192, 7)]       # (N, tile) of a 28 x 28 Linear2; (96, 4) is NPAD
HOOKED_MLPS = [(4096, 96, 0), (9000, 96, 0), (20000, 96, 0), (65536, 96, 0), (1024, 192, 0), (5000, 192, 0),
               (16384, 192, 0), (25088, 192, 0), (16384, 192, 256)]


@pytest.mark.gpu
def test_hooked_launches_carry_the_recorded_label_and_change_nothing(gpu):
    """With a launch hook set (bench.py's roofline pass) every MFMA launch hands the hook the recorded label of
    its shape, and computes bit for bit what the same call computes without a hook."""
    import torch
    recorded = {(r["family"], tuple(r["args"])): r["label"] for r in GOLDEN["rows"]}
    g = torch.Generator().manual_seed(7)
    rn = lambda *s: torch.randn(*s, generator=g).to(gpu)      # noqa: E731
    bf = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).to(gpu)      # noqa: E731
    calls = []          # (recorded case, launch)
    for m, n, k in HOOKED_GEMMS:
        a, w = rn(m, k), rn(n, k)
        calls.append((("gemm", (m, n, k, _lib.EPI_NONE, 0, K.splitk_factor(m, n, k))), lambda a=a, w=w: K.linear(a, w)))
    for h, cin, cout, k, s, pad, epi, tile in HOOKED_CONVS:
        x, b = bf(1, h, h, cin), rn(cout)
        wp = K.pack_conv_weight_bf16(rn(cout, k, k, cin) / (k * k * cin) ** 0.5)
        calls.append((("conv", (1, h, h, cin, cout, k, k, s, pad, epi, tile)),
                      lambda x=x, wp=wp, b=b, k=k, s=s, pad=pad, epi=epi, tile=tile:
                      K.conv2d_nhwc_bf16(x, wp, k, k, b, s, pad, epi, tile=tile)))
    x, b = bf(1, 28, 28, 256), rn(768)
    wp = torch.cat([K.pack_conv_weight_bf16(rn(512, 1, 1, 256) / 16), K.pack_conv_weight_bf16(rn(256, 1, 1, 256) / 16)])
    calls.append((("dual", (784, 256, 512, 256)), lambda x=x, wp=wp, b=b: torch.cat(
        [y.flatten() for y in K.conv1x1_bf16_dual(x, wp, b, 512, 256)])))
    for n, tile in HOOKED_S3:
        x2, b = K.split_planes(rn(1, 28, 28, 4 * n)), rn(n)
        wp = K.split_planes_weight(rn(n, 1, 1, 4 * n) / (4 * n) ** 0.5)
        calls.append((("s3", (1, 28, 28, 4 * n, n, 1, 1, 1, 0, _lib.EPI_F32_BIAS, tile)),
                      lambda x2=x2, wp=wp, b=b, n=n, tile=tile:
                      K.conv_s3(x2, wp, 1, 1, n, b, 1, 0, _lib.EPI_F32_BIAS, tile=tile)))
    for m, c, hw in HOOKED_MLPS:
        t, x0 = rn(m, c), rn(m, c)
        ws = [rn(4 * c, c) / c ** 0.5, rn(4 * c), rn(c, 4 * c) / (4 * c) ** 0.5, rn(c), rn(c)]
        calls.append((("mlp", (m, c, hw)), lambda t=t, x0=x0, ws=ws, hw=hw: K.cnblock_mlp(t, *ws, x0.clone(), hw=hw)))
    # every call reaches another instantiation; only the split-K main kernel is the 64-row tile's
    assert len({recorded[case] for case, _ in calls}) == len(calls) - 1
    plain = [launch() for _, launch in calls]
    seen = []
    K.set_launch_hook(lambda name, flops, fn: (seen.append(name), fn()))
    try:
        hooked = [launch() for _, launch in calls]
    finally:
        K.set_launch_hook(None)
    assert seen == [recorded[case] for case, _ in calls]
    for (case, _), y0, y1 in zip(calls, plain, hooked):
        assert torch.equal(y0, y1), case
