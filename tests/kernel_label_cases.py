"""The launches whose profiling labels tests/golden/kernel_labels.json pins (tests/test_kernel_labels.py).

A case is (family, args), args being what the library's label query of that family takes:
  gemm  (M, N, K, epilogue, aload, splits)                                   pipnet_linear_f32_label
  conv  (B, H, W, Cin, Cout, KH, KW, stride, pad, epilogue, tile)            pipnet_conv2d_nhwc_bf16_label
  s3    the same arguments, Cin the fp32 channels                           pipnet_conv2d_nhwc_s3_label
  dual  (M, Cin, N1, N2)                                                     pipnet_conv1x1_bf16_dual_label
  mlp   (M, C, hw)                                                           pipnet_cnblock_mlp_label
``explicit_cases`` are stored one by one; ``sweep_cases`` only as one sha256 per family (``sweep_digest``).
Nothing here calls the library: tests/golden/gen_kernel_labels.py and the test do.
"""
import hashlib
import itertools

import gemm_matrix_ref as R
from count_pipnet_amd import _lib
from test_capi_symbols import C3_LAYERS

IMAGES = (1, 16, 32, 64)
# ConvNeXt-tiny at 224 x 224: (channels, map side) per stage and (Cin, Cout, input side, stride) per 2x2 downsample
CONVNEXT = {
    26: ([(96, 56), (192, 28), (384, 27), (768, 26)], [(96, 192, 56, 2), (192, 384, 28, 1), (384, 768, 27, 1)]),
    13: ([(96, 56), (192, 28), (384, 14), (768, 13)], [(96, 192, 56, 2), (192, 384, 28, 2), (384, 768, 14, 1)]),
}
CAPI_GEMMS = [(200704, 384, 96, _lib.EPI_BIAS_GELU, 0), (200704, 96, 384, _lib.EPI_RESID, 0),
              (50176, 768, 192, _lib.EPI_BIAS_GELU, 0), (50176, 192, 768, _lib.EPI_RESID, 0),
              (46656, 1536, 384, _lib.EPI_BIAS_GELU, 0), (46656, 384, 1536, _lib.EPI_RESID, 0),
              (43264, 3072, 768, _lib.EPI_BIAS_GELU, 0), (43264, 768, 3072, _lib.EPI_RESID, 0),
              (50176, 192, 384, _lib.EPI_BIAS, 1), (46656, 384, 768, _lib.EPI_BIAS, 1),
              (43264, 768, 1536, _lib.EPI_BIAS, 1), (43264, 768, 768, _lib.EPI_NONE, 0),
              (1024, 16, 192, _lib.EPI_NONE, 0), (46656, 384, 1536, _lib.EPI_RESID_ROWSCALE, 0)]
CAPI_MLPS = [(200704, 96, 0), (20000, 96, 0), (9000, 96, 0), (4096, 96, 0), (50176, 192, 0), (16384, 192, 0),
             (5000, 192, 0), (1024, 192, 0), (16384, 192, 256), (65536, 96, 0), (25088, 192, 0)]
CAPI_S3 = [(96, _lib.EPI_F32_RESID), (384, _lib.EPI_S3_GELU), (192, _lib.EPI_F32_RESID)]     # (N, epilogue), Cin = 4 N
CONV_TILES = tuple(range(-1, 12))
S3_TILES = (-1, 0, 4, 5, 7)
S3_EPILOGUES = (_lib.EPI_S3_GELU, _lib.EPI_F32_BIAS, _lib.EPI_F32_RESID)
BF16_EPILOGUES = (_lib.EPI_NONE, _lib.EPI_BIAS, _lib.EPI_BIAS_RELU, _lib.EPI_BIAS_RESID_RELU)


def _out(h, k, s, p):
    return (h + 2 * p - k) // s + 1


def explicit_cases():
    c = []
    c += [("gemm", s + (1,)) for s in CAPI_GEMMS]
    # tests/gemm_matrix_ref.py: every row that names a variant, on the entry it goes through
    for m, n, k, _, _ in R.DENSE_ROWS:
        c += [("gemm", (m, n, k, e, 0, 1)) for e in (_lib.EPI_NONE, _lib.EPI_BIAS_GELU, _lib.EPI_RESID_ROWSCALE)]
    for m, n, k, _, _ in R.GELU_ROWS:
        c += [("gemm", (m, n, k, e, 0, 1)) for e in (_lib.EPI_BIAS_GELU, _lib.EPI_GELU_BWD)]
    c += [("gemm", (m, n, k, _lib.EPI_BIAS, 0, slabs)) for m, n, k, slabs in R.SPLITK_ROWS]     # both split-K labels
    c += [("gemm", (3, 8, 544, _lib.EPI_NONE, 0, 2)), ("gemm", (1, 4096, 16384, _lib.EPI_NONE, 0, 64))]
    for b, h, w, cin, cout, kh, kw, s, p, _, _ in R.CONV_ROWS:
        al = 0 if (kh, kw, s, p) == (1, 1, 1, 0) else 2
        c += [("gemm", (b * _out(h, kh, s, p) * _out(w, kw, s, p), cout, kh * kw * cin, R.EXACT_MODES[e][0], al, 1))
              for e in R.CONV_EPILOGUES]
    for b, h, w, cin, cout, s, _ in R.CONV2X2_ROWS:
        c += [("gemm", (b * _out(h, 2, s, 0) * _out(w, 2, s, 0), cout, 4 * cin, e, 1, 1))
              for e in (_lib.EPI_NONE, _lib.EPI_BIAS)]
    # the ConvNeXt-26 / 13 backbones at 1, 16, 32 and 64 images: fp32 and split-bf16 forms of every GEMM
    for (stages, downs), img in itertools.product(CONVNEXT.values(), IMAGES):
        for ch, side in stages:
            m = img * side * side
            c += [("gemm", (m, 4 * ch, ch, _lib.EPI_BIAS_GELU, 0, 1)), ("gemm", (m, ch, 4 * ch, _lib.EPI_RESID, 0, 1)),
                  ("s3", (img, side, side, ch, 4 * ch, 1, 1, 1, 0, _lib.EPI_S3_GELU, -1)),
                  ("s3", (img, side, side, 4 * ch, ch, 1, 1, 1, 0, _lib.EPI_F32_RESID, -1))]
            if ch in (96, 192):
                c += [("mlp", (m, ch, 0)), ("mlp", (m, ch, side * side))]
        for cin, cout, side, s in downs:
            o = _out(side, 2, s, 0)
            c += [("gemm", (img * o * o, cout, 4 * cin, _lib.EPI_BIAS, 1, 1)),
                  ("s3", (img, side, side, cin, cout, 2, 2, s, 0, _lib.EPI_F32_BIAS, -1))]
    c += [("s3", (64, 56, 56, 4 * n, n, 1, 1, 1, 0, e, -1)) for n, e in CAPI_S3]
    c += [("mlp", a) for a in CAPI_MLPS]
    c += [("dual", (64 * 56 * 56, 64, 256, 256)), ("dual", (1 * 28 * 28, 256, 512, 256)), ("dual", (7, 8, 256, 1024))]
    # the C3 ResNet-50 layers at 64 images and at one, and every tile a caller may request for them
    for _, h, cin, cout, k, s, p, e, _ in C3_LAYERS:
        c += [("conv", (b, h, h, cin, cout, k, k, s, p, e, -1)) for b in (64, 1)]
        c += [("conv", (1, h, h, cin, cout, k, k, s, p, e, t)) for t in CONV_TILES[1:]]
    for n, e in itertools.product((96, 192, 384, 768), S3_EPILOGUES):
        c += [("s3", (1, 28, 28, 4 * n, n, 1, 1, 1, 0, e, t)) for t in S3_TILES[1:]]
        c += [("s3", (1, 28, 28, n, 2 * n, 2, 2, 2, 0, e, t)) for t in S3_TILES[1:]]
    return list(dict.fromkeys(c))


GEMM_M = (1, 63, 64, 65, 200, 512, 513, 4096, 19199, 23328, 46656, 200704)
GEMM_N = (16, 96, 100, 128, 192, 384, 768, 1536, 3072)
GEMM_K = (32, 36, 64, 96, 192, 384, 768, 1536, 3072)


def sweep_cases(family):
    if family == "gemm":
        return [("gemm", a + (1,)) for a in itertools.product(GEMM_M, GEMM_N, GEMM_K, range(_lib.EPI_GELU_BWD + 1),
                                                              range(3))]
    if family == "conv":
        chans = [(64, 64), (128, 128), (64, 256), (256, 64), (256, 128), (256, 512), (512, 512), (128, 136),
                 (1024, 2048), (16, 64), (72, 200)]
        geo = [(1, 1, 0), (1, 2, 0), (3, 1, 1), (3, 2, 1), (7, 2, 3)]
        return [("conv", (b, h, h + dw, ci, co, k, k, s, p, e, t))
                for b, (h, dw), (ci, co), (k, s, p), e, t in itertools.product(
                    (1, 16, 64), ((7, 0), (14, 0), (28, 3), (32, 0), (56, 0), (63, 0), (64, 0)), chans, geo,
                    BF16_EPILOGUES, CONV_TILES)]
    if family == "s3":
        chans = [(96, 384), (384, 96), (192, 768), (768, 192), (384, 1536), (1536, 384), (768, 3072), (3072, 768),
                 (96, 192), (192, 384), (384, 768), (64, 256), (32, 200)]
        return [("s3", (b, h, h, ci, co, k, k, s, 0, e, t))
                for b, h, (ci, co), (k, s), e, t in itertools.product(
                    IMAGES, (13, 14, 26, 27, 28, 56), chans, ((1, 1), (2, 2), (2, 1)), S3_EPILOGUES, S3_TILES)]
    if family == "mlp":
        ms = (0, 1, 1024, 4095, 4096, 8191, 8192, 16383, 16384, 24575, 24576, 25088, 50176, 65535, 65536, 98303, 98304,
              200704)
        return [("mlp", a) for a in itertools.product(ms, (96, 192), (0, 169, 256, 257, 3136))]
    if family == "dual":
        return [("dual", a) for a in itertools.product((1, 784, 200704), (64, 256), (256, 512), (256, 1024))]
    raise ValueError(family)


FAMILIES = ("gemm", "conv", "s3", "dual", "mlp")


def sweep_digest(family, label_of):
    """sha256 over the sorted ``args -> label`` lines of the family's sweep; a launch the library refuses has
    the empty label.  ``label_of(family, args)`` returns the label or raises RuntimeError."""
    lines = []
    for fam, args in sweep_cases(family):
        try:
            label = label_of(fam, args)
        except RuntimeError:
            label = ""
        lines.append(f"{args} -> {label}\n")
    return hashlib.sha256("".join(sorted(lines)).encode()).hexdigest()
