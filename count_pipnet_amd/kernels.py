"""Tensor-level wrappers over the C-ABI (one function per HIP entry point).

Every wrapper holds each tensor operand against ``_operand`` (dtype, device, size, layout) before its
pointer reaches the library, allocates its outputs on the input's device and enqueues on torch's
*current* HIP stream, so the calls compose with torch streams, events and graph capture.  Nothing
here computes on the host.
"""
from __future__ import annotations

import contextlib
import copy
import ctypes
import dataclasses
import functools
import numbers
import threading
from collections import namedtuple

from typing import Callable, Optional, Tuple

import os

import torch

from . import _lib

Tensor = torch.Tensor


# Optional instrumentation: hook(kernel_name, algorithmic_flops, launch_fn) wraps every MFMA
# GEMM launch (bench.py brackets them with HIP events on the launching stream).
_launch_hook = None


def set_launch_hook(hook) -> None:
    global _launch_hook
    _launch_hook = hook


def _launch(kname: str, flops: float, fn) -> None:
    if _launch_hook is None:
        fn()
    else:
        _launch_hook(kname, flops, fn)


@functools.lru_cache(maxsize=4096)
def gemm_variant(m: int, n: int, k: int, epilogue: int = _lib.EPI_NONE, aload: int = 0) -> int:
    """The fp32 GEMM variant the library launches for an m x n x k product (pipnet_linear_f32_plan:
    the library's own rule, csrc/gemm_f32.hip gemm_variant -- never mirrored here)."""
    v = _lib.load().pipnet_linear_f32_plan(m, n, k, epilogue, aload)
    if v < 0:
        raise RuntimeError(f"linear: no GEMM variant for {m} x {n} x {k} (epilogue {epilogue}, aload {aload})")
    return v


@functools.lru_cache(maxsize=4096)
def gemm_kernel_name(m: int, n: int, k: int, epilogue: int, aload: int, splits: int = 1) -> str:
    """The rocprof name of the GEMM instantiation the library launches (pipnet_linear_f32_label: dense,
    unit-stride, 16-B aligned torch operands); ``splits`` > 1: the split-K main kernel."""
    return _lib.label("pipnet_linear_f32_label", m, n, k, epilogue, aload, splits)


SPLITK_WG_PER_CU = int(os.environ.get("PIPNET_SPLITK_WG_PER_CU", "2"))   # env: A/B runs (tools)
SPLITK_MIN_K = int(os.environ.get("PIPNET_SPLITK_MIN_K", "256"))          # env: A/B runs (tools)
SPLITK_MAX_M = 512               # longer products never split K


def splitk_factor(m: int, n: int, k: int, cus: int = 256) -> int:
    """K slabs for short-M GEMMs, which stream their weights once (C5's Bilinear intermediate
    at M = batch: 48 tiles of 64 x 128 over 151 MB of W / V): enough workgroups for
    SPLITK_WG_PER_CU per CU -- about 100 KB of LDS-DMA in flight per CU, what HBM latency
    needs -- each slab >= 8 K-tiles of 32."""
    if n % 4 or k % 32 or m > SPLITK_MAX_M:     # backbone GEMMs (M = pixels) stay batch-invariant
        return 1
    tiles = -(-m // 64) * -(-n // 128)
    if tiles >= cus:
        return 1
    return max(1, min(-(-SPLITK_WG_PER_CU * cus // tiles), k // SPLITK_MIN_K, 64))


# On small feature maps (batch * pixels <= SPLITK_MAX_M) the split-K rule above does see the batch
# size, so a forward's last bits there depend on how many images share the call.  A caller whose
# results must not depend on its batching (topk.prototype_topk) plans each product for ONE image's
# rows: the slab count is then the one a single-image forward takes, and a row's arithmetic in the
# split-K kernels depends on (K, slabs) only -- every image gets its batch-1 bits at any batch size.
_PLAN = threading.local()


@contextlib.contextmanager
def per_image_gemm_plan(images: int):
    """Inside, ``linear`` plans split-K as for m / images rows (pixel GEMMs of an ``images``-image batch)."""
    prev = getattr(_PLAN, "images", 1)
    _PLAN.images = max(int(images), 1)
    try:
        yield
    finally:
        _PLAN.images = prev


def _plan_rows(m: int) -> int:
    images = getattr(_PLAN, "images", 1)
    return m // images if images > 1 and m % images == 0 else m


def _ptr(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _stream(t: Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def require_device(t: Tensor, what: str = "input") -> None:
    if not (t.is_cuda and t.dtype == torch.float32):
        raise RuntimeError(
            f"count_pipnet_amd: the HIP inference path needs a float32 ROCm device tensor for {what} "
            f"(got device={t.device}, dtype={t.dtype}); there is no CPU fallback. Move the model and "
            "inputs to a GPU, or run the autograd path (train mode / grad enabled).")


def _operand(fn: str, what: str, t: Optional[Tensor], dtype=torch.float32, shape=None, device=None,
             layout: Optional[str] = "contiguous", optional: bool = False) -> None:
    """The one operand test of this file.  The library only sees a pointer: a wrong dtype, device, size or
    stride would read or write the wrong memory silently, so every tensor handed to it is first held
    against what the entry point documents (include/pipnet_amd.h): a ``dtype`` ROCm tensor, on ``device``
    (the primary operand's; None for the primary itself), of ``shape`` (a tuple, or an int: that many
    elements, or None: any) and ``layout`` ("contiguous"; "rows": 2-D row-major with unit column stride;
    None: any).  Attribute comparisons only: no host sync, no copy."""
    if t is None:
        if optional:
            return
        raise RuntimeError(f"{fn}: {what} is missing")
    if not (t.is_cuda and t.dtype == dtype):           # the label is only built on the way to an error
        if dtype is not torch.float32:
            raise RuntimeError(f"count_pipnet_amd: {fn} {what} must be a {dtype} ROCm device tensor "
                               f"(got device={t.device}, dtype={t.dtype}); there is no CPU fallback")
        require_device(t, f"{fn} {what}")               # float32: the public check and its message
    ok = device is None or t.device == device
    if shape is not None:
        ok = ok and (t.numel() == shape if isinstance(shape, int) else t.shape == shape)
    if layout == "contiguous":
        ok = ok and t.is_contiguous()
    elif layout == "rows":
        ok = ok and t.dim() == 2 and (t.shape[1] <= 1 or t.stride(1) == 1) and \
            (t.shape[0] <= 1 or t.stride(0) >= t.shape[1])
    if not ok:
        size = f"{shape} elements" if isinstance(shape, int) else f"shape {'any' if shape is None else tuple(shape)}"
        kind = {"contiguous": "contiguous", "rows": "row-major (unit column stride)", None: "strided"}[layout]
        raise RuntimeError(f"{fn}: {what} must be a {kind} {dtype} tensor of {size} on {device or t.device} "
                           f"(got shape {tuple(t.shape)}, stride {t.stride()}, device {t.device})")


def _chk(t: Tensor, what: str, contiguous: bool = True) -> None:
    """A float32 primary operand (``what`` names the wrapper too)."""
    _operand("count_pipnet_amd", what, t, layout="contiguous" if contiguous else None)


_EPI_READS_R = (_lib.EPI_RESID, _lib.EPI_MUL, _lib.EPI_BIAS_RESID_RELU, _lib.EPI_RESID_ROWSCALE, _lib.EPI_GELU_BWD)


def _chk_gemm_operands(fn: str, a: Tensor, m: int, n: int, epilogue: int, bias: Optional[Tensor],
                       scale: Optional[Tensor], r: Optional[Tensor], out: Optional[Tensor]) -> None:
    """The epilogue operands of a GEMM: bias / scale [n], r / out (m, n) row-major views, on a's device."""
    _chk_vec(fn, a, n, bias=bias, scale=scale)
    _operand(fn, "r", r, shape=(m, n), device=a.device, layout="rows", optional=True)
    _operand(fn, "out", out, shape=(m, n), device=a.device, layout="rows", optional=True)
    if r is None and epilogue in _EPI_READS_R:
        raise RuntimeError(f"{fn}: epilogue {epilogue} reads r, which is missing")


def _chk_rows(fn: str, t: Tensor, what: str, ndim: int) -> None:
    """The primary operand of a training kernel: a contiguous float32 device tensor of ``ndim`` dimensions."""
    _operand(fn, what, t)
    if t.dim() != ndim:
        raise RuntimeError(f"{fn}: {what} must be a contiguous {ndim}-D tensor (got shape {tuple(t.shape)})")


def _chk_same(fn: str, ref: Tensor, **operands: Optional[Tensor]) -> None:
    """Optional operands the library indexes exactly as ``ref``: same shape, contiguous, same device."""
    for what, t in operands.items():
        _operand(fn, what, t, shape=ref.shape, device=ref.device, optional=True)


def _chk_vec(fn: str, ref: Tensor, n: int, **operands: Optional[Tensor]) -> None:
    """Optional per-channel operands: ``n`` contiguous floats on ``ref``'s device."""
    for what, t in operands.items():
        _operand(fn, what, t, shape=n, device=ref.device, optional=True)


def _chk_row_scale(fn: str, ref: Tensor, m: int, row_scale: Optional[Tensor], rows_per_scale: int) -> None:
    _operand(fn, "row_scale", row_scale, device=ref.device, optional=True)
    if row_scale is not None and (rows_per_scale <= 0 or row_scale.numel() * rows_per_scale < m):
        raise RuntimeError(f"{fn}: row_scale ({row_scale.numel()} floats, {rows_per_scale} rows each) does not cover "
                           f"{m} rows")


def linear(a: Tensor, w: Tensor, bias: Optional[Tensor] = None, epilogue: int = _lib.EPI_NONE,
           scale: Optional[Tensor] = None, r: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """out[M,N] = epi(a[M,K] @ w[N,K]^T).  a, r and out may be any 2-D row-major views with unit col stride."""
    _operand("linear", "input", a, layout="rows")
    m, k = a.shape
    if w.dim() != 2 or w.shape[1] != k:
        raise RuntimeError(f"linear: K mismatch {tuple(a.shape)} x {tuple(w.shape)}")
    _operand("linear", "weight", w, device=a.device)
    n = w.shape[0]
    _chk_gemm_operands("linear", a, m, n, epilogue, bias, scale, r, out)
    if out is None:
        out = torch.empty((m, n), device=a.device, dtype=torch.float32)
    ldr = r.stride(0) if r is not None else 0
    splits = splitk_factor(_plan_rows(m), n, k)
    if splits > 1:
        ws = torch.empty((splits, m, n), device=a.device, dtype=torch.float32)
        _launch(gemm_kernel_name(m, n, k, epilogue, 0, splits), 2.0 * m * n * k,
                lambda: _lib.call("pipnet_linear_splitk_f32", a.data_ptr(), a.stride(0), w.data_ptr(), _ptr(bias),
                                  _ptr(scale), _ptr(r), ldr, out.data_ptr(), out.stride(0), m, n, k, epilogue, splits,
                                  ws.data_ptr(), _stream(a)))
        return out
    _launch(gemm_kernel_name(m, n, k, epilogue, 0), 2.0 * m * n * k,
            lambda: _lib.call("pipnet_linear_f32", a.data_ptr(), a.stride(0), w.data_ptr(), _ptr(bias), _ptr(scale),
                              _ptr(r), ldr, out.data_ptr(), out.stride(0), m, n, k, epilogue, _stream(a)))
    return out


def linear_pair_mul(a: Tensor, w_pair: Tensor) -> Tensor:
    """(a @ w_pair[Nh:]^T) * (a @ w_pair[:Nh]^T) for a [M,K] and w_pair [2 Nh, K] (the stacked
    folded BilinearIntermediate weights) as ONE split-K GEMM + one reduction that takes the product
    (include/pipnet_amd.h pipnet_linear_pair_mul_f32)."""
    _operand("linear_pair_mul", "input", a, layout="rows")
    m, k = a.shape
    _operand("linear_pair_mul", "paired weight", w_pair, device=a.device)
    n2 = w_pair.shape[0]
    if w_pair.dim() != 2 or w_pair.shape[1] != k or n2 % 2:
        raise RuntimeError(f"linear_pair_mul: shapes {tuple(a.shape)} x {tuple(w_pair.shape)}")
    nh = n2 // 2
    splits = max(1, splitk_factor(m, n2, k))
    out = torch.empty((m, nh), device=a.device, dtype=torch.float32)
    ws = torch.empty((splits, m, n2), device=a.device, dtype=torch.float32)
    _launch(gemm_kernel_name(m, n2, k, _lib.EPI_NONE, 0, 2), 2.0 * m * n2 * k,      # always the split-K main kernel
            lambda: _lib.call("pipnet_linear_pair_mul_f32", a.data_ptr(), a.stride(0), w_pair.data_ptr(),
                              out.data_ptr(), out.stride(0), m, nh, k, splits, ws.data_ptr(), _stream(a)))
    return out


def matmul_f64acc(a: Tensor, b: Tensor) -> Tensor:
    """[M,K] @ [K,N] (row-major fp32) with fp64 products and sums, rounded once to fp32
    (include/pipnet_amd.h pipnet_matmul_f64acc_f32): the inference-time weight folds."""
    _operand("matmul_f64acc", "A", a)
    _operand("matmul_f64acc", "B", b, device=a.device)
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[0]:
        raise RuntimeError(f"matmul_f64acc: shapes {tuple(a.shape)} x {tuple(b.shape)}")
    m, k = a.shape
    n = b.shape[1]
    out = torch.empty((m, n), device=a.device, dtype=torch.float32)
    _lib.call("pipnet_matmul_f64acc_f32", a.data_ptr(), k, b.data_ptr(), n, out.data_ptr(), n, m, n, k, _stream(a))
    return out


def matmul2_f64acc(a0: Tensor, a1: Tensor, b: Tensor) -> Tensor:
    """torch.stack((a0 @ b, a1 @ b)) ([2, M, N]) as ``matmul_f64acc`` in ONE launch
    (pipnet_matmul2_f64acc_f32): the bilinear fold's W.E and V.E share the embedding operand."""
    _operand("matmul2_f64acc", "A0", a0)
    _operand("matmul2_f64acc", "A1", a1, shape=a0.shape, device=a0.device)
    _operand("matmul2_f64acc", "B", b, device=a0.device)
    if a0.dim() != 2 or b.dim() != 2 or a0.shape[1] != b.shape[0]:
        raise RuntimeError(f"matmul2_f64acc: shapes {tuple(a0.shape)}, {tuple(a1.shape)} x {tuple(b.shape)}")
    m, k = a0.shape
    n = b.shape[1]
    out = torch.empty((2, m, n), device=a0.device, dtype=torch.float32)
    _lib.call("pipnet_matmul2_f64acc_f32", a0.data_ptr(), a1.data_ptr(), k, b.data_ptr(), n, out[0].data_ptr(),
              out[1].data_ptr(), n, m, n, k, _stream(a0))
    return out


def linear_rowscale(a: Tensor, w: Tensor, bias: Optional[Tensor], scale: Tensor, r: Tensor, row_scale: Tensor,
                    rows_per_scale: int) -> Tensor:
    """In place on ``r`` ([M,N]): r = r + row_scale[m // rows_per_scale] * (scale * (a w^T + bias))
    (CNBlock Linear2 under train-mode stochastic depth)."""
    _operand("linear_rowscale", "input", a, layout="rows")
    m, k = a.shape
    if w.dim() != 2 or w.shape[1] != k:
        raise RuntimeError(f"linear_rowscale: K mismatch {tuple(a.shape)} x {tuple(w.shape)}")
    _operand("linear_rowscale", "weight", w, device=a.device)
    n = w.shape[0]
    _chk_gemm_operands("linear_rowscale", a, m, n, _lib.EPI_RESID_ROWSCALE, bias, scale, r, None)
    _chk_row_scale("linear_rowscale", a, m, row_scale, rows_per_scale)
    _launch(gemm_kernel_name(m, n, k, _lib.EPI_RESID_ROWSCALE, 0), 2.0 * m * n * k,
            lambda: _lib.call("pipnet_linear_rowscale_f32", a.data_ptr(), a.stride(0), w.data_ptr(), _ptr(bias),
                              _ptr(scale), r.data_ptr(), r.stride(0), r.data_ptr(), r.stride(0), m, n, k,
                              row_scale.data_ptr(), rows_per_scale, _stream(a)))
    return r


def conv2x2(x_nhwc: Tensor, w_packed: Tensor, bias: Optional[Tensor], stride: int) -> Tensor:
    _chk_rows("conv2x2", x_nhwc, "input", 4)
    b, h, w, cin = x_nhwc.shape
    cout = w_packed.shape[0]
    _operand("conv2x2", "w_packed", w_packed, shape=cout * 4 * cin, device=x_nhwc.device)
    _operand("conv2x2", "bias", bias, shape=cout, device=x_nhwc.device, optional=True)
    oh, ow = (h - 2) // stride + 1, (w - 2) // stride + 1
    y = torch.empty((b, oh, ow, cout), device=x_nhwc.device, dtype=torch.float32)
    epi = _lib.EPI_BIAS if bias is not None else _lib.EPI_NONE
    _launch(gemm_kernel_name(b * oh * ow, cout, 4 * cin, epi, 1), 2.0 * b * oh * ow * cout * 4 * cin,
            lambda: _lib.call("pipnet_conv2x2_f32", x_nhwc.data_ptr(), b, h, w, cin, w_packed.data_ptr(), _ptr(bias),
                              cout, stride, y.data_ptr(), _stream(x_nhwc)))
    return y


def conv2d_nhwc(x: Tensor, w_packed: Tensor, bias: Optional[Tensor], stride: int, pad: int,
                epilogue: int = _lib.EPI_BIAS, r: Optional[Tensor] = None) -> Tensor:
    """NHWC implicit-GEMM convolution; w_packed [Cout, KH, KW, Cin]; r = residual (NHWC)."""
    _chk_rows("conv2d_nhwc", x, "input", 4)
    _operand("conv2d_nhwc", "weight", w_packed, device=x.device)
    b, h, w, cin = x.shape
    if w_packed.dim() != 4 or w_packed.shape[3] != cin:
        raise RuntimeError(f"conv2d_nhwc: input has {cin} channels, weight shape {tuple(w_packed.shape)}")
    cout, kh, kw, _ = w_packed.shape
    oh, ow = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    _operand("conv2d_nhwc", "bias", bias, shape=cout, device=x.device, optional=True)
    _operand("conv2d_nhwc", "r", r, shape=(b, oh, ow, cout), device=x.device, optional=True)
    y = torch.empty((b, oh, ow, cout), device=x.device, dtype=torch.float32)
    m, k = b * oh * ow, kh * kw * cin
    aload = 0 if (kh == 1 and kw == 1 and stride == 1 and pad == 0) else 2
    _launch(gemm_kernel_name(m, cout, k, epilogue, aload), 2.0 * m * cout * k,
            lambda: _lib.call("pipnet_conv2d_nhwc_f32", x.data_ptr(), b, h, w, cin, w_packed.data_ptr(), _ptr(bias),
                              cout, kh, kw, stride, pad, _ptr(r), epilogue, y.data_ptr(), _stream(x)))
    return y


def maxpool2d_nhwc(x: Tensor, k: int, stride: int, pad: int) -> Tensor:
    _chk(x, "maxpool input")
    b, h, w, c = x.shape
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    y = torch.empty((b, oh, ow, c), device=x.device, dtype=torch.float32)
    _lib.call("pipnet_maxpool2d_nhwc_f32", x.data_ptr(), b, h, w, c, k, stride, pad, y.data_ptr(), _stream(x))
    return y


def nchw_to_nhwc(x: Tensor, cpad: int) -> Tensor:
    _chk(x, "network input (NCHW)")
    b, c, h, w = x.shape
    y = torch.empty((b, h, w, cpad), device=x.device, dtype=torch.float32)
    _lib.call("pipnet_nchw_to_nhwc_f32", x.data_ptr(), b, c, h, w, cpad, y.data_ptr(), _stream(x))
    return y


# ---- bf16 ResNet path (BASELINE C3) ---------------------------------------------------

BF16_KTILE = 64


def _chk_bf(t: Tensor, what: str) -> None:
    _operand("count_pipnet_amd", what, t, dtype=torch.bfloat16)


@functools.lru_cache(maxsize=4096)
def bf16_conv_plan(b: int, h: int, w: int, cin: int, cout: int, kh: int, kw: int, stride: int, pad: int,
                   epilogue: int, tile: int = -1) -> int:
    """The workgroup tile the library takes for this bf16 conv (pipnet_conv2d_nhwc_bf16_plan: the
    library's own rule, csrc/conv_bf16.hip plan_conv -- never mirrored here):
    9 = the persistent ping-pong tile (1x1 stride-1 convs with N % 256 == 0, plain epilogues),
    11 = 3x3 stride-1 pad-1 Cin = N = 64 (W <= 63) / 128 (W <= 31) convs on an LDS input halo,
    8 = the ping-pong tile with an LDS input halo (3x3 stride-1 pad-1, Cin % 64 == 0, W <= 31, N >= 256),
    5 = 256x256 ping-pong on 16x16x32 MFMAs, 6 = 256x64 (N <= 64), 0 = 64x128, 3 = 256x256,
    4 = 128x128.  ``tile`` >= 0 is validated instead of chosen."""
    v = _lib.load().pipnet_conv2d_nhwc_bf16_plan(b, h, w, cin, cout, kh, kw, stride, pad, epilogue, tile)
    if v < 0:
        raise RuntimeError(f"conv2d_nhwc_bf16: no tile {tile} for {b}x{h}x{w}x{cin} -> {cout} k{kh}x{kw} s{stride} "
                           f"p{pad} epilogue {epilogue}")
    return v


@functools.lru_cache(maxsize=4096)
def bf16_conv_kernel_name(b: int, h: int, w: int, cin: int, cout: int, kh: int, kw: int, stride: int, pad: int,
                          epilogue: int, tile: int = -1, s3: bool = False, mix: bool = False) -> str:
    """rocprof name of the instantiation conv2d_nhwc_bf16 (``s3``: conv_s3, ``cin`` its fp32 channels;
    ``mix``: conv_bf16_mix) launches for this conv and requested ``tile`` (pipnet_conv2d_nhwc_bf16_label /
    _s3_label / _bf16_mix_label); RuntimeError when the library has none, as the launch would answer."""
    if s3 and mix:
        raise ValueError("bf16_conv_kernel_name: s3 and mix name different entry points")
    args = (b, h, w, cin, cout, kh, kw, stride, pad, epilogue, tile)
    if s3 or mix:
        return _lowp_label(LOWP_FORMATS["bf16x3" if s3 else "bf16"].conv_label, *args)
    return _lib.label("pipnet_conv2d_nhwc_bf16_label", *args)


def pack_conv_weight_bf16(w_ohwi: Tensor) -> Tensor:
    """[Cout, KH, KW, Cin] (fp32) -> [Cout, Kp] bf16, Kp = KH*KW*Cin rounded up to 64 (zeros)."""
    cout = w_ohwi.shape[0]
    k = w_ohwi[0].numel()
    kp = -(-k // BF16_KTILE) * BF16_KTILE
    out = torch.zeros((cout, kp), device=w_ohwi.device, dtype=torch.bfloat16)
    out[:, :k] = w_ohwi.reshape(cout, k).to(torch.bfloat16)
    return out


# Tile 11 (3x3 Cin = N = 64 / 128 on the LDS input halo) for automatic launches; False = the generic
# tile (6 / 4 / 0: bitwise the same outputs) (in-process A/B: tools/ab_toggle.py count_pipnet_amd.kernels.CONV3X3_N64_HALO c3)
CONV3X3_N64_HALO = True


def conv2d_nhwc_bf16(x: Tensor, w_packed: Tensor, kh: int, kw: int, bias: Optional[Tensor], stride: int,
                     pad: int, epilogue: int = _lib.EPI_BIAS, r: Optional[Tensor] = None, tile: int = -1) -> Tensor:
    """NHWC bf16 implicit-GEMM convolution; w_packed from pack_conv_weight_bf16; bias fp32;
    tile -1 = automatic, 0 = 64x128 (32-deep K, 4 stages), 1/2 = 128x128 / 256x256 (64-deep K,
    2 stages), 3/4 = 256x256 / 128x128 (32-deep K, 4 stages), 5 = 256x256 ping-pong, 6 = 256x64,
    8 = ping-pong with the LDS input halo (3x3 stride-1 pad-1 only), 9 = persistent ping-pong
    (1x1 stride-1, N % 256 == 0), 11 = 3x3 stride-1 pad-1 N = 64 on an LDS input halo."""
    _chk_bf(x, "conv input")
    b, h, w, cin = x.shape
    dev, bf = x.device, torch.bfloat16
    _operand("conv2d_nhwc_bf16", "weight", w_packed, dtype=bf, device=dev)
    cout, kp = w_packed.shape
    k = kh * kw * cin
    if kp != -(-k // BF16_KTILE) * BF16_KTILE:
        raise RuntimeError(f"conv2d_nhwc_bf16: packed weight K {kp} does not match {kh}x{kw}x{cin}")
    oh, ow = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    _operand("conv2d_nhwc_bf16", "bias", bias, shape=cout, device=dev, optional=True)
    _operand("conv2d_nhwc_bf16", "residual", r, dtype=bf, shape=(b, oh, ow, cout), device=dev, optional=True)
    y = torch.empty((b, oh, ow, cout), device=x.device, dtype=torch.bfloat16)
    m = b * oh * ow
    if tile < 0 and not CONV3X3_N64_HALO and bf16_conv_plan(b, h, w, cin, cout, kh, kw, stride, pad, epilogue) == 11:
        tile = 6 if cout == 64 else 4       # the same arithmetic on the generic tile (A/B arm)
    _launch(bf16_conv_kernel_name(b, h, w, cin, cout, kh, kw, stride, pad, epilogue, tile),
            2.0 * m * cout * k,
            lambda: _lib.call("pipnet_conv2d_nhwc_bf16_tile", x.data_ptr(), b, h, w, cin, w_packed.data_ptr(),
                              _ptr(bias), cout, kh, kw, stride, pad, _ptr(r), epilogue, y.data_ptr(), tile,
                              _stream(x)))
    return y


def stem_pool_bf16(s2d: Tensor, w_packed: Tensor, bias: Tensor) -> Tensor:
    """ResNet stem over the space-to-depth image (4x4 stride 1, 16 -> 64, + bias + ReLU) fused
    with MaxPool2d(3, 2, 1) (pipnet_stem_pool_bf16): bitwise conv2d_nhwc_bf16 + maxpool2d_nhwc_bf16."""
    _chk_bf(s2d, "stem s2d input")
    b, sh, sw, c = s2d.shape
    if c != 16:
        raise RuntimeError(f"stem_pool_bf16: expects a 16-channel s2d image, got {tuple(s2d.shape)}")
    _operand("stem_pool_bf16", "weight", w_packed, dtype=torch.bfloat16, shape=(64, 256), device=s2d.device)
    _operand("stem_pool_bf16", "bias", bias, shape=64, device=s2d.device)
    ph, pw = (sh - 4) // 2 + 1, (sw - 4) // 2 + 1
    y = torch.empty((b, ph, pw, 64), device=s2d.device, dtype=torch.bfloat16)
    _launch("pipnet_bf16::stem_pool_bf16_kernel", 2.0 * b * (sh - 3) * (sw - 3) * 64 * 256,
            lambda: _lib.call("pipnet_stem_pool_bf16", s2d.data_ptr(), b, sh, sw, w_packed.data_ptr(),
                              bias.data_ptr(), y.data_ptr(), _stream(s2d)))
    return y


def maxpool2d_nhwc_bf16(x: Tensor, k: int, stride: int, pad: int) -> Tensor:
    _chk_bf(x, "maxpool input")
    b, h, w, c = x.shape
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    y = torch.empty((b, oh, ow, c), device=x.device, dtype=torch.bfloat16)
    _lib.call("pipnet_maxpool2d_nhwc_bf16", x.data_ptr(), b, h, w, c, k, stride, pad, y.data_ptr(), _stream(x))
    return y


def nchw_to_nhwc_bf16(x: Tensor, cpad: int) -> Tensor:
    _chk(x, "network input (NCHW)")
    b, c, h, w = x.shape
    y = torch.empty((b, h, w, cpad), device=x.device, dtype=torch.bfloat16)
    _lib.call("pipnet_nchw_to_nhwc_bf16", x.data_ptr(), b, c, h, w, cpad, y.data_ptr(), _stream(x))
    return y


@functools.lru_cache(maxsize=256)
def conv1x1_bf16_dual_kernel_name(m: int, cin: int, n1: int, n2: int) -> str:
    """rocprof name of conv1x1_bf16_dual's kernel (pipnet_conv1x1_bf16_dual_label)."""
    return _lib.label("pipnet_conv1x1_bf16_dual_label", m, cin, n1, n2)


def conv1x1_bf16_dual(x: Tensor, w_packed: Tensor, bias: Tensor, n1: int, n2: int) -> Tuple[Tensor, Tensor]:
    """Two 1x1 stride-1 bf16 convs over one NHWC input in one launch (pipnet_conv1x1_bf16_dual):
    w_packed = the two packed weights stacked [n1 + n2, Kp], bias [n1 + n2] fp32 ->
    (x W1^T + b1, relu(x W2^T + b2)), each bit-equal to its own pipnet_conv2d_nhwc_bf16."""
    _chk_bf(x, "conv input")
    b, h, w, cin = x.shape
    if n1 % 256 or n2 % 256:
        raise RuntimeError(f"conv1x1_bf16_dual: n1 {n1}, n2 {n2} must be multiples of 256")
    kp = -(-cin // BF16_KTILE) * BF16_KTILE
    _operand("conv1x1_bf16_dual", "weight", w_packed, dtype=torch.bfloat16, shape=(n1 + n2, kp), device=x.device)
    _operand("conv1x1_bf16_dual", "bias", bias, shape=n1 + n2, device=x.device)
    y1 = torch.empty((b, h, w, n1), device=x.device, dtype=torch.bfloat16)
    y2 = torch.empty((b, h, w, n2), device=x.device, dtype=torch.bfloat16)
    m = b * h * w
    _launch(conv1x1_bf16_dual_kernel_name(m, cin, n1, n2), 2.0 * m * (n1 + n2) * cin,
            lambda: _lib.call("pipnet_conv1x1_bf16_dual", x.data_ptr(), m, cin, w_packed.data_ptr(), bias.data_ptr(),
                              n1, y1.data_ptr(), n2, y2.data_ptr(), _stream(x)))
    return y1, y2


def nchw_to_s2d_bf16(x: Tensor) -> Tensor:
    """[B,3,H,W] fp32 -> [B, (H-1)//2 + 4, (W-1)//2 + 4, 16] bf16 space-to-depth stem input
    (pipnet_nchw_to_s2d_bf16): the k7 s2 p3 ResNet stem becomes a 4x4 stride-1 conv over it."""
    _chk(x, "network input (NCHW)")
    b, c, h, w = x.shape
    if c != 3:
        raise RuntimeError(f"nchw_to_s2d_bf16: expects 3 channels, got {c}")
    y = torch.empty((b, (h - 1) // 2 + 4, (w - 1) // 2 + 4, 16), device=x.device, dtype=torch.bfloat16)
    _lib.call("pipnet_nchw_to_s2d_bf16", x.data_ptr(), b, h, w, y.data_ptr(), _stream(x))
    return y


def stem_weight_s2d(w_ohwi: Tensor) -> Tensor:
    """[Cout, 7, 7, 3] (fp32, BatchNorm folded) -> [Cout, 4, 4, 16]: the taps of the k7 s2 conv
    regrouped for the 4x4 conv over the space-to-depth image, W'[o][a][a'][(2 bi + bj) * 4 + c] =
    w[o][2a+bi-1][2a'+bj-1][c], zero for the tap index -1 and the c = 3 slot."""
    co = w_ohwi.shape[0]
    w8 = torch.nn.functional.pad(w_ohwi, (0, 1, 1, 0, 1, 0))            # [Cout, 8 (ky+1), 8 (kx+1), 4]
    return w8.view(co, 4, 2, 4, 2, 4).permute(0, 1, 3, 2, 4, 5).reshape(co, 4, 4, 16).contiguous()


def _head_out(out, b, h, w, p, dev):
    """Caller-provided (proto [B,h,w,P], pooled [B,P]) fp32 contiguous outputs, or new ones."""
    if out is None:
        return (torch.empty((b, h, w, p), device=dev, dtype=torch.float32),
                torch.empty((b, p), device=dev, dtype=torch.float32))
    proto, pooled = out
    _operand("softmax_pool", "proto out", proto, shape=(b, h, w, p), device=dev)
    _operand("softmax_pool", "pooled out", pooled, shape=(b, p), device=dev)
    return proto, pooled


def softmax_pool_bf16(feat_nhwc: Tensor, pool_mode: int, out=None) -> Tuple[Tensor, Tensor]:
    """bf16 logits [B,h,w,P] -> fp32 (proto [B,h,w,P], pooled [B,P])."""
    _chk_bf(feat_nhwc, "prototype logits")
    b, h, w, p = feat_nhwc.shape
    proto, pooled = _head_out(out, b, h, w, p, feat_nhwc.device)
    _lib.call("pipnet_softmax_pool_bf16", feat_nhwc.data_ptr(), b, h * w, p, pool_mode, proto.data_ptr(),
              pooled.data_ptr(), _stream(feat_nhwc))
    return proto, pooled


def convnext_stem(x_nchw: Tensor, w: Tensor, b: Tensor, ln_w: Tensor, ln_b: Tensor) -> Tensor:
    _chk_rows("convnext_stem", x_nchw, "network input (NCHW)", 4)
    n, c, h, wd = x_nchw.shape
    if c != 3:
        raise RuntimeError(f"convnext stem expects 3 input channels, got {c}")
    for t, what, numel in ((w, "w", 96 * 3 * 4 * 4), (b, "b", 96), (ln_w, "ln_w", 96), (ln_b, "ln_b", 96)):
        _operand("convnext_stem", what, t, shape=numel, device=x_nchw.device)
    y = torch.empty((n, h // 4, wd // 4, 96), device=x_nchw.device, dtype=torch.float32)
    _lib.call("pipnet_convnext_stem_f32", x_nchw.data_ptr(), n, h, wd, w.data_ptr(), b.data_ptr(), ln_w.data_ptr(),
              ln_b.data_ptr(), y.data_ptr(), _stream(x_nchw))
    return y


MLP_FUSED_CHANNELS = (96, 192)


@functools.lru_cache(maxsize=1024)
def cnblock_mlp_kernel_name(c: int, m: int = 1 << 20, hw: int = 0) -> str:
    """rocprof name of the fused MLP instantiation the library launches (pipnet_cnblock_mlp_label)."""
    return _lib.label("pipnet_cnblock_mlp_label", m, c, hw)


def cnblock_mlp(t: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, gamma: Tensor, x: Tensor,
                hw: int = 0) -> Tensor:
    """In place on ``x`` [M, C]: x += gamma * (W2 gelu(W1 t + b1) + b2) -- the whole CNBlock MLP
    of a narrow stage (C = 96 / 192) in one kernel, the hidden activation kept in registers
    (csrc/mlp_f32.hip).  ``hw`` = the layer's pixels per image (0 = unknown): picks the
    instantiation by map size, never by M."""
    _chk_rows("cnblock_mlp", t, "mlp input", 2)
    m, c = t.shape
    if c not in MLP_FUSED_CHANNELS:
        raise RuntimeError(f"cnblock_mlp: {c} channels, supported {MLP_FUSED_CHANNELS}")
    for v, what, shape in ((w1, "fc1 weight", (4 * c, c)), (b1, "fc1 bias", 4 * c), (w2, "fc2 weight", (c, 4 * c)),
                           (b2, "fc2 bias", c), (gamma, "layer scale", c), (x, "residual", (m, c))):
        _operand("cnblock_mlp", what, v, shape=shape, device=t.device)
    _launch(cnblock_mlp_kernel_name(c, m, hw), 2.0 * 2 * m * 4 * c * c,
            lambda: _lib.call("pipnet_cnblock_mlp_hw_f32", t.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
                              b2.data_ptr(), gamma.data_ptr(), x.data_ptr(), m, c, hw, _stream(t)))
    return x


# ---- the low-precision ConvNeXt paths: split bf16 ("bf16x3", pipnet_conv2d_nhwc_s3) and plain bf16 ("bf16",
# ---- pipnet_conv2d_nhwc_bf16_mix), include/pipnet_amd.h ----
S3_KTILE = 32          # split weights: K padded to the 32-deep K tiles of the split kernels
def split_planes_weight(w_ohwi: Tensor) -> Tensor:
    """fp32 weight [Cout, KH, KW, Cin] -> packed split-bf16 B operand [Cout, Kp] bf16: per tap
    [hi | hi | lo] over 3 Cin (hi = RNE(w), lo = RNE(w - hi)), Kp = KH*KW*3Cin rounded up to 32."""
    hi = w_ohwi.to(torch.bfloat16)
    lo = (w_ohwi - hi.float()).to(torch.bfloat16)
    cout, kh, kw, cin = w_ohwi.shape
    k = kh * kw * 3 * cin
    kp = -(-k // S3_KTILE) * S3_KTILE
    out = torch.zeros((cout, kp), device=w_ohwi.device, dtype=torch.bfloat16)
    out[:, :k] = torch.cat([hi, hi, lo], dim=-1).reshape(cout, k)
    return out


def split_planes(x: Tensor) -> Tensor:
    """fp32 [..., C] -> split planes [..., 2C] bf16 [hi | lo] (what the producer kernels
    write; for tests and for inputs that do not come from a split-writing kernel)."""
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return torch.cat([hi, lo], dim=-1).contiguous()


@dataclasses.dataclass(frozen=True)
class OperandFormat:
    """What differs between the low-precision operand formats of the ConvNeXt GEMMs, and nothing else: the one place
    a new format is added."""
    a_planes: int          # bf16 values per input channel in A: 2 = split planes [hi | lo], 1 = plain bf16
    k_factor: int          # packed-K entries per input channel and tap
    ktile: int             # the K tile the packed weight is padded to
    pack: Callable[[Tensor], Tensor]    # fp32 [Cout, KH, KW, Cin] -> the packed B operand
    gelu_epilogue: int     # writes gelu(conv + b) as the next GEMM's A operand, a_planes * Cout bf16 wide
    flop_div: int          # products per multiply: the launch hook is told the algorithmic flops
    conv: str              # library entries
    conv_label: str
    rowscale: str
    rowscale_label: str
    dwconv7_ln: str
    layernorm: str
    conv_fn: str           # the public wrappers of those entries in this module: their name opens every message, and
    rowscale_fn: str       # the executor looks them up by it at call time, so a tool can swap one (tools/ab/)
    dwconv7_ln_fn: str
    layernorm_fn: str
    conv_takes_cout: bool  # conv_s3 has a ``cout`` argument after kw, conv_bf16_mix reads it off the weight
    cache_suffix: str      # of the packed weights' keys in a model's weight cache


LOWP_FORMATS = {
    "bf16x3": OperandFormat(
        a_planes=2, k_factor=3, ktile=S3_KTILE, pack=split_planes_weight, gelu_epilogue=_lib.EPI_S3_GELU, flop_div=3,
        conv="pipnet_conv2d_nhwc_s3", conv_label="pipnet_conv2d_nhwc_s3_label", rowscale="pipnet_linear_s3_rowscale",
        rowscale_label="pipnet_linear_s3_rowscale_label", dwconv7_ln="pipnet_dwconv7_ln_s3",
        layernorm="pipnet_layernorm_s3", conv_fn="conv_s3", rowscale_fn="linear_s3_rowscale",
        dwconv7_ln_fn="dwconv7_ln_s3", layernorm_fn="layernorm_s3", conv_takes_cout=True, cache_suffix=".s3"),
    "bf16": OperandFormat(
        a_planes=1, k_factor=1, ktile=BF16_KTILE, pack=pack_conv_weight_bf16, gelu_epilogue=_lib.EPI_BIAS_GELU,
        flop_div=1, conv="pipnet_conv2d_nhwc_bf16_mix", conv_label="pipnet_conv2d_nhwc_bf16_mix_label",
        rowscale="pipnet_linear_bf16_mix_rowscale", rowscale_label="pipnet_linear_bf16_mix_rowscale_label",
        dwconv7_ln="pipnet_dwconv7_ln_bf16", layernorm="pipnet_layernorm_bf16", conv_fn="conv_bf16_mix",
        rowscale_fn="linear_bf16_mix_rowscale", dwconv7_ln_fn="dwconv7_ln_bf16", layernorm_fn="layernorm_bf16",
        conv_takes_cout=False, cache_suffix=".bf16"),
}
_S3, _MIX = LOWP_FORMATS["bf16x3"], LOWP_FORMATS["bf16"]


@functools.lru_cache(maxsize=4096)
def _lowp_label(entry: str, *args: int) -> str:
    """rocprof name of the instantiation a format's conv / rowscale entry launches (``entry``: its label entry)."""
    return _lib.label(entry, *args)


def _conv_lowp(fmt: OperandFormat, x: Tensor, w_packed: Tensor, kh: int, kw: int, bias: Optional[Tensor],
               stride: int, pad: int, epilogue: int, scale: Optional[Tensor] = None, r: Optional[Tensor] = None,
               out: Optional[Tensor] = None, tile: int = -1, cout: Optional[int] = None) -> Tensor:
    """conv_s3 / conv_bf16_mix: ``x`` [B,H,W,a_planes * Cin] bf16 against a weight packed by ``fmt.pack``."""
    fn = fmt.conv_fn
    _operand(fn, "input", x, dtype=torch.bfloat16)
    if x.dim() != 4 or x.shape[3] % fmt.a_planes:
        raise RuntimeError(f"{fn}: input must be [B,H,W,{fmt.a_planes} x Cin] (got shape {tuple(x.shape)})")
    b, h, w, width = x.shape
    dev, cin = x.device, width // fmt.a_planes
    k = kh * kw * fmt.k_factor * cin
    _operand(fn, "weight", w_packed, dtype=torch.bfloat16, device=dev)
    if w_packed.dim() != 2 or w_packed.shape[1] != -(-k // fmt.ktile) * fmt.ktile or \
            cout not in (None, w_packed.shape[0]):
        raise RuntimeError(f"{fn}: packed weight {tuple(w_packed.shape)} does not match {kh}x{kw}x{cin}"
                           f"{'' if cout is None else f' -> {cout}'} (K padded to {fmt.ktile})")
    cout = w_packed.shape[0]
    if epilogue not in (fmt.gelu_epilogue, _lib.EPI_F32_BIAS, _lib.EPI_F32_RESID):
        raise RuntimeError(f"{fn}: epilogue {epilogue} is not the format's GELU ({fmt.gelu_epilogue}), EPI_F32_BIAS or "
                           "EPI_F32_RESID")
    _chk_vec(fn, x, cout, bias=bias, scale=scale)
    oh, ow = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    m = b * oh * ow
    if epilogue == _lib.EPI_F32_RESID and scale is None:
        raise RuntimeError(f"{fn}: EPI_F32_RESID needs r and scale")
    _operand(fn, "residual", r, shape=m * cout, device=dev, optional=epilogue != _lib.EPI_F32_RESID)
    if epilogue == fmt.gelu_epilogue:
        shape, dt = (b, oh, ow, fmt.a_planes * cout), torch.bfloat16
    else:
        shape, dt = (b, oh, ow, cout), torch.float32
    if out is None:
        out = torch.empty(shape, device=dev, dtype=dt)
    else:
        _operand(fn, "out", out, dtype=dt, shape=m * shape[-1], device=dev)
    _launch(_lowp_label(fmt.conv_label, b, h, w, cin, cout, kh, kw, stride, pad, epilogue, tile),
            2.0 * m * cout * k / fmt.flop_div,
            lambda: _lib.call(fmt.conv, x.data_ptr(), b, h, w, cin, w_packed.data_ptr(), _ptr(bias), _ptr(scale),
                              _ptr(r), cout, kh, kw, stride, pad, epilogue, out.data_ptr(), tile, _stream(x)))
    return out


def conv_s3(x2: Tensor, w_packed: Tensor, kh: int, kw: int, cout: int, bias: Optional[Tensor], stride: int, pad: int,
            epilogue: int, scale: Optional[Tensor] = None, r: Optional[Tensor] = None, out: Optional[Tensor] = None,
            tile: int = -1) -> Tensor:
    """Split-bf16 conv / linear: x2 [B,H,W,2Cin] split planes, w_packed [cout, Kp] from split_planes_weight.
    EPI_S3_GELU -> split planes [B,OH,OW,2Cout] of gelu(conv + b); EPI_F32_BIAS -> fp32
    [B,OH,OW,Cout]; EPI_F32_RESID -> fp32 r + scale * (conv + b) (``out`` may be ``r``).
    tile -1 = automatic, or 0 / 4 / 5 / 7."""
    return _conv_lowp(_S3, x2, w_packed, kh, kw, bias, stride, pad, epilogue, scale, r, out, tile, cout)


def conv_bf16_mix(x: Tensor, w_packed: Tensor, kh: int, kw: int, bias: Optional[Tensor], stride: int, pad: int,
                  epilogue: int, scale: Optional[Tensor] = None, r: Optional[Tensor] = None,
                  out: Optional[Tensor] = None, tile: int = -1) -> Tensor:
    """Plain bf16 conv / linear with the ConvNeXt epilogues: x [B,H,W,Cin] bf16, w_packed from
    pack_conv_weight_bf16, fp32 accumulation.  EPI_BIAS_GELU -> bf16 [B,OH,OW,Cout] of gelu(conv + b);
    EPI_F32_BIAS -> fp32 conv + b; EPI_F32_RESID -> fp32 r + scale * (conv + b) (``out`` may be ``r``).
    tile -1 = automatic, or 0 / 4 / 5 / 7 (the split GEMM's tiles)."""
    return _conv_lowp(_MIX, x, w_packed, kh, kw, bias, stride, pad, epilogue, scale, r, out, tile)


def _form_out(fmt: Optional[OperandFormat], x: Tensor) -> Tensor:
    """The output of a producer kernel over fp32 ``x`` [..., C]: fp32 (``fmt`` None), or ``fmt``'s A operand."""
    if fmt is None:
        return torch.empty_like(x)
    return torch.empty(tuple(x.shape[:-1]) + (fmt.a_planes * x.shape[-1],), device=x.device, dtype=torch.bfloat16)


def _dwconv7_ln(fmt: Optional[OperandFormat], x_nhwc: Tensor, w_packed: Tensor, bias: Tensor, ln_w: Tensor,
                ln_b: Tensor, out: Optional[Tensor] = None) -> Tensor:
    fn = "dwconv7_ln" if fmt is None else fmt.dwconv7_ln_fn
    _chk_rows(fn, x_nhwc, "input", 4)
    b, h, w, c = x_nhwc.shape
    _operand(fn, "w_packed", w_packed, shape=49 * c, device=x_nhwc.device)
    for what, t in (("bias", bias), ("ln_w", ln_w), ("ln_b", ln_b)):
        _operand(fn, what, t, shape=c, device=x_nhwc.device)
    _chk_same(fn, x_nhwc, out=out)
    y = _form_out(fmt, x_nhwc) if out is None else out
    _lib.call("pipnet_dwconv7_ln_f32" if fmt is None else fmt.dwconv7_ln, x_nhwc.data_ptr(), b, h, w, c,
              w_packed.data_ptr(), bias.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(), y.data_ptr(), _stream(x_nhwc))
    return y


def dwconv7_ln(x_nhwc: Tensor, w_packed: Tensor, bias: Tensor, ln_w: Tensor, ln_b: Tensor,
               out: Optional[Tensor] = None) -> Tensor:
    """Depthwise 7x7 conv (pad 3) + bias + LayerNorm over channels, NHWC fp32 (pipnet_dwconv7_ln_f32)."""
    return _dwconv7_ln(None, x_nhwc, w_packed, bias, ln_w, ln_b, out)


def dwconv7_ln_s3(x_nhwc: Tensor, w_packed: Tensor, bias: Tensor, ln_w: Tensor, ln_b: Tensor) -> Tensor:
    """pipnet_dwconv7_ln_f32 writing split planes [B,H,W,2C] bf16."""
    return _dwconv7_ln(_S3, x_nhwc, w_packed, bias, ln_w, ln_b)


def dwconv7_ln_bf16(x_nhwc: Tensor, w_packed: Tensor, bias: Tensor, ln_w: Tensor, ln_b: Tensor) -> Tensor:
    """pipnet_dwconv7_ln_f32 rounded once (RNE) to bf16 [B,H,W,C]: the hi plane of dwconv7_ln_s3."""
    return _dwconv7_ln(_MIX, x_nhwc, w_packed, bias, ln_w, ln_b)


def _layernorm(fmt: Optional[OperandFormat], x: Tensor, w: Tensor, b: Tensor, out: Optional[Tensor] = None) -> Tensor:
    fn = "layernorm" if fmt is None else fmt.layernorm_fn
    _operand(fn, "input", x)
    c = x.shape[-1]
    _chk_vec(fn, x, c, w=w, b=b)
    _chk_same(fn, x, out=out)
    y = _form_out(fmt, x) if out is None else out
    _lib.call("pipnet_layernorm_f32" if fmt is None else fmt.layernorm, x.data_ptr(), x.numel() // c, c, w.data_ptr(),
              b.data_ptr(), y.data_ptr(), _stream(x))
    return y


def layernorm(x: Tensor, w: Tensor, b: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """Row LayerNorm over the last dimension, fp32 (pipnet_layernorm_f32)."""
    return _layernorm(None, x, w, b, out)


def layernorm_s3(x: Tensor, w: Tensor, b: Tensor) -> Tensor:
    """Row LayerNorm writing split planes [..., 2C] bf16."""
    return _layernorm(_S3, x, w, b)


def layernorm_bf16(x: Tensor, w: Tensor, b: Tensor) -> Tensor:
    """Row LayerNorm rounded once (RNE) to bf16 [..., C]: the hi plane of layernorm_s3."""
    return _layernorm(_MIX, x, w, b)


# ---- CNBlock Linear2 under train-mode stochastic depth on the low-precision operands ----
LOWP_ROWSCALE_TILES = (-1, 0, 4, 5, 7)      # what EPI_F32_RESID takes on either operand format


@functools.lru_cache(maxsize=4096)
def linear_lowp_rowscale_kernel_name(m: int, cin: int, cout: int, tile: int = -1, s3: bool = False) -> str:
    """rocprof name of the instantiation linear_bf16_mix_rowscale (``s3``: linear_s3_rowscale, ``cin`` its fp32
    channels) launches (pipnet_linear_bf16_mix_rowscale_label / pipnet_linear_s3_rowscale_label)."""
    return _lowp_label(LOWP_FORMATS["bf16x3" if s3 else "bf16"].rowscale_label, m, cin, cout, tile)


def _linear_lowp_rowscale(fmt: OperandFormat, a: Tensor, w_packed: Tensor, bias: Optional[Tensor], scale: Tensor,
                          r: Tensor, row_scale: Tensor, rows_per_scale: int, out: Optional[Tensor] = None,
                          tile: int = -1) -> Tensor:
    fn = fmt.rowscale_fn
    _operand(fn, "input", a, dtype=torch.bfloat16)
    if a.dim() < 2 or a.shape[-1] % fmt.a_planes:
        raise RuntimeError(f"{fn}: input must be rows [..., {fmt.a_planes} x Cin] (got shape {tuple(a.shape)})")
    width = a.shape[-1]
    cin, m = width // fmt.a_planes, a.numel() // width
    k = fmt.k_factor * cin
    kp = -(-k // fmt.ktile) * fmt.ktile
    _operand(fn, "weight", w_packed, dtype=torch.bfloat16, device=a.device)
    if w_packed.dim() != 2 or w_packed.shape[1] != kp:
        raise RuntimeError(f"{fn}: packed weight {tuple(w_packed.shape)} does not match {cin} input channels "
                           f"(packed K {kp})")
    cout = w_packed.shape[0]
    if tile not in LOWP_ROWSCALE_TILES:
        raise RuntimeError(f"{fn}: tile {tile} is not one of {LOWP_ROWSCALE_TILES}")
    _chk_vec(fn, a, cout, bias=bias)
    _operand(fn, "scale", scale, shape=cout, device=a.device)
    _operand(fn, "residual", r, shape=m * cout, device=a.device)
    _operand(fn, "row_scale", row_scale, device=a.device)
    _chk_row_scale(fn, a, m, row_scale, rows_per_scale)
    if out is None:
        out = r
    else:
        _operand(fn, "out", out, shape=m * cout, device=a.device)
    _launch(_lowp_label(fmt.rowscale_label, m, cin, cout, tile), 2.0 * m * cout * k / fmt.flop_div,
            lambda: _lib.call(fmt.rowscale, a.data_ptr(), m, cin, w_packed.data_ptr(), _ptr(bias), scale.data_ptr(),
                              r.data_ptr(), cout, row_scale.data_ptr(), rows_per_scale, out.data_ptr(), tile,
                              _stream(a)))
    return out


def linear_bf16_mix_rowscale(a: Tensor, w_packed: Tensor, bias: Optional[Tensor], scale: Tensor, r: Tensor,
                             row_scale: Tensor, rows_per_scale: int, out: Optional[Tensor] = None,
                             tile: int = -1) -> Tensor:
    """fp32 r + row_scale[m // rows_per_scale] * (scale * (a w^T + bias)) on plain bf16 rows ``a`` [..., Cin]
    and a pack_conv_weight_bf16 weight: conv_bf16_mix's EPI_F32_RESID with one stochastic-depth factor per
    sample (same tile, same K order).  In place on ``r`` unless ``out`` is given; tile -1 / 0 / 4 / 5 / 7."""
    return _linear_lowp_rowscale(_MIX, a, w_packed, bias, scale, r, row_scale,
                                 rows_per_scale, out, tile)


def linear_s3_rowscale(a2: Tensor, w_packed: Tensor, bias: Optional[Tensor], scale: Tensor, r: Tensor,
                       row_scale: Tensor, rows_per_scale: int, out: Optional[Tensor] = None, tile: int = -1) -> Tensor:
    """The same on split planes ``a2`` [..., 2 Cin] and a split_planes_weight weight: conv_s3's EPI_F32_RESID
    with one stochastic-depth factor per sample."""
    return _linear_lowp_rowscale(_S3, a2, w_packed, bias, scale, r, row_scale,
                                 rows_per_scale, out, tile)


def softmax_pool(feat_nhwc: Tensor, pool_mode: int, out=None) -> Tuple[Tensor, Tensor]:
    """feat [B,h,w,P] -> (proto [B,h,w,P], pooled [B,P]); pool 0 = max, 1 = sum.
    ``out`` = (proto, pooled) to write into (e.g. batch slices of a larger output)."""
    _chk(feat_nhwc, "prototype logits")
    b, h, w, p = feat_nhwc.shape
    proto, pooled = _head_out(out, b, h, w, p, feat_nhwc.device)
    _lib.call("pipnet_softmax_pool_f32", feat_nhwc.data_ptr(), b, h * w, p, pool_mode, proto.data_ptr(),
              pooled.data_ptr(), _stream(feat_nhwc))
    return proto, pooled


def softmax_pool_argmax(feat_nhwc: Tensor, write_proto: bool = False, out=None):
    """softmax_pool(feat, 0) that also says where each prototype's maximum sits: feat [B,h,w,P] ->
    (proto [B,h,w,P] or None, pooled [B,P], loc [B,P] int32 = h_idx * w + w_idx by the reference's
    two-step torch.max, util/vis_pipnet.py:235-238).  pooled (and proto, written only when
    ``write_proto``) equal softmax_pool's bit for bit.  ``out`` = (pooled, loc) to write into."""
    _chk(feat_nhwc, "prototype logits")
    b, h, w, p = feat_nhwc.shape
    dev = feat_nhwc.device
    pooled, loc = _argmax_out(out, b, p, dev, "softmax_pool_argmax")
    proto =torch.empty((b, h, w, p), device=dev, dtype=torch.float32) if write_proto else None
    ws = torch.empty((max(b * p, 1),), device=dev, dtype=torch.int64)       # the packed (value, rank) keys
    _lib.call("pipnet_softmax_pool_argmax_f32", feat_nhwc.data_ptr(), b, h, w, p, _ptr(proto), pooled.data_ptr(),
              loc.data_ptr(), ws.data_ptr(), _stream(feat_nhwc))
    return proto, pooled, loc


def _argmax_out(out, b: int, p: int, dev, what: str) -> Tuple[Tensor, Tensor]:
    """Caller-provided (value [B,P] float32, loc [B,P] int32) contiguous outputs, or new ones."""
    if out is None:
        return (torch.empty((b, p), device=dev, dtype=torch.float32),
                torch.empty((b, p), device=dev, dtype=torch.int32))
    val, loc = out
    _operand(what, "value out", val, shape=(b, p), device=dev)
    _operand(what, "loc out", loc, dtype=torch.int32, shape=(b, p), device=dev)
    return val, loc


def map_argmax(map_nhwc: Tensor, out=None) -> Tuple[Tensor, Tensor]:
    """Maximum and its location of a stored fp32 map [B,h,w,P] (NHWC memory) per (image, prototype):
    (val [B,P], loc [B,P] int32 = h_idx * w + w_idx), the location rule of softmax_pool_argmax.
    ``out`` = (val, loc) to write into."""
    _chk(map_nhwc, "prototype map")
    b, h, w, p = map_nhwc.shape
    val, loc = _argmax_out(out, b, p, map_nhwc.device, "map_argmax")
    _lib.call("pipnet_map_argmax_f32", map_nhwc.data_ptr(), b, h, w, p, val.data_ptr(), loc.data_ptr(),
              _stream(map_nhwc))
    return val, loc


TOPK_MAX_K = _lib.CONSTANTS["TOPK_MAX_K"]
STATE_MERGE_MAX_RANKS = _lib.CONSTANTS["STATE_MERGE_MAX_RANKS"]


class PackedState:
    """What the states of the dataset passes share when ranks exchange them: ``PACK`` names the tensors in
    descending element size, so that in ``pack()``'s byte buffer (padded to a multiple of 8) every field stays
    aligned, and ``unpack`` reads a state of this one's dimensions back out of such a buffer as views."""
    PACK: Tuple[str, ...] = ()

    def packed_bytes(self) -> int:
        n = sum(getattr(self, f).numel() * getattr(self, f).element_size() for f in self.PACK)
        return -(-n // 8) * 8

    def pack(self) -> Tensor:
        parts = [getattr(self, f).contiguous().view(-1).view(torch.uint8) for f in self.PACK]
        pad = self.packed_bytes() - sum(p.numel() for p in parts)
        if pad:
            parts.append(torch.zeros(pad, dtype=torch.uint8, device=parts[0].device))
        return torch.cat(parts)

    def unpack(self, buf: Tensor):
        if buf.dtype != torch.uint8 or buf.dim() != 1 or buf.numel() != self.packed_bytes() or not buf.is_contiguous():
            raise RuntimeError(f"{type(self).__name__}.unpack: needs {self.packed_bytes()} contiguous uint8 bytes "
                               f"(got {buf.dtype} {tuple(buf.shape)})")
        out = copy.copy(self)
        at = 0
        for f in self.PACK:
            t = getattr(self, f)
            n = t.numel() * t.element_size()
            setattr(out, f, buf[at:at + n].view(t.dtype).view(t.shape))
            at += n
        return out


def _merge_operands(fn: str, states, cls, dims: Tuple[str, ...]):
    """The checked inputs of a state merge: ``states`` is a non-empty sequence of ``cls`` states of equal ``dims``
    on one device.  Returns (states, byte stride between consecutive ranks, common to every field): states that
    already are views into one gathered buffer are taken as they lie, anything else is packed into one first."""
    states = list(states)
    if not states:
        raise RuntimeError(f"{fn}: needs at least one state (W = 0)")
    if len(states) > STATE_MERGE_MAX_RANKS:
        raise RuntimeError(f"{fn}: {len(states)} states, at most {STATE_MERGE_MAX_RANKS} are merged in one call")
    s0 = states[0]
    dev = getattr(s0, cls.PACK[0]).device
    for r, s in enumerate(states):
        if not isinstance(s, cls):
            raise RuntimeError(f"{fn}: state {r} is a {type(s).__name__}, expected {cls.__name__}")
        if any(getattr(s, d) != getattr(s0, d) for d in dims):
            raise RuntimeError(f"{fn}: state {r} has {[(d, getattr(s, d)) for d in dims]}, state 0 "
                               f"{[(d, getattr(s0, d)) for d in dims]}")
        for f in cls.PACK:
            t, t0 = getattr(s, f), getattr(s0, f)
            if t.device != dev or t.dtype != t0.dtype or t.shape != t0.shape or not t.is_contiguous():
                raise RuntimeError(f"{fn}: {f} of state {r} is {t.dtype} {tuple(t.shape)} (stride {t.stride()}) on "
                                   f"{t.device}, state 0 holds contiguous {t0.dtype} {tuple(t0.shape)} on {dev}")
    if len(states) == 1 or dev.type != "cuda":
        return states, 0
    live = [f for f in cls.PACK if getattr(s0, f).numel()]
    d = getattr(states[1], live[0]).data_ptr() - getattr(s0, live[0]).data_ptr()
    lie = d > 0 and d % 8 == 0 and all(
        getattr(s, f).is_contiguous() and getattr(s, f).data_ptr() - getattr(s0, f).data_ptr() == r * d
        for r, s in enumerate(states) for f in live)
    if not lie:
        buf = torch.stack([s.pack() for s in states])
        states, d = [s0.unpack(row) for row in buf], buf.stride(0)
    return states, d


class TopkState(PackedState):
    """Device state of the streaming top-k (pipnet_topk_update): per (group, prototype) the k best
    (score, dataset index, loc) so far, the fill counts and the abstain counter."""
    PACK = ("index", "abstained", "score", "loc", "fill")

    def __init__(self, groups: int, prototypes: int, k: int, device):
        if not 1 <= k <= TOPK_MAX_K:
            raise ValueError(f"top-k: k must be in 1..{TOPK_MAX_K}, got {k}")
        if groups < 1 or prototypes < 1:
            raise ValueError("top-k: needs at least one group and one prototype")
        self.groups, self.prototypes, self.k = groups, prototypes, k
        self.score = torch.zeros((groups, prototypes, k), device=device, dtype=torch.float32)
        self.index = torch.full((groups, prototypes, k), -1, device=device, dtype=torch.int64)
        self.loc = torch.full((groups, prototypes, k), -1, device=device, dtype=torch.int32)
        self.fill = torch.zeros((groups, prototypes), device=device, dtype=torch.int32)
        self.abstained = torch.zeros((1,), device=device, dtype=torch.int64)


def topk_update(state: TopkState, score: Tensor, loc: Tensor, i0: int, group: Optional[Tensor] = None,
                min_score: Optional[float] = None, out: Optional[Tensor] = None) -> TopkState:
    """Merge one batch into ``state``: score / loc [B,P] (image b = dataset index ``i0 + b``),
    ``group`` [B] int32 (None: all in group 0; -1 skips the image), ``min_score`` skips candidates
    below it, ``out`` [B,K] logits feed the abstain counter.  Enqueues one kernel, no host sync."""
    _chk_rows("topk_update", score, "scores", 2)
    b, p = score.shape
    dev = score.device
    if p != state.prototypes or state.score.device != dev:
        raise RuntimeError(f"topk_update: score {tuple(score.shape)} on {dev} does not match the state's "
                           f"{state.prototypes} prototypes on {state.score.device}")
    _operand("topk_update", "loc", loc, dtype=torch.int32, shape=(b, p), device=dev)
    _operand("topk_update", "group", group, dtype=torch.int32, shape=(b,), device=dev, optional=True)
    if out is not None:
        _operand("topk_update", "logits", out, device=dev)
        if out.dim() != 2 or out.shape[0] != b:
            raise RuntimeError(f"topk_update: logits {tuple(out.shape)} vs batch {b}")
    _lib.call("pipnet_topk_update", score.data_ptr(), loc.data_ptr(), b, p, int(i0), _ptr(group), state.groups,
              0 if min_score is None else 1, 0.0 if min_score is None else float(min_score), _ptr(out),
              0 if out is None else out.shape[1], state.k, state.score.data_ptr(), state.index.data_ptr(),
              state.loc.data_ptr(), state.fill.data_ptr(), state.abstained.data_ptr(), _stream(score))
    return state


def _torch_topk_merge(states, out: TopkState) -> TopkState:
    """pipnet_topk_merge with torch ops: the union's entries by (score descending, index ascending), empty
    slots last -- three stable sorts, least significant key first."""
    k = out.k
    score = torch.cat([s.score for s in states], dim=2)
    index = torch.cat([s.index for s in states], dim=2)
    loc = torch.cat([s.loc for s in states], dim=2)
    slot = torch.arange(k, device=score.device)
    empty = torch.cat([slot >= s.fill.clamp(0, k)[:, :, None] for s in states], dim=2)
    order = torch.sort(index, dim=2, stable=True).indices
    order = order.gather(2, torch.sort(score.gather(2, order), dim=2, descending=True, stable=True).indices)
    order = order.gather(2, torch.sort(empty.gather(2, order).to(torch.uint8), dim=2, stable=True).indices)[:, :, :k]
    fill = torch.stack([s.fill.clamp(0, k) for s in states]).sum(dim=0).clamp(max=k).to(torch.int32)
    unused = slot >= fill[:, :, None]
    out.score.copy_(score.gather(2, order).masked_fill(unused, 0.0))
    out.index.copy_(index.gather(2, order).masked_fill(unused, -1))
    out.loc.copy_(loc.gather(2, order).masked_fill(unused, -1))
    out.fill.copy_(fill)
    out.abstained.copy_(torch.stack([s.abstained for s in states]).sum(dim=0))
    return out


def topk_merge(states) -> TopkState:
    """The top-k state of the whole dataset from the states of its blocks (``states``: a sequence of TopkState
    of equal groups / prototypes / k on one device, one per rank, each updated with its block's dataset
    indices): per (group, prototype) the k best of the union by (score descending, dataset index ascending),
    fill = min(k, sum of fills), the abstain counters added.  Bit for bit the state of one pass over all blocks.
    States that are views into one gathered buffer are read where they lie; one kernel, no host sync.  CPU
    states: the same rule by torch ops."""
    states, stride = _merge_operands("topk_merge", states, TopkState, ("groups", "prototypes", "k"))
    s0 = states[0]
    out = TopkState(s0.groups, s0.prototypes, s0.k, s0.score.device)
    if not s0.score.is_cuda:
        return _torch_topk_merge(states, out)
    _lib.call("pipnet_topk_merge", s0.score.data_ptr(), s0.index.data_ptr(), s0.loc.data_ptr(), s0.fill.data_ptr(),
              s0.abstained.data_ptr(), stride, len(states), s0.groups, s0.prototypes, s0.k, out.score.data_ptr(),
              out.index.data_ptr(), out.loc.data_ptr(), out.fill.data_ptr(), out.abstained.data_ptr(), _stream(s0.score))
    return out


PROTO_STATS_MAX_BINS = _lib.CONSTANTS["PROTO_STATS_MAX_BINS"]


class ProtoStatsState(PackedState):
    """Device state of the streaming class-conditional statistics (pipnet_proto_stats_update_f32):
    per (class, prototype) the counters, fp64 sums, maximum and histogram so far, the images per
    class and the count of labels outside [0, classes).  ``edges``: ascending fp32 [NB + 1], or
    None for no histogram."""
    PACK = ("n_class", "n_ge", "n_gt", "total", "total_gt", "bad", "vmax", "hist")

    def __init__(self, classes: int, prototypes: int, threshold: float, edges: Optional[Tensor], device):
        if classes < 1 or prototypes < 1:
            raise ValueError("prototype statistics: need at least one class and one prototype")
        if edges is not None:
            edges = torch.as_tensor(edges, dtype=torch.float32).to(device).contiguous()
            if edges.dim() != 1 or not 2 <= edges.numel() <= PROTO_STATS_MAX_BINS + 1:
                raise ValueError(f"prototype statistics: edges must be 1-D with 2..{PROTO_STATS_MAX_BINS + 1} "
                                 f"entries, got {tuple(edges.shape)}")
        self.classes, self.prototypes, self.edges = classes, prototypes, edges
        self.bins = 0 if edges is None else edges.numel() - 1
        self.threshold = float(torch.tensor(threshold, dtype=torch.float32))     # the fp32 value compared against
        kp = (classes, prototypes)
        self.n_class = torch.zeros((classes,), device=device, dtype=torch.int64)
        self.n_ge = torch.zeros(kp, device=device, dtype=torch.int64)
        self.n_gt = torch.zeros(kp, device=device, dtype=torch.int64)
        self.total = torch.zeros(kp, device=device, dtype=torch.float64)
        self.total_gt = torch.zeros(kp, device=device, dtype=torch.float64)
        self.vmax = torch.full(kp, float("-inf"), device=device, dtype=torch.float32)
        self.hist = torch.zeros(kp + (self.bins,), device=device, dtype=torch.int32)
        self.bad = torch.zeros((1,), device=device, dtype=torch.int64)

    def tensors(self):
        return (self.n_class, self.n_ge, self.n_gt, self.total, self.total_gt, self.vmax, self.hist, self.bad)


def proto_stats_update(state: ProtoStatsState, act: Tensor, labels: Tensor) -> ProtoStatsState:
    """Merge one batch into ``state``: act [B,P] float32 (any row stride, unit column stride), labels
    [B] int64 on the device; a label outside [0, classes) only raises ``state.bad``.  Every entry is
    accumulated in image order by one owner thread, so the state does not depend on the batching.
    Enqueues one kernel, no host sync."""
    _operand("proto_stats_update", "act", act, layout="rows")
    b, p = act.shape
    if p != state.prototypes or state.n_ge.device != act.device:
        raise RuntimeError(f"proto_stats_update: act {tuple(act.shape)} on {act.device} does not match the state's "
                           f"{state.prototypes} prototypes on {state.n_ge.device}")
    _operand("proto_stats_update", "labels", labels, dtype=torch.int64, shape=(b,), device=act.device)
    if b == 0:
        return state
    lda = act.stride(0) if b > 1 else max(act.stride(0), p)
    _lib.call("pipnet_proto_stats_update_f32", act.data_ptr(), lda, labels.data_ptr(), b, p, state.classes,
              state.threshold, _ptr(state.edges), state.bins, *[t.data_ptr() for t in state.tensors()], _stream(act))
    return state


def colsum_accum_f64(acc: Tensor, x: Tensor) -> Tensor:
    """acc [D] float64 += the column sums of x [B,D] float32 (any row stride), the rows added in
    order by one owner thread per column (pipnet_colsum_accum_f64).  One kernel, no host sync."""
    _operand("colsum_accum_f64", "input", x, layout="rows")
    b, d = x.shape
    _operand("colsum_accum_f64", "acc", acc, dtype=torch.float64, shape=(d,), device=x.device)
    if b == 0:
        return acc
    _lib.call("pipnet_colsum_accum_f64", x.data_ptr(), x.stride(0) if b > 1 else max(x.stride(0), d), b, d,
              acc.data_ptr(), _stream(x))
    return acc


def proto_stats_merge(states) -> ProtoStatsState:
    """The statistics of the whole dataset from the states of its blocks (``states``: a sequence of
    ProtoStatsState of equal classes / prototypes / bins on one device, one per rank in rank order; threshold
    and edges are state 0's): the counters, the histogram and ``bad`` are integer sums, ``vmax`` the maximum,
    ``total`` / ``total_gt`` the ranks' fp64 sums added in rank order by one owner thread per entry -- bitwise
    the one-pass sums when the addends are integers, else within 2 (n + W) 2^-53 of them (relative to the sum
    of |x|): they depend on the partition in the last bits.  One kernel, no host sync; CPU states: the same
    rule by torch ops in the same order."""
    states, stride = _merge_operands("proto_stats_merge", states, ProtoStatsState, ("classes", "prototypes", "bins"))
    s0 = states[0]
    out = ProtoStatsState(s0.classes, s0.prototypes, s0.threshold, s0.edges, s0.n_ge.device)
    if not s0.n_ge.is_cuda:
        for f in ("n_class", "n_ge", "n_gt", "total", "total_gt", "hist", "bad"):
            acc = getattr(s0, f).clone()
            for s in states[1:]:                    # rank order: the kernel's chain of fp64 adds
                acc += getattr(s, f)
            getattr(out, f).copy_(acc)
        for s in states:
            torch.fmax(out.vmax, s.vmax, out=out.vmax)
        return out
    _lib.call("pipnet_proto_stats_merge", *[t.data_ptr() for t in s0.tensors()], stride, len(states), s0.classes,
              s0.prototypes, s0.bins, *[t.data_ptr() for t in out.tensors()], _stream(s0.n_ge))
    return out


def colsum_merge_f64(accs: Tensor) -> Tensor:
    """[D] float64 = accs [W,D] float64 (the ranks' ``colsum_accum_f64`` accumulators, any row stride that is a
    multiple of 8 bytes) added in rank order by one owner thread per column.  One kernel, no host sync; a CPU
    tensor: the same chain by torch ops."""
    if accs.dim() != 2 or accs.dtype != torch.float64 or accs.shape[0] < 1 or accs.shape[1] < 1:
        raise RuntimeError(f"colsum_merge_f64: needs a [W >= 1, D >= 1] float64 tensor, got {accs.dtype} "
                           f"{tuple(accs.shape)}")
    w, d = accs.shape
    if w > STATE_MERGE_MAX_RANKS:
        raise RuntimeError(f"colsum_merge_f64: {w} rows, at most {STATE_MERGE_MAX_RANKS} are merged in one call")
    if not accs.is_cuda:
        out = accs[0].clone()
        for r in range(1, w):
            out += accs[r]
        return out
    _operand("colsum_merge_f64", "accs", accs, dtype=torch.float64, layout="rows")
    out = torch.empty((d,), device=accs.device, dtype=torch.float64)
    _lib.call("pipnet_colsum_merge_f64", accs.data_ptr(), accs.stride(0) * 8 if w > 1 else 0, w, d, out.data_ptr(),
              _stream(accs))
    return out


PART_PURITY_MAX_PARTS = _lib.CONSTANTS["PART_PURITY_MAX_PARTS"]


class PartPurityState(PackedState):
    """Device state of the part-purity evaluation (pipnet_part_purity_update / _rows): per
    (prototype, merged part) the rows in which the part is visible, those in which it lies in the
    patch and the key of its first appearance; the rows per prototype; the count of dataset indices
    outside the annotation table.  All integer."""
    PACK = ("n", "hits", "first_key", "rows", "bad")

    def __init__(self, prototypes: int, merged_parts: int, device):
        if prototypes < 1 or not 1 <= merged_parts <= PART_PURITY_MAX_PARTS:
            raise ValueError(f"part purity: needs at least one prototype and 1..{PART_PURITY_MAX_PARTS} merged parts")
        self.prototypes, self.merged_parts = prototypes, merged_parts
        pm = (prototypes, merged_parts)
        self.n = torch.zeros(pm, device=device, dtype=torch.int64)
        self.hits = torch.zeros(pm, device=device, dtype=torch.int64)
        self.first_key = torch.full(pm, -1, device=device, dtype=torch.int64)      # the bits of uint64 all ones
        self.rows = torch.zeros((prototypes,), device=device, dtype=torch.int64)
        self.bad = torch.zeros((1,), device=device, dtype=torch.int64)

    def tensors(self):
        return (self.n, self.hits, self.first_key, self.rows, self.bad)


def _part_table_args(state: PartPurityState, table, relevant: Tensor, geometry, what: str):
    """Checked (geometry + annotation table + state) argument tail shared by the two row kernels.
    ``table``: (xy [N,Q,2] float64, vis [N,Q] uint8, size [N,2] int32, merged [Q] int32, is_left [Q]
    uint8, pair_index [Q] int32); ``geometry``: (H, W, image_size, skip, small_map)."""
    xy, vis, size, merged, is_left, pair_index = table
    dev = state.n.device
    n_img, q = vis.shape
    want = ((xy, (n_img, q, 2), torch.float64), (vis, (n_img, q), torch.uint8), (size, (n_img, 2), torch.int32),
            (merged, (q,), torch.int32), (is_left, (q,), torch.uint8), (pair_index, (q,), torch.int32),
            (relevant, (state.prototypes,), torch.uint8))
    for name, (t, shape, dtype) in zip(("xy", "vis", "size", "merged", "is_left", "pair_index", "relevant"), want):
        _operand(what, name, t, dtype=dtype, shape=shape, device=dev)
    h, w, image_size, skip, small_map = geometry
    return (int(h), int(w), int(image_size), int(skip), 1 if small_map else 0, xy.data_ptr(), vis.data_ptr(),
            size.data_ptr(), n_img, merged.data_ptr(), is_left.data_ptr(), pair_index.data_ptr(), q,
            state.merged_parts, *[t.data_ptr() for t in state.tensors()])


def part_purity_update(state: PartPurityState, pooled: Tensor, loc: Tensor, relevant: Tensor, i0: int,
                       threshold: float, geometry, table) -> PartPurityState:
    """Merge the rows of one batch (mode "all"): image b is dataset index ``i0 + b``; prototype p
    with ``relevant[p]`` and ``pooled[b, p] > threshold`` gives a row whose patch follows from
    ``loc[b, p]``.  pooled [B,P] float32 (any row stride, unit column stride), loc [B,P] int32.
    One owner thread per prototype walks the images in order: the state does not depend on the
    batching.  Enqueues one kernel, no host sync."""
    _operand("part_purity_update", "pooled", pooled, layout="rows", device=state.n.device)
    b, p = pooled.shape
    if p != state.prototypes:
        raise RuntimeError(f"part_purity_update: pooled {tuple(pooled.shape)} must be [B, {state.prototypes}]")
    _operand("part_purity_update", "loc", loc, dtype=torch.int32, shape=(b, p), device=pooled.device)
    tail = _part_table_args(state, table, relevant, geometry, "part_purity_update")
    if b == 0:
        return state
    lda = pooled.stride(0) if b > 1 else max(pooled.stride(0), p)
    _launch("part_purity_update_kernel", 0.0,
            lambda: _lib.call("pipnet_part_purity_update", pooled.data_ptr(), lda, loc.data_ptr(), relevant.data_ptr(),
                              b, p, int(i0), float(threshold), *tail, _stream(pooled)))
    return state


def part_purity_rows(state: PartPurityState, index: Tensor, loc: Tensor, relevant: Tensor, geometry,
                     table) -> PartPurityState:
    """Merge explicit rows (mode "topk"): index [P,k] int64 dataset indices (< 0: empty slot) and loc
    [P,k] int32 of a top-k state; slot j of a relevant prototype is its j-th row.  One kernel."""
    if index.dim() != 2 or index.shape[0] != state.prototypes or not 1 <= index.shape[1] <= TOPK_MAX_K:
        raise RuntimeError(f"part_purity_rows: index {tuple(index.shape)} must be [{state.prototypes}, "
                           f"k <= {TOPK_MAX_K}]")
    _operand("part_purity_rows", "index", index, dtype=torch.int64, device=state.n.device)
    _operand("part_purity_rows", "loc", loc, dtype=torch.int32, shape=index.shape, device=state.n.device)
    tail = _part_table_args(state, table, relevant, geometry, "part_purity_rows")
    _launch("part_purity_rows_kernel", 0.0,
            lambda: _lib.call("pipnet_part_purity_rows", index.data_ptr(), loc.data_ptr(), relevant.data_ptr(),
                              state.prototypes, index.shape[1], *tail, _stream(index)))
    return state


def part_purity_merge(states) -> PartPurityState:
    """The mode-"all" part-purity state of the whole dataset from the states of its blocks (``states``: a
    sequence of PartPurityState of equal prototypes / merged parts on one device, one per rank, each updated
    with its block's dataset indices): ``n`` / ``hits`` / ``rows`` / ``bad`` are integer sums, ``first_key`` the
    unsigned minimum (keys hold the global row ordinal; all ones: never inserted).  All integer: bitwise the
    state of one pass.  One kernel, no host sync; CPU states: the same rule by torch ops."""
    states, stride = _merge_operands("part_purity_merge", states, PartPurityState, ("prototypes", "merged_parts"))
    s0 = states[0]
    out = PartPurityState(s0.prototypes, s0.merged_parts, s0.n.device)
    if not s0.n.is_cuda:
        flip = torch.iinfo(torch.int64).min                 # x ^ flip orders int64 bits as uint64
        for f in ("n", "hits", "rows", "bad"):
            getattr(out, f).copy_(torch.stack([getattr(s, f) for s in states]).sum(dim=0))
        out.first_key.copy_(torch.stack([s.first_key ^ flip for s in states]).amin(dim=0) ^ flip)
        return out
    _launch("part_purity_merge_kernel", 0.0,
            lambda: _lib.call("pipnet_part_purity_merge", *[t.data_ptr() for t in s0.tensors()], stride, len(states),
                              s0.prototypes, s0.merged_parts, *[t.data_ptr() for t in out.tensors()], _stream(s0.n)))
    return out


def part_purity_finish(state: PartPurityState):
    """The per-prototype results of the reference's evaluation loop from ``state``: (in_csv [P] bool,
    max_purity [P] float64, max_part [P] int32, max_sum [P] int64, most_part [P] int32 (-1: none),
    most_sum [P] int64, most_purity [P] float64, purity [P,M] float64 with NaN where the part never
    was visible).  One kernel, no host sync."""
    dev = state.n.device
    if not state.n.is_cuda:
        raise RuntimeError("part_purity_finish: the state must be on a ROCm device; there is no CPU fallback")
    p, m = state.prototypes, state.merged_parts
    in_csv = torch.empty((p,), device=dev, dtype=torch.uint8)
    f64 = [torch.empty((p,), device=dev, dtype=torch.float64) for _ in range(2)]
    i32 = [torch.empty((p,), device=dev, dtype=torch.int32) for _ in range(2)]
    i64 = [torch.empty((p,), device=dev, dtype=torch.int64) for _ in range(2)]
    purity = torch.empty((p, m), device=dev, dtype=torch.float64)
    _launch("part_purity_finish_kernel", 0.0,
            lambda: _lib.call("pipnet_part_purity_finish", state.n.data_ptr(), state.hits.data_ptr(),
                              state.first_key.data_ptr(), state.rows.data_ptr(), p, m, in_csv.data_ptr(),
                              f64[0].data_ptr(), i32[0].data_ptr(), i64[0].data_ptr(), i32[1].data_ptr(),
                              i64[1].data_ptr(), f64[1].data_ptr(), purity.data_ptr(), _stream(state.n)))
    return in_csv.bool(), f64[0], i32[0], i64[0], i32[1], i64[1], f64[1], purity


LOCAL_EXPLAIN_MAX = _lib.CONSTANTS["LOCAL_EXPLAIN_MAX"]         # prototypes / classes per image


def local_explain(pooled: Tensor, loc: Tensor, out: Tensor, weight: Tensor, top_classes: int, max_entries: int,
                  min_abs: float = 0.01):
    """Per image the ``top_classes`` best classes and each one's contributing prototypes
    (pipnet_local_explain_f32; util/visualize_prediction.py:63-75): pooled [B,P] scores, loc [B,P]
    int32, out [B,K] logits, weight [K,P] (any row stride) -> (cls [B,C] int32, cls_logit [B,C],
    n [B,C] int32, e_proto [B,C,M] int32, e_sim, e_w, e_simw [B,C,M] float32, e_loc [B,C,M] int32)
    with C = top_classes, M = max_entries.  Classes by logit, prototypes by score, both descending
    with the lower index first among equals; (c, p) kept iff |pooled * weight| > min_abs in fp64;
    n is the true count, empty slots hold (-1, 0, 0, 0, -1).  One kernel, no host sync."""
    _chk_rows("local_explain", pooled, "pooled scores", 2)
    _chk_rows("local_explain", out, "logits", 2)
    b, p = pooled.shape
    k = out.shape[1]
    dev = pooled.device
    if out.shape[0] != b or out.device != dev:
        raise RuntimeError(f"local_explain: pooled {tuple(pooled.shape)} on {dev} and out {tuple(out.shape)} on "
                           f"{out.device} do not match")
    _operand("local_explain", "loc", loc, dtype=torch.int32, shape=(b, p), device=dev)
    _operand("local_explain", "weight", weight, shape=(k, p), device=dev, layout="rows")
    c, m = int(top_classes), int(max_entries)
    if not (1 <= c <= k <= LOCAL_EXPLAIN_MAX and 1 <= p <= LOCAL_EXPLAIN_MAX and m >= 1):
        raise RuntimeError(f"local_explain: needs 1 <= top_classes ({c}) <= classes ({k}) <= {LOCAL_EXPLAIN_MAX}, "
                           f"1 <= prototypes ({p}) <= {LOCAL_EXPLAIN_MAX} and max_entries ({m}) >= 1")
    if not float(min_abs) >= 0.0:
        raise RuntimeError(f"local_explain: min_abs must be >= 0, got {min_abs}")
    ldw = weight.stride(0) if k > 1 else max(weight.stride(0), p)
    i32 = dict(device=dev, dtype=torch.int32)
    f32 = dict(device=dev, dtype=torch.float32)
    res = (torch.empty((b, c), **i32), torch.empty((b, c), **f32), torch.empty((b, c), **i32),
           torch.empty((b, c, m), **i32), torch.empty((b, c, m), **f32), torch.empty((b, c, m), **f32),
           torch.empty((b, c, m), **f32), torch.empty((b, c, m), **i32))
    if b == 0:
        return res
    _lib.call("pipnet_local_explain_f32", pooled.data_ptr(), loc.data_ptr(), out.data_ptr(), weight.data_ptr(), ldw,
              b, p, k, c, m, float(min_abs), *[t.data_ptr() for t in res], _stream(pooled))
    return res


def softmax_pool_linear(feat_nhwc: Tensor, w: Tensor, bias: Optional[Tensor], thresh: Optional[float],
                        out=None) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """The PIP-Net head in one launch (pipnet.py:33-37): fp32 or bf16 logits [B,h,w,P] ->
    (proto [B,h,w,P], pooled [B,P], x' [B,P], logits [B,K]) with x' = where(pooled < thresh, 0,
    pooled) (or pooled when ``thresh`` is None) and logits = x' relu(w)^T + bias, w read at call
    time.  ``out`` = (proto, pooled, x', logits) to write into (batch slices of a larger output).
    Bitwise equal to softmax_pool(..., 0) + nonneg_linear.  Under HIP-graph capture the call keeps
    using the capture stream's cached scratch (one graph node): serialise replays with eager calls
    on that stream."""
    bf = feat_nhwc.dtype == torch.bfloat16
    _operand("softmax_pool_linear", "prototype logits", feat_nhwc, dtype=torch.bfloat16 if bf else torch.float32)
    b, h, wd, p = feat_nhwc.shape
    dev = feat_nhwc.device
    if w.dim() != 2 or w.shape[1] != p:
        raise RuntimeError(f"softmax_pool_linear: weight {tuple(w.shape)} vs {p} prototypes")
    _operand("softmax_pool_linear", "classifier weight", w, device=dev)
    k = w.shape[0]
    _operand("softmax_pool_linear", "bias", bias, shape=k, device=dev, optional=True)
    if out is None:
        proto, pooled = _head_out(None, b, h, wd, p, dev)
        x_out = torch.empty((b, p), device=dev, dtype=torch.float32)
        logits = torch.empty((b, k), device=dev, dtype=torch.float32)
    else:
        proto, pooled = _head_out((out[0], out[1]), b, h, wd, p, dev)
        x_out, logits = out[2], out[3]
        _operand("softmax_pool_linear", "classifier input out", x_out, shape=(b, p), device=dev)
        _operand("softmax_pool_linear", "logits out", logits, shape=(b, k), device=dev)
    part, tickets = _head_workspace(dev, _stream(feat_nhwc), int(_lib.load().pipnet_softmax_pool_linear_part_floats(
        b, h * wd, p)), b)
    _lib.call("pipnet_softmax_pool_linear_bf16" if bf else "pipnet_softmax_pool_linear_f32", feat_nhwc.data_ptr(), b,
              h * wd, p, proto.data_ptr(), pooled.data_ptr(), w.data_ptr(), _ptr(bias), k,
              0 if thresh is None else 1, 0.0 if thresh is None else float(thresh), x_out.data_ptr(),
              logits.data_ptr(), part.data_ptr(), tickets.data_ptr(), _stream(feat_nhwc))
    return proto, pooled, x_out, logits


# Fused-head scratch, one (running maxima, tickets) pair per (device, stream): both are zeroed once
# here and left zero by every completed launch (include/pipnet_amd.h), so
# the head needs no memset per call; per stream because two concurrent heads (the split forward's
# sub-batch streams) must not share them.  Buffers only grow; a grown one is allocated (zeroed) on
# the stream that uses it.
_HEAD_WS = {}


def _head_workspace(dev: torch.device, stream: int, nfloats: int, b: int) -> Tuple[Tensor, Tensor]:
    key = (dev.index, stream)
    # A capture reuses this stream's cached scratch when it is large enough (so the captured head
    # stays ONE graph node: a graph-owned buffer would add its zero-fill nodes).  The graph then
    # shares the scratch -- and its self-resetting tickets -- with eager calls on the capture
    # stream: replays must be serialised with such calls (replay on the capture stream, or
    # synchronise first); a replay on another stream racing an eager call would corrupt both.
    part, tickets = _HEAD_WS.get(key, (None, None))
    capturing = torch.cuda.is_current_stream_capturing()
    if part is None or part.numel() < nfloats:
        part = torch.zeros(max(nfloats, 4), device=dev, dtype=torch.float32)
    if tickets is None or tickets.numel() < b:
        tickets = torch.zeros(max(b, 64), device=dev, dtype=torch.int32)
    if not capturing:          # graph-owned buffers (their zero-fill replays with them) are never cached
        _HEAD_WS[key] = (part, tickets)
    return part, tickets


def nonneg_linear(x: Tensor, w: Tensor, bias: Optional[Tensor], thresh: Optional[float],
                  out=None) -> Tuple[Tensor, Tensor]:
    """(x', out) with x' = where(x < thresh, 0, x) (or x) and out = x' relu(w)^T + bias.
    ``out`` = (x', logits) to write into."""
    _chk_rows("nonneg_linear", x, "classifier input", 2)
    b, d = x.shape
    k = w.shape[0]
    _operand("nonneg_linear", "classifier weight", w, shape=(k, d), device=x.device)
    _operand("nonneg_linear", "bias", bias, shape=k, device=x.device, optional=True)
    if out is None:
        x_out = torch.empty_like(x)
        out = torch.empty((b, k), device=x.device, dtype=torch.float32)
    else:
        x_out, out = out
        _operand("nonneg_linear", "classifier input out", x_out, shape=(b, d), device=x.device)
        _operand("nonneg_linear", "logits out", out, shape=(b, k), device=x.device)
    _lib.call("pipnet_nonneg_linear_f32", x.data_ptr(), b, d, w.data_ptr(), _ptr(bias), k,
              0 if thresh is None else 1, 0.0 if thresh is None else float(thresh), x_out.data_ptr(),
              out.data_ptr(), _stream(x))
    return x_out, out


def count_gumbel(logits_nhwc: Tensor, tau: float, exp_noise_nchw: Optional[Tensor], seed: int,
                 offset: int = 0, out=None) -> Tuple[Tensor, Tensor]:
    """Hard Gumbel-softmax one-hot map [B,h,w,P] + int32 histogram [B,P].  ``offset`` (Philox
    blocks) shifts the noise stream: image b0 of a batch starts at b0*h*w*P/4.  ``out`` =
    (proto, hist) to write into (batch slices of a larger output)."""
    _chk(logits_nhwc, "prototype logits")
    b, h, w, p = logits_nhwc.shape
    _operand("count_gumbel", "exp noise", exp_noise_nchw, shape=(b, p, h, w), device=logits_nhwc.device,
             optional=True)
    proto, hist = _gumbel_out(out, logits_nhwc)
    _lib.call("pipnet_count_gumbel_f32", logits_nhwc.data_ptr(), b, h * w, p, float(tau), _ptr(exp_noise_nchw),
              int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), proto.data_ptr(), hist.data_ptr(),
              _stream(logits_nhwc))
    return proto, hist


def _gumbel_out(out, logits_nhwc: Tensor) -> Tuple[Tensor, Tensor]:
    """Caller-provided (proto [B,h,w,P] float32, hist [B,P] int32) contiguous outputs, or new ones."""
    b, h, w, p = logits_nhwc.shape
    if out is None:
        return torch.empty_like(logits_nhwc), torch.empty((b, p), device=logits_nhwc.device, dtype=torch.int32)
    proto, hist = out
    _operand("count_gumbel", "proto out", proto, shape=(b, h, w, p), device=logits_nhwc.device)
    _operand("count_gumbel", "hist out", hist, dtype=torch.int32, shape=(b, p), device=logits_nhwc.device)
    return proto, hist


def count_gumbel_soft(logits_nhwc: Tensor, tau: float, exp_noise_nchw: Optional[Tensor], seed: int,
                      offset: int = 0) -> Tuple[Tensor, Tensor]:
    """Train-mode (soft) Gumbel-softmax map [B,h,w,P] + fp32 spatial sums (raw counts) [B,P]."""
    _chk(logits_nhwc, "prototype logits")
    b, h, w, p = logits_nhwc.shape
    _operand("count_gumbel_soft", "exp noise", exp_noise_nchw, shape=(b, p, h, w), device=logits_nhwc.device,
             optional=True)
    proto = torch.empty_like(logits_nhwc)
    sums = torch.empty((b, p), device=logits_nhwc.device, dtype=torch.float32)
    _lib.call("pipnet_count_gumbel_soft_f32", logits_nhwc.data_ptr(), b, h * w, p, float(tau), _ptr(exp_noise_nchw),
              int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), proto.data_ptr(), sums.data_ptr(),
              _stream(logits_nhwc))
    return proto, sums


def nonneg_linear_dx(d_out: Tensor, w: Tensor) -> Tensor:
    """d_out [N,K] relu(w [K,D]) -> [N,D] (NonNegLinear input gradient)."""
    _chk_rows("nonneg_linear_dx", d_out, "d_out", 2)
    n, k = d_out.shape
    if w.dim() != 2 or w.shape[0] != k:
        raise RuntimeError(f"nonneg_linear_dx: d_out {tuple(d_out.shape)} vs W {tuple(w.shape)}")
    _operand("nonneg_linear_dx", "classifier weight", w, device=d_out.device)
    dx = torch.empty((n, w.shape[1]), device=d_out.device, dtype=torch.float32)
    _lib.call("pipnet_nonneg_linear_dx_f32", d_out.data_ptr(), w.data_ptr(), n, w.shape[1], k, dx.data_ptr(),
              _stream(d_out))
    return dx


def bilinear_bwd_prep(g: Tensor, u: Tensor, v: Tensor) -> Tuple[Tensor, Tensor]:
    """(g * v, g * u) for out = u * v."""
    _operand("bilinear_bwd_prep", "grad", g)
    _chk_same("bilinear_bwd_prep", g, **{"W(e)": u, "V(e)": v})
    du, dv = torch.empty_like(g), torch.empty_like(g)
    _lib.call("pipnet_bilinear_bwd_prep_f32", g.data_ptr(), u.data_ptr(), v.data_ptr(), g.numel(), du.data_ptr(),
              dv.data_ptr(), _stream(g))
    return du, dv


ONEHOT_STRATEGY = {None: 0, "none": 0, "current_grad": 1, "max_grad": 2}


def count_ste_backward(counts: Tensor, d_clamped: Tensor, max_count: int, use_ste: bool, gated: bool) -> Tensor:
    """d raw counts from d clamped counts through STE_Round / ClampSTE (count_pipnet.py:90-97)."""
    _operand("count_ste_backward", "counts", counts)
    _operand("count_ste_backward", "d clamped counts", d_clamped, shape=counts.shape, device=counts.device)
    d = torch.empty_like(counts)
    _lib.call("pipnet_count_ste_bwd_f32", counts.data_ptr(), counts.numel(), int(max_count), int(bool(use_ste)),
              int(bool(gated)), d_clamped.data_ptr(), d.data_ptr(), _stream(counts))
    return d


def onehot_ste_backward(x: Tensor, g: Tensor, strategy: Optional[str] = None, respect_active: bool = False) -> Tensor:
    """ModifiedSTEFunction.backward (count_pipnet_utils.py:226-321): x [B,P] encoder input,
    g [B,P*M] (or [B,P,M]) encoding gradient -> d x [B,P]."""
    _operand("onehot_ste_backward", "encoder input", x)
    _operand("onehot_ste_backward", "encoding gradient", g, device=x.device)
    b, p = x.shape
    if g.numel() % max(x.numel(), 1) or g.shape[0] != b:
        raise RuntimeError(f"onehot_ste_backward: x {tuple(x.shape)} vs grad {tuple(g.shape)}")
    if strategy not in ONEHOT_STRATEGY:
        raise ValueError(f"Unknown positive_grad_strategy {strategy!r}")
    m = g.numel() // max(x.numel(), 1)
    dx = torch.empty_like(x)
    flag = torch.empty(1, device=x.device, dtype=torch.int32)
    _lib.call("pipnet_onehot_ste_bwd_f32", x.data_ptr(), x.numel(), m, g.data_ptr(), ONEHOT_STRATEGY[strategy],
              int(bool(respect_active)), flag.data_ptr(), dx.data_ptr(), _stream(x))
    return dx


def linear_intermediate_backward(x: Tensor, g: Tensor, w: Tensor, want_dx: bool = True,
                                 dw_out: Optional[Tensor] = None) -> Tuple[Optional[Tensor], Tensor]:
    """LinearIntermediate backward (count_pipnet_utils.py:471-519): x [B,P] counts, g [B,P*E]
    output gradient, w [E,1] -> (d x [B,P] or None, d w [E,1])."""
    fn = "linear_intermediate_backward"
    _operand(fn, "input", x)
    e = w.numel()
    if g.dim() < 1 or g.shape[0] != x.shape[0]:
        raise RuntimeError(f"{fn}: x {tuple(x.shape)}, grad {tuple(g.shape)}, E={e}")
    _operand(fn, "output gradient", g, shape=x.numel() * e, device=x.device)
    wv = w.detach().reshape(-1).contiguous()
    _operand(fn, "weight", wv, device=x.device)
    _operand(fn, "dw_out", dw_out, shape=e, device=x.device, optional=True)
    dx = torch.empty_like(x) if want_dx else None
    dw = torch.empty(e, 1, device=x.device, dtype=torch.float32) if dw_out is None else dw_out
    part = torch.empty(int(_lib.load().pipnet_linear_inter_partials_floats(e)), device=x.device,
                       dtype=torch.float32)
    _lib.call("pipnet_linear_inter_bwd_f32", x.data_ptr(), x.numel(), e, g.data_ptr(), wv.data_ptr(),
              dx.data_ptr() if dx is not None else None, dw.data_ptr(), 0, part.data_ptr(), _stream(x))
    return dx, dw


def count_head_backward(proto_nhwc: Tensor, counts: Tensor, d_counts: Optional[Tensor], w_align: float,
                        w_tanh: float, tanh_coeff: float, tau: float, counts_all: Optional[Tensor] = None) -> Tensor:
    """d loss / d logits of the CountPIPNet head (soft Gumbel-softmax / softmax, spatial sum)
    for the align / tanh terms of calculate_loss plus the classifier chain's d counts.  ``counts_all``
    [2 Bh_all, P]: the operands are one rank's rows of a batch whose raw counts these are
    (pipnet_count_head_bwd_rows_f32)."""
    _chk_rows("count_head_backward", proto_nhwc, "proto features", 4)
    n, h, ww, p = proto_nhwc.shape
    if n % 2:
        raise RuntimeError(f"count_head_backward: the batch holds both views, so it must be even (got {n})")
    _operand("count_head_backward", "counts", counts, shape=(n, p), device=proto_nhwc.device)
    _operand("count_head_backward", "d counts", d_counts, shape=(n, p), device=proto_nhwc.device, optional=True)
    d_logits = torch.empty_like(proto_nhwc)
    dcnt = torch.empty((n, p), device=proto_nhwc.device, dtype=torch.float32)
    if counts_all is not None:
        bh_all = _chk_all_rows("count_head_backward", counts, counts_all)
        tcoef = torch.empty((2, p), device=proto_nhwc.device, dtype=torch.float32)
        _lib.call("pipnet_count_head_bwd_rows_f32", proto_nhwc.data_ptr(), counts.data_ptr(), n // 2, h * ww, p,
                  _ptr(d_counts), counts_all.data_ptr(), bh_all, float(w_align), float(w_tanh), float(tanh_coeff),
                  1.0 / float(tau), dcnt.data_ptr(), tcoef.data_ptr(), d_logits.data_ptr(), _stream(proto_nhwc))
        return d_logits
    _lib.call("pipnet_count_head_bwd_f32", proto_nhwc.data_ptr(), counts.data_ptr(), n // 2, h * ww, p,
              _ptr(d_counts), float(w_align), float(w_tanh), float(tanh_coeff), 1.0 / float(tau), dcnt.data_ptr(),
              d_logits.data_ptr(), _stream(proto_nhwc))
    return d_logits


def philox_exp1(seed: int, offset: int, n: int, device, log_e: bool = False) -> Tensor:
    """The Gumbel heads' Exp(1) draw on its own (pipnet_philox_exp1_f32): element i = the value
    count_gumbel uses for element i of its NHWC [B, HW, P] stream under (seed, offset) -- E, or
    log E on the hard head's hardware-log form.  For parity tests (oracle/philox_ref.py)."""
    if n % 4:
        raise RuntimeError(f"philox_exp1: n = {n} must be a multiple of 4")
    out = torch.empty(n, device=device, dtype=torch.float32)
    require_device(out, "philox output")
    _lib.call("pipnet_philox_exp1_f32", int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), n, int(log_e),
              out.data_ptr(), _stream(out))
    return out


def count_gumbel_devseed(logits_nhwc: Tensor, tau: float, seed_state: Tensor, out=None) -> Tuple[Tensor, Tensor]:
    """count_gumbel with the Philox key in device memory (seed_state: int64[2] on the device),
    advanced on the stream per call -- the form a captured HIP graph replays.  ``out`` as there."""
    _chk(logits_nhwc, "prototype logits")
    _operand("count_gumbel_devseed", "seed_state", seed_state, dtype=torch.int64, shape=2,
             device=logits_nhwc.device)
    b, h, w, p = logits_nhwc.shape
    proto, hist = _gumbel_out(out, logits_nhwc)
    _lib.call("pipnet_count_gumbel_devseed_f32", logits_nhwc.data_ptr(), b, h * w, p, float(tau),
              seed_state.data_ptr(), proto.data_ptr(), hist.data_ptr(), _stream(logits_nhwc))
    return proto, hist


def count_finish(hist: Optional[Tensor], sums: Optional[Tensor], max_count: int, do_round: bool) -> Tuple[Tensor, Tensor]:
    ref = hist if hist is not None else sums
    _operand("count_finish", "hist", hist, dtype=torch.int32, optional=True)
    _operand("count_finish", "sums", sums, shape=ref.shape, device=ref.device, optional=hist is not None)
    b, p = ref.shape
    raw = torch.empty((b, p), device=ref.device, dtype=torch.float32)
    clamped = torch.empty_like(raw)
    _lib.call("pipnet_count_finish_f32", _ptr(hist), _ptr(sums), b, p, int(max_count), int(do_round),
              raw.data_ptr(), clamped.data_ptr(), _stream(ref))
    return raw, clamped


def count_encode(x: Tensor, c: int, kind: int, do_round: bool, w: Optional[Tensor] = None) -> Tensor:
    _chk_rows("count_encode", x, "counts", 2)
    b, p = x.shape
    _operand("count_encode", "w", w, shape=c, device=x.device, optional=kind != 1)
    out = torch.empty((b, p * c), device=x.device, dtype=torch.float32)
    _lib.call("pipnet_count_encode_f32", x.data_ptr(), b, p, c, kind, int(do_round), _ptr(w), out.data_ptr(),
              _stream(x))
    return out


# ---- eval_pipnet metric loop ------------------------------------------------------------

def _mutated(*ts: Tensor) -> None:
    """A kernel wrote these tensors through raw pointers: bump their in-place version
    counters, as a torch in-place op would, so version-keyed caches (packed weights) and
    autograd's saved-tensor checks see the change."""
    for t in ts:
        torch.autograd.graph.increment_version(t)


def weight_sparsify_(w: Tensor, delta: float = 1e-3) -> Tensor:
    """In place: w = max(w - delta, 0) (pipnet/test.py:73)."""
    _chk(w, "classification weight")
    _lib.call("pipnet_weight_sparsify_f32", w.data_ptr(), w.numel(), delta, _stream(w))
    _mutated(w)
    return w


def eval_batch(pooled: Tensor, out: Tensor, w: Tensor, ys: Tensor, multiplier: Optional[Tensor], thr: float,
               cm: Tensor, acc: Tensor, abstained: Tensor) -> Tuple[Tensor, Tensor]:
    """One eval_pipnet batch on the device; accumulates into cm [K,K] int64, acc [5] fp64,
    abstained [1] int64.  Returns (ys_pred [B] int32, score [B] fp32)."""
    _chk_rows("eval_batch", out, "logits", 2)
    b, k = out.shape
    dev, i64 = out.device, torch.int64
    p = pooled.shape[-1]
    for what, t, dtype, shape in (("pooled", pooled, torch.float32, (b, p)), ("weights", w, torch.float32, (k, p)),
                                  ("labels", ys, i64, (b,)), ("multiplier", multiplier, torch.float32, 1),
                                  ("cm", cm, i64, (k, k)), ("acc", acc, torch.float64, 5),
                                  ("abstained", abstained, i64, 1)):
        _operand("eval_batch", what, t, dtype=dtype, shape=shape, device=dev, optional=what == "multiplier")
    ys_pred = torch.empty(b, device=out.device, dtype=torch.int32)
    score = torch.empty(b, device=out.device, dtype=torch.float32)
    ws = torch.empty(5 * b + k, device=out.device, dtype=torch.int32)
    _lib.call("pipnet_eval_batch_f32", pooled.data_ptr(), out.data_ptr(), w.data_ptr(), b, p, k, ys.data_ptr(),
              _ptr(multiplier), thr, ys_pred.data_ptr(), score.data_ptr(), cm.data_ptr(), acc.data_ptr(),
              abstained.data_ptr(), ws.data_ptr(), _stream(out))
    return ys_pred, score


# ---- evaluation input transform (util/data.py transform_no_augment) ----------------------

def _ragged_batch(fn: str, pixels: Tensor, offsets: Tensor, sizes: Tensor, sizes_host):
    """The checked operands of a ragged batch of packed HWC uint8 images: (host [B,2] int32 size table, B)."""
    import numpy as np
    _operand(fn, "pixels", pixels, dtype=torch.uint8)
    sizes_np = np.ascontiguousarray(np.asarray(sizes_host, dtype=np.int32).reshape(-1, 2))
    b = sizes_np.shape[0]
    _operand(fn, "offsets", offsets, dtype=torch.int64, shape=(b,), device=pixels.device)
    _operand(fn, "sizes", sizes, dtype=torch.int32, shape=(b, 2), device=pixels.device)
    return sizes_np, b


def resize_normalize_rgb8(pixels: Tensor, offsets: Tensor, sizes: Tensor, sizes_host, out_hw: Tuple[int, int],
                          mean, std, grayscale: bool = False, want_u8: bool = False):
    """Resize(out_hw, BILINEAR) [+ Grayscale(3)] + ToTensor + Normalize of a ragged batch of
    decoded RGB images packed HWC uint8 on the device (image b at byte offsets[b], shape
    sizes[b] = (h, w)); ``sizes_host`` is the same [B,2] int32 table on the host.
    Returns [B,3,oh,ow] fp32 (and the [B,oh,ow,3] uint8 resized image when ``want_u8``)."""
    sizes_np, b = _ragged_batch("resize_normalize_rgb8", pixels, offsets, sizes, sizes_host)
    oh, ow = int(out_hw[0]), int(out_hw[1])
    kmax, wsb = ctypes.c_int(0), ctypes.c_int64(0)
    _lib.call("pipnet_resize_plan", sizes_np.ctypes.data, b, oh, ow, ctypes.byref(kmax), ctypes.byref(wsb))
    dev = pixels.device
    out = torch.empty((b, 3, oh, ow), device=dev, dtype=torch.float32)
    out_u8 = torch.empty((b, oh, ow, 3), device=dev, dtype=torch.uint8) if want_u8 else None
    ws = torch.empty(max(1, wsb.value // 4), device=dev, dtype=torch.int32)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in std])
    _lib.call("pipnet_resize_normalize_rgb8", pixels.data_ptr(), offsets.data_ptr(), sizes.data_ptr(), b, oh, ow,
              kmax.value, int(bool(grayscale)), m, s, ws.data_ptr(), out.data_ptr(), _ptr(out_u8),
              torch.cuda.current_stream(dev).cuda_stream)
    return (out, out_u8) if want_u8 else out


# ---- explanation images (csrc/gallery_ops.hip) --------------------------------------------------

def _host_i32(fn: str, what: str, t, cols: Optional[int]):
    """A host table of integers as a contiguous int32 numpy array ([N, cols], or [N] without ``cols``)."""
    import numpy as np
    a = np.asarray(t.cpu() if torch.is_tensor(t) else t)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise RuntimeError(f"{fn}: {what} must hold integers, got {a.dtype}")
    a = a.astype(np.int64).reshape((-1, cols) if cols else (-1,))
    if a.size and np.abs(a).max() >= 1 << 30:
        raise RuntimeError(f"{fn}: {what} out of range")
    return np.ascontiguousarray(a.astype(np.int32))


def _frames(fn: str, what: str, t: Tensor, device=None) -> None:
    _operand(fn, what, t, dtype=torch.uint8, device=device)
    if t.dim() != 4 or t.shape[3] != 3 or t.shape[1] < 1 or t.shape[2] < 1:
        raise RuntimeError(f"{fn}: {what} must be [N,H,W,3] uint8 with H, W >= 1, got {tuple(t.shape)}")


def patch_compose_rgb8(frames: Tensor, items, canvases: Tensor) -> Tensor:
    """``canvases[canvas, y:, x:] = frames[frame, h0:min(h1, fh), w0:min(w1, fw)]`` for every row
    (frame, h0, h1, w0, w1, canvas, y, x) of the host integer table ``items`` [N,8], in one launch (none for
    N == 0).  ``frames`` [F,fh,fw,3] and ``canvases`` [C,ch,cw,3] are uint8 on one device; the canvases are
    written in place and returned.  A window that runs past the frame is cut short, as a Python slice is.  Every
    row is held against both shapes first -- non-negative origins, frame < F, canvas < C, the cut window fits at
    (y, x) -- and a row that fails raises RuntimeError before anything is launched."""
    fn = "patch_compose_rgb8"
    import numpy as np
    _frames(fn, "frames", frames)
    _frames(fn, "canvases", canvases, frames.device)
    it = _host_i32(fn, "items", items, 8)
    n = it.shape[0]
    if n == 0:
        return canvases
    (f, fh, fw), (c, ch, cw) = frames.shape[:3], canvases.shape[:3]
    rows = np.minimum(it[:, 2], fh) - it[:, 1]
    cols = np.minimum(it[:, 4], fw) - it[:, 3]
    bad = ((it[:, [0, 1, 3, 5, 6, 7]] < 0).any(axis=1) | (it[:, 0] >= f) | (it[:, 5] >= c) |
           (it[:, 6] + np.maximum(rows, 0) > ch) | (it[:, 7] + np.maximum(cols, 0) > cw))
    if bad.any():
        i = int(np.argmax(bad))
        raise RuntimeError(f"{fn}: item {i} {tuple(int(v) for v in it[i])} leaves the frames {tuple(frames.shape)} "
                           f"or the canvases {tuple(canvases.shape)}")
    dev = frames.device
    it_dev = torch.from_numpy(it).to(dev, non_blocking=True)
    _lib.call("pipnet_patch_compose_rgb8", frames.data_ptr(), f, fh, fw, it_dev.data_ptr(), n, canvases.data_ptr(), c,
              ch, cw, torch.cuda.current_stream(dev).cuda_stream)
    return canvases


YELLOW = (255, 255, 0)          # PIL's 'yellow'


def rect_outline_check(rects, width: int) -> None:
    """ValueError unless every (x0, y0, x1, y1) row spans at least ``2 * width + 1`` pixels each way: the
    outline rule of ``draw_rects_rgb8`` is Pillow's from there on only."""
    import numpy as np
    r = np.asarray(rects, dtype=np.int64).reshape(-1, 4)
    if width < 1:
        raise ValueError(f"draw_rects_rgb8: the line width must be at least 1, got {width}")
    small = (r[:, 2] - r[:, 0] + 1 < 2 * width + 1) | (r[:, 3] - r[:, 1] + 1 < 2 * width + 1)
    if small.any():
        i = int(np.argmax(small))
        raise ValueError(f"draw_rects_rgb8: rectangle {i} {tuple(int(v) for v in r[i])} is narrower than "
                         f"2 * width + 1 = {2 * width + 1} pixels; Pillow draws such a box otherwise")


def draw_rects_rgb8(frames: Tensor, src, rects, width: int = 2, colour=YELLOW) -> Tensor:
    """[N,fh,fw,3] uint8: ``out[n]`` is ``frames[src[n]]`` with the outline that Pillow's
    ``ImageDraw.rectangle([(x0, y0), (x1, y1)], outline=colour, width=width)`` draws for
    ``rects[n] = (x0, y0, x1, y1)``, clipped to the frame (``x1 == fw`` is legal).  ``src`` [N] and ``rects``
    [N,4] are host integer tables.  A box narrower than ``2 * width + 1`` raises ValueError (Pillow's outline
    follows another rule there), a frame index out of range RuntimeError; nothing is launched then."""
    fn = "draw_rects_rgb8"
    _frames(fn, "frames", frames)
    s = _host_i32(fn, "src", src, None)
    r = _host_i32(fn, "rects", rects, 4)
    n = s.shape[0]
    if r.shape[0] != n:
        raise RuntimeError(f"{fn}: {n} frame indices but {r.shape[0]} rectangles")
    width = int(width)
    rect_outline_check(r, width)
    col = tuple(int(v) for v in colour)
    if len(col) != 3 or not all(0 <= v <= 255 for v in col) or width >= 1 << 30:
        raise RuntimeError(f"{fn}: colour must be three values in 0..255 (got {colour}), width below 2^30")
    f, fh, fw = frames.shape[:3]
    if n and (int(s.min()) < 0 or int(s.max()) >= f):
        raise RuntimeError(f"{fn}: a frame index lies outside the {f} frames")
    dev = frames.device
    out = torch.empty((n, fh, fw, 3), device=dev, dtype=torch.uint8)
    if n == 0:
        return out
    s_dev = torch.from_numpy(s).to(dev, non_blocking=True)
    r_dev = torch.from_numpy(r).to(dev, non_blocking=True)
    _lib.call("pipnet_draw_rects_rgb8", frames.data_ptr(), f, fh, fw, s_dev.data_ptr(), r_dev.data_ptr(), n, width,
              *col, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return out


# ---- prototype similarity heatmaps (csrc/heatmap_ops.hip) ---------------------------------------
BICUBIC_TAPS = 5                # coefficients per row of an upscale: 2 * support + 1
HEATMAP_WEIGHTS = (0.2, 0.6)    # visualize_prediction.py:99


def _bicubic(x: float) -> float:
    """Pillow's bicubic filter (a = -0.5, support 2), in doubles."""
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


@functools.lru_cache(maxsize=256)
def _bicubic_rows(in_size: int, out_size: int) -> Tuple[Tuple[int, ...], ...]:
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ss = 1.0 / filterscale
    rows = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        k = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in k:                         # a sequential sum, as the C loop's
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        q = [int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22)) for v in k]
        assert n <= BICUBIC_TAPS, (in_size, out_size, xx, n)
        rows.append((xmin, n) + tuple(q) + (0,) * (BICUBIC_TAPS - n))
    return tuple(rows)


def bicubic_rows(in_size: int, out_size: int) -> Tensor:
    """int32 [out_size, 2 + 5] on the host: per output coordinate the row (xmin, n, k[0..5)) of Pillow's
    ``ImagingResample`` with ``BICUBIC`` for an 8-bit axis resized ``in_size`` -> ``out_size``: ``precompute_coeffs``
    in Python doubles (sequential sums, weights normalised by their sum), then 22-bit fixed point rounded half away
    from zero (``normalize_coeffs_8bpc``).  Upscale only (``1 <= in_size <= out_size``): a row then has at most 5
    coefficients.  ``pipnet_heatmap_rgb8`` reads these tables; tests/test_heatmap_cpu.py holds them against Pillow."""
    in_size, out_size = int(in_size), int(out_size)
    if not 1 <= in_size <= out_size:
        raise ValueError(f"bicubic_rows: only 1 <= in_size <= out_size is supported, got {in_size} -> {out_size}")
    return torch.tensor(_bicubic_rows(in_size, out_size), dtype=torch.int32).reshape(out_size, 2 + BICUBIC_TAPS)


_BICUBIC_DEV = {}


def _bicubic_rows_on(in_size: int, out_size: int, dev: torch.device) -> Tensor:
    """``bicubic_rows`` on ``dev``, uploaded once per (sizes, device)."""
    key = (int(in_size), int(out_size), dev)
    t = _BICUBIC_DEV.get(key)
    if t is None:
        t = _BICUBIC_DEV[key] = bicubic_rows(in_size, out_size).to(dev)
    return t


def heatmap_weights(weights) -> Tuple[float, float]:
    """(w_heat, w_img) as floats; ValueError unless both are >= 0 and their float32 sum is at most 1, the range in
    which ``plt.imsave`` accepts the blended image."""
    import numpy as np
    try:
        wh, wi = (float(v) for v in weights)
    except (TypeError, ValueError):
        raise ValueError(f"heatmap_rgb8: weights must be two numbers (w_heat, w_img), got {weights!r}") from None
    if not (wh >= 0 and wi >= 0 and np.float32(wh) + np.float32(wi) <= np.float32(1)):
        raise ValueError(f"heatmap_rgb8: weights must be >= 0 and sum to at most 1, got {weights!r}")
    return wh, wi


def heatmap_shapes(proto_nhwc: Tensor, frames: Tensor, lut: Tensor) -> Tuple[int, int, int, int, int, int]:
    """(B, h, w, P, F, S) of the operands of ``heatmap_rgb8``; ValueError where a dtype or a shape is not the
    documented one.  Attribute comparisons only, on any device."""
    fn = "heatmap_rgb8"
    for what, t in (("proto_nhwc", proto_nhwc), ("frames", frames), ("lut", lut)):
        if not torch.is_tensor(t):
            raise ValueError(f"{fn}: {what} must be a tensor, got {type(t).__name__}")
    if proto_nhwc.dtype != torch.float32 or proto_nhwc.dim() != 4 or min(proto_nhwc.shape[1:]) < 1:
        raise ValueError(f"{fn}: proto_nhwc must be float32 [B,h,w,P] with h, w, P >= 1, got {proto_nhwc.dtype} "
                         f"{tuple(proto_nhwc.shape)}")
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[1] != frames.shape[2] \
            or frames.shape[1] < 1:
        raise ValueError(f"{fn}: frames must be uint8 [F,S,S,3], got {frames.dtype} {tuple(frames.shape)}")
    if lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 3):
        raise ValueError(f"{fn}: lut must be uint8 [256,3] (RGB), got {lut.dtype} {tuple(lut.shape)}")
    b, h, w, p = proto_nhwc.shape
    f, s = frames.shape[:2]
    if h > s or w > s:
        raise ValueError(f"{fn}: the {h} x {w} map is larger than the {s} x {s} frame; only the upscale is supported")
    return b, h, w, p, f, s


def heatmap_rgb8(proto_nhwc: Tensor, frames: Tensor, items, lut: Tensor, *, weights=HEATMAP_WEIGHTS,
                 out: Optional[Tensor] = None, resized: Optional[Tensor] = None) -> Tensor:
    """[N,S,S,3] uint8: per row (b, p, frame) of the host integer table ``items`` [N,3] the ``heatmap_p{p}.png``
    pixels of visualize_prediction.py:92-100 -- the map ``proto_nhwc[b, :, :, p]`` quantised to bytes, resized to
    S x S as Pillow's ``BICUBIC`` does, looked up in ``lut`` [256,3] uint8 (RGB) and blended in float32 as
    ``weights[0] * colour / 255 + weights[1] * frames[frame] / 255``, then ``(v * 255).astype(uint8)``
    (pipnet_heatmap_rgb8; bit for bit).  ``proto_nhwc`` [B,h,w,P] float32 with ``h, w <= S``, ``frames`` [F,S,S,3]
    uint8, all dense and on one ROCm device.  ``out`` [N,S,S,3] uint8 and ``resized`` [N,S,S] uint8 (the bytes
    after the resize) are written when given.  A wrong dtype, shape or weight raises ValueError, a wrong device
    or layout or a row of ``items`` out of range RuntimeError; nothing is launched then.  ``items`` may also be
    an int32 [N,3] tensor already on the device (one upload for many launches): its rows cannot be read here, the
    caller has checked them, and the kernel writes nothing for a row out of range.  One launch (none for N == 0),
    on the current stream."""
    fn = "heatmap_rgb8"
    b, h, w, p, f, s = heatmap_shapes(proto_nhwc, frames, lut)
    wh, wi = heatmap_weights(weights)
    _operand(fn, "proto_nhwc", proto_nhwc)
    dev = proto_nhwc.device
    _frames(fn, "frames", frames, dev)
    _operand(fn, "lut", lut, dtype=torch.uint8, shape=torch.Size((256, 3)), device=dev)
    if torch.is_tensor(items) and items.is_cuda:       # a table already on the device: the caller has checked it
        if items.dim() != 2:
            raise RuntimeError(f"{fn}: a device table of items must be int32 [N,3], got shape {tuple(items.shape)}")
        _operand(fn, "items", items, dtype=torch.int32, shape=torch.Size((items.shape[0], 3)), device=dev)
        it_dev, n = items, items.shape[0]
    else:
        it = _host_i32(fn, "items", items, 3)
        n = it.shape[0]
        bad = (it < 0).any(axis=1) | (it[:, 0] >= b) | (it[:, 1] >= p) | (it[:, 2] >= f)
        if bad.any():
            i = int(bad.argmax())
            raise RuntimeError(f"{fn}: item {i} {tuple(int(v) for v in it[i])} lies outside the {b} images, {p} "
                               f"prototypes or {f} frames")
        it_dev = torch.from_numpy(it).to(dev, non_blocking=True) if n else None
    if out is None:
        out = torch.empty((n, s, s, 3), device=dev, dtype=torch.uint8)
    else:
        _operand(fn, "out", out, dtype=torch.uint8, shape=torch.Size((n, s, s, 3)), device=dev)
    _operand(fn, "resized", resized, dtype=torch.uint8, shape=torch.Size((n, s, s)), device=dev, optional=True)
    if n == 0:
        return out
    rows_h, rows_v = _bicubic_rows_on(w, s, dev), _bicubic_rows_on(h, s, dev)
    _lib.call("pipnet_heatmap_rgb8", proto_nhwc.data_ptr(), b, h, w, p, frames.data_ptr(), f, s, it_dev.data_ptr(), n,
              lut.data_ptr(), rows_h.data_ptr(), rows_v.data_ptr(), wh, wi, out.data_ptr(), _ptr(resized),
              torch.cuda.current_stream(dev).cuda_stream)
    return out


# ---- prototype feature-map overlays (csrc/overlay_ops.hip) ---------------------------------------
OVERLAY_ALPHA = 0.7             # vis_pipnet.py:475
MapOverlay = namedtuple("MapOverlay", "maps resized mask colour overlay")


def overlay_shapes(proto_nhwc: Tensor, lut: Tensor, size, alpha=OVERLAY_ALPHA) -> Tuple[int, int, int, int, int]:
    """(B, h, w, P, S) of the operands of ``map_overlay``; ValueError where a dtype, a shape, the size or alpha is not
    the documented one.  Attribute comparisons only, on any device."""
    fn = "map_overlay"
    for what, t in (("proto_nhwc", proto_nhwc), ("lut", lut)):
        if not torch.is_tensor(t):
            raise ValueError(f"{fn}: {what} must be a tensor, got {type(t).__name__}")
    if proto_nhwc.dtype != torch.float32 or proto_nhwc.dim() != 4 or min(proto_nhwc.shape[1:3]) < 3 or \
            proto_nhwc.shape[3] < 1:
        raise ValueError(f"{fn}: proto_nhwc must be float32 [B,h,w,P] with h, w >= 3 (a cubic spline needs three "
                         f"samples) and P >= 1, got {proto_nhwc.dtype} {tuple(proto_nhwc.shape)}")
    if lut.dtype != torch.float64 or tuple(lut.shape) != (256, 3):
        raise ValueError(f"{fn}: lut must be float64 [256,3] (RGB), got {lut.dtype} {tuple(lut.shape)}")
    if isinstance(size, bool) or not isinstance(size, numbers.Integral) or not 2 <= size < 1 << 14:
        raise ValueError(f"{fn}: size must be an integer in 2 .. 16383, got {size!r}")
    if isinstance(alpha, bool) or not isinstance(alpha, numbers.Real) or not 0.0 <= alpha <= 1.0:
        raise ValueError(f"{fn}: alpha must be a number in 0 .. 1, got {alpha!r}")
    b, h, w, p = proto_nhwc.shape
    # the library's own size rule: it holds the dimensions against its LDS budget before it looks at N == 0
    if _lib.load().pipnet_map_overlay(None, 0, h, w, p, None, 0, None, int(size), float(alpha), None, None, None, None,
                                      None, None) != 0:
        raise ValueError(f"{fn}: the {h} x {w} map does not fit the 64 KiB of LDS beside a row of {size} pixels")
    return b, h, w, p, int(size)


def map_overlay(proto_nhwc: Tensor, items, lut: Tensor, size: int, *, alpha: float = OVERLAY_ALPHA,
                out: Optional[MapOverlay] = None) -> MapOverlay:
    """Per row (b, p) of the host integer table ``items`` [N,2] the arrays behind the ``*_overlay.png`` of
    vis_pipnet.py:454-475: ``MapOverlay(maps [N,h,w] float32, resized [N,S,S] float32, mask [N,S,S] uint8, colour
    [N,S,S] uint8, overlay [N,S,S,4] float64)`` with S = ``size`` -- the map ``proto_nhwc[b, :, :, p]``, its
    ``scipy.ndimage.zoom`` to S x S, ``resized > 0.1``, the row of the 256-entry colour table ``cmap(resized)`` reads
    (0 off the mask) and ``(*lut[colour], alpha)`` on the mask, zeros elsewhere (pipnet_map_overlay; the arithmetic
    contract is in include/pipnet_amd.h, bit for bit tests/overlay_ref.py).  ``proto_nhwc`` [B,h,w,P] float32 with
    h, w >= 3 and ``lut`` [256,3] float64, dense and on one ROCm device.  ``out``: a ``MapOverlay`` of tensors to
    write into, None for a member that is not wanted (returned as given); without it all five are allocated.  A wrong
    dtype, shape, size or alpha raises ValueError, a wrong device or layout or a row of ``items`` out of range
    RuntimeError; nothing is launched then.  ``items`` may also be an int32 [N,2] tensor already on the device (one
    upload for many launches): its rows cannot be read here, the caller has checked them, and the kernel writes
    nothing for a row out of range.  One launch (none for N == 0), on the current stream."""
    fn = "map_overlay"
    b, h, w, p, s = overlay_shapes(proto_nhwc, lut, size, alpha)
    _operand(fn, "proto_nhwc", proto_nhwc)
    dev = proto_nhwc.device
    _operand(fn, "lut", lut, dtype=torch.float64, shape=torch.Size((256, 3)), device=dev)
    if torch.is_tensor(items) and items.is_cuda:       # a table already on the device: the caller has checked it
        if items.dim() != 2:
            raise RuntimeError(f"{fn}: a device table of items must be int32 [N,2], got shape {tuple(items.shape)}")
        _operand(fn, "items", items, dtype=torch.int32, shape=torch.Size((items.shape[0], 2)), device=dev)
        it_dev, n = items, items.shape[0]
    else:
        it = _host_i32(fn, "items", items, 2)
        n = it.shape[0]
        bad = (it < 0).any(axis=1) | (it[:, 0] >= b) | (it[:, 1] >= p)
        if bad.any():
            i = int(bad.argmax())
            raise RuntimeError(f"{fn}: item {i} {tuple(int(v) for v in it[i])} lies outside the {b} images or {p} "
                               f"prototypes")
        it_dev = torch.from_numpy(it).to(dev, non_blocking=True) if n else None
    spec = (("maps", torch.float32, (n, h, w)), ("resized", torch.float32, (n, s, s)), ("mask", torch.uint8, (n, s, s)),
            ("colour", torch.uint8, (n, s, s)), ("overlay", torch.float64, (n, s, s, 4)))
    if out is None:
        out = MapOverlay(*(torch.empty(shape, device=dev, dtype=dtype) for _, dtype, shape in spec))
    else:
        if not isinstance(out, MapOverlay):
            raise ValueError(f"{fn}: out must be a MapOverlay of tensors (None: not wanted), got {type(out).__name__}")
        for (what, dtype, shape), t in zip(spec, out):
            _operand(fn, what, t, dtype=dtype, shape=torch.Size(shape), device=dev, optional=True)
    if n == 0:
        return out
    _lib.call("pipnet_map_overlay", proto_nhwc.data_ptr(), b, h, w, p, it_dev.data_ptr(), n, lut.data_ptr(), s,
              float(alpha), *(_ptr(t) for t in out), torch.cuda.current_stream(dev).cuda_stream)
    return out


# ---- two-view training augmentation (csrc/augment_ops.hip) ----------------------------------
AUG_GEOM_PARAMS, AUG_VIEW_PARAMS = _lib.CONSTANTS["AUG_GEOM_PARAMS"], _lib.CONSTANTS["AUG_VIEW_PARAMS"]
AUG_OP_SHARPNESS, AUG_OP_LAST = 4, 8


def _host_params(t, shape, what: str) -> Tensor:
    t = torch.as_tensor(t)
    if t.is_cuda or t.dtype != torch.float64 or tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{what}: expected a host float64 tensor of shape {tuple(shape)}, got "
                           f"{t.dtype} {tuple(t.shape)} on {t.device}")
    if not bool(torch.isfinite(t).all()):
        raise RuntimeError(f"{what}: parameters must be finite")
    return t.contiguous()


def augment_geometry_rgb8(pixels: Tensor, offsets: Tensor, sizes: Tensor, sizes_host, gparams, s1: int,
                          s2: int) -> Tensor:
    """transform1 of the reference's training sets on a ragged batch packed as for
    ``resize_normalize_rgb8``: Resize((s1, s1)) -> affine warp (NEAREST) -> flip ->
    crop(box).resize((s2, s2), BILINEAR).  ``gparams`` is the host [B,13] float64 table of
    include/pipnet_amd.h (augment.sample_params draws it).  Returns [B,s2,s2,3] uint8."""
    sizes_np, b = _ragged_batch("augment_geometry_rgb8", pixels, offsets, sizes, sizes_host)
    s1, s2 = int(s1), int(s2)
    gp = _host_params(gparams, (b, AUG_GEOM_PARAMS), "augment_geometry_rgb8 gparams")
    if b:
        top, left, ch, cw = (gp[:, k] for k in range(9, 13))
        if bool(((top < 0) | (left < 0) | (ch < 1) | (cw < 1) | (top + ch > s1) | (left + cw > s1)).any()):
            raise RuntimeError(f"augment_geometry_rgb8: a crop box leaves the {s1}x{s1} image")
        if bool(((ch > 100 * cw) & (ch > s2)).any()):
            raise RuntimeError("augment_geometry_rgb8: crop boxes taller than 100x their width are not supported")
        if bool((gp[:, 1:7].abs() >= 16384).any()) or bool(((gp[:, 0] < 0) | (gp[:, 0] > 2)).any()):
            raise RuntimeError("augment_geometry_rgb8: affine matrix out of range")
    dev = pixels.device
    kmax1, kmax2, wsb = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
    _lib.call("pipnet_augment_geometry_plan", sizes_np.ctypes.data, b, s1, s2, ctypes.byref(kmax1),
              ctypes.byref(kmax2), ctypes.byref(wsb))
    out = torch.empty((b, s2, s2, 3), device=dev, dtype=torch.uint8)
    ws = torch.empty(max(1, wsb.value // 4), device=dev, dtype=torch.int32)
    gp_dev = gp.to(dev, non_blocking=True)
    _lib.call("pipnet_augment_geometry_rgb8", pixels.data_ptr(), offsets.data_ptr(), sizes.data_ptr(),
              gp_dev.data_ptr(), b, s1, s2, kmax1.value, kmax2.value, ws.data_ptr(), out.data_ptr(),
              torch.cuda.current_stream(dev).cuda_stream)
    return out


def augment_view_rgb8(images: Tensor, vparams, s: int, mean, std, grayscale: bool = False, noise_std: float = 0.1,
                      seed: int = 0, noise: Optional[Tensor] = None) -> Tensor:
    """transform2 of the reference's training sets, once per view: colour operation(s) ->
    RandomCrop(s) -> [Grayscale(3)] -> ToTensor -> [+ noise] -> Normalize.  ``images``
    [B,S2,S2,3] uint8 (augment_geometry_rgb8's output), ``vparams`` the host [V,B,8] float64
    table of include/pipnet_amd.h.  ``noise`` [V,B,3,s,s] injects the addends of the flagged
    images; None draws N(0, noise_std^2) from Philox keyed by ``seed``.  Returns [V,B,3,s,s] fp32."""
    _operand("augment_view_rgb8", "images", images, dtype=torch.uint8)
    if images.dim() != 4 or images.shape[1] != images.shape[2] or images.shape[3] != 3:
        raise RuntimeError(f"augment_view_rgb8: images must be [B,S,S,3], got {tuple(images.shape)}")
    b, s2, s = int(images.shape[0]), int(images.shape[1]), int(s)
    vp = torch.as_tensor(vparams)
    if vp.dim() != 3:
        raise RuntimeError("augment_view_rgb8: vparams must be [V,B,8]")
    v = int(vp.shape[0])
    vp = _host_params(vp, (v, b, AUG_VIEW_PARAMS), "augment_view_rgb8 vparams")
    if not 0 < s <= s2:
        raise RuntimeError(f"augment_view_rgb8: crop {s} does not fit the {s2}x{s2} image")
    if b:
        ops = vp[:, :, [0, 2]]
        if bool(((ops < 0) | (ops > AUG_OP_LAST) | (ops != ops.round())).any()):
            raise RuntimeError("augment_view_rgb8: unknown colour operation")
        if bool((vp[:, :, 2] == AUG_OP_SHARPNESS).any()):
            raise RuntimeError("augment_view_rgb8: Sharpness cannot be the second operation of a chain")
        if bool(((vp[:, :, 4:6] < 0) | (vp[:, :, 4:6] > s2 - s)).any()):
            raise RuntimeError("augment_view_rgb8: a crop offset leaves the image")
        if bool(((vp[:, :, 7] < 0) | (vp[:, :, 7] >= 2 ** 31)).any()):
            raise RuntimeError("augment_view_rgb8: image ids must be in [0, 2^31)")
    dev = images.device
    _operand("augment_view_rgb8", "noise", noise, shape=(v, b, 3, s, s), device=dev, optional=True)
    out = torch.empty((v, b, 3, s, s), device=dev, dtype=torch.float32)
    m = (ctypes.c_float * 3)(*[float(x) for x in mean])
    sd = (ctypes.c_float * 3)(*[float(x) for x in std])
    vp_dev = vp.to(dev, non_blocking=True)
    _lib.call("pipnet_augment_view_rgb8", images.data_ptr(), vp_dev.data_ptr(), v, b, s2, s, int(bool(grayscale)),
              m, sd, float(noise_std), int(seed) & ((1 << 64) - 1), _ptr(noise), out.data_ptr(),
              torch.cuda.current_stream(dev).cuda_stream)
    return out


# ---- training step, finetune phase (csrc/train_ops.hip) -------------------------------------
TRAIN_MODE = {"train": 0, "pretrain": 1, "finetune": 2}


def train_loss(proto_nhwc: Tensor, pooled: Tensor, out: Tensor, ys: Tensor, mult: Optional[Tensor],
               enforce: bool, tanh_coeff: float, w_align: float, w_tanh: float, w_class: float,
               mode: str) -> Tuple[Tensor, Optional[Tensor]]:
    """calculate_loss (pipnet/train.py:154-250) on the device: returns (stats [8] fp32 =
    align, tanh, class, loss, correct, w_align, w_tanh, w_class; d_out [N,K] or None)."""
    _chk_rows("train_loss", proto_nhwc, "proto features (NHWC)", 4)
    n, h, w, p = proto_nhwc.shape
    _operand("train_loss", "classifier output", out, device=proto_nhwc.device)
    if n % 2 or out.dim() != 2 or out.shape[0] != n:
        raise RuntimeError(f"train_loss: proto {tuple(proto_nhwc.shape)} and out {tuple(out.shape)} must share an "
                           f"even batch = cat([xs1, xs2])")
    _operand("train_loss", "pooled", pooled, shape=(n, p), device=out.device)
    return train_loss_from_partial(train_align_partial(proto_nhwc), h * w, pooled, out, ys, mult, enforce, tanh_coeff,
                                   w_align, w_tanh, w_class, mode)


def train_align_partial(proto_nhwc: Tensor) -> Tensor:
    """The align term's fp64 partial sums over this map's pixel pairs (rows [view 1 | view 2]): one double per
    workgroup of a fixed grid.  train_loss_from_partial sums them and divides by the pair count it is given, so
    the partials of row shards add up elementwise to a batch's (count_pipnet_amd.dist_train)."""
    _chk_rows("train_align_partial", proto_nhwc, "proto features (NHWC)", 4)
    n, h, w, p = proto_nhwc.shape
    if n % 2 or n == 0:
        raise RuntimeError(f"train_align_partial: the batch holds both views, so it must be even and non-empty "
                           f"(got {n})")
    partial = torch.empty(_lib.load().pipnet_train_align_partials(), device=proto_nhwc.device, dtype=torch.float64)
    _lib.call("pipnet_train_align_partial_f32", proto_nhwc.data_ptr(), n // 2, h * w, p, partial.data_ptr(),
              _stream(proto_nhwc))
    return partial


def train_loss_from_partial(partial: Tensor, hw: int, pooled: Tensor, out: Tensor, ys: Tensor, mult: Optional[Tensor],
                            enforce: bool, tanh_coeff: float, w_align: float, w_tanh: float, w_class: float,
                            mode: str) -> Tuple[Tensor, Optional[Tensor]]:
    """train_loss after the align partial sums: pooled [N,P], out [N,K], ys [N/2] and ``hw`` pixels per map."""
    _operand("train_loss", "classifier output", out)
    if out.dim() != 2 or out.shape[0] % 2 or out.shape[0] == 0 or pooled.dim() != 2:
        raise RuntimeError(f"train_loss: out {tuple(out.shape)} must be [even N, K] and pooled {tuple(pooled.shape)} "
                           f"[N, P]")
    (n, k), p = out.shape, pooled.shape[1]
    bh = n // 2
    _operand("train_loss", "pooled", pooled, shape=(n, p), device=out.device)
    _operand("train_loss", "labels", ys, dtype=torch.int64, shape=(bh,), device=out.device)
    _operand("train_loss", "normalization_multiplier", mult, shape=1, device=out.device, optional=True)
    _operand("train_loss", "align partial sums", partial, dtype=torch.float64,
             shape=_lib.load().pipnet_train_align_partials(), device=out.device)
    stats = torch.empty(8, device=out.device, dtype=torch.float32)
    m = TRAIN_MODE[mode]
    d_out = None if m == 1 else torch.empty_like(out)
    _lib.call("pipnet_train_loss_f32", partial.data_ptr(), bh, hw, pooled.data_ptr(), out.data_ptr(),
              ys.data_ptr(), p, k, _ptr(mult), int(bool(enforce)), float(tanh_coeff), float(w_align),
              float(w_tanh), float(w_class), m, _ptr(d_out), stats.data_ptr(), _stream(out))
    return stats, d_out


def nonneg_linear_backward(d_out: Tensor, x: Tensor, w: Tensor, want_bias: bool) -> Tuple[Tensor, Optional[Tensor]]:
    """Gradients of F.linear(x, relu(w), b) (pipnet.py:54-71): (dW, db or None)."""
    _chk_rows("nonneg_linear_backward", w, "classifier weight", 2)
    k, d = w.shape
    n = x.shape[0]
    _operand("nonneg_linear_backward", "classifier input", x, shape=(n, d), device=w.device)
    _operand("nonneg_linear_backward", "d_out", d_out, shape=(n, k), device=w.device)
    dw = torch.empty_like(w)
    db = torch.empty(k, device=w.device, dtype=torch.float32) if want_bias else None
    _lib.call("pipnet_nonneg_linear_bwd_f32", d_out.data_ptr(), x.data_ptr(), n, d, w.data_ptr(), k,
              dw.data_ptr(), _ptr(db), _stream(w))
    return dw, db


def adamw_step_(param: Tensor, grad: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, lr: float, beta1: float,
                beta2: float, eps: float, weight_decay: float, step: int,
                post: Optional[Tuple[float, float]] = None) -> None:
    """torch.optim.AdamW's update of one tensor in place at optimizer step ``step`` (1-based;
    bias corrections from the double hyper-parameters, as torch computes them for a
    non-capturable optimizer); ``post`` = (delta, floor) applies p = max(p - delta, floor)
    afterwards (pipnet/train.py:134-140)."""
    _operand("adamw_step_", "parameter", param)
    _chk_same("adamw_step_", param, gradient=grad, exp_avg=exp_avg, exp_avg_sq=exp_avg_sq)
    delta, floor = post if post is not None else (0.0, 0.0)
    _lib.call("pipnet_adamw_step_f32", param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(),
              exp_avg_sq.data_ptr(), param.numel(), lr, beta1, beta2, eps, weight_decay, int(step),
              int(post is not None), delta, floor, _stream(param))
    _mutated(param, exp_avg, exp_avg_sq)


def clamp_min_(x: Tensor, lo: float) -> Tensor:
    _chk(x, "tensor")
    _lib.call("pipnet_clamp_min_f32", x.data_ptr(), x.numel(), lo, _stream(x))
    _mutated(x)
    return x


# ---- backward building blocks (csrc/backward_ops.hip) ----------------------------------------
def wgrad(a: Tensor, b: Tensor, out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    """out[N1,N2] (+)= a[M,N1]^T @ b[M,N2] (weight gradient dY^T X), deterministic."""
    _operand("wgrad", "A", a, layout="rows")
    _operand("wgrad", "B", b, device=a.device, layout="rows")
    m, n1 = a.shape
    if b.shape[0] != m:
        raise RuntimeError(f"wgrad: row counts differ {tuple(a.shape)} vs {tuple(b.shape)}")
    n2 = b.shape[1]
    _operand("wgrad", "out", out, shape=(n1, n2), device=a.device, layout="rows", optional=not accumulate)
    if out is None:
        out = torch.empty((n1, n2), device=a.device, dtype=torch.float32)
    nbytes = _lib.load().pipnet_wgrad_workspace_bytes(m, n1, n2)
    ws = torch.empty(max(nbytes // 4, 1), device=a.device, dtype=torch.float32)
    _lib.call("pipnet_wgrad_f32", a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), m, n1, n2, out.data_ptr(),
              out.stride(0), int(accumulate), ws.data_ptr(), _stream(a))
    return out


def colsum(a: Tensor, out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    """out[N] (+)= a[M,N].sum(0), deterministic."""
    _operand("colsum", "input", a, layout="rows")
    m, n = a.shape
    if n < 1:
        raise RuntimeError(f"colsum: needs at least one column (got shape {tuple(a.shape)})")
    _operand("colsum", "out", out, shape=n, device=a.device, optional=not accumulate)
    if out is None:
        out = torch.empty(n, device=a.device, dtype=torch.float32)
    ws = torch.empty(_lib.load().pipnet_colsum_workspace_bytes(n) // 4, device=a.device, dtype=torch.float32)
    _lib.call("pipnet_colsum_f32", a.data_ptr(), a.stride(0) if m > 1 else n, m, n, out.data_ptr(), int(accumulate),
              ws.data_ptr(), _stream(a))
    return out


def _partials(c: int, device) -> Tensor:
    return torch.empty(int(_lib.load().pipnet_train_partials_floats(c)), device=device, dtype=torch.float32)


def gelu_fwd(h: Tensor) -> Tensor:
    _chk(h, "gelu input")
    g = torch.empty_like(h)
    _lib.call("pipnet_gelu_fwd_f32", h.data_ptr(), g.data_ptr(), h.numel(), _stream(h))
    return g


def resid_scale(x: Tensor, y2: Tensor, ls: Tensor, row_scale: Optional[Tensor], rows_per_scale: int,
                out: Optional[Tensor] = None) -> Tensor:
    """out = x + row_scale[m // rows_per_scale] * (ls * y2) on [M, C] rows."""
    _chk_rows("resid_scale", x, "residual", 2)
    m, c = x.shape
    _chk_same("resid_scale", x, branch=y2, out=out)
    _chk_vec("resid_scale", x, c, layer_scale=ls)
    _chk_row_scale("resid_scale", x, m, row_scale, rows_per_scale)
    out = torch.empty_like(x) if out is None else out
    _lib.call("pipnet_resid_scale_f32", x.data_ptr(), y2.data_ptr(), ls.data_ptr(), _ptr(row_scale), rows_per_scale,
              m, c, out.data_ptr(), _stream(x))
    return out


def ls_backward(dy: Tensor, y2: Tensor, ls: Tensor, row_scale: Optional[Tensor], rows_per_scale: int,
                d_ls: Tensor, d_b2: Tensor, accumulate: bool = False) -> Tensor:
    """Backward of resid_scale w.r.t. y2 (returned), ls and the Linear2 bias (into d_ls / d_b2)."""
    _chk_rows("ls_backward", dy, "dy", 2)
    m, c = dy.shape
    _chk_same("ls_backward", dy, y2=y2)
    _chk_vec("ls_backward", dy, c, layer_scale=ls, d_ls=d_ls, d_b2=d_b2)
    _chk_row_scale("ls_backward", dy, m, row_scale, rows_per_scale)
    dy2 = torch.empty_like(dy)
    _lib.call("pipnet_ls_bwd_f32", dy.data_ptr(), y2.data_ptr(), ls.data_ptr(), _ptr(row_scale), rows_per_scale, m, c,
              dy2.data_ptr(), d_ls.data_ptr(), d_b2.data_ptr(), int(accumulate), _partials(c, dy.device).data_ptr(),
              _stream(dy))
    return dy2


def ln_backward(z: Tensor, dt: Tensor, gamma: Tensor, d_gamma: Tensor, d_beta: Tensor, want_dz: bool = True,
                accumulate: bool = False) -> Optional[Tensor]:
    """LayerNorm(C, eps 1e-6) backward from the pre-norm rows z [M, C]."""
    _chk_rows("ln_backward", z, "LN input", 2)
    m, c = z.shape
    _chk_same("ln_backward", z, dt=dt)
    _chk_vec("ln_backward", z, c, gamma=gamma, d_gamma=d_gamma, d_beta=d_beta)
    dz = torch.empty_like(z) if want_dz else None
    _lib.call("pipnet_ln_bwd_f32", z.data_ptr(), dt.data_ptr(), gamma.data_ptr(), m, c, _ptr(dz), d_gamma.data_ptr(),
              d_beta.data_ptr(), int(accumulate), _partials(c, z.device).data_ptr(), _stream(z))
    return dz


def dwconv7_plain(x_nhwc: Tensor, w_packed: Tensor, bias: Optional[Tensor], out: Optional[Tensor] = None,
                  accumulate: bool = False) -> Tensor:
    """(out +)= [bias] + depthwise 7x7 pad 3 of x (w_packed [49, C])."""
    _chk_rows("dwconv7_plain", x_nhwc, "input", 4)
    b, h, w, c = x_nhwc.shape
    _chk_same("dwconv7_plain", x_nhwc, out=out)
    _chk_vec("dwconv7_plain", x_nhwc, 49 * c, w_packed=w_packed)
    _chk_vec("dwconv7_plain", x_nhwc, c, bias=bias)
    if out is None and accumulate:
        raise RuntimeError("dwconv7_plain: accumulate needs out")
    out = torch.empty_like(x_nhwc) if out is None else out
    _lib.call("pipnet_dwconv7_plain_f32", x_nhwc.data_ptr(), b, h, w, c, w_packed.data_ptr(), _ptr(bias),
              int(accumulate), out.data_ptr(), _stream(x_nhwc))
    return out


def dwconv7_wgrad(dz_nhwc: Tensor, x_nhwc: Tensor, dw_packed: Tensor, db: Tensor, accumulate: bool = False) -> None:
    """(dw_packed [49, C], db [C]) (+)= the depthwise 7x7 weight / bias gradient from dz and the conv's input x."""
    _chk_rows("dwconv7_wgrad", x_nhwc, "input", 4)
    b, h, w, c = x_nhwc.shape
    _chk_same("dwconv7_wgrad", x_nhwc, dz=dz_nhwc)
    _chk_vec("dwconv7_wgrad", x_nhwc, 49 * c, dw_packed=dw_packed)
    _chk_vec("dwconv7_wgrad", x_nhwc, c, db=db)
    _lib.call("pipnet_dwconv7_wgrad_f32", dz_nhwc.data_ptr(), x_nhwc.data_ptr(), b, h, w, c, dw_packed.data_ptr(),
              db.data_ptr(), int(accumulate), _partials(c, x_nhwc.device).data_ptr(), _stream(x_nhwc))


def wgrad_conv(dy_nhwc: Tensor, x_nhwc: Tensor, kh: int, kw: int, stride: int, out: Tensor,
               accumulate: bool = False, pad: int = 0) -> Tensor:
    """Packed [Cout, KH*KW*Cin] weight gradient of a KHxKW conv (stride, zero padding)."""
    _chk_rows("wgrad_conv", x_nhwc, "conv input", 4)
    b, h, w, cin = x_nhwc.shape
    cout = dy_nhwc.shape[-1]
    oh, ow = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    _operand("wgrad_conv", "d conv output", dy_nhwc, shape=(b, oh, ow, cout), device=x_nhwc.device)
    _operand("wgrad_conv", "out", out, shape=cout * kh * kw * cin, device=x_nhwc.device)
    nbytes = _lib.load().pipnet_wgrad_workspace_bytes(b * oh * ow, cout, kh * kw * cin)
    ws = torch.empty(max(nbytes // 4, 1), device=x_nhwc.device, dtype=torch.float32)
    _lib.call("pipnet_wgrad_conv_f32", dy_nhwc.data_ptr(), x_nhwc.data_ptr(), b, h, w, cin, kh, kw, stride, pad, cout,
              out.data_ptr(), int(accumulate), ws.data_ptr(), _stream(x_nhwc))
    return out


def wgrad_conv2x2(dy_nhwc: Tensor, x_nhwc: Tensor, stride: int, out: Tensor, accumulate: bool = False) -> Tensor:
    """Packed [Cout, 4*Cin] weight gradient of the 2x2 downsample conv."""
    _chk_rows("wgrad_conv2x2", x_nhwc, "conv input", 4)
    b, h, w, cin = x_nhwc.shape
    cout = dy_nhwc.shape[-1]
    if stride not in (1, 2) or h < 2 or w < 2:
        raise RuntimeError(f"wgrad_conv2x2: x {tuple(x_nhwc.shape)}, stride {stride}")
    _operand("wgrad_conv2x2", "d conv output", dy_nhwc, device=x_nhwc.device,
             shape=(b, (h - 2) // stride + 1, (w - 2) // stride + 1, cout))
    _operand("wgrad_conv2x2", "out", out, shape=cout * 4 * cin, device=x_nhwc.device)
    nbytes = _lib.load().pipnet_wgrad_workspace_bytes(dy_nhwc.numel() // cout, cout, 4 * cin)
    ws = torch.empty(max(nbytes // 4, 1), device=x_nhwc.device, dtype=torch.float32)
    _lib.call("pipnet_wgrad_conv2x2_f32", dy_nhwc.data_ptr(), x_nhwc.data_ptr(), b, h, w, cin, stride, cout,
              out.data_ptr(), int(accumulate), ws.data_ptr(), _stream(x_nhwc))
    return out


def _chk_all_rows(fn: str, rows: Tensor, all_rows: Tensor) -> int:
    """The gathered rows of every rank beside one rank's ``rows`` [2 Bh, P]: [2 Bh_all, P] -> Bh_all."""
    _operand(fn, "gathered rows of every rank", all_rows, device=rows.device)
    if all_rows.dim() != 2 or all_rows.shape[1] != rows.shape[1] or all_rows.shape[0] % 2 or \
            all_rows.shape[0] < rows.shape[0]:
        raise RuntimeError(f"{fn}: the gathered rows must be [2 Bh_all, {rows.shape[1]}] with Bh_all >= "
                           f"{rows.shape[0] // 2} (got {tuple(all_rows.shape)})")
    return all_rows.shape[0] // 2


def head_backward(proto_nhwc: Tensor, pooled: Tensor, d_out: Optional[Tensor], w: Optional[Tensor],
                  w_align: float, w_tanh: float, tanh_coeff: float = 1.0,
                  pooled_all: Optional[Tensor] = None) -> Tensor:
    """d loss / d logits of the PIP-Net head (softmax + max-pool) for the align / tanh /
    classifier terms of calculate_loss (pipnet/train.py:154-265).  ``pooled_all`` [2 Bh_all, P]: the
    operands are one rank's rows of a batch whose pooled rows these are (pipnet_head_bwd_rows_f32)."""
    _chk_rows("head_backward", proto_nhwc, "proto features", 4)
    n, h, ww, p = proto_nhwc.shape
    if n % 2 or n == 0:
        raise RuntimeError(f"head_backward: the batch holds both views, so it must be even and non-empty (got {n})")
    _chk_vec("head_backward", proto_nhwc, n * p, pooled=pooled)
    if d_out is not None:
        if w is None:
            raise RuntimeError("head_backward: d_out needs the classifier weight")
        if w.dim() != 2 or w.shape[0] < 1:
            raise RuntimeError(f"head_backward: the classifier weight must be (K, {p}), got {tuple(w.shape)}")
        _operand("head_backward", "classifier weight", w, shape=(w.shape[0], p), device=proto_nhwc.device)
        _chk_vec("head_backward", proto_nhwc, n * w.shape[0], d_out=d_out)
    d_logits = torch.empty_like(proto_nhwc)
    amax = torch.empty((n, p), device=proto_nhwc.device, dtype=torch.int32)
    dpool = torch.empty((n, p), device=proto_nhwc.device, dtype=torch.float32)
    k = 0 if w is None else w.shape[0]
    if pooled_all is not None:
        bh_all = _chk_all_rows("head_backward", pooled.view(n, p), pooled_all)
        tcoef = torch.empty((2, p), device=proto_nhwc.device, dtype=torch.float32)
        _lib.call("pipnet_head_bwd_rows_f32", proto_nhwc.data_ptr(), pooled.data_ptr(), n // 2, h * ww, p, _ptr(d_out),
                  _ptr(w), k, pooled_all.data_ptr(), bh_all, w_align, w_tanh, tanh_coeff, amax.data_ptr(),
                  dpool.data_ptr(), tcoef.data_ptr(), d_logits.data_ptr(), _stream(proto_nhwc))
        return d_logits
    _lib.call("pipnet_head_bwd_f32", proto_nhwc.data_ptr(), pooled.data_ptr(), n // 2, h * ww, p, _ptr(d_out), _ptr(w),
              k, w_align, w_tanh, tanh_coeff, amax.data_ptr(), dpool.data_ptr(), d_logits.data_ptr(),
              _stream(proto_nhwc))
    return d_logits


def pack_tensors(table: Tensor, arena: Tensor) -> None:
    """One launch gathers fp32 tensors into ``arena`` (pipnet_pack_tensors_f32).  ``table``: device int64 [n, 3]
    = source address, arena offset in floats (a multiple of 4), element count; the slot padding is zeroed.  The
    rows are the caller's to get right (count_pipnet_amd.dist_train.GradArena builds them from live tensors)."""
    _operand("pack_tensors", "arena", arena)
    _operand("pack_tensors", "table", table, dtype=torch.int64, device=arena.device)
    if table.dim() != 2 or table.shape[1] != 3:
        raise RuntimeError(f"pack_tensors: the table must be [n, 3] (got {tuple(table.shape)})")
    _lib.call("pipnet_pack_tensors_f32", table.data_ptr(), table.shape[0], arena.data_ptr(), _stream(arena))


# ---- ResNet training: BatchNorm2d in train mode (csrc/bn_ops.hip) ----------------------------
def _bn_ws(c: int, device) -> Tensor:
    return torch.empty(int(_lib.load().pipnet_bn_workspace_floats(c)), device=device, dtype=torch.float32)


def bn_stats(x: Tensor, eps: float, momentum: float, running_mean: Optional[Tensor] = None,
             running_var: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """Batch mean / invstd over the rows of NHWC ``x`` (train-mode BatchNorm2d); updates the
    running statistics in place when given (momentum, unbiased variance)."""
    _chk(x, "BN input")
    if x.dim() < 2 or x.shape[-1] < 1:
        raise RuntimeError(f"bn_stats: expects channel-last rows [..., C] (got shape {tuple(x.shape)})")
    c = x.shape[-1]
    m = x.numel() // c
    if (running_mean is None) != (running_var is None):
        raise RuntimeError("bn_stats: running_mean and running_var go together")
    _chk_vec("bn_stats", x, c, running_mean=running_mean, running_var=running_var)
    mean = torch.empty(c, device=x.device, dtype=torch.float32)
    invstd = torch.empty_like(mean)
    _lib.call("pipnet_bn_stats_f32", x.data_ptr(), m, c, eps, momentum, mean.data_ptr(), invstd.data_ptr(),
              _ptr(running_mean), _ptr(running_var), _bn_ws(c, x.device).data_ptr(), _stream(x))
    if running_mean is not None:
        _mutated(running_mean, running_var)
    return mean, invstd


def bn_apply(x: Tensor, mean: Tensor, invstd: Tensor, gamma: Tensor, beta: Tensor, residual: Optional[Tensor] = None,
             relu: bool = False, out: Optional[Tensor] = None) -> Tensor:
    """gamma * (x - mean) * invstd + beta [+ residual] [ReLU] on NHWC rows."""
    _chk(x, "BN input")
    if x.dim() < 2 or x.shape[-1] < 1:
        raise RuntimeError(f"bn_apply: expects channel-last rows [..., C] (got shape {tuple(x.shape)})")
    c = x.shape[-1]
    _chk_vec("bn_apply", x, c, mean=mean, invstd=invstd, gamma=gamma, beta=beta)
    _chk_same("bn_apply", x, residual=residual, out=out)
    y = torch.empty_like(x) if out is None else out
    _lib.call("pipnet_bn_apply_f32", x.data_ptr(), x.numel() // c, c, mean.data_ptr(), invstd.data_ptr(),
              gamma.data_ptr(), beta.data_ptr(), _ptr(residual), int(relu), y.data_ptr(), _stream(x))
    return y


def bn_backward(x: Tensor, dy: Tensor, mean: Tensor, invstd: Tensor, gamma: Tensor, relu_out: Optional[Tensor] = None,
                want_dx: bool = True, want_masked: bool = False
                ) -> Tuple[Optional[Tensor], Optional[Tensor], Tensor, Tensor]:
    """Train-mode BatchNorm2d backward from the pre-norm rows ``x``; ``relu_out`` (the output of
    the ReLU that follows, when there is one) masks dy.  Returns (dx, masked dy, d_gamma, d_beta)."""
    _chk(x, "BN input")
    if x.dim() < 2 or x.shape[-1] < 1:
        raise RuntimeError(f"bn_backward: expects channel-last rows [..., C] (got shape {tuple(x.shape)})")
    c = x.shape[-1]
    _chk_same("bn_backward", x, dy=dy, relu_out=relu_out)
    _chk_vec("bn_backward", x, c, mean=mean, invstd=invstd, gamma=gamma)
    dx = torch.empty_like(x) if want_dx else None
    dm = torch.empty_like(x) if want_masked else None
    dg = torch.empty(c, device=x.device, dtype=torch.float32)
    db = torch.empty_like(dg)
    _lib.call("pipnet_bn_backward_f32", x.data_ptr(), dy.data_ptr(), _ptr(relu_out), x.numel() // c, c, mean.data_ptr(),
              invstd.data_ptr(), gamma.data_ptr(), _ptr(dx), _ptr(dm), dg.data_ptr(), db.data_ptr(),
              _bn_ws(c, x.device).data_ptr(), _stream(x))
    return dx, dm, dg, db


def stride_scatter(x: Tensor, h: int, w: int, stride: int, out: Optional[Tensor] = None,
                   accumulate: bool = False) -> Tensor:
    """NHWC [B, OH, OW, C] -> [B, h, w, C] with x on the stride lattice, zeros elsewhere
    (added into ``out`` when accumulate)."""
    _chk_rows("stride_scatter", x, "input", 4)
    b, oh, ow, c = x.shape
    _operand("stride_scatter", "out", out, shape=(b, h, w, c), device=x.device, optional=not accumulate)
    if out is None:
        out = torch.empty((b, h, w, c), device=x.device, dtype=torch.float32)
    _lib.call("pipnet_stride_scatter_f32", x.data_ptr(), b, oh, ow, c, h, w, stride, int(accumulate), out.data_ptr(),
              _stream(x))
    return out


# ---- integrated-gradients attribution (csrc/attribution.hip) ------------------------------

ATTR_METHOD = {"ig": 0, "lig": 1, "idg": 2}
LIG_ALPHA_STAR = 0.9             # interpret_idg.py:105


def _attr_baseline(fn: str, x: Tensor, baseline) -> Tuple[Optional[Tensor], float]:
    """(baseline image pointer operand or None, constant baseline value)."""
    if torch.is_tensor(baseline):
        _chk_same(fn, x, baseline=baseline)
        return baseline, 0.0
    return None, float(baseline)


def attr_path_images(x: Tensor, baseline, alpha: Tensor) -> Tensor:
    """x [3,H,W], baseline (float or [3,H,W]), alpha [S] -> the path images baseline + alpha_i (x - baseline) as
    [S,H,W,4] NHWC with a zero fourth channel (``nchw_to_nhwc(..., 4)``'s layout)."""
    _chk_rows("attr_path_images", x, "image", 3)
    if x.shape[0] != 3:
        raise RuntimeError(f"attr_path_images: image must be [3,H,W], got {tuple(x.shape)}")
    _operand("attr_path_images", "alpha", alpha, shape=(alpha.numel(),), device=x.device)
    bt, bv = _attr_baseline("attr_path_images", x, baseline)
    _, h, w = x.shape
    out = torch.empty((alpha.numel(), h, w, 4), device=x.device, dtype=torch.float32)
    _lib.call("pipnet_attr_path_images_f32", x.data_ptr(), _ptr(bt), bv, alpha.data_ptr(), alpha.numel(), h, w,
              out.data_ptr(), _stream(x))
    return out


def attr_head_backward(soft_nhwc: Tensor, u: Tensor, loc: Optional[Tensor], pool_mode: int, tau: float = 1.0) -> Tensor:
    """d target / d logits [B,h,w,P] of the prototype head for the upstream vector u [B,P]: pool_mode 0 =
    softmax + max-pool (loc [B,P] int32 from softmax_pool_argmax), 1 = (Gumbel-)softmax at temperature tau +
    spatial sum.  Any P and any batch."""
    _chk_rows("attr_head_backward", soft_nhwc, "soft map", 4)
    b, h, w, p = soft_nhwc.shape
    _operand("attr_head_backward", "upstream vector", u, shape=(b, p), device=soft_nhwc.device)
    if pool_mode not in (0, 1):
        raise RuntimeError(f"attr_head_backward: pool_mode {pool_mode}")
    if pool_mode == 0:                                        # max mode reads where each maximum sits
        _operand("attr_head_backward", "loc", loc, dtype=torch.int32, shape=(b, p), device=soft_nhwc.device)
    d = torch.empty_like(soft_nhwc)
    _lib.call("pipnet_attr_head_bwd_f32", soft_nhwc.data_ptr(), u.data_ptr(), _ptr(loc) if pool_mode == 0 else None,
              b, h * w, p, pool_mode, 1.0 / float(tau), d.data_ptr(), _stream(soft_nhwc))
    return d


def attr_stem_dx(dz_nhwc: Tensor, w: Tensor, h: int, wd: int, out: Optional[Tensor] = None) -> Tensor:
    """Input gradient of Conv2d(3, O, 4, stride 4): dz [B,h/4,w/4,O] NHWC, w [O,3,4,4] -> [B,3,h,w] NCHW.
    ``out``: [B, ld] rows (ld >= 3 h w) to write the images into (a slice of the path's gradient store)."""
    _chk_rows("attr_stem_dx", dz_nhwc, "dz", 4)
    b, zh, zw, o = dz_nhwc.shape
    _operand("attr_stem_dx", "stem weight", w, shape=(o, 3, 4, 4), device=dz_nhwc.device)
    if (zh, zw) != (h // 4, wd // 4):
        raise RuntimeError(f"attr_stem_dx: dz {tuple(dz_nhwc.shape)} does not belong to an image {(h, wd)}")
    n = 3 * h * wd
    if out is None:
        out = torch.empty((b, 3, h, wd), device=dz_nhwc.device, dtype=torch.float32)
        ld = n
    else:
        _operand("attr_stem_dx", "out", out, device=dz_nhwc.device, layout="rows")
        if out.shape[0] != b or out.shape[1] < n or out.stride(0) < n:
            raise RuntimeError(f"attr_stem_dx: out {tuple(out.shape)} stride {out.stride()} cannot hold {(b, n)}")
        ld = out.stride(0)
    _lib.call("pipnet_attr_stem_dx_f32", dz_nhwc.data_ptr(), w.data_ptr(), b, h, wd, o, ld, out.data_ptr(),
              _stream(dz_nhwc))
    return out


def attr_path_weights(scores: Tensor, method: str, alphas: Optional[Tensor] = None,
                      substep: Optional[Tensor] = None, out=None) -> Tuple[Tensor, Tensor]:
    """(weights [S], cutoff [] int64) of one target from its scores [S] (ig / lig / idg), on the device.
    ``out`` = (weights, cutoff) to write into (rows of the per-target outputs)."""
    _chk_rows("attr_path_weights", scores, "scores", 1)
    s = scores.numel()
    if method not in ATTR_METHOD:
        raise ValueError(f"attr_path_weights: unknown method {method!r}")
    if method == "idg":
        if alphas is None or substep is None:
            raise RuntimeError("attr_path_weights: idg needs alphas and substep")
        _chk_same("attr_path_weights", scores, alphas=alphas, substep=substep)
    if out is None:
        weights = torch.empty(s, device=scores.device, dtype=torch.float32)
        cutoff = torch.empty((), device=scores.device, dtype=torch.int64)
    else:
        weights, cutoff = out
        _chk_same("attr_path_weights", scores, weights=weights)
        _operand("attr_path_weights", "cutoff out", cutoff, dtype=torch.int64, shape=1, device=scores.device)
    _lib.call("pipnet_attr_path_weights_f32", scores.data_ptr(), _ptr(alphas) if method == "idg" else None,
              _ptr(substep) if method == "idg" else None, s, ATTR_METHOD[method], LIG_ALPHA_STAR, weights.data_ptr(),
              cutoff.data_ptr(), _stream(scores))
    return weights, cutoff


def attr_path_reduce(grads: Tensor, weights: Tensor, x: Tensor, baseline, out: Optional[Tensor] = None) -> Tensor:
    """(x - baseline) * sum_i weights[i] * grads[i] summed in step order: grads [S, ld] rows holding one image's
    gradient each (the first x.numel() floats of a row), x of any shape -> a map of x's shape."""
    _operand("attr_path_reduce", "image", x)
    n = x.numel()
    _operand("attr_path_reduce", "grads", grads, device=x.device, layout="rows")
    if grads.shape[1] < n or grads.stride(0) < n:
        raise RuntimeError(f"attr_path_reduce: grads {tuple(grads.shape)} stride {grads.stride()} vs image {n}")
    s = grads.shape[0]
    _chk_vec("attr_path_reduce", x, s, weights=weights)
    bt, bv = _attr_baseline("attr_path_reduce", x, baseline)
    if out is None:
        out = torch.empty_like(x)
    else:
        _chk_same("attr_path_reduce", x, out=out)
    _lib.call("pipnet_attr_path_reduce_f32", grads.data_ptr(), grads.stride(0), weights.data_ptr(), x.data_ptr(),
              _ptr(bt), bv, s, n, out.data_ptr(), _stream(x))
    return out


# ---- attribution images (csrc/saliency_ops.hip) -----------------------------------------------

def _saliency_maps(fn: str, what: str, t: Tensor, ndim: int, device=None) -> None:
    """A dense float32 stack of maps: [T,3,H,W] (ndim 4) or [T,H,W] (ndim 3), H * W >= 1 and below 2^31."""
    _operand(fn, what, t, device=device)
    if t.dim() != ndim or (ndim == 4 and t.shape[1] != 3) or t.shape[-2] * t.shape[-1] < 1:
        want = "[T,3,H,W]" if ndim == 4 else "[T,H,W]"
        raise RuntimeError(f"{fn}: {what} must be {want} with H, W >= 1, got {tuple(t.shape)}")
    if t.shape[-2] * t.shape[-1] >= 1 << 31:
        raise RuntimeError(f"{fn}: {what} has {t.shape[-2] * t.shape[-1]} values per map; the counts are 32-bit")


def _saliency_out(fn: str, what: str, out: Optional[Tensor], shape, dtype, ref: Tensor) -> Tensor:
    if out is None:
        return torch.empty(shape, device=ref.device, dtype=dtype)
    _operand(fn, what, out, dtype=dtype, shape=torch.Size(shape), device=ref.device)
    return out


def saliency_abs_sum(maps: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """[T,3,H,W] -> [T,H,W]: ``(|a0| + |a1|) + |a2|`` over the channels, numpy's ``np.sum(np.abs(.), axis=2)`` of
    the transposed map (interpret_idg.py:413-415), bit for bit."""
    fn = "saliency_abs_sum"
    _saliency_maps(fn, "maps", maps, 4)
    t, _, h, w = maps.shape
    out = _saliency_out(fn, "out", out, (t, h, w), torch.float32, maps)
    _lib.call("pipnet_saliency_abs_sum_f32", maps.data_ptr(), t, h * w, out.data_ptr(), _stream(maps))
    return out


def saliency_order_stats(folded: Tensor, k: int, gamma: float, out=None):
    """(vmin, vtop, lo, hi, vq), each [T]: per map of ``folded`` [T,H,W] the exact minimum and maximum, the k-th
    and (k+1)-th smallest values (0-based; hi = lo past the last element) and numpy's interpolation between them
    at weight ``gamma`` (a float32 value).  ``out``: five [T] tensors to write into."""
    fn = "saliency_order_stats"
    _saliency_maps(fn, "folded", folded, 3)
    t, n = folded.shape[0], folded.shape[1] * folded.shape[2]
    if not 0 <= int(k) < n:
        raise RuntimeError(f"{fn}: rank {k} outside 0..{n - 1}")
    names = ("vmin", "vtop", "lo", "hi", "vq")
    if out is None:
        out = (None,) * 5
    if len(out) != 5:
        raise RuntimeError(f"{fn}: out must be the five tensors {names}")
    res = tuple(_saliency_out(fn, nm, o, (t,), torch.float32, folded) for nm, o in zip(names, out))
    _lib.call("pipnet_saliency_order_stats_f32", folded.data_ptr(), t, n, int(k), float(gamma),
              *(r.data_ptr() for r in res), _stream(folded))
    return res


def saliency_normalize(folded: Tensor, vmin: Tensor, vq: Tensor, vtop: Tensor, fallback: bool = True, out=None):
    """(rule [T] int32, normalized [T,H,W]): ``clip((folded - vmin) / den, 0, 1)`` with the denominator chosen per
    map on the device (rule 0: vq - vmin, 1: vtop - vmin, 2: a zero map; pipnet_saliency_normalize_f32).
    ``out`` = (rule, normalized) to write into."""
    fn = "saliency_normalize"
    _saliency_maps(fn, "folded", folded, 3)
    t = folded.shape[0]
    for nm, v in (("vmin", vmin), ("vq", vq), ("vtop", vtop)):
        _operand(fn, nm, v, shape=torch.Size((t,)), device=folded.device)
    rule, norm = (None, None) if out is None else out
    rule = _saliency_out(fn, "rule out", rule, (t,), torch.int32, folded)
    norm = _saliency_out(fn, "out", norm, tuple(folded.shape), torch.float32, folded)
    _lib.call("pipnet_saliency_normalize_f32", folded.data_ptr(), vmin.data_ptr(), vq.data_ptr(), vtop.data_ptr(), t,
              folded.shape[1] * folded.shape[2], 1 if fallback else 0, rule.data_ptr(), norm.data_ptr(), _stream(folded))
    return rule, norm


def saliency_blend(normalized: Tensor, colours: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """[H,W,4] float64: RGB = clip(sum_t colours[t] * normalized[t], 0, 1) added in map order in float64, alpha =
    the running maximum from 0 (interpret_idg.py:419-427, :454-457).  ``colours`` [T,3] float64."""
    fn = "saliency_blend"
    _saliency_maps(fn, "normalized", normalized, 3)
    t, h, w = normalized.shape
    _operand(fn, "colours", colours, dtype=torch.float64, shape=torch.Size((t, 3)), device=normalized.device)
    out = _saliency_out(fn, "out", out, (h, w, 4), torch.float64, normalized)
    _lib.call("pipnet_saliency_blend_f64", normalized.data_ptr(), colours.data_ptr(), t, h * w, out.data_ptr(),
              _stream(normalized))
    return out


def saliency_unnormalize(x: Tensor, mean, std, out: Optional[Tensor] = None) -> Tensor:
    """x [3,H,W] -> [H,W,3] float32 ``clip(x * std + mean, 0, 1)`` per channel, product and sum rounded separately
    (interpret_idg.py:442-446).  ``mean`` / ``std``: three floats each (their float32 values are used)."""
    fn = "saliency_unnormalize"
    _operand(fn, "image", x)
    if x.dim() != 3 or x.shape[0] != 3 or x.shape[1] * x.shape[2] < 1 or x.shape[1] * x.shape[2] >= 1 << 31:
        raise RuntimeError(f"{fn}: image must be [3,H,W] with 1 <= H * W < 2^31, got {tuple(x.shape)}")
    mean, std = [float(v) for v in mean], [float(v) for v in std]
    if len(mean) != 3 or len(std) != 3:
        raise RuntimeError(f"{fn}: mean and std must hold three values each")
    _, h, w = x.shape
    out = _saliency_out(fn, "out", out, (h, w, 3), torch.float32, x)
    _lib.call("pipnet_saliency_unnormalize_f32", x.data_ptr(), h * w, *mean, *std, out.data_ptr(), _stream(x))
    return out


def saliency_colormap_rgba8(normalized: Tensor, lut: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """[..., 4] uint8: ``lut[min(int(v * 256), 255)]`` for every value v in [0, 1] of ``normalized`` (any shape),
    ``lut`` [256,4] uint8 -- matplotlib's byte colour map of a map whose minimum is 0 and maximum is 1."""
    fn = "saliency_colormap_rgba8"
    _operand(fn, "normalized", normalized)
    _operand(fn, "lut", lut, dtype=torch.uint8, shape=torch.Size((256, 4)), device=normalized.device)
    out = _saliency_out(fn, "out", out, tuple(normalized.shape) + (4,), torch.uint8, normalized)
    if out.data_ptr() % 4:
        raise RuntimeError(f"{fn}: out must start 4-byte aligned (one 4-byte store per pixel)")
    _lib.call("pipnet_saliency_colormap_rgba8", normalized.data_ptr(), lut.data_ptr(), normalized.numel(),
              out.data_ptr(), _stream(normalized))
    return out
