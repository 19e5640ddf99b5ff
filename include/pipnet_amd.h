/*
 * pipnet_amd.h -- C-ABI of the MI355X-native PIP-Net / CountPIPNet inference path.
 *
 * The reference (TarasKutsyk/Count_PIPNet) has no native code and no FFI: its boundary is
 * the Python nn.Module contract of pipnet/pipnet.py and pipnet/count_pipnet.py
 * (SURVEY.md 8b).  These entry points are what a ctypes / torch-extension binding of that
 * forward binds: every op of the hot path's ATen sequence as one
 * stream-ordered call.  Plain pointers and sizes only (no torch types).
 *
 * Conventions
 *   - all tensors are float32 device pointers (HBM), activations NHWC ("channels_last"),
 *     the network input NCHW exactly as the reference receives it;
 *   - ``stream`` is a hipStream_t (NULL = default stream); calls only enqueue work;
 *   - the return value is a PIPNET_* status; the Python host layer raises RuntimeError
 *     on anything but PIPNET_OK (the reference raises Python exceptions).
 *   - re-entrant: no global mutable state; callers own every buffer.
 */
#ifndef PIPNET_AMD_H
#define PIPNET_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PIPNET_OK 0
#define PIPNET_ERR_ARG 1        /* bad shape / size / unsupported configuration */
#define PIPNET_ERR_ALIGN 2      /* pointer or leading dimension not 16-byte aligned */
#define PIPNET_ERR_LAUNCH 3     /* hipLaunchKernel failed (hipGetLastError) */
#define PIPNET_ERR_HIP 4        /* other HIP runtime error */

/* GEMM epilogues for pipnet_linear_f32 */
#define PIPNET_EPI_NONE 0       /* C = A W^T                                              */
#define PIPNET_EPI_BIAS 1       /* C = A W^T + b                                          */
#define PIPNET_EPI_BIAS_GELU 2  /* C = gelu_erf(A W^T + b)          (CNBlock Linear1+GELU) */
#define PIPNET_EPI_RESID 3      /* C = R + s * (A W^T + b)   (CNBlock Linear2*layer_scale+x)*/
#define PIPNET_EPI_MUL 4        /* C = (A W^T) * R          (BilinearIntermediate W(e)*V(e)) */
#define PIPNET_EPI_BIAS_RELU 5  /* C = relu(A W^T + b)            (ResNet conv+BN+ReLU)      */
#define PIPNET_EPI_BIAS_RESID_RELU 6 /* C = relu(A W^T + b + R) (Bottleneck conv3+BN+identity+ReLU) */
#define PIPNET_EPI_RESID_ROWSCALE 7  /* C = R + rs[m/g] * (s * (A W^T + b))  (pipnet_linear_rowscale_f32:
                                        CNBlock Linear2 with train-mode stochastic depth)              */
#define PIPNET_EPI_GELU_BWD 8        /* C = (A W^T) * gelu_erf'(R)   (training: d pre-GELU activation) */
/* split-bf16 ("bf16x3") epilogues of pipnet_conv2d_nhwc_s3 (fp32 results, see there) */
#define PIPNET_EPI_S3_GELU 9         /* g = gelu_erf(A W^T + b) stored as split planes [hi|lo] bf16    */
#define PIPNET_EPI_F32_BIAS 10       /* C = A W^T + b, fp32                                            */
#define PIPNET_EPI_F32_RESID 11      /* C = R + s * (A W^T + b), fp32 C and R (R may alias C)          */
#define PIPNET_EPI_DUAL_BIAS_RELU 12 /* columns < N1: C = A W^T + b; columns >= N1: C2 = relu(A W^T + b) (bf16 1x1 convs, pipnet_conv1x1_bf16_dual) */

/* ABI version: bumped whenever an exported signature changes.  2: pipnet_wgrad_conv_f32 gained
 * its `pad` argument (round 2).  3: the process-wide A/B switches (pipnet_gemm_persist /
 * _stream / _bk16x3 / _plain_store, pipnet_conv_bf16_rb, pipnet_head_bf16_quads) and
 * pipnet_linear_agelu_f32 are gone -- kernel selection is a fixed per-shape rule with no
 * mutable library state -- and the one-launch fused head pipnet_softmax_pool_linear_f32 / _bf16
 * (+ _part_floats) and pipnet_matmul2_f64acc_f32 are new (round 5).  A caller built against an older version must not bind this library.
 * Round 6 only ADDED entry points (pipnet_philox_exp1_f32, pipnet_conv2d_nhwc_bf16_plan,
 * pipnet_linear_f32_plan); no signature changed.  The prototype
 * explanation entry points (pipnet_softmax_pool_argmax_f32, pipnet_map_argmax_f32,
 * pipnet_topk_update) are additions as well, and so are pipnet_local_explain_f32 and the
 * attribution entry points (pipnet_attr_*).  4: the fused-MLP plan query is gone (its packed code had to be
 * decoded by the caller); the label queries (pipnet_*_label) are new.  The plain bf16 ConvNeXt
 * entry points (pipnet_conv2d_nhwc_bf16_mix + _label, pipnet_dwconv7_ln_bf16, pipnet_layernorm_bf16)
 * were added since, and so were the explanation-image entry points (pipnet_patch_compose_rgb8,
 * pipnet_draw_rects_rgb8) and the attribution-image entry points (pipnet_saliency_*), and the row-scaled
 * low-precision Linear2 (pipnet_linear_bf16_mix_rowscale, pipnet_linear_s3_rowscale + _label), and the state
 * merges of the sharded dataset passes (pipnet_topk_merge, pipnet_proto_stats_merge, pipnet_colsum_merge_f64,
 * pipnet_part_purity_merge), and the similarity-heatmap entry point (pipnet_heatmap_rgb8), and the feature-map
 * overlay entry point (pipnet_map_overlay); no signature changed. */
#define PIPNET_AMD_ABI_VERSION 4
int pipnet_amd_abi_version(void);
const char* pipnet_amd_status_string(int status);
/* sha256 (hex) of the sources this library was compiled from (build provenance). */
const char* pipnet_amd_source_digest(void);

/* Dense fp32 linear / 1x1 conv on MFMA (v_mfma_f32_32x32x2_f32, exact fp32):
 *   C[M,N] (ldc) = epi( A[M,K] (lda) * W[N,K]^T )
 * Replaces F.linear / nn.Linear (torchvision CNBlock block.3 / block.5),
 * the 1x1 add-on Conv2d (pipnet.py:99-104, count_pipnet.py:376-381) and the
 * Bilinear/LinearFull intermediate Linears (count_pipnet_utils.py:342-385, :387-444).
 * K % 4 == 0, lda/ldc/ldr % 4 == 0, pointers 16-B aligned.  bias/scale: [N] or NULL;
 * R (resid / other): [M,N] with leading dimension ldr (may alias C for in-place residual). */
int pipnet_linear_f32(const float* A, int64_t lda, const float* W, const float* bias,
                      const float* scale, const float* R, int64_t ldr, float* C, int64_t ldc,
                      int M, int N, int K, int epilogue, void* stream);

/* pipnet_linear_f32 with PIPNET_EPI_RESID_ROWSCALE: C = R + row_scale[m / rows_per_scale] *
 * (scale * (A W^T + bias)).  The CNBlock's Linear2 * layer_scale + residual under
 * torchvision's StochasticDepth("row") in train mode: rows_per_scale = H*W (one factor per
 * sample), row_scale[b] = keep_b / (1 - p) -- 0 leaves a dropped sample's rows equal to R. */
int pipnet_linear_rowscale_f32(const float* A, int64_t lda, const float* W, const float* bias, const float* scale,
                               const float* R, int64_t ldr, float* C, int64_t ldc, int M, int N, int K,
                               const float* row_scale, int rows_per_scale, void* stream);

/* Split-K variant for short-M products (M <= a few hundred rows, long K: the Bilinear /
 * LinearFull intermediate GEMMs at M = batch, count_pipnet_utils.py:342-385): the K range
 * is cut into `splits` slabs computed by separate workgroups into `workspace`
 * (splits * M * N floats), then one reduction kernel sums the slabs and applies the
 * epilogue.  N % 4 == 0, K % 32 == 0, splits <= K/32. */
int pipnet_linear_splitk_f32(const float* A, int64_t lda, const float* W, const float* bias,
                             const float* scale, const float* R, int64_t ldr, float* C, int64_t ldc,
                             int M, int N, int K, int epilogue, int splits, float* workspace,
                             void* stream);
/* BilinearIntermediate on the folded pair in one GEMM: Wpair = [W1; W2] ([2 Nh, K], the
 * pipnet_matmul2_f64acc_f32 output), C[M, Nh] = (A W2^T) * (A W1^T) elementwise, K split into
 * `splits` slabs (workspace: splits * M * 2 Nh floats) summed in slab order by the reduction that
 * also takes the product -- count_pipnet_utils.py:378-385 W(e) * V(e) with e folded in. */
int pipnet_linear_pair_mul_f32(const float* A, int64_t lda, const float* Wpair, float* C, int64_t ldc, int M, int Nh,
                               int K, int splits, float* workspace, void* stream);

/* ConvNeXt downsample conv, k=2, stride s in {1,2}, no padding, as implicit GEMM on MFMA.
 * x: [B,H,W,Cin] NHWC (already LayerNorm2d-normalised), w_packed: [Cout][2][2][Cin]
 * (torch weight [Cout,Cin,2,2] permuted), y: [B,OH,OW,Cout], OH=(H-2)/s+1.
 * Replaces features.{2,4,6}.1 of torchvision ConvNeXt with the stride patch of
 * features/convnext_features.py:5-15.  Cin % 32 == 0. */
int pipnet_conv2x2_f32(const float* x, int B, int H, int W, int Cin, const float* w_packed,
                       const float* bias, int Cout, int stride, float* y, void* stream);

/* General NHWC convolution as implicit GEMM on MFMA (ResNet backbones, eval BatchNorm
 * folded into w/bias by the caller):  y = epi(conv(x, w) + bias), epilogue one of
 * PIPNET_EPI_NONE / _BIAS / _BIAS_RELU / _BIAS_RESID_RELU (R: [B,OH,OW,Cout]).
 * x: [B,H,W,Cin] NHWC, w_packed: [Cout][KH][KW][Cin], y: [B,OH,OW,Cout] with
 * OH = (H + 2 pad - KH)/stride + 1.  Replaces the Conv2d+BatchNorm2d(+ReLU)(+identity)
 * sequences of features/resnet_features.py:77-124,126-229.  Cin % 4 == 0. */
int pipnet_conv2d_nhwc_f32(const float* x, int B, int H, int W, int Cin, const float* w_packed,
                           const float* bias, int Cout, int KH, int KW, int stride, int pad,
                           const float* R, int epilogue, float* y, void* stream);

/* MaxPool2d(k, stride, pad) on NHWC (ResNet stem, resnet_features.py:136). */
int pipnet_maxpool2d_nhwc_f32(const float* x, int B, int H, int W, int C, int k, int stride, int pad,
                              float* y, void* stream);

/* NCHW -> NHWC with the channel dimension zero-padded to Cpad (network input of the ResNet
 * stem, so every implicit-GEMM tap is a 16-byte vector). */
int pipnet_nchw_to_nhwc_f32(const float* x, int B, int C, int H, int W, int Cpad, float* y, void* stream);

/* ---- bf16 ResNet path (BASELINE C3 "ResNet50 ... bf16 inference") -------------------
 * Activations are bf16 NHWC (passed as void*: raw 16-bit bfloat16 storage), accumulation
 * fp32 on v_mfma_f32_32x32x16_bf16, folded-BN bias fp32, outputs rounded to nearest even.
 * Same epilogues and semantics as pipnet_conv2d_nhwc_f32; w_packed: [Cout][Kp] bf16 with
 * Kp = KH*KW*Cin rounded up to a multiple of 64 (taps [KH][KW][Cin], zero beyond).
 * Cin % 8 == 0, Cout % 8 == 0, x / w / y / R 16-byte aligned. */
int pipnet_conv2d_nhwc_bf16(const void* x, int B, int H, int W, int Cin, const void* w_packed,
                            const float* bias, int Cout, int KH, int KW, int stride, int pad,
                            const void* R, int epilogue, void* y, void* stream);

/* Same, with the workgroup tile forced (tuning / tests): tile 0 = 64x128 (32-deep K tiles,
 * 4 LDS stages), 1 = 128x128 and 2 = 256x256 (64-deep, 2 stages), 3 = 256x256 and
 * 4 = 128x128 (32-deep, 4 stages), 5 = 256x256 ping-pong on 16x16x32 MFMAs (Cin % 32 == 0
 * unless 1x1 stride 1), 6 = 256x64 (32-deep, 4 stages), -1 = automatic (what
 * pipnet_conv2d_nhwc_bf16 uses: tile 5 for every N >= 256 layer it can serve, tile 6 for
 * N <= 64, whatever M; the MFMA shape and K order never depend on the batch size, so
 * neither do the results). */
int pipnet_conv2d_nhwc_bf16_tile(const void* x, int B, int H, int W, int Cin, const void* w_packed,
                                 const float* bias, int Cout, int KH, int KW, int stride, int pad,
                                 const void* R, int epilogue, void* y, int tile, void* stream);

/* ---- CountPIPNet finetune phase (pipnet/train.py:75-140, main.py:333-343: classifier +
 * intermediate layer train) ------------------------------------------------------------
 * Train-mode (soft) Gumbel head, F.gumbel_softmax(hard=False) (count_pipnet_utils.py:34-35):
 * proto = softmax((x - log E) / tau) [B,HW,P] NHWC, sums [B,P] = spatial sums = the raw
 * counts (count_pipnet.py:88), added in a fixed order: the same bits in every run.  With
 * HW > 16 the call takes a scratch of B * ceil(HW / 16) * P floats from the device's
 * stream-ordered pool on `stream` and returns it there.  exp_noise / seed / offset as
 * pipnet_count_gumbel_f32. */
int pipnet_count_gumbel_soft_f32(const float* logits, int B, int HW, int P, float tau, const float* exp_noise,
                                 uint64_t seed, uint64_t offset, float* proto, float* sums, void* stream);

/* dx = d_out relu(W)  (NonNegLinear input gradient; d_out [N,K], W [K,D], dx [N,D]). */
int pipnet_nonneg_linear_dx_f32(const float* d_out, const float* W, int N, int D, int K, float* dx, void* stream);

/* BilinearIntermediate backward front: du = g * v, dv = g * u (n elements). */
int pipnet_bilinear_bwd_prep_f32(const float* g, const float* u, const float* v, int64_t n, float* du, float* dv,
                                 void* stream);

/* LinearIntermediate backward (count_pipnet_utils.py:471-519, Linear(1, E, bias=False) over
 * the counts x [n = B*P]): g [n][E] -> dx [n] = g w (dx may be NULL) and dw [E] = g^T x
 * (accumulate adds); partial: pipnet_linear_inter_partials_floats(E) floats; E <= 16. */
int pipnet_linear_inter_partials_floats(int E);
int pipnet_linear_inter_bwd_f32(const float* x, int64_t n, int E, const float* g, const float* w, float* dx,
                                float* dw, int accumulate, float* partial, void* stream);

/* ---- split-bf16 ("bf16x3") fp32 path of the ConvNeXt backbone -------------------------
 * An fp32 operand x is carried as two bf16 values, hi = RNE(x) and lo = RNE(x - hi)
 * (x = hi + lo to ~2^-17 relative).  A product x.w is then hi.hi + lo.hi + hi.lo (the
 * lo.lo term, ~2^-16 relative, is dropped), accumulated in fp32 -- a bf16 GEMM over K' = 3K
 * whose A rows are read as [hi(x) | lo(x) | hi(x)] and whose weight rows are
 * [hi(w) | hi(w) | lo(w)] per tap.  Activations are stored as "split planes" [hi | lo]
 * (2 Cin bf16 per pixel = the fp32 bytes); the kernel reads the third K segment from the
 * hi plane again.  Per-product error ~1e-5 relative (fp32: 6e-8) at 3/16 of the fp32-MFMA
 * cost (v_mfma_f32_16x16x32_bf16 / 32x32x16_bf16 vs v_mfma_f32_32x32x2_f32).  Replaces the
 * same torchvision CNBlock Linears and downsample convs as pipnet_linear_f32 /
 * pipnet_conv2x2_f32.
 *   x: [B,H,W,2 Cin] split planes (Cin % 32 == 0), w_packed: [Cout][Kp] bf16 with taps
 *   [KH][KW][3 Cin] (Kp = KH*KW*3Cin rounded up to 32, zero beyond), bias / scale [Cout]
 *   fp32 or NULL.  epilogue PIPNET_EPI_S3_GELU: y = split planes [B,OH,OW,2 Cout] bf16 of
 *   gelu(conv + bias); PIPNET_EPI_F32_BIAS: y fp32 [B,OH,OW,Cout]; PIPNET_EPI_F32_RESID:
 *   y = R + scale * (conv + bias), fp32, R [B,OH,OW,Cout] (may equal y).  tile as
 *   pipnet_conv2d_nhwc_bf16_tile (only -1, 0, 4, 5). */
int pipnet_conv2d_nhwc_s3(const void* x, int B, int H, int W, int Cin, const void* w_packed,
                          const float* bias, const float* scale, const float* R, int Cout, int KH, int KW,
                          int stride, int pad, int epilogue, void* y, int tile, void* stream);

/* pipnet_dwconv7_ln_f32 writing its output as split planes [B,H,W,2C] bf16 [hi | lo] (the A
 * operand of the split-bf16 Linear1). */
int pipnet_dwconv7_ln_s3(const float* x, int B, int H, int W, int C, const float* w_packed,
                         const float* bias, const float* ln_w, const float* ln_b, void* y, void* stream);

/* pipnet_layernorm_f32 writing split planes [rows, 2C] bf16 (input of a split-bf16 downsample conv). */
int pipnet_layernorm_s3(const float* x, int64_t rows, int C, const float* w, const float* b, void* y,
                        void* stream);

/* ---- plain bf16 build of the ConvNeXt backbone ("bf16") ---------------------------------
 * The CNBlock Linears and the downsample convs with ONE bf16 product per multiply (a third of the
 * split GEMM's MFMA work): A is plain bf16 [B,H,W,Cin] (Cin % 32 == 0), w_packed what
 * pipnet_pack_conv_weight_bf16 makes ([Cout][Kp], Kp = KH*KW*Cin rounded up to 64, zero beyond),
 * fp32 accumulation on the split GEMM's tiles (tile: -1 automatic, 0, 4, 5, 7; any other tile is
 * PIPNET_ERR_ARG; the choice is per layer, so per-image results do not depend on the batch size).
 *   PIPNET_EPI_BIAS_GELU: y = bf16 [B,OH,OW,Cout], gelu_erf(conv + bias) rounded once (RNE);
 *   PIPNET_EPI_F32_BIAS:  y = fp32 conv + bias;
 *   PIPNET_EPI_F32_RESID: y = R + scale * (conv + bias), fp32 R [B,OH,OW,Cout] (may equal y).
 * bias / scale [Cout] fp32 (bias may be NULL); the residual stream stays fp32. */
int pipnet_conv2d_nhwc_bf16_mix(const void* x, int B, int H, int W, int Cin, const void* w_packed,
                                const float* bias, const float* scale, const float* R, int Cout, int KH, int KW,
                                int stride, int pad, int epilogue, void* y, int tile, void* stream);

/* The CNBlock's Linear2 * layer_scale + residual under torchvision's StochasticDepth("row") in train mode,
 * on the low-precision operands -- what pipnet_linear_rowscale_f32 is to pipnet_linear_f32:
 *   y[M,Cout] = R + row_scale[min(m, M-1) / rows_per_scale] * (scale * (x W^T + bias)),   fp32 y and R,
 * R may equal y; rows_per_scale = H*W (one factor per sample), row_scale[b] = keep_b / (1 - p) -- 0 leaves a
 * dropped sample's rows equal to R (bit for bit); the multiplication order is the fp32 entry's.  The dense
 * 1x1 form only: x = [M,Cin] plain bf16 rows against a pipnet_pack_conv_weight_bf16 weight (_bf16_mix_), or
 * [M,2 Cin] split planes against a split weight (_s3_), operands and tiles (-1, 0, 4, 5, 7) exactly as
 * PIPNET_EPI_F32_RESID of pipnet_conv2d_nhwc_bf16_mix / pipnet_conv2d_nhwc_s3 takes them, so a block with
 * p = 0 and a block with p > 0 share their tile and their K order.  scale, R and row_scale are required
 * (row_scale: at least ceil(M / rows_per_scale) floats, not checked here); rows_per_scale > 0.  The kernels
 * carry epilogue code 13 (PIPNET_EPI_F32_RESID_ROWSCALE, csrc/gemm_bf16_impl.hpp): no `epilogue` argument
 * of this header accepts it. */
int pipnet_linear_bf16_mix_rowscale(const void* x, int64_t M, int Cin, const void* w_packed, const float* bias,
                                    const float* scale, const float* R, int Cout, const float* row_scale,
                                    int rows_per_scale, void* y, int tile, void* stream);
int pipnet_linear_s3_rowscale(const void* x, int64_t M, int Cin, const void* w_packed, const float* bias,
                              const float* scale, const float* R, int Cout, const float* row_scale,
                              int rows_per_scale, void* y, int tile, void* stream);

/* pipnet_dwconv7_ln_f32 / pipnet_layernorm_f32 with the result rounded once (RNE) to bf16
 * ([B,H,W,C] / [rows,C]): bitwise the hi plane of the _s3 producers (one shared kernel body). */
int pipnet_dwconv7_ln_bf16(const float* x, int B, int H, int W, int C, const float* w_packed,
                           const float* bias, const float* ln_w, const float* ln_b, void* y, void* stream);
int pipnet_layernorm_bf16(const float* x, int64_t rows, int C, const float* w, const float* b, void* y,
                          void* stream);

/* MaxPool2d(k, stride, pad) on NHWC bf16 (C % 8 == 0). */
int pipnet_maxpool2d_nhwc_bf16(const void* x, int B, int H, int W, int C, int k, int stride, int pad,
                               void* y, void* stream);

/* fp32 NCHW -> bf16 NHWC (round to nearest even), channels zero-padded to Cpad (% 8 == 0). */
int pipnet_nchw_to_nhwc_bf16(const float* x, int B, int C, int H, int W, int Cpad, void* y, void* stream);

/* Two 1x1 stride-1 bf16 convs over the same input in one launch (a ResNet stage's first
 * Bottleneck: the downsample conv + BN and conv1 + BN + ReLU, resnet_features.py:95-117):
 * w_packed = [N1 + N2, Kp] (rows 0..N1-1 the first conv), bias [N1 + N2];
 *   y1[M,N1] = x W1^T + b1,   y2[M,N2] = relu(x W2^T + b2).
 * x: [M, Cin] bf16 (NHWC pixels), N1 % 256 == 0, N2 % 256 == 0.  Each output equals the
 * single-conv launch bit for bit (same tile, same K order); the input is read once. */
int pipnet_conv1x1_bf16_dual(const void* x, int64_t M, int Cin, const void* w_packed, const float* bias, int N1,
                             void* y1, int N2, void* y2, void* stream);

/* ResNet stem input for a 3-channel k7 s2 p3 conv run as a 4x4 stride-1 conv: fp32 NCHW [B,3,H,W]
 * -> bf16 2x2 space-to-depth image [B, SH, SW, 16], SH = (H-1)/2 + 4, SW = (W-1)/2 + 4,
 * y[b][i][j][(2 bi + bj) * 4 + c] = x[b][c][2(i-2)+bi][2(j-2)+bj] (zero outside the image and for
 * c = 3).  The matching weights are W'[o][a][a'][(2 bi + bj) * 4 + c] = w[o][c][2a+bi-1][2a'+bj-1]. */
int pipnet_nchw_to_s2d_bf16(const float* x, int B, int H, int W, void* y, void* stream);
/* ResNet stem (4x4 stride-1 conv over the s2d image, 16 -> 64 channels, + bias + ReLU) fused
 * with MaxPool2d(3, 2, 1) -- replaces the conv1 / bn1 / relu / maxpool sequence of
 * resnet_features.py:161-164 in the bf16 build.  s2d: [B][SH][SW][16] bf16 from
 * pipnet_nchw_to_s2d_bf16; w: packed [64][256] bf16 (the regrouped 4x4x16 stem weight, BN
 * folded); bias: [64] fp32; y: [B][PH][PW][64] bf16, PH = (SH - 4) / 2 + 1.  SW - 3 <= 112.
 * Bitwise equal to pipnet_conv2d_nhwc_bf16 (4x4, EPI_BIAS_RELU) + pipnet_maxpool2d_nhwc_bf16. */
int pipnet_stem_pool_bf16(const void* s2d, int B, int SH, int SW, const void* w, const float* bias, void* y,
                          void* stream);

/* pipnet_softmax_pool_f32 reading bf16 logits (fp32 softmax, fp32 proto / pooled out).  Both, and
 * the fused forms below: B == 0 with valid HW, P, pool_mode is PIPNET_OK whatever the pointers
 * (an empty batch has none). */
int pipnet_softmax_pool_bf16(const void* feat, int B, int HW, int P, int pool_mode, float* proto,
                             float* pooled, void* stream);

/* The whole PIP-Net head in ONE kernel launch (pipnet.py:33-37; replaces pipnet_softmax_pool_f32
 * (pool_mode 0) + pipnet_nonneg_linear_f32): per-pixel softmax over P channels, proto written
 * once, spatial max into pooled [B,P], then -- in the last workgroup to finish image b (an
 * arrival ticket) -- x' = where(pooled < thresh, 0, pooled) when apply_thresh, else pooled,
 * written to x_out [B,P] (may be NULL), and out [B,K] = x' relu(W)^T + bias, W [K,P] read at
 * call time.  Bitwise equal to the two-kernel path.  W 16-B aligned when P % 4 == 0.  _bf16:
 * bf16 logits.
 * part: pipnet_softmax_pool_linear_part_floats(B, HW, P) (= B * P) floats of scratch for the
 * running maxima, tickets: int32 [B] arrival counters -- BOTH must be ZERO on entry: zero them once
 * at allocation; every completed call leaves part[0 .. B*P) and tickets[0 .. B) zero again, so no
 * memset is needed between calls.  Calls that may run concurrently (different streams) need
 * separate part / tickets buffers. */
int64_t pipnet_softmax_pool_linear_part_floats(int B, int HW, int P);
int pipnet_softmax_pool_linear_f32(const float* feat, int B, int HW, int P, float* proto, float* pooled,
                                   const float* W, const float* bias, int K, int apply_thresh, float thresh,
                                   float* x_out, float* out, float* part, int32_t* tickets, void* stream);
int pipnet_softmax_pool_linear_bf16(const void* feat, int B, int HW, int P, float* proto, float* pooled,
                                    const float* W, const float* bias, int K, int apply_thresh, float thresh,
                                    float* x_out, float* out, float* part, int32_t* tickets, void* stream);

/* ---- eval_pipnet metric loop (pipnet/test.py:67-131,266-319) -------
 * One evaluation batch, entirely on the device (no host sync):
 *   pooled [B,P] (clamped presence / counts), out [B,K] logits, W [K,P] the prototype->class
 *   weights the reference multiplies with (PIP-Net: the sparsified classification weight;
 *   CountPIPNet: get_prototype_importance_per_class stacked), ys [B] int64 labels,
 *   multiplier -> normalization_multiplier (device scalar, may be NULL = 1), thr = 1e-3.
 * Writes ys_pred [B] (torch.max index) and score [B] (amax softmax(log1p(out^m))); adds into
 * cm [K,K] int64 (cm[y][pred]), acc[5] fp64 running sums of the per-batch means
 * {true-class local size, all-class local size, prototypes per class, almost-nonzeros,
 * top-1}, *abstained (images whose max logit is 0).  workspace: int32 [5B + K]. */
int pipnet_eval_batch_f32(const float* pooled, const float* out, const float* W, int B, int P, int K,
                          const int64_t* ys, const float* multiplier, float thr, int32_t* ys_pred,
                          float* score, int64_t* cm, double* acc, int64_t* abstained, int32_t* workspace,
                          void* stream);

/* In-place classifier sparsification of eval_pipnet (test.py:71-73): w = max(w - delta, 0). */
int pipnet_weight_sparsify_f32(float* w, int64_t n, float delta, void* stream);

/* ConvNeXt stem: Conv2d(3,96,k4,s4,bias) + LayerNorm2d(96, eps 1e-6)  (features.0).
 * x: [B,3,H,W] NCHW (the reference's own input layout), w: [96,3,4,4] as torch stores it,
 * y: [B,H/4,W/4,96] NHWC.  H, W multiples of 4; x, w, b, ln_w, ln_b, y 16-byte aligned. */
int pipnet_convnext_stem_f32(const float* x, int B, int H, int W, const float* w, const float* b,
                             const float* ln_w, const float* ln_b, float* y, void* stream);

/* CNBlock front half: depthwise Conv2d 7x7 pad 3 (+bias) + LayerNorm(C, eps 1e-6).
 * x, y: [B,H,W,C] NHWC, w_packed: [49][C] (torch [C,1,7,7] transposed).
 * C in {96,192,384,768}. */
int pipnet_dwconv7_ln_f32(const float* x, int B, int H, int W, int C, const float* w_packed,
                          const float* bias, const float* ln_w, const float* ln_b, float* y,
                          void* stream);

/* Row LayerNorm over the last dim (LayerNorm2d on NHWC), eps 1e-6: y = LN(x) * w + b. */
int pipnet_layernorm_f32(const float* x, int64_t rows, int C, const float* w, const float* b,
                         float* y, void* stream);

/* PIP-Net head, part 1 (pipnet.py:33-34): per-pixel softmax over P prototype channels
 * (nn.Softmax(dim=1)), proto written once (NHWC), fused spatial pooling:
 *   pool_mode 0 -> pooled[b,p] = max over pixels (AdaptiveMaxPool2d(1)+Flatten)
 *   pool_mode 1 -> pooled[b,p] = sum over pixels (CountPIPNet softmax activation, :88)
 * feat, proto: [B,HW,P]; pooled: [B,P] (zeroed by this call before accumulation). */
int pipnet_softmax_pool_f32(const float* feat, int B, int HW, int P, int pool_mode, float* proto,
                            float* pooled, void* stream);

/* ---- prototype explanations (util/vis_pipnet.py:187-275, 652-755: the top-k patches per
 * prototype; csrc/explain.hip) -------------------------------------------------------------
 * Location rule, everywhere below: the reference's two-step max (vis_pipnet.py:235-238)
 *   max_h, h_idx = torch.max(map, dim=0); max_w, w_idx = torch.max(max_h, dim=0)
 * i.e. among the pixels holding the map's maximum the smallest w, then the smallest h in that
 * column (column-major first, NOT the flat row-major argmax).  loc = h * W + w.
 *
 * pipnet_softmax_pool_argmax_f32: pipnet_softmax_pool_f32 (pool_mode 0) that also reports where
 *   each prototype's maximum sits.  feat [B,H,W,P] NHWC logits; pooled [B,P] and proto (when
 *   non-NULL; NULL skips the store of the map) are bit for bit pipnet_softmax_pool_f32's; loc
 *   [B,P] int32; an all-zero map gives value 0 at (0,0).  workspace: B * P * 8 bytes, 8-B aligned
 *   (zeroed by this call).  B <= 65535.
 * pipnet_map_argmax_f32: value and location of the maximum of a stored fp32 NHWC map [B,H,W,P] of
 *   any sign (the CountPIPNet 0/1 map, the bf16 head's fp32 proto map).  NaN entries are passed over.
 * pipnet_topk_update: one batch merged into the running top-k of every (group, prototype):
 *   score / loc [B,P] (loc >= 0), image b has dataset index i0 + b; group [B] int32 or NULL (all in group 0),
 *   an id outside [0, G) -- e.g. -1 -- skips the image; use_min: candidates with score < min_score
 *   are skipped.  State (caller-owned, device): st_score [G,P,k] fp32, st_index [G,P,k] int64
 *   (initialise to -1 = empty slot), st_loc [G,P,k] int32, st_fill [G,P] int32 (initialise to 0).
 *   After any sequence of calls the state is the reference's one-image-at-a-time list
 *   (vis_pipnet.py:248-274): the k best by (score descending, dataset index ascending).
 *   1 <= k <= PIPNET_TOPK_MAX_K.  out [B,K] (NULL to skip): images with amax(out) == 0 are added to *abstained
 *   (device int64; vis_pipnet.py:217-219), whatever their group.  The test is torch's: a maximum of +0.0 or
 *   -0.0 abstains, a subnormal maximum does not (fp32 subnormals are kept, not flushed), and a NaN anywhere in
 *   the row means not abstained (torch.amax propagates it and NaN == 0 is false).  A negative st_fill entry is
 *   read as 0, one above k as k, and a stored st_loc below -1 as -1. */
#define PIPNET_TOPK_MAX_K 32
int pipnet_softmax_pool_argmax_f32(const float* feat, int B, int H, int W, int P, float* proto, float* pooled,
                                   int32_t* loc, void* workspace, void* stream);
int pipnet_map_argmax_f32(const float* map, int B, int H, int W, int P, float* val, int32_t* loc, void* stream);
int pipnet_topk_update(const float* score, const int32_t* loc, int B, int P, int64_t i0, const int32_t* group,
                       int G, int use_min, float min_score, const float* out, int K, int k, float* st_score,
                       int64_t* st_index, int32_t* st_loc, int32_t* st_fill, int64_t* abstained, void* stream);

/* ---- local explanations (util/visualize_prediction.py:63-75, 139-154: which prototypes were
 * found in this image, where, and what each adds to each top class; csrc/explain.hip) ---------
 * pipnet_local_explain_f32: per image the C best classes and, for each, its contributing
 *   prototypes.  pooled [B,P] (clamped pooled scores or counts), loc [B,P] (h * W + w, as the
 *   arg-location entry points write it), out [B,K] logits, W [K,P] with row stride ldw >= P.
 *   Class order: logit descending, equal logits lower class index first (C == K: all classes,
 *     vis_pred_experiments; C = 3: vis_pred).
 *   Prototype order: pooled descending, equal scores lower prototype index first -- a stable
 *     descending sort (torch.sort leaves ties open; counts tie all the time).
 *   Keep test: pair (c, p) is kept iff |pooled[p] * W[c,p]| > min_abs, the product taken in fp64
 *     (exact for two fp32 factors): the decision of the reference's Python-float product for
 *     every input.  min_abs >= 0, so a score of +-0 is never kept.
 *   Per (image, class rank r): cls [B,C] the class, cls_logit [B,C] its logit, n [B,C] the number
 *     of kept pairs -- the true number, also when it exceeds M.  Per slot, e_* [B,C,M]: slots
 *     0 .. min(n, M) - 1 hold the kept pairs in prototype order (prototype, pooled, weight, the
 *     product rounded to fp32, loc), the others (-1, 0, 0, 0, -1).  Every output element is
 *     written by the one kernel (no zeroed buffer, no memset: graph-capturable).
 *   1 <= C <= K <= PIPNET_LOCAL_EXPLAIN_MAX, 1 <= P <= PIPNET_LOCAL_EXPLAIN_MAX, M >= 1, B >= 0; a limit violation, a negative (or NaN)
 *   min_abs or a NULL pointer returns PIPNET_ERR_ARG before any HIP call; B == 0 is PIPNET_OK.
 *   Non-finite scores / logits land somewhere in the order (a NaN product is never kept); they
 *   cannot make the kernel read or write out of bounds or loop. */
#define PIPNET_LOCAL_EXPLAIN_MAX 2048 /* the limit on P and K above */
int pipnet_local_explain_f32(const float* pooled, const int32_t* loc, const float* out, const float* W, int64_t ldw,
                             int B, int P, int K, int C, int M, double min_abs, int32_t* cls, float* cls_logit,
                             int32_t* n, int32_t* e_proto, float* e_sim, float* e_w, float* e_simw, int32_t* e_loc,
                             void* stream);

/* Fused CNBlock MLP of the narrow ConvNeXt stages (torchvision CNBlock block.3-5 + layer_scale +
 * residual; the Linear / GELU / Linear of features.1 and features.3):
 *   x[M,C] += gamma * (W2 gelu_erf(W1 t + b1) + b2)        in place on x
 * t: [M,C] (dwconv7 + LayerNorm output), W1: [4C,C], b1: [4C], W2: [C,4C], b2 / gamma: [C];
 * C = 96 or 192; exact fp32 (v_mfma_f32_16x16x4_f32), the 4C-wide hidden activation never
 * leaves the registers.  All pointers 16-B aligned. */
int pipnet_cnblock_mlp_f32(const float* t, const float* W1, const float* b1, const float* W2, const float* b2,
                           const float* gamma, float* x, int64_t M, int C, void* stream);
/* Same, told the layer's feature-map size hw = H*W per image (0 = unknown, as above): C = 192 on
 * maps of <= 256 pixels splits the hidden dimension over two waves per 16-pixel group (another
 * fixed summation order, chosen by hw only, so a pixel's result never depends on M). */
int pipnet_cnblock_mlp_hw_f32(const float* t, const float* W1, const float* b1, const float* W2, const float* b2,
                              const float* gamma, float* x, int64_t M, int C, int hw, void* stream);

/* NonNegLinear (pipnet.py:54-71, count_pipnet.py:176-224): out = x' relu(W)^T + b with
 * x' = where(x < thresh, 0, x) when apply_thresh (pipnet.py:36, inference) else x.
 * x: [B,D], W: [K,D] read at call time (callers mutate it in place, test.py:73),
 * bias [K] or NULL, x_out: [B,D] receives x' (may be NULL), out: [B,K]. */
int pipnet_nonneg_linear_f32(const float* x, int B, int D, const float* W, const float* bias,
                             int K, int apply_thresh, float thresh, float* x_out, float* out,
                             void* stream);

/* CountPIPNet Gumbel-softmax (eval, hard=True) + spatial count (count_pipnet_utils.py:36-38,
 * count_pipnet.py:88): per pixel z = (x - log E)/tau, one-hot at argmax written as the
 * straight-through value (1 - y) + y, all other channels exactly 0, and hist[b,p] += 1.
 * E ~ Exp(1) is read from exp_noise ([B,P,HW], the NCHW layout of torch's draw) when
 * non-NULL, else generated in-kernel by Philox4x32-10 keyed by (seed, offset + element/4):
 * one 128-bit block feeds channels 4k..4k+3 of a pixel.
 * logits, proto: [B,HW,P], 16-byte aligned, P % 4 == 0; hist: [B,P] int32 (zeroed by this call).
 * B == 0 with valid HW, P, tau is PIPNET_OK whatever the pointers (an empty batch has none). */
int pipnet_count_gumbel_f32(const float* logits, int B, int HW, int P, float tau,
                            const float* exp_noise, uint64_t seed, uint64_t offset, float* proto,
                            int32_t* hist, void* stream);

/* Same, graph-replayable: the Philox key is device memory.  seed_state: uint64[2] on the
 * device ([0] a splitmix64 counter, [1] the key); each call first advances the counter and
 * derives a new key on the stream (fresh noise per call, as the reference draws fresh
 * noise), so a captured hipGraph replays with new noise every time. */
int pipnet_count_gumbel_devseed_f32(const float* logits, int B, int HW, int P, float tau,
                                    uint64_t* seed_state, float* proto, int32_t* hist, void* stream);

/* The Gumbel heads' Exp(1) noise on its own (parity tests; oracle/philox_ref.py restates it):
 * out[i] for i < n (n % 4 == 0) = the draw count_gumbel_kernel uses for element i of its NHWC
 * [B,HW,P] stream under (seed, offset): word i % 4 of Philox4x32-10 block offset + i/4, E = -log u
 * with u = (top 24 bits + 1/2) 2^-24 floored at E >= 2^-25.  log_e = 0: E (the soft head's libm
 * form); log_e = 1: log E on the hard head's hardware-log form.  Replaces the
 * `-torch.empty_like(x).exponential_().log()` draw inside F.gumbel_softmax (count_pipnet_utils.py:36-38). */
int pipnet_philox_exp1_f32(uint64_t seed, uint64_t offset, int64_t n, int log_e, float* out, void* stream);

/* fp32 GEMM variant plan: the variant pipnet_linear_f32 (and the conv / rowscale forms) launch for an
 * M x N x K product with dense 16-B aligned operands, PIPNET_EPI_* epilogue and A-operand gather
 * (0 dense / linear, 1 the 2x2 patch conv, 2 the general NHWC conv) -- 0 K-tail kernel, 1 BK16
 * 128-row, 2 BK32 64-row, 3 BK32 128-row, 5 BK32 192 x 384 on 12 waves -- or -PIPNET_ERR_ARG. */
int pipnet_linear_f32_plan(int M, int N, int K, int epilogue, int aload);

/* bf16 conv tile plan: the tile id pipnet_conv2d_nhwc_bf16_tile takes for this shape / epilogue
 * (tile -1 = the automatic choice, >= 0 validated), or -PIPNET_ERR_ARG.  The library's own rule. */
int pipnet_conv2d_nhwc_bf16_plan(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                                 int epilogue, int tile);

/* Profiling labels: the name of the kernel a launch with these shape arguments runs, as rocprof and nm -C
 * print it (e.g. "pipnet_bf16::conv_bf16_pp_kernel<5, 0, 4, 0, 2>").  Each query runs the selection of its
 * launch (pipnet_linear_f32 and its rowscale / conv forms, splits > 1: the main kernel of the split-K
 * entries; pipnet_conv2d_nhwc_bf16_tile; pipnet_conv2d_nhwc_s3; pipnet_conv2d_nhwc_bf16_mix;
 * pipnet_linear_bf16_mix_rowscale; pipnet_linear_s3_rowscale; pipnet_conv1x1_bf16_dual;
 * pipnet_cnblock_mlp_hw_f32) on dense 16-B aligned operands, as the plan queries do, without a HIP call.
 * Writes the NUL-terminated label into buf[cap] and returns its length, or -PIPNET_ERR_ARG when the launch
 * would be refused or the label does not fit. */
int pipnet_linear_f32_label(int M, int N, int K, int epilogue, int aload, int splits, char* buf, int cap);
int pipnet_conv2d_nhwc_bf16_label(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                                  int epilogue, int tile, char* buf, int cap);
int pipnet_conv2d_nhwc_s3_label(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                                int epilogue, int tile, char* buf, int cap);
int pipnet_conv2d_nhwc_bf16_mix_label(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                                      int epilogue, int tile, char* buf, int cap);
int pipnet_linear_bf16_mix_rowscale_label(int64_t M, int Cin, int Cout, int tile, char* buf, int cap);
int pipnet_linear_s3_rowscale_label(int64_t M, int Cin, int Cout, int tile, char* buf, int cap);
int pipnet_conv1x1_bf16_dual_label(int64_t M, int Cin, int N1, int N2, char* buf, int cap);
int pipnet_cnblock_mlp_label(int64_t M, int C, int hw, char* buf, int cap);

/* Count finish (count_pipnet.py:88-97): counts_raw = float(hist) (or sums when hist is
 * NULL), clamped = clamp(round?(counts), 0, max_count) -- round when do_round.
 * sums: [B,P] float (softmax activation path) used when hist == NULL. */
int pipnet_count_finish_f32(const int32_t* hist, const float* sums, int B, int P, int max_count,
                            int do_round, float* counts_raw, float* clamped, void* stream);

/* Elementwise count encodings into [B, P*C] (p-major):
 *   kind 0 (OneHotEncoder, count_pipnet_utils.py:141-185): one-hot at clamp(int(x)-1,0,C-1)
 *          where x > 0.1, x rounded first when do_round (ModifiedSTEFunction :201-217);
 *   kind 1 (LinearIntermediate, :471-539): out[b,p*C+c] = x[b,p] * w[c]. */
int pipnet_count_encode_f32(const float* x, int B, int P, int C, int kind, int do_round,
                            const float* w, float* out, void* stream);

/* ---- evaluation input transform ----------------------------------
 * transform_no_augment of util/data.py (:264-269, :314-321, :500-505, :537-542, :568-574):
 * Resize((out_h, out_w)) [+ Grayscale(3)] + ToTensor + Normalize(mean, std), applied to a
 * ragged batch of decoded RGB images (ImageFolder's pil_loader: Image.open().convert('RGB')).
 * Resize restates Pillow's ImagingResample(BILINEAR) integer arithmetic exactly (torchvision
 * forwards a PIL image's Resize to it), so the uint8 resized image is bit-identical to
 * Pillow's and the fp32 output to ToTensor/Normalize of it.
 *
 * pipnet_resize_plan (host only): sizes_host [B][2] = (h, w) per image -> kmax (taps per
 *   output coordinate) and the device workspace size in bytes.
 * pipnet_resize_normalize_rgb8: pixels = the B images packed HWC uint8 (image b at byte
 *   offsets[b], device), sizes [B][2] int32 (device), mean3/std3 host float[3], workspace
 *   (device, from pipnet_resize_plan), out [B,3,out_h,out_w] fp32 NCHW, out_u8 optional
 *   [B,out_h,out_w,3] uint8 copy of the resized (and grayscaled) image, NULL to skip. */
int pipnet_resize_plan(const int32_t* sizes_host, int B, int out_h, int out_w, int* kmax,
                       int64_t* workspace_bytes);
int pipnet_resize_normalize_rgb8(const uint8_t* pixels, const int64_t* offsets, const int32_t* sizes,
                                 int B, int out_h, int out_w, int kmax, int grayscale,
                                 const float* mean3, const float* std3, int32_t* workspace,
                                 float* out, uint8_t* out_u8, void* stream);

/* ---- two-view training augmentation (util/data.py:261-617) --------------------------------
 * TwoAugSupervisedDataset's transform1 (once per image) and transform2 (once per view) on a
 * ragged batch of decoded RGB images.  The random parameters are drawn on the host
 * (count_pipnet_amd/augment.py) and passed as doubles; given the same parameters the pixel
 * arithmetic is bit-identical to Pillow 12.2.0 ("Training augmentation").
 *
 * gparams [B][PIPNET_AUG_GEOM_PARAMS] (device):
 *   0      warp path: 0 none, 1 Pillow's 16.16 fixed-point affine (m1 != 0 or m3 != 0),
 *          2 Pillow's double-precision affine (m1 == m3 == 0: translate / scale only)
 *   1..6   m0..m5, the output -> input matrix of Image.transform(AFFINE, NEAREST)
 *   7      fill colour (all three bands)        8  horizontal flip (0 / 1)
 *   9..12  crop box of RandomResizedCrop in the S1 x S1 image: top, left, height, width
 * vparams [V][B][PIPNET_AUG_VIEW_PARAMS] (device):
 *   0, 1   first colour operation and its parameter; 2, 3 the second (never Sharpness)
 *          0 identity, 1 Brightness, 2 Color, 3 Contrast, 4 Sharpness (parameter = ImageEnhance
 *          factor), 5 Posterize (bits), 6 Solarize (threshold), 7 AutoContrast, 8 Equalize
 *   4, 5   RandomCrop offset (top, left) of the s x s window in the S2 x S2 image
 *   6      add noise (0 / 1)                    7  image id (< 2^32) of the Philox counter
 *
 * pipnet_augment_geometry_plan (host only): sizes_host [B][2] = (h, w) -> taps per output
 *   coordinate of the two resamples and the device workspace size in bytes.
 * pipnet_augment_geometry_rgb8: Resize((S1, S1)) -> affine warp -> flip -> crop(box)
 *   .resize((S2, S2), BILINEAR) -> out_u8 [B,S2,S2,3].  pixels / offsets / sizes as
 *   pipnet_resize_normalize_rgb8.
 * pipnet_augment_view_rgb8: images [B,S2,S2,3] uint8 -> out [V,B,3,s,s] fp32 = colour
 *   operations (whole-image statistics from the S2 x S2 image), crop, [Grayscale(3)], / 255,
 *   [+ noise], (x - mean) / std.  noise: optional [V,B,3,s,s] addends for the flagged images;
 *   NULL draws N(0, noise_std^2) from Philox4x32-10 keyed by seed, counter (view, image id,
 *   pixel). */
#define PIPNET_AUG_GEOM_PARAMS 13
#define PIPNET_AUG_VIEW_PARAMS 8
int pipnet_augment_geometry_plan(const int32_t* sizes_host, int B, int S1, int S2, int* kmax1, int* kmax2,
                                 int64_t* workspace_bytes);
int pipnet_augment_geometry_rgb8(const uint8_t* pixels, const int64_t* offsets, const int32_t* sizes,
                                 const double* gparams, int B, int S1, int S2, int kmax1, int kmax2,
                                 int32_t* workspace, uint8_t* out_u8, void* stream);
int pipnet_augment_view_rgb8(const uint8_t* images, const double* vparams, int V, int B, int S2, int s,
                             int grayscale, const float* mean3, const float* std3, float noise_std,
                             uint64_t seed, const float* noise, float* out, void* stream);

/* ---- training step, finetune phase (pipnet/train.py:75-140) ----
 * The batch is cat([xs1, xs2]) (train.py:84): N = 2*Bh rows, proto features NHWC
 * [N][HW][P] (rows n and Bh*HW + n are the two views of one pixel), pooled [N][P],
 * out [N][K], ys int64 [Bh] (row r's label is ys[r % Bh], train.py:155).
 *
 * pipnet_train_align_partial_f32: align_loss (train.py:259-265) partial sums, one double
 *   per workgroup into partial[pipnet_train_align_partials()].  P % 4 == 0 needs pf
 *   16-byte aligned.
 * pipnet_train_loss_f32 (train.py:154-250): stats[8] = {align, tanh, class, total loss,
 *   correct count, w_align, w_tanh, w_class}; mode 0 train, 1 pretrain (no class term, no
 *   d_out), 2 finetune (loss = w_class * class).  mult = normalization_multiplier (device
 *   float[1]); enforce = enforce_weight_sparsity (class input log1p(out^mult)).
 *   d_out [N][K] = d loss / d out (w_class * d class).
 * pipnet_nonneg_linear_bwd_f32 (pipnet.py:54-71 backward): dW = (W > 0) * d_out^T x,
 *   db = sum_r d_out (db may be NULL).  x [N][D], W/dW [K][D].
 * pipnet_adamw_step_f32: torch.optim.AdamW on one tensor at optimizer step ``step`` (1-based),
 *   hyper-parameters in double as torch's param_groups hold them (the float constants the
 *   kernel uses -- 1 - lr*wd, 1 - beta1, 1 - beta2, lr/(1 - beta1^t), sqrt(1 - beta2^t) --
 *   are derived from them in double, as torch does), then if post != 0
 *   p = max(p - post_delta, post_floor) (train.py:134-140's clamps).
 * pipnet_clamp_min_f32: x = max(x, lo) (normalization_multiplier clamp, train.py:137). */
int pipnet_train_align_partials(void);
int pipnet_train_align_partial_f32(const float* pf, int Bh, int HW, int P, double* partial, void* stream);
int pipnet_train_loss_f32(const double* align_partial, int Bh, int HW, const float* pooled, const float* out,
                          const int64_t* ys, int P, int K, const float* mult, int enforce, float tanh_coeff,
                          float w_align, float w_tanh, float w_class, int mode, float* d_out, float* stats,
                          void* stream);
int pipnet_nonneg_linear_bwd_f32(const float* d_out, const float* x, int N, int D, const float* W, int K,
                                 float* dW, float* db, void* stream);
int pipnet_adamw_step_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                          double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                          int post, float post_delta, float post_floor, void* stream);
int pipnet_clamp_min_f32(float* x, int64_t n, float lo, void* stream);

/* ---- backward building blocks (trainable ConvNeXt stages) ----
 * pipnet_wgrad_f32: C[N1][N2] (ldc) = (accumulate ? C : 0) + sum_m A[m][n1] B[m][n2]
 *   (A [M][N1] lda, B [M][N2] ldb, both pixel-major as the forward stores activations):
 *   the weight gradient dW = dY^T X of a Linear / 1x1 conv.  fp32 MFMA, deterministic
 *   (fixed pixel slabs, fixed-order reduction).  N1, N2, lda, ldb % 4 == 0, A/B 16-B
 *   aligned; workspace: pipnet_wgrad_workspace_bytes(M, N1, N2) bytes (needed unless the
 *   call runs as a single slab without accumulate; pass it whenever that size is > 0).
 *   M = 0 is the empty sum (C = 0, or C unchanged with accumulate; A, B may be NULL, the
 *   workspace is not touched).
 * pipnet_colsum_f32: out[n] = (accumulate ? out[n] : 0) + sum_m A[m][n] (bias gradients);
 *   workspace of pipnet_colsum_workspace_bytes(N) bytes. */
int64_t pipnet_wgrad_workspace_bytes(int M, int N1, int N2);
int pipnet_wgrad_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int M, int N1, int N2, float* C,
                     int64_t ldc, int accumulate, float* workspace, void* stream);
/* pipnet_wgrad_conv2x2_f32: weight gradient of the 2x2 downsample conv (stride 1 or 2):
 *   dW[co][(ky*2+kx)*Cin + ci] (+)= sum_{b,oy,ox} dY[b,oy,ox,co] x[b, oy*s+ky, ox*s+kx, ci]
 *   (the packed layout of pipnet_conv2x2_f32's weights); dY NHWC [B,OH,OW,Cout], x NHWC
 *   [B,H,W,Cin]; workspace: pipnet_wgrad_workspace_bytes(B*OH*OW, Cout, 4*Cin) bytes. */
int pipnet_wgrad_conv2x2_f32(const float* dY, const float* x, int B, int H, int W, int Cin, int stride, int Cout,
                             float* dW, int accumulate, float* workspace, void* stream);
/* pipnet_wgrad_conv_f32: weight gradient of a KHxKW conv, stride s, zero padding p (the
 * ConvNeXt stem, Conv2d(3, 96, 4, 4) with Cin zero-padded to 4; the ResNet 3x3 / strided 1x1
 * convs, features/resnet_features.py:17-28): dY NHWC [B][OH][OW][Cout], x NHWC [B][H][W][Cin]
 * -> dW [Cout][KH][KW][Cin] (accumulate adds); OH = (H + 2p - KH) / s + 1; workspace:
 * pipnet_wgrad_workspace_bytes(B*OH*OW, Cout, KH*KW*Cin). */
int pipnet_wgrad_conv_f32(const float* dY, const float* x, int B, int H, int W, int Cin, int KH, int KW, int stride,
                          int pad, int Cout, float* dW, int accumulate, float* workspace, void* stream);
int pipnet_colsum_workspace_bytes(int N);
int pipnet_colsum_f32(const float* A, int64_t lda, int M, int N, float* out, int accumulate, float* workspace,
                      void* stream);

/* ---- training backward of the trainable ConvNeXt suffix + PIP-Net head ----
 * Per-channel parameter gradients go through ``partial`` (device scratch of
 * pipnet_train_partials_floats(C) floats) and a fixed-order reduction; ``accumulate``
 * adds into the output instead of overwriting.  M = pixels (B*H*W), rows of C channels.
 * pipnet_gelu_fwd_f32: g = gelu_erf(h) (train forward keeps h for the backward).
 * pipnet_resid_scale_f32: out = x + row_scale[m / rows_per_scale] * (ls * y2)
 *   (CNBlock output with layer scale and stochastic depth; row_scale may be NULL).
 * pipnet_ls_bwd_f32: its backward w.r.t. y2 (dy2 = dy * ls * r), ls and the Linear2 bias.
 * pipnet_ln_bwd_f32: LayerNorm(C, eps 1e-6) backward from the pre-norm input z:
 *   dz (NULL to skip), d_gamma, d_beta.
 * pipnet_dwconv7_plain_f32: y (+)= [bias] + depthwise 7x7 pad 3 of x, w_packed [49][C]
 *   (the input gradient uses the spatially flipped taps, no bias, accumulate = 1).
 * pipnet_dwconv7_wgrad_f32: depthwise 7x7 weight ([49][C] packed) and bias gradients.
 * pipnet_head_bwd_f32: d loss / d logits of the PIP-Net head (softmax over P, max-pool over
 *   HW) for the align (w_align), tanh (w_tanh) and -- when d_out != NULL -- classifier terms
 *   (pipnet/train.py:154-265); proto NHWC [2Bh][HW][P], pooled [2Bh][P], W [K][P];
 *   argmax_ws int32 [2Bh*P], dpool_ws float [2Bh*P]. */
int64_t pipnet_train_partials_floats(int C);
int pipnet_gelu_fwd_f32(const float* h, float* g, int64_t n, void* stream);
int pipnet_resid_scale_f32(const float* x, const float* y2, const float* ls, const float* row_scale,
                           int rows_per_scale, int64_t M, int C, float* out, void* stream);
int pipnet_ls_bwd_f32(const float* dy, const float* y2, const float* ls, const float* row_scale, int rows_per_scale,
                      int64_t M, int C, float* dy2, float* d_ls, float* d_b2, int accumulate, float* partial,
                      void* stream);
int pipnet_ln_bwd_f32(const float* z, const float* dt, const float* gamma, int64_t M, int C, float* dz,
                      float* d_gamma, float* d_beta, int accumulate, float* partial, void* stream);
int pipnet_dwconv7_plain_f32(const float* x, int B, int H, int W, int C, const float* w_packed, const float* bias,
                             int accumulate, float* y, void* stream);
int pipnet_dwconv7_wgrad_f32(const float* dz, const float* x, int B, int H, int W, int C, float* dw_packed,
                             float* db, int accumulate, float* partial, void* stream);
int pipnet_head_bwd_f32(const float* proto, const float* pooled, int Bh, int HW, int P, const float* d_out,
                        const float* W, int K, float w_align, float w_tanh, float tanh_coeff, int32_t* argmax_ws,
                        float* dpool_ws, float* d_logits, void* stream);

/* ---- CountPIPNet pretrain / joint backward (pipnet/train.py:75-140 with is_count_pipnet;
 * count_pipnet.py:70-110, count_pipnet_utils.py:41-84, 188-321) ----------------------------
 * pipnet_count_ste_bwd_f32: d counts_raw from d clamped through STE_Round (identity) and
 *   ClampSTE(0, max_count) -- gated = 1 ("Gated": pass where the clamp input, rint(counts)
 *   with use_ste, the raw counts without, lies in [0, max_count]), 0 ("Identity").
 * pipnet_onehot_ste_bwd_f32: ModifiedSTEFunction.backward over rows = B*P of the encoding
 *   gradient g [rows][M]; x = the encoder input (clamped counts); strategy 0 = None/'none',
 *   1 = 'current_grad', 2 = 'max_grad'; flag_ws one int of workspace.  Reproduces the
 *   reference's effective behaviour (zero-count rows and the non-all-positive rows of a
 *   'max_grad' batch get 0: its chained mask assignments write temporaries).
 * pipnet_count_head_bwd_f32: d logits of the count head -- counts = spatial sums of
 *   proto = softmax((logits + g) * inv_tau) -- for the align (w_align), tanh (w_tanh on
 *   tanh_coeff * counts) terms plus d_counts_in (NULL or [2Bh][P], the classifier chain);
 *   proto NHWC [2Bh][HW][P], dcnt_ws float [2Bh*P]. */
int pipnet_count_ste_bwd_f32(const float* counts, int64_t n, int max_count, int use_ste, int gated,
                             const float* d_clamped, float* d_counts, void* stream);
int pipnet_onehot_ste_bwd_f32(const float* x, int64_t rows, int M, const float* g, int strategy, int respect_active,
                              int* flag_ws, float* dx, void* stream);
int pipnet_count_head_bwd_f32(const float* proto, const float* counts, int Bh, int HW, int P, const float* d_counts_in,
                              float w_align, float w_tanh, float tanh_coeff, float inv_tau, float* dcnt_ws,
                              float* d_logits, void* stream);

/* ---- data-parallel training (count_pipnet_amd/dist_train.py; csrc/backward_ops.hip, dist_train_ops.hip) ----
 * One process per GPU; a rank holds Bh of the global batch's Bh_all rows per view (both views of its rows).
 * pipnet_head_bwd_rows_f32 / pipnet_count_head_bwd_rows_f32: pipnet_head_bwd_f32 / pipnet_count_head_bwd_f32 for
 *   a shard of rows.  proto, pooled / counts, d_out / d_counts_in and d_logits cover the rank's 2 Bh rows
 *   ([view 1 | view 2]); the tanh term's column sums run over pooled_all / counts_all [2 Bh_all][P], the gathered
 *   rows of every rank in global order ([view 1 of all ranks | view 2 of all ranks]), each half's rows in
 *   ascending order; the align factor is 0.5 w_align / (Bh_all HW).  tcoef_ws float [2 P]: the tanh term per
 *   (half, prototype), computed once by a small kernel ahead of the d pooled kernel.  The device code is the
 *   full-batch entry points' own: a shard's d_logits equals the same rows of the full-batch call bit for bit,
 *   and with pooled_all == pooled, Bh_all == Bh the whole output does.
 * pipnet_pack_tensors_f32: one launch gathers n fp32 tensors into a flat arena (the gradients, ahead of the one
 *   all-reduce).  table: device int64 [n][3] = source address, arena offset in floats (a multiple of 4: slots
 *   start on 16 bytes), element count; a slot is the count rounded up to a multiple of 4 and its padding is
 *   written as 0; nothing outside the slots is written.  arena 16-byte aligned, n <= 65535; 16-byte loads and
 *   stores where the source is 16-byte aligned, element by element otherwise. */
int pipnet_head_bwd_rows_f32(const float* proto, const float* pooled, int Bh, int HW, int P, const float* d_out,
                             const float* W, int K, const float* pooled_all, int Bh_all, float w_align, float w_tanh,
                             float tanh_coeff, int32_t* argmax_ws, float* dpool_ws, float* tcoef_ws, float* d_logits,
                             void* stream);
int pipnet_count_head_bwd_rows_f32(const float* proto, const float* counts, int Bh, int HW, int P,
                                   const float* d_counts_in, const float* counts_all, int Bh_all, float w_align,
                                   float w_tanh, float tanh_coeff, float inv_tau, float* dcnt_ws, float* tcoef_ws,
                                   float* d_logits, void* stream);
int pipnet_pack_tensors_f32(const int64_t* table, int n, float* arena, void* stream);

/* fp64-accumulated product for inference-time weight folds (csrc/fold_f64.hip):
 *   C[M,N] (ldc) = RNE_f32( sum_k double(A[m,k]) * double(B[k,n]) ), A [M,K] (lda) and B [K,N]
 *   (ldb) row-major fp32, products and sums in fp64 on v_mfma_f64_16x16x4_f64, any sizes.
 * Replaces the float64 torch matmul of the BilinearIntermediate fold (the embedding folded into
 * W and V: W(embed(x)) * V(embed(x)) = (W E) x * (V E) x, count_pipnet_utils.py:378-385) --
 * run once per weight version, off the steady-state forward. */
int pipnet_matmul_f64acc_f32(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc,
                             int M, int N, int K, void* stream);
/* Two such products sharing B in one launch: C0 = A0 B, C1 = A1 B (A0, A1 [M,K] with one lda; C0, C1
 * [M,N] with one ldc).  The fold of W and V against the same embedding E (count_pipnet_utils.py:
 * 378-385) as one grid of 2 x ceil(M/128) x ceil(N/128) tiles. */
int pipnet_matmul2_f64acc_f32(const float* A0, const float* A1, int64_t lda, const float* B, int64_t ldb,
                              float* C0, float* C1, int64_t ldc, int M, int N, int K, void* stream);

/* ---- ResNet training step (csrc/bn_ops.hip): BatchNorm2d in train mode ------------------
 * Replaces the autograd of nn.BatchNorm2d(C) under net.train() in the ResNet Bottleneck /
 * stem (features/resnet_features.py:77-119, 137-140; pipnet/train.py:14), NHWC rows
 * x[M][C], M = B*H*W, C % 4 == 0 (and C/4 >= 64 or dividing 256), 16-B aligned operands.
 * pipnet_bn_stats_f32: mean / invstd of the batch (two-pass biased variance, eps), and when
 *   running_mean / running_var are given the momentum update with the unbiased variance
 *   (torch semantics); M >= 2 (torch: "Expected more than 1 value per channel").
 * pipnet_bn_apply_f32: y = gamma (x - mean) invstd + beta [+ residual] [ReLU].
 * pipnet_bn_backward_f32: g = dy [* (relu_out > 0)]; d_beta = sum g, d_gamma = sum g xhat,
 *   dx = gamma invstd (g - d_beta/M - xhat d_gamma/M) (dx NULL: parameters only); d_masked
 *   (optional) receives g -- the identity-path gradient of a residual block.
 *   workspace: pipnet_bn_workspace_floats(C) floats, for both calls.
 * pipnet_stride_scatter_f32: out[B][H][W][C] (+)= in[B][OH][OW][C] placed on the stride
 *   lattice (zeros elsewhere): the input gradient of a stride-s 1x1 conv, and the
 *   zero-inserted gradient a stride-s 3x3 conv's input gradient is convolved from.
 * pipnet_bn_slabs: host only, the number of row slabs the two column reductions split (M, C)
 *   over (1 .. 1024; 0 for a shape they reject). */
int64_t pipnet_bn_workspace_floats(int C);
int pipnet_bn_slabs(int64_t M, int C);
int pipnet_bn_stats_f32(const float* x, int64_t M, int C, float eps, float momentum, float* mean, float* invstd,
                        float* running_mean, float* running_var, float* workspace, void* stream);
int pipnet_bn_apply_f32(const float* x, int64_t M, int C, const float* mean, const float* invstd, const float* gamma,
                        const float* beta, const float* residual, int relu, float* y, void* stream);
int pipnet_bn_backward_f32(const float* x, const float* dy, const float* relu_out, int64_t M, int C,
                           const float* mean, const float* invstd, const float* gamma, float* dx, float* d_masked,
                           float* d_gamma, float* d_beta, float* workspace, void* stream);
int pipnet_stride_scatter_f32(const float* in, int B, int OH, int OW, int C, int H, int W, int stride, int accumulate,
                              float* out, void* stream);

/* ---- Integrated-gradients pixel attribution (util/saliency_methods.py IG / IDG behind the
 * wrappers of util/interpret_idg.py:101-135; csrc/attribution.hip) ---------------------------
 * The path is image_i = baseline + alpha_i (x - baseline); g_i = d target / d image_i.  No entry
 * point here uses an atomic: every result is bitwise reproducible.
 * pipnet_attr_path_images_f32: x [3,H,W] NCHW, baseline [3,H,W] or NULL (then the constant
 *   baseline_value), alpha [S] on the device -> out [S,H,W,4] NHWC, channel 3 zero (the layout
 *   pipnet_nchw_to_nhwc_f32 with cpad = 4 writes, which the unfused stem conv reads); each value
 *   is fma(alpha, x - b, b).  out 16-byte aligned, S <= 65535.
 * pipnet_attr_head_bwd_f32: d target / d logits [B,HW,P] of the prototype head from the upstream
 *   vector u [B,P] and the head's soft map soft [B,HW,P] (NHWC), any P >= 1 and any B <= 65535:
 *   pool_mode 0 (softmax + max-pool; loc [B,P] int32 = the pixel of each prototype's maximum,
 *   pipnet_softmax_pool_argmax_f32): d[b,pix,q] = [loc[b,q] == pix] u_q s_q - s_q a[b,pix] with
 *   a[b,pix] = sum_{p: loc[b,p] == pix} u_p s_p (inv_tau is not read);
 *   pool_mode 1 (soft-max or Gumbel-softmax + spatial sum; loc not read):
 *   d[b,pix,q] = inv_tau y_q (u_q - sum_p u_p y_p).
 * pipnet_attr_stem_dx_f32: input gradient of the ConvNeXt stem's Conv2d(3, O, 4, stride 4):
 *   dz [B,H/4,W/4,O] NHWC, w [O,3,4,4] (the module's weight) -> image b at dx + b * ldx as NCHW
 *   [3,H,W], dx[c, 4i+kh, 4j+kw] = sum_o dz[i,j,o] w[o,c,kh,kw]; rows / columns beyond the last
 *   whole patch get 0.  O <= 128, H, W >= 4, ldx >= 3 H W, B <= 65535.
 * pipnet_attr_path_weights_f32: the per-step coefficients of one target from its scores [S]:
 *   method 0 (ig) w_i = 1 / S; 1 (lig) cutoff = the first i with s_i > max(s) * alpha_star (fp32
 *   product; none -> 1, 0 -> 1), w_i = 1 / cutoff below it and 0 from it; 2 (idg, alphas [S] and
 *   substep [S] of the gradient pass) slope_0 = 0, slope_i = (s_i - s_{i-1}) / (alpha_i -
 *   alpha_{i-1}), w_i = slope_i substep_i / S.  *cutoff (device int64) = the steps averaged.
 * pipnet_attr_path_reduce_f32: out[e] = (x[e] - b[e]) * sum_i weights[i] grads[i * ldg + e], e < N,
 *   the sum taken in step order (a chain of FMAs); baseline NULL -> baseline_value.  16-byte loads
 *   and stores where ldg % 4 == 0 and the operands are 16-byte aligned, a scalar tail. */
int pipnet_attr_path_images_f32(const float* x, const float* baseline, float baseline_value, const float* alpha,
                                int S, int H, int W, float* out, void* stream);
int pipnet_attr_head_bwd_f32(const float* soft, const float* u, const int32_t* loc, int B, int HW, int P,
                             int pool_mode, float inv_tau, float* d_logits, void* stream);
int pipnet_attr_stem_dx_f32(const float* dz, const float* w, int B, int H, int W, int O, int64_t ldx, float* dx,
                            void* stream);
int pipnet_attr_path_weights_f32(const float* scores, const float* alphas, const float* substep, int S, int method,
                                 float alpha_star, float* weights, int64_t* cutoff, void* stream);
int pipnet_attr_path_reduce_f32(const float* grads, int64_t ldg, const float* weights, const float* x,
                                const float* baseline, float baseline_value, int S, int64_t N, float* out,
                                void* stream);

/* ---- class-conditional prototype activation statistics (util/histograms.py:206-209, 320,
 * 521-522, 590-591, 617-661, 687-707, 1031-1065; pipnet/count_pipnet.py:272-276: the dataset
 * mean behind the virtual weights; csrc/proto_stats.hip) -------------------------------------
 * pipnet_proto_stats_update_f32: one batch merged into the running per-(class, prototype)
 *   statistics.  act [B,P] fp32 with row stride lda >= P, labels [B] int64, thr the near-zero
 *   threshold, edges [NB+1] ascending fp32 (NB == 0: no histogram, edges / hist not read).
 *   State (caller-owned, device, zeroed before the first call; vmax starts at -inf):
 *     n_class [K] int64 images of class k;  n_ge / n_gt [K,P] int64 act >= thr / act > thr;
 *     total [K,P] fp64 sum of act;  total_gt [K,P] fp64 sum of act over act > thr;
 *     vmax [K,P] fp32 largest act (NaN passed over);
 *     hist [K,P,NB] int32 over the values with act > thr: bin i holds edges[i] <= act < edges[i+1],
 *       the last bin also act == edges[NB], values outside [edges[0], edges[NB]] (and NaN) are
 *       not counted -- np.histogram(values, bins=edges);
 *     bad [1] int64 labels outside [0, K): such an image changes nothing else.
 *   Every (k, p) entry of the state is owned by one thread, which walks the batch's images in
 *   order and updates with plain loads and stores (no floating-point atomic, no cross-thread
 *   sum): counters and both fp64 sums are accumulated in dataset order and are bitwise
 *   independent of how the dataset is cut into batches.
 *   1 <= B, P, K; lda >= P; 0 <= NB <= PIPNET_PROTO_STATS_MAX_BINS; a violation or a NULL pointer
 *   returns PIPNET_ERR_ARG before any HIP call.
 * pipnet_colsum_accum_f64: acc[d] += sum_b x[b][d] for x [B,D] fp32 (row stride ldx >= D) and
 *   acc [D] fp64, the images added in order by the one thread that owns column d (the streaming
 *   form of intermediate_features.mean(dim=0)).  1 <= B, D; same argument rule. */
#define PIPNET_PROTO_STATS_MAX_BINS 1024
int pipnet_proto_stats_update_f32(const float* act, int64_t lda, const int64_t* labels, int B, int P, int K, float thr,
                                  const float* edges, int NB, int64_t* n_class, int64_t* n_ge, int64_t* n_gt,
                                  double* total, double* total_gt, float* vmax, int32_t* hist, int64_t* bad,
                                  void* stream);
int pipnet_colsum_accum_f64(const float* x, int64_t ldx, int B, int D, double* acc, void* stream);

/* ---- prototype part purity (util/eval_cub_csv.py:16-175 evaluated from the rows of :178-215
 * "all" and :218-283 "topk"; csrc/part_purity.hip, row function csrc/part_purity_row.hpp) ------
 * A row is (prototype p, image i, loc = h_idx * W + w_idx of p's maximum in i).  Its patch is
 * util/vis_pipnet.py get_img_coordinates for the map shape (P, H, W) with patch size 32 and the
 * given skip (small_map != 0: the 26 x 26 small-stride rule), scaled to the original image in
 * fp64 as (height / (double)image_size) * h (width for w); a visible part (x, y) is in the patch
 * iff hmin <= y <= hmax and wmin <= x <= wmax.
 * Annotation table (device, whole dataset): xy [N,Q,2] fp64 (x, y), vis [N,Q] uint8, size [N,2]
 *   int32 (width, height); fold table merged [Q] int32 (merged part 0 .. M-1 of each id),
 *   is_left [Q] uint8 (the id is folded into its right partner), pair_index [Q] int32 (a left
 *   id's pair, in pair order).
 * State (caller-owned, device): n / hits [P,M] int64 zeroed (rows in which a member of m is
 *   visible / in which a visible member lies in the patch); first_key [P,M] uint64 all ones
 *   (smallest ordinal << 6 | slot over the rows in which m is present, slot = the visible own
 *   id's index q, or Q + pair_index through the left partner only: the insertion order of the
 *   reference's dict); rows [P] int64 zeroed; bad [1] int64 zeroed (dataset indices outside
 *   [0, N): such a row changes nothing else).
 * pipnet_part_purity_update ("all"): image b of the batch is dataset index i0 + b and gives a row
 *   for every p with relevant[p] != 0 and (double)pooled[b][p] > threshold (pooled [B,P] fp32, row
 *   stride lda >= P; loc [B,P] int32), ordinal i0 + b.  One owner thread per prototype walks the
 *   images in order with plain loads and stores: the state is bitwise independent of the batching.
 * pipnet_part_purity_rows ("topk"): index / loc [P,k] (a top-k state, k <= 32): slot j of a
 *   relevant p is a row with ordinal j; index < 0 is an empty slot.
 * pipnet_part_purity_finish: per prototype, over its present parts in ascending first_key:
 *   purity = hits / n (fp64); max_purity / max_part / max_sum by the reference's rules (higher
 *   purity; at equal non-zero purity the strictly larger hits; at purity 0 the last part), most_part
 *   / most_sum / most_purity of the first part with the strictly largest hits > 0 (-1, 0, 0 when
 *   none), in_csv = rows > 0, purity [P,M] (NaN where n == 0).
 * 1 <= B, P, k, N, H, W; B * P <= INT_MAX; 1 <= M <= Q <= PIPNET_PART_PURITY_MAX_PARTS;
 * image_size >= 32; skip >= 0; a violation or a NULL pointer returns PIPNET_ERR_ARG before any
 * HIP call. */
#define PIPNET_PART_PURITY_MAX_PARTS 32
int pipnet_part_purity_update(const float* pooled, int64_t lda, const int32_t* loc, const uint8_t* relevant, int B,
                              int P, int64_t i0, double threshold, int H, int W, int image_size, int skip,
                              int small_map, const double* xy, const uint8_t* vis, const int32_t* size, int64_t N,
                              const int32_t* merged, const uint8_t* is_left, const int32_t* pair_index, int Q, int M,
                              int64_t* n, int64_t* hits, uint64_t* first_key, int64_t* rows, int64_t* bad,
                              void* stream);
int pipnet_part_purity_rows(const int64_t* index, const int32_t* loc, const uint8_t* relevant, int P, int k, int H,
                            int W, int image_size, int skip, int small_map, const double* xy, const uint8_t* vis,
                            const int32_t* size, int64_t N, const int32_t* merged, const uint8_t* is_left,
                            const int32_t* pair_index, int Q, int M, int64_t* n, int64_t* hits, uint64_t* first_key,
                            int64_t* rows, int64_t* bad, void* stream);
int pipnet_part_purity_finish(const int64_t* n, const int64_t* hits, const uint64_t* first_key, const int64_t* rows,
                              int P, int M, uint8_t* in_csv, double* max_purity, int32_t* max_part, int64_t* max_sum,
                              int32_t* most_part, int64_t* most_sum, double* most_purity, double* purity,
                              void* stream);

/* ---- merges of the per-rank states of the dataset passes (csrc/state_merge.hip) --------------------
 * When the top-k, statistics and part-purity passes are sharded over ranks (contiguous blocks of the
 * dataset in rank order), each rank's state is all-gathered once and merged into the state one process
 * reaches over the whole dataset.  Every input pointer is rank 0's field; field f of rank r lies
 * rank_stride BYTES further per rank (one stride for all fields: a gathered buffer of W packed states;
 * a multiple of 8, not read at W == 1).  The out_* state is separate memory of one state's shapes.
 * One owner thread per output entry, plain loads in rank order r = 0 .. W-1 and one store; no atomic.
 * pipnet_topk_merge: per (group, prototype) the k best of the union of the ranks' lists by (score
 *   descending, dataset index ascending) -- a W-way merge of the sorted lists, heads in LDS --
 *   out_fill = min(k, sum of fill), empty slots score 0 / index -1 / loc -1, out_abstained the sum.
 *   This is the one-pass list bit for bit (each list is the k best of its block in that order).
 * pipnet_proto_stats_merge: n_class / n_ge / n_gt / hist / bad integer sums, vmax the maximum, total
 *   and total_gt the fp64 chain ((s_0 + s_1) + s_2) + ...: bitwise the one-pass sums when the addends
 *   are integers, else within 2 (n + W) 2^-53 * sum|x| of them.  NB == 0: hist / out_hist not read.
 * pipnet_colsum_merge_f64: out[d] = the same chain over acc [W][D] (pipnet_colsum_accum_f64's state).
 * pipnet_part_purity_merge: n / hits / rows / bad integer sums, first_key the UNSIGNED minimum (all
 *   ones: never inserted; keys hold the global row ordinal): bitwise the one-pass state.
 * 1 <= W <= PIPNET_STATE_MERGE_MAX_RANKS; 1 <= G, P, K, D; 1 <= k <= PIPNET_TOPK_MAX_K; 0 <= NB <=
 * PIPNET_PROTO_STATS_MAX_BINS; 1 <= M <= PIPNET_PART_PURITY_MAX_PARTS; a violation or a NULL pointer
 * returns PIPNET_ERR_ARG before any HIP call. */
#define PIPNET_STATE_MERGE_MAX_RANKS 16
int pipnet_topk_merge(const float* score, const int64_t* index, const int32_t* loc, const int32_t* fill,
                      const int64_t* abstained, int64_t rank_stride, int W, int G, int P, int k, float* out_score,
                      int64_t* out_index, int32_t* out_loc, int32_t* out_fill, int64_t* out_abstained, void* stream);
int pipnet_proto_stats_merge(const int64_t* n_class, const int64_t* n_ge, const int64_t* n_gt, const double* total,
                             const double* total_gt, const float* vmax, const int32_t* hist, const int64_t* bad,
                             int64_t rank_stride, int W, int K, int P, int NB, int64_t* out_n_class, int64_t* out_n_ge,
                             int64_t* out_n_gt, double* out_total, double* out_total_gt, float* out_vmax,
                             int32_t* out_hist, int64_t* out_bad, void* stream);
int pipnet_colsum_merge_f64(const double* acc, int64_t rank_stride, int W, int D, double* out, void* stream);
int pipnet_part_purity_merge(const int64_t* n, const int64_t* hits, const uint64_t* first_key, const int64_t* rows,
                             const int64_t* bad, int64_t rank_stride, int W, int P, int M, int64_t* out_n,
                             int64_t* out_hits, uint64_t* out_first_key, int64_t* out_rows, int64_t* out_bad,
                             void* stream);

/* ---- explanation images (util/vis_pipnet.py:298-319 / :836-849 patch grids, util/visualize_prediction.py
 * :80-88 patch and rectangle images; csrc/gallery_ops.hip) ----------------------------------------------
 * Frames and canvases are dense uint8 HWC images on the device: frames [F,fh,fw,3] (the out_u8 of
 * pipnet_resize_normalize_rgb8), canvases [C,ch,cw,3].
 * pipnet_patch_compose_rgb8: items [N,8] int32 (device), one row (frame, h0, h1, w0, w1, canvas, y, x) per
 *   item: canvases[canvas, y:, x:] = frames[frame, h0:min(h1,fh), w0:min(w1,fw)] (a window that runs past
 *   the frame is cut short, as a Python slice is).  The kernel also cuts the window at the canvas edge and
 *   passes over a row with a negative origin or a frame / canvas index out of range: it never reads outside
 *   a frame or writes outside a canvas.  Items whose cells overlap are written in no defined order.
 *   N == 0 launches nothing.
 * pipnet_draw_rects_rgb8: out [N,fh,fw,3]; out[n] = frames[src[n]] with the outline of
 *   rects[n] = (x0, y0, x1, y1) (both corners inclusive, PIL ImageDraw.rectangle(outline=, width=)) in the
 *   colour (r, g, b): pixel (x, y) is coloured iff x0 <= x <= x1 and y0 <= y <= y1 and (x < x0 + width or
 *   x > x1 - width or y < y0 + width or y > y1 - width), clipped to the frame.  That is Pillow's outline for
 *   boxes at least 2 * width + 1 pixels wide and tall; the caller refuses narrower ones.  |coordinate| and
 *   width below 2^30.  src [N] int32, rects [N,4] int32 (device).
 * fh * fw and ch * cw below 2^29; byte offsets are 64-bit.  A violation or a NULL pointer returns
 * PIPNET_ERR_ARG before any HIP call. */
int pipnet_patch_compose_rgb8(const uint8_t* frames, int F, int fh, int fw, const int32_t* items, int N,
                              uint8_t* canvases, int C, int ch, int cw, void* stream);
int pipnet_draw_rects_rgb8(const uint8_t* frames, int F, int fh, int fw, const int32_t* src, const int32_t* rects,
                           int N, int width, int r, int g, int b, uint8_t* out, void* stream);

/* ---- prototype similarity heatmaps (util/visualize_prediction.py:92-100, heatmap_p{p}.png;
 * csrc/heatmap_ops.hip) ------------------------------------------------------------------------------------
 * pipnet_heatmap_rgb8: per row (b, p, frame) of items [N,3] int32 (device) the S x S RGB picture the reference
 *   writes for prototype p of image b, bit for bit:
 *     q   = uint8(trunc(m * 255f)) of the map m = proto[b, :, :, p], saturated to 0..255 (domain 0 <= m <= 1 +
 *           2^-22; NaN is outside the contract and reads as 0);
 *     r   = Pillow's Image.resize((S, S), BICUBIC) of the 8-bit band q: horizontal pass, uint8 intermediate,
 *           vertical pass, each clip8(((1 << 21) + sum(u8 * k)) >> 22); a pass whose axis keeps its size is
 *           skipped;
 *     v   = fl(fl(w_heat * fl(lut[r][c] / 255f)) + fl(w_img * fl(frames[frame][y][x][c] / 255f))), float32, no
 *           fused multiply-add, correctly rounded divisions;
 *     out = uint8(trunc(fl(v * 255f))), saturated to 0..255 (plt.imsave(vmin=0, vmax=1) without its alpha band).
 *   proto [B,h,w,P] float32 (the NHWC storage of a forward's proto_features), frames [F,S,S,3] uint8, lut [256,3]
 *   uint8 (RGB; the caller's colour table, cv2.COLORMAP_JET reversed to RGB in the reference), out [N,S,S,3]
 *   uint8, resized [N,S,S] uint8 or NULL: the bytes r.  rows_h / rows_v [S,7] int32 (device): the coefficient
 *   row (xmin, n, k[0..5)) of every output column (w -> S) and output row (h -> S): Pillow's precompute_coeffs
 *   for the bicubic filter (a = -0.5, support 2) in doubles, normalised, in 22-bit fixed point rounded half away
 *   from zero (normalize_coeffs_8bpc); n <= 5.  Both pointers must be non-NULL; a table is read only where its
 *   pass runs.  The kernel
 *   clamps every index it reads from them, so a wrong table gives wrong pixels and no access outside an operand.
 *   Upscale only: 1 <= h, w <= S.  A row of items with b, p or frame out of range writes nothing.  Four pixels
 *   per lane (12-byte accesses) when S % 4 == 0 and frames, out and resized are 4-byte aligned, one byte per lane
 *   otherwise; the same bytes.  S * S below 2^29, N * ceil(S / 16) workgroups of 256 threads below 2^24 (a grid holds fewer than 2^32
 *   threads), and 4096 + 22 * (ceil16(S) +
 *   ceil16(w)) bytes of LDS within 64 KiB (S + w up to about 2,700); byte offsets are 64-bit.  N == 0 launches
 *   nothing.  A violation or a NULL pointer (but resized) returns PIPNET_ERR_ARG before any HIP call. */
int pipnet_heatmap_rgb8(const float* proto, int B, int h, int w, int P, const uint8_t* frames, int F, int S,
                        const int32_t* items, int N, const uint8_t* lut, const int32_t* rows_h, const int32_t* rows_v,
                        float w_heat, float w_img, uint8_t* out, uint8_t* resized, void* stream);

/* ---- prototype feature-map overlays (util/vis_pipnet.py:454-475 and :1000-1021, *_overlay.png;
 * csrc/overlay_ops.hip) ------------------------------------------------------------------------------------
 * pipnet_map_overlay: per row (b, p) of items [N,2] int32 (device) the arrays behind the reference's overlay of
 *   prototype p on image b: scipy.ndimage.zoom(m, (S / h, S / w)) of the map m = proto[b, :, :, p] (order 3, mode
 *   'constant', grid_mode False), mask = resized > 0.1 and overlay[y, x] = (*cmap(resized[y, x])[:3], alpha).
 *   The arithmetic contract.  h, w >= 3 and S >= 2.  Up to the final rounding everything is float64, every
 *   operation below is one IEEE operation (correctly rounded divisions), nothing is contracted into a fused
 *   multiply-add, and the order is the one written:
 *   prefilter (spline_filter, order 3; mode 'constant' takes the mirror boundary and pads nothing), along axis 0
 *     (every column) first, then along axis 1 (every row), with z = sqrt(3) - 2 and gain = (1 - z) * (1 - 1 / z);
 *     on a line c[0..n):
 *       1. c[i] *= gain for every i;
 *       2. zn = pow(z, n - 1), computed on the host with libm inside this entry point, once for h and once for w;
 *       3. c[0] = c[0] + zn * c[n-1];
 *       4. for i = 1 .. n-2: c[0] += zi * (c[i] + zn * c[n-1-i]); zi *= z, starting from zi = z;
 *       5. c[0] /= 1 - zn * zn;
 *       6. causal pass, i = 1 .. n-1: c[i] += z * c[i-1];
 *       7. c[n-1] = (z * c[n-2] + c[n-1]) * z / (z * z - 1);
 *       8. anticausal pass, i = n-2 .. 0: c[i] = z * (c[i+1] - c[i]);
 *   zoom: per axis zoom = (n - 1) / (S - 1), a double computed on the host; output index i has the coordinate
 *     x = i * zoom, f = floor(x), y = x - f, t = 1 - y; its taps run from f - 1 to f + 2 with the weights
 *       w0 = t * t * t / 6, w1 = (y * y * (y - 2) * 3 + 4) / 6, w2 = (t * t * (t - 2) * 3 + 4) / 6,
 *       w3 = 1 - w0 - w1 - w2;
 *     a tap index is mirrored once: idx < 0 -> -idx, idx >= n -> 2 * (n - 1) - idx;
 *     s = 0; for a = 0 .. 3 over the rows, then b = 0 .. 3 over the columns: v = c[ya][xb]; v *= wy[a]; v *= wx[b];
 *     s += v; resized = (float) s (zoom's output takes the input's dtype);
 *   threshold and colour, in float32: mask = resized > 0.1f; colour = min(trunc(resized * 256f), 255), clamped
 *     before the conversion so that huge values read 255, and 0 where the mask is false; NaN is outside the
 *     contract, its mask is false;
 *   overlay [S,S,4] float64: (lut[colour][0..2], alpha) where the mask is true, zeros elsewhere.
 *   proto [B,h,w,P] float32 (the NHWC storage of a forward's proto_features); lut [256,3] float64, 16-byte aligned
 *   (the caller's colour table: matplotlib.colormaps['viridis'](np.arange(256))[:, :3] in the reference; read only
 *   when overlay is asked for, but never NULL); alpha: the reference's 0.7.  Outputs, each NULL or written: maps
 *   [N,h,w] float32 (the map itself, dense), resized [N,S,S] float32, mask [N,S,S] uint8 (0 / 1), colour [N,S,S]
 *   uint8, overlay [N,S,S,4] float64 (16-byte aligned); with maps alone the call is a gather of the maps and
 *   resizes nothing.  A row of items with b or p out of range writes nothing.
 *   One workgroup of 256 threads per (row, band of up to 32 output rows); the prefiltered map is staged in LDS as
 *   doubles beside the colour table, the row taps and the band's float32 tile: ceil2(h * (w | 1)) * 8 + 6144 +
 *   band * (48 + 4 * S) bytes must fit 64 KiB for some band in 32, 16, .., 1 (the largest that fits is taken; band 32
 *   at 26 x 26 -> 224, and a square map of up to 85 x 85 at S = 224, 83 x 83 at S = 1024), N * ceil(S / band) below 2^24, S * S below 2^29; byte offsets are
 *   64-bit.  16-byte stores throughout when S % 4 == 0 and resized is 16-byte, mask and colour 4-byte aligned; one
 *   element per lane for those three otherwise; the same values.  N == 0 launches nothing.  A violation or a NULL
 *   proto, items or lut returns PIPNET_ERR_ARG before any HIP call. */
int pipnet_map_overlay(const float* proto, int B, int h, int w, int P, const int32_t* items, int N, const double* lut,
                       int S, double alpha, float* maps, float* resized, uint8_t* mask, uint8_t* colour,
                       double* overlay, void* stream);

/* ---- attribution images (util/interpret_idg.py:413-427 fold / normalise / blend, :183-204
 * normalize_attribution_map, :442-446 un-normalised image, :626-641 logit mode; csrc/saliency_ops.hip) ----
 * T maps of N = H * W float32 values each, dense; every result is bitwise what numpy / torch give on the
 * host for finite inputs (no a * b + c is contracted).
 * pipnet_saliency_abs_sum_f32: maps [T,3,N] -> folded [T,N] = (|a0| + |a1|) + |a2| (np.sum(np.abs(.), axis=2)).
 *   16-byte loads when N % 4 == 0 and both pointers are 16-byte aligned, scalar otherwise; same bits.
 * pipnet_saliency_order_stats_f32: per map the exact minimum vmin[t], maximum vtop[t], the k-th and (k+1)-th
 *   smallest values lo[t], hi[t] (0-based; hi = lo where k + 1 == N) and numpy's linear interpolation
 *   vq[t] = gamma >= 0.5 ? hi - (hi - lo) * (1 - gamma) : lo + (hi - lo) * gamma in float32.  k and gamma are the
 *   caller's (np.percentile's virtual index, split on the host).  Exact selection, one workgroup per map: a
 *   radix select over the order-preserving 32-bit key of the float, integer LDS atomics only, so the result
 *   does not depend on any execution order.  -0.0 sorts below +0.0.  NaN inputs stay in bounds and terminate;
 *   their result is unspecified.  0 <= k < N.
 * pipnet_saliency_normalize_f32: out[t] = clip((folded[t] - vmin[t]) / den, 0, 1), den and rule[t] chosen per
 *   map from the device-resident statistics.  fallback = 1: den = vq - vmin when that is > 1e-3f (rule 0), else
 *   vtop - vmin when that is > 1e-5f (rule 1), else a zero map (rule 2).  fallback = 0 (logit mode): den =
 *   vq - vmin (rule 0), a zero map where vq == vmin (rule 2; the reference divides by zero there).
 * pipnet_saliency_blend_f64: out [N,4] float64: RGB = clip(sum_t colours[t] * normalized[t], 0, 1) added in
 *   the order t = 0 .. T-1 (product and sum rounded separately), alpha = max_t normalized[t] from 0.
 *   colours [T,3] float64.  T == 0 writes zeros.
 * pipnet_saliency_unnormalize_f32: x [3,N] (NCHW) -> out [N,3] (HWC) = clip(x * s_c + m_c, 0, 1), the product
 *   and the sum rounded separately.
 * pipnet_saliency_colormap_rgba8: out [total,4] uint8 = lut[min((int)(v * 256), 255)] for v in [0, 1] (below 0
 *   or NaN: entry 0; above 1: entry 255); lut [256,4] uint8; out 4-byte aligned (PIPNET_ERR_ALIGN).
 * 1 <= N < 2^31 (32-bit counts); T >= 0 (T == 0 launches nothing, but for the blend); a violation or a NULL
 * pointer returns PIPNET_ERR_ARG before any HIP call. */
int pipnet_saliency_abs_sum_f32(const float* maps, int T, int64_t N, float* folded, void* stream);
int pipnet_saliency_order_stats_f32(const float* folded, int T, int64_t N, int64_t k, float gamma, float* vmin,
                                    float* vtop, float* lo, float* hi, float* vq, void* stream);
int pipnet_saliency_normalize_f32(const float* folded, const float* vmin, const float* vq, const float* vtop, int T,
                                  int64_t N, int fallback, int32_t* rule, float* out, void* stream);
int pipnet_saliency_blend_f64(const float* normalized, const double* colours, int T, int64_t N, double* out,
                              void* stream);
int pipnet_saliency_unnormalize_f32(const float* x, int64_t N, float m0, float m1, float m2, float s0, float s1,
                                    float s2, float* out, void* stream);
int pipnet_saliency_colormap_rgba8(const float* normalized, const uint8_t* lut, int64_t total, uint8_t* out,
                                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PIPNET_AMD_H */
