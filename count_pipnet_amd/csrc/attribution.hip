// Integrated-gradients pixel attribution on gfx950 -- the device side of util/interpret_idg.py and
// util/saliency_methods.py (IG, LeftIG, IDG), count_pipnet_amd/attribution.py:
//   * path_images   the interpolated images baseline + alpha_i (x - baseline) of a chunk of path
//                   steps, written in the 4-channel NHWC form the unfused stem conv reads
//   * head_bwd      d target / d logits of the prototype head for an arbitrary upstream vector
//                   u = d target / d pooled (max-pool) or d target / d counts (spatial sum)
//   * stem_dx       the input gradient of the stem's Conv2d(3, O, 4, 4): patches do not overlap
//   * path_weights  the per-step coefficients (and the LeftIG cutoff) of the three methods
//   * path_reduce   map = (x - baseline) * sum_i weights_i * g_i, summed in step order
// All of them are bandwidth-bound or tiny; none uses an atomic, so every result is bitwise
// reproducible run to run.
#include <limits.h>

#include "common.hpp"

namespace {

constexpr int ATTR_THREADS = 256;

PIPNET_DEV int64_t wave_min_i64(int64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int64_t t = __shfl_xor(v, o, 64);
    v = t < v ? t : v;
  }
  return v;
}

// One thread per pixel: the three channel planes of x are read coalesced, the pixel goes out as one
// 16-byte store (r, g, b, 0).  One fused multiply-add per element: fma(alpha, x - b, b).
__global__ __launch_bounds__(ATTR_THREADS) void path_images_kernel(const float* __restrict__ x,
                                                                   const float* __restrict__ base, float base_value,
                                                                   const float* __restrict__ alpha, int HW,
                                                                   float* __restrict__ out) {
  const int pix = blockIdx.x * ATTR_THREADS + threadIdx.x;
  if (pix >= HW) return;
  const int s = blockIdx.y;
  const float a = alpha[s];
  f32x4 v;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float b = base ? base[(int64_t)c * HW + pix] : base_value;
    v[c] = fmaf(a, x[(int64_t)c * HW + pix] - b, b);
  }
  v[3] = 0.f;
  st4(out + ((int64_t)s * HW + pix) * 4, v);
}

// One wave per pixel, a workgroup of four waves takes four pixels of one image.  Lane l holds
// channels l, l + 64, ...; the one sum over P is a wave butterfly.
//   MAX (softmax + max-pool): a = sum_{p: loc[p] == pix} u_p s_p;
//        d[q] = [loc[q] == pix] u_q s_q - s_q a
//   SUM (soft-max / Gumbel-softmax + spatial sum): d[q] = inv_tau y_q (u_q - sum_p u_p y_p)
template <bool MAX>
__global__ __launch_bounds__(ATTR_THREADS) void attr_head_bwd_kernel(const float* __restrict__ soft,
                                                                     const float* __restrict__ u,
                                                                     const int32_t* __restrict__ loc, int HW, int P,
                                                                     float inv_tau, float* __restrict__ d_logits) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int pix = blockIdx.x * (ATTR_THREADS / 64) + wv;
  if (pix >= HW) return;
  const int b = blockIdx.y;
  const int64_t base = ((int64_t)b * HW + pix) * P;
  const float* ub = u + (int64_t)b * P;
  const int32_t* lb = MAX ? loc + (int64_t)b * P : nullptr;
  float acc = 0.f;
  for (int c = lane; c < P; c += 64) {
    const float t = ub[c] * soft[base + c];
    if (MAX) acc += lb[c] == pix ? t : 0.f;
    else acc += t;
  }
  acc = wave_sum(acc);
  for (int c = lane; c < P; c += 64) {
    const float s = soft[base + c];
    float d;
    if (MAX) d = (lb[c] == pix ? ub[c] * s : 0.f) - s * acc;
    else d = inv_tau * s * (ub[c] - acc);
    d_logits[base + c] = d;
  }
}

// dx[b, c, 4i + kh, 4j + kw] = sum_o dz[b, i, j, o] W[o, c, kh, kw].  A workgroup takes STEM_PATCHES
// neighbouring patches of one latent row; the O x 48 weights and the patches' dz rows sit in LDS
// (dz rows padded by one float: the 16 rows a wave reads fall on 16 banks) and every thread
// produces three of the 16 * 48 outputs with plain FMAs over o.  Element order (c, kh) slow, patch,
// kw fast: a wave writes 64 consecutive floats of one image row.
constexpr int STEM_PATCHES = 16;
constexpr int STEM_K = 48;

__global__ __launch_bounds__(ATTR_THREADS) void stem_dx_kernel(const float* __restrict__ dz,
                                                               const float* __restrict__ w, int h, int wl, int H,
                                                               int W, int O, int64_t ldx, float* __restrict__ dx) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* ws = smem;                         // [O][48]
  float* zs = smem + (int64_t)O * STEM_K;   // [STEM_PATCHES][O + 1]
  const int jb = blockIdx.x * STEM_PATCHES, i = blockIdx.y, b = blockIdx.z;
  for (int e = threadIdx.x; e < O * STEM_K; e += ATTR_THREADS) ws[e] = w[e];
  for (int e = threadIdx.x; e < STEM_PATCHES * O; e += ATTR_THREADS) {
    const int pl = e / O, o = e - pl * O;
    zs[pl * (O + 1) + o] = jb + pl < wl ? dz[(((int64_t)b * h + i) * wl + jb + pl) * O + o] : 0.f;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < STEM_PATCHES * STEM_K; e += ATTR_THREADS) {
    const int kw = e & 3, pl = (e >> 2) % STEM_PATCHES, ck = e / (4 * STEM_PATCHES);   // ck = c * 4 + kh
    if (jb + pl >= wl) continue;
    const float* zr = zs + pl * (O + 1);
    const float* wr = ws + ck * 4 + kw;
    float acc = 0.f;
    for (int o = 0; o < O; ++o) acc = fmaf(zr[o], wr[o * STEM_K], acc);
    const int c = ck >> 2, kh = ck & 3;
    dx[(int64_t)b * ldx + ((int64_t)c * H + 4 * i + kh) * W + 4 * (jb + pl) + kw] = acc;
  }
}

// rows / columns the stride-4 conv never reads (H or W not a multiple of 4) get a zero gradient
__global__ __launch_bounds__(ATTR_THREADS) void stem_dx_border_kernel(int h, int wl, int H, int W, int64_t ldx,
                                                                      float* __restrict__ dx) {
  const int64_t n = (int64_t)3 * H * W;
  const int b = blockIdx.y;
  for (int64_t e = (int64_t)blockIdx.x * ATTR_THREADS + threadIdx.x; e < n; e += (int64_t)gridDim.x * ATTR_THREADS) {
    const int col = (int)(e % W), row = (int)((e / W) % H);
    if (row >= 4 * h || col >= 4 * wl) dx[(int64_t)b * ldx + e] = 0.f;
  }
}

// One workgroup; S is a path length (a few hundred).  The arithmetic on the [S] vectors runs in
// double and is rounded once; the LeftIG test is the reference's fp32 one, s_i > fp32(max * alpha_star).
//   method 0 (ig)   w_i = 1 / S, cutoff = S
//   method 1 (lig)  cutoff = first i with s_i > max(s) * alpha_star (none: 1; 0 -> 1);
//                   w_i = 1 / cutoff for i < cutoff, else 0
//   method 2 (idg)  slope_0 = 0, slope_i = (s_i - s_{i-1}) / (alpha_i - alpha_{i-1});
//                   w_i = slope_i * substep_i / S, cutoff = S
__global__ __launch_bounds__(ATTR_THREADS) void path_weights_kernel(const float* __restrict__ scores,
                                                                    const float* __restrict__ alphas,
                                                                    const float* __restrict__ substep, int S,
                                                                    int method, float alpha_star,
                                                                    float* __restrict__ weights,
                                                                    int64_t* __restrict__ cutoff) {
  __shared__ float red_max[ATTR_THREADS / 64];
  __shared__ int64_t red_first[ATTR_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (method == 1) {
    float m = -INFINITY;
    for (int i = tid; i < S; i += ATTR_THREADS) m = fmaxf(m, scores[i]);
    m = wave_max(m);
    if (lane == 0) red_max[wv] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red_max[0], red_max[1]), fmaxf(red_max[2], red_max[3]));
    const float thr = m * alpha_star;
    int64_t first = S;
    for (int i = tid; i < S; i += ATTR_THREADS)
      if (scores[i] > thr && i < first) first = i;
    first = wave_min_i64(first);
    if (lane == 0) red_first[wv] = first;
    __syncthreads();
    first = red_first[0];
    for (int k = 1; k < ATTR_THREADS / 64; ++k) first = red_first[k] < first ? red_first[k] : first;
    int64_t cut = first >= S ? 1 : first;
    if (cut == 0) cut = 1;
    const float wgt = (float)(1.0 / (double)cut);
    for (int i = tid; i < S; i += ATTR_THREADS) weights[i] = i < cut ? wgt : 0.f;
    if (tid == 0) *cutoff = cut;
    return;
  }
  for (int i = tid; i < S; i += ATTR_THREADS) {
    double wgt;
    if (method == 0) {
      wgt = 1.0 / (double)S;
    } else {
      const double slope =
          i == 0 ? 0.0 : ((double)scores[i] - (double)scores[i - 1]) / ((double)alphas[i] - (double)alphas[i - 1]);
      wgt = slope * (double)substep[i] / (double)S;
    }
    weights[i] = (float)wgt;
  }
  if (tid == 0) *cutoff = S;
}

// acc_e = sum_i w_i g[i][e] as a chain of FMAs in step order, then (x_e - b_e) * acc_e.  VEC: four
// elements per thread through 16-byte loads and stores; the scalar form takes the tail (and
// everything when an operand is not 16-byte aligned).
template <bool VEC>
__global__ __launch_bounds__(ATTR_THREADS) void path_reduce_kernel(const float* __restrict__ g, int64_t ldg,
                                                                   const float* __restrict__ wgt,
                                                                   const float* __restrict__ x,
                                                                   const float* __restrict__ base, float base_value,
                                                                   int S, int64_t e0, int64_t n,
                                                                   float* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * ATTR_THREADS + threadIdx.x;
  if (VEC) {
    if (t >= n) return;           // n vectors from element e0 = 0
    const int64_t e = 4 * t;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < S; ++i) acc = __builtin_elementwise_fma((f32x4)wgt[i], ld4(g + (int64_t)i * ldg + e), acc);
    const f32x4 xv = ld4(x + e);
    const f32x4 bv = base ? ld4(base + e) : (f32x4)base_value;
    st4(out + e, (xv - bv) * acc);
  } else {
    if (t >= n) return;           // n elements from element e0
    const int64_t e = e0 + t;
    float acc = 0.f;
    for (int i = 0; i < S; ++i) acc = fmaf(wgt[i], g[(int64_t)i * ldg + e], acc);
    out[e] = (x[e] - (base ? base[e] : base_value)) * acc;
  }
}

}  // namespace

extern "C" int pipnet_attr_path_images_f32(const float* x, const float* baseline, float baseline_value,
                                           const float* alpha, int S, int H, int W, float* out, void* stream) {
  if (S < 0 || S > 65535 || H <= 0 || W <= 0 || (int64_t)H * W > INT_MAX / 4) return PIPNET_ERR_ARG;   // S: grid.y
  if (!x || !alpha || !out) return PIPNET_ERR_ARG;
  if (!aligned16(out)) return PIPNET_ERR_ALIGN;
  if (S == 0) return PIPNET_OK;
  const int HW = H * W;
  hipLaunchKernelGGL(path_images_kernel, dim3((HW + ATTR_THREADS - 1) / ATTR_THREADS, S), dim3(ATTR_THREADS), 0,
                     (hipStream_t)stream, x, baseline, baseline_value, alpha, HW, out);
  PIPNET_CHECK_LAUNCH();
  return PIPNET_OK;
}

extern "C" int pipnet_attr_head_bwd_f32(const float* soft, const float* u, const int32_t* loc, int B, int HW, int P,
                                        int pool_mode, float inv_tau, float* d_logits, void* stream) {
  if (B < 0 || B > 65535 || HW <= 0 || P <= 0 || (pool_mode != 0 && pool_mode != 1)) return PIPNET_ERR_ARG;   // B: grid.y
  if (!soft || !u || !d_logits || (pool_mode == 0 && !loc)) return PIPNET_ERR_ARG;
  if (B == 0) return PIPNET_OK;
  const dim3 grid((HW + ATTR_THREADS / 64 - 1) / (ATTR_THREADS / 64), B);
  if (pool_mode == 0)
    hipLaunchKernelGGL(attr_head_bwd_kernel<true>, grid, dim3(ATTR_THREADS), 0, (hipStream_t)stream, soft, u, loc, HW,
                       P, 1.0f, d_logits);
  else
    hipLaunchKernelGGL(attr_head_bwd_kernel<false>, grid, dim3(ATTR_THREADS), 0, (hipStream_t)stream, soft, u, loc, HW,
                       P, inv_tau, d_logits);
  PIPNET_CHECK_LAUNCH();
  return PIPNET_OK;
}

extern "C" int pipnet_attr_stem_dx_f32(const float* dz, const float* w, int B, int H, int W, int O, int64_t ldx,
                                       float* dx, void* stream) {
  // O: the weights and 16 dz rows stay within 48 KB of LDS (O = 96 takes 24 KB)
  if (B < 0 || B > 65535 || H < 4 || W < 4 || O <= 0 || O > 128 || (int64_t)H * W > INT_MAX / 3) return PIPNET_ERR_ARG;
  if (ldx < (int64_t)3 * H * W) return PIPNET_ERR_ARG;
  if (!dz || !w || !dx) return PIPNET_ERR_ARG;
  if (B == 0) return PIPNET_OK;
  const int h = H / 4, wl = W / 4;
  if (h > 65535) return PIPNET_ERR_ARG;                                                   // grid.y
  if (H % 4 || W % 4) {
    const int64_t n = (int64_t)3 * H * W;
    const int blocks = (int)((n + ATTR_THREADS - 1) / ATTR_THREADS < 1024 ? (n + ATTR_THREADS - 1) / ATTR_THREADS : 1024);
    hipLaunchKernelGGL(stem_dx_border_kernel, dim3(blocks, B), dim3(ATTR_THREADS), 0, (hipStream_t)stream, h, wl, H, W,
                       ldx, dx);
    PIPNET_CHECK_LAUNCH();
  }
  const size_t lds = ((size_t)O * STEM_K + (size_t)STEM_PATCHES * (O + 1)) * sizeof(float);
  hipLaunchKernelGGL(stem_dx_kernel, dim3((wl + STEM_PATCHES - 1) / STEM_PATCHES, h, B), dim3(ATTR_THREADS), lds,
                     (hipStream_t)stream, dz, w, h, wl, H, W, O, ldx, dx);
  PIPNET_CHECK_LAUNCH();
  return PIPNET_OK;
}

extern "C" int pipnet_attr_path_weights_f32(const float* scores, const float* alphas, const float* substep, int S,
                                            int method, float alpha_star, float* weights, int64_t* cutoff,
                                            void* stream) {
  if (S < 1 || method < 0 || method > 2) return PIPNET_ERR_ARG;
  if (!scores || !weights || !cutoff || (method == 2 && (!alphas || !substep))) return PIPNET_ERR_ARG;
  hipLaunchKernelGGL(path_weights_kernel, dim3(1), dim3(ATTR_THREADS), 0, (hipStream_t)stream, scores, alphas, substep,
                     S, method, alpha_star, weights, cutoff);
  PIPNET_CHECK_LAUNCH();
  return PIPNET_OK;
}

extern "C" int pipnet_attr_path_reduce_f32(const float* grads, int64_t ldg, const float* weights, const float* x,
                                           const float* baseline, float baseline_value, int S, int64_t N, float* out,
                                           void* stream) {
  if (S < 1 || N < 0 || ldg < N) return PIPNET_ERR_ARG;
  if (!grads || !weights || !x || !out) return PIPNET_ERR_ARG;
  if (N == 0) return PIPNET_OK;
  const bool vec = ldg % 4 == 0 && aligned16(grads) && aligned16(x) && aligned16(out) && (!baseline || aligned16(baseline));
  const int64_t nvec = vec ? N / 4 : 0, tail = N - 4 * nvec;
  if ((nvec + ATTR_THREADS - 1) / ATTR_THREADS > INT_MAX || (tail + ATTR_THREADS - 1) / ATTR_THREADS > INT_MAX)
    return PIPNET_ERR_ARG;
  if (nvec > 0) {
    hipLaunchKernelGGL(path_reduce_kernel<true>, dim3((unsigned)((nvec + ATTR_THREADS - 1) / ATTR_THREADS)),
                       dim3(ATTR_THREADS), 0, (hipStream_t)stream, grads, ldg, weights, x, baseline, baseline_value, S,
                       (int64_t)0, nvec, out);
    PIPNET_CHECK_LAUNCH();
  }
  if (tail > 0) {
    hipLaunchKernelGGL(path_reduce_kernel<false>, dim3((unsigned)((tail + ATTR_THREADS - 1) / ATTR_THREADS)),
                       dim3(ATTR_THREADS), 0, (hipStream_t)stream, grads, ldg, weights, x, baseline, baseline_value, S,
                       4 * nvec, tail, out);
    PIPNET_CHECK_LAUNCH();
  }
  return PIPNET_OK;
}
