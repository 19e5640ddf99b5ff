// Attribution maps to saliency images on the GPU: what util/interpret_idg.py does, in numpy on the host, to
// the [T,3,H,W] maps of IG / LeftIG / IDG before anybody looks at them (:413-427, :442-457, :626-641):
//   * abs_sum_kernel: np.sum(np.abs(.), axis=2) of the three channel planes, (|a0| + |a1|) + |a2|;
//   * order_stats_kernel: per map the exact minimum, maximum, the k-th and (k+1)-th smallest value and numpy's
//     linear interpolation between the two (np.percentile).  One workgroup per map, an exact selection: a
//     most-significant-digit radix select over the order-preserving 32-bit key of the float (four 8-bit passes
//     with a 256-bin LDS histogram, integer atomics only, so the result does not depend on the order in which
//     the lanes arrive), then one counting pass for the upper neighbour;
//   * normalize_kernel: normalize_attribution_map (:183-204) with its two fallbacks, or logit mode (:632-635);
//     the statistics are read from device memory;
//   * blend_kernel: the additive colour overlay with its max-alpha channel, in float64, maps in order;
//   * unnormalize_kernel: clip(x * std + mean, 0, 1), NCHW -> HWC;
//   * colormap_kernel: what plt.imsave(cmap=) does to a map with minimum 0 and maximum 1 (byte LUT).
// Bits are promised against numpy / torch, so nothing here may contract a * b + c: fp contract(off) throughout.
// Integer keys make the select total on every bit pattern: NaN inputs stay in bounds and terminate, their value
// is unspecified.
#include "common.hpp"

namespace {

constexpr int TPB = 256;

// float -> unsigned key with the same order (negatives: all bits flipped; others: sign bit set); -0.0 < +0.0
PIPNET_DEV uint32_t key_of(float v) {
  const uint32_t b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
PIPNET_DEV float value_of(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

template <bool VEC>
__global__ __launch_bounds__(TPB) void abs_sum_kernel(const float* __restrict__ maps, int64_t N, int64_t per,
                                                      int64_t total, float* __restrict__ folded) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= total) return;
  const int64_t t = i / per, r = i - t * per;
  const float* a = maps + t * 3 * N;
  float* o = folded + t * N;
  if (VEC) {                                   // N % 4 == 0 and both bases 16-byte aligned: so is every row
    const f32x4 a0 = ld4(a + 4 * r), a1 = ld4(a + N + 4 * r), a2 = ld4(a + 2 * N + 4 * r);
    f32x4 s;
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = (fabsf(a0[j]) + fabsf(a1[j])) + fabsf(a2[j]);
    st4(o + 4 * r, s);
  } else {
    o[r] = (fabsf(a[r]) + fabsf(a[N + r])) + fabsf(a[2 * N + r]);
  }
}

// LDS words after the 256 histogram bins (one __shared__ array)
enum { S_PREFIX = 256, S_RANK, S_MIN, S_MAX, S_LE, S_ABOVE, S_WORDS };

__global__ __launch_bounds__(TPB) void order_stats_kernel(const float* __restrict__ folded, int N, int k, float gamma,
                                                          float* __restrict__ vmin, float* __restrict__ vtop,
                                                          float* __restrict__ lo, float* __restrict__ hi,
                                                          float* __restrict__ vq) {
#pragma clang fp contract(off)
  __shared__ uint32_t sh[S_WORDS];
  const float* x = folded + (int64_t)blockIdx.x * N;
  const int tid = threadIdx.x;
  if (tid == 0) {
    sh[S_PREFIX] = 0u;
    sh[S_RANK] = (uint32_t)k;                  // 0 <= k < N: the rank looked for among the keys that match the prefix
    sh[S_MIN] = 0xFFFFFFFFu;
    sh[S_MAX] = 0u;
    sh[S_LE] = 0u;
    sh[S_ABOVE] = 0xFFFFFFFFu;
  }
  uint32_t mask = 0u;
  for (int shift = 24; shift >= 0; shift -= 8) {
    sh[tid] = 0u;
    __syncthreads();
    const uint32_t prefix = sh[S_PREFIX];
    uint32_t mn = 0xFFFFFFFFu, mx = 0u;
    for (int64_t i = tid; i < N; i += TPB) {
      const uint32_t key = key_of(x[i]);
      mn = min(mn, key);
      mx = max(mx, key);
      if ((key & mask) == prefix) atomicAdd(&sh[(key >> shift) & 255u], 1u);
    }
    if (shift == 24) {
      atomicMin(&sh[S_MIN], mn);
      atomicMax(&sh[S_MAX], mx);
    }
    __syncthreads();
    if (tid == 0) {                            // the bucket that holds the rank: 256 LDS reads
      const uint32_t rank = sh[S_RANK];
      uint32_t cum = 0u, b = 0u;
      for (; b < 255u; ++b) {
        const uint32_t c = sh[b];
        if (rank < cum + c) break;
        cum += c;
      }
      sh[S_RANK] = rank - cum;
      sh[S_PREFIX] = prefix | (b << shift);
    }
    mask |= 0xFFu << shift;
    __syncthreads();
  }
  const uint32_t key_k = sh[S_PREFIX];
  uint32_t le = 0u, above = 0xFFFFFFFFu;
  for (int64_t i = tid; i < N; i += TPB) {
    const uint32_t key = key_of(x[i]);
    if (key <= key_k) ++le;
    else above = min(above, key);
  }
  atomicAdd(&sh[S_LE], le);
  atomicMin(&sh[S_ABOVE], above);
  __syncthreads();
  if (tid == 0) {
    // rank k + 1: key_k again when more than k + 1 keys are <= key_k, else the smallest key above it; past the
    // last element (k + 1 == N) numpy takes the k-th value for both neighbours
    const int64_t next = (int64_t)k + 1;
    const uint32_t key_hi = (next >= N || (int64_t)sh[S_LE] > next) ? key_k : sh[S_ABOVE];
    const float a = value_of(key_k), b = value_of(key_hi);
    const float d = b - a;
    const int t = blockIdx.x;
    vmin[t] = value_of(sh[S_MIN]);
    vtop[t] = value_of(sh[S_MAX]);
    lo[t] = a;
    hi[t] = b;
    vq[t] = gamma >= 0.5f ? b - d * (1.0f - gamma) : a + d * gamma;      // numpy's _lerp
  }
}

__global__ __launch_bounds__(TPB) void normalize_kernel(const float* __restrict__ folded, const float* __restrict__ vmin,
                                                        const float* __restrict__ vq, const float* __restrict__ vtop,
                                                        int64_t N, int64_t total, int fallback,
                                                        int32_t* __restrict__ rule, float* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= total) return;
  const int64_t t = i / N;
  const float lo = vmin[t];
  float den = vq[t] - lo;
  int r;
  if (fallback) {                              // the constants are the float32 values of 1e-3 and 1e-5
    r = 0;
    if (!(den > 1e-3f)) {
      den = vtop[t] - lo;
      r = den > 1e-5f ? 1 : 2;
    }
  } else {
    r = vq[t] == lo ? 2 : 0;                   // logit mode has no fallback; the reference divides by zero here
  }
  if (i == t * N) rule[t] = r;
  out[i] = r == 2 ? 0.0f : fminf(fmaxf((folded[i] - lo) / den, 0.0f), 1.0f);
}

__global__ __launch_bounds__(TPB) void blend_kernel(const float* __restrict__ normalized,
                                                    const double* __restrict__ colours, int T, int64_t N,
                                                    double* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= N) return;
  double r = 0.0, g = 0.0, b = 0.0, a = 0.0;
  for (int t = 0; t < T; ++t) {
    const double v = (double)normalized[(int64_t)t * N + i];
    r = r + colours[3 * t] * v;
    g = g + colours[3 * t + 1] * v;
    b = b + colours[3 * t + 2] * v;
    a = fmax(a, v);
  }
  double* o = out + 4 * i;
  o[0] = fmin(fmax(r, 0.0), 1.0);
  o[1] = fmin(fmax(g, 0.0), 1.0);
  o[2] = fmin(fmax(b, 0.0), 1.0);
  o[3] = a;
}

__global__ __launch_bounds__(TPB) void unnormalize_kernel(const float* __restrict__ x, int64_t N, float m0, float m1,
                                                          float m2, float s0, float s1, float s2,
                                                          float* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= N) return;
  const float p0 = x[i] * s0, p1 = x[N + i] * s1, p2 = x[2 * N + i] * s2;      // torch: the product is rounded,
  float* o = out + 3 * i;                                                       // then the sum
  o[0] = fminf(fmaxf(p0 + m0, 0.0f), 1.0f);
  o[1] = fminf(fmaxf(p1 + m1, 0.0f), 1.0f);
  o[2] = fminf(fmaxf(p2 + m2, 0.0f), 1.0f);
}

__global__ __launch_bounds__(TPB) void colormap_kernel(const float* __restrict__ normalized,
                                                       const uint8_t* __restrict__ lut, int64_t total,
                                                       uint32_t* __restrict__ out) {
  __shared__ uint32_t table[256];
  const uint8_t* e = lut + 4 * threadIdx.x;    // one entry per thread; the table need not be 4-byte aligned
  table[threadIdx.x] = (uint32_t)e[0] | ((uint32_t)e[1] << 8) | ((uint32_t)e[2] << 16) | ((uint32_t)e[3] << 24);
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= total) return;
  const float s = normalized[i] * 256.0f;      // exact; xa == N becomes N - 1, then truncation
  const int idx = s >= 255.0f ? 255 : (s >= 0.0f ? (int)s : 0);       // anything else (NaN included): entry 0
  out[i] = table[idx];
}

bool grid_for(int64_t items, unsigned* blocks) {
  const int64_t b = (items + TPB - 1) / TPB;
  if (b >= ((int64_t)1 << 31)) return false;
  *blocks = (unsigned)b;
  return true;
}

}  // namespace

extern "C" int pipnet_saliency_abs_sum_f32(const float* maps, int T, int64_t N, float* folded, void* stream) {
  if (T < 0 || N < 1 || N >= ((int64_t)1 << 31)) return PIPNET_ERR_ARG;
  if (T == 0) return PIPNET_OK;
  if (!maps || !folded) return PIPNET_ERR_ARG;
  const bool vec = N % 4 == 0 && aligned16(maps) && aligned16(folded);
  const int64_t per = vec ? N / 4 : N;
  unsigned blocks;
  if (!grid_for((int64_t)T * per, &blocks)) return PIPNET_ERR_ARG;
  if (vec)
    hipLaunchKernelGGL(abs_sum_kernel<true>, dim3(blocks), dim3(TPB), 0, (hipStream_t)stream, maps, N, per,
                       (int64_t)T * per, folded);
  else
    hipLaunchKernelGGL(abs_sum_kernel<false>, dim3(blocks), dim3(TPB), 0, (hipStream_t)stream, maps, N, per,
                       (int64_t)T * per, folded);
  PIPNET_CHECK_LAUNCH();
  return PIPNET_OK;
}

extern "C" int pipnet_saliency_order_stats_f32(const float* folded, int T, int64_t N, int64_t k, float gamma,
                                               float* vmin, float* vtop, float* lo, float* hi, float* vq,
                                               void* stream) {
  if (T < 0 || N < 1 || N >= ((int64_t)1 << 31) || k < 0 || k >= N) return PIPNET_ERR_ARG;     // 32-bit counts
  if (T == 0) return PIPNET_OK;
  if (!folded || !vmin || !vtop || !lo || !hi || !vq) return PIPNET_ERR_ARG;
  hipLaunchKernelGGL(order_stats_kernel, dim3((unsigned)T), dim3(TPB), 0, (hipStream_t)stream, folded, (int)N, (int)k,
                     gamma, vmin, vtop, lo, hi, vq);
  PIPNET_CHECK_LAUNCH();
  return PIPNET_OK;
}

extern "C" int pipnet_saliency_normalize_f32(const float* folded, const float* vmin, const float* vq,
                                             const float* vtop, int T, int64_t N, int fallback, int32_t* rule,
                                             float* out, void* stream) {
  if (T < 0 || N < 1 || N >= ((int64_t)1 << 31) || (fallback != 0 && fallback != 1)) return PIPNET_ERR_ARG;
  if (T == 0) return PIPNET_OK;
  if (!folded || !vmin || !vq || !vtop || !rule || !out) return PIPNET_ERR_ARG;
  unsigned blocks;
  if (!grid_for((int64_t)T * N, &blocks)) return PIPNET_ERR_ARG;
  hipLaunchKernelGGL(normalize_kernel, dim3(blocks), dim3(TPB), 0, (hipStream_t)stream, folded, vmin, vq, vtop, N,
                     (int64_t)T * N, fallback, rule, out);
  PIPNET_CHECK_LAUNCH();
  return PIPNET_OK;
}

extern "C" int pipnet_saliency_blend_f64(const float* normalized, const double* colours, int T, int64_t N, double* out,
                                         void* stream) {
  if (T < 0 || N < 1 || N >= ((int64_t)1 << 31)) return PIPNET_ERR_ARG;
  if (!out || (T > 0 && (!normalized || !colours))) return PIPNET_ERR_ARG;
  unsigned blocks;
  if (!grid_for(N, &blocks)) return PIPNET_ERR_ARG;
  hipLaunchKernelGGL(blend_kernel, dim3(blocks), dim3(TPB), 0, (hipStream_t)stream, normalized, colours, T, N, out);
  PIPNET_CHECK_LAUNCH();
  return PIPNET_OK;
}

extern "C" int pipnet_saliency_unnormalize_f32(const float* x, int64_t N, float m0, float m1, float m2, float s0,
                                               float s1, float s2, float* out, void* stream) {
  if (N < 1 || N >= ((int64_t)1 << 31) || !x || !out) return PIPNET_ERR_ARG;
  unsigned blocks;
  if (!grid_for(N, &blocks)) return PIPNET_ERR_ARG;
  hipLaunchKernelGGL(unnormalize_kernel, dim3(blocks), dim3(TPB), 0, (hipStream_t)stream, x, N, m0, m1, m2, s0, s1, s2,
                     out);
  PIPNET_CHECK_LAUNCH();
  return PIPNET_OK;
}

extern "C" int pipnet_saliency_colormap_rgba8(const float* normalized, const uint8_t* lut, int64_t total, uint8_t* out,
                                              void* stream) {
  if (total < 0) return PIPNET_ERR_ARG;
  if (total == 0) return PIPNET_OK;
  if (!normalized || !lut || !out) return PIPNET_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(out) & 3u) return PIPNET_ERR_ALIGN;          // one 4-byte store per pixel
  unsigned blocks;
  if (!grid_for(total, &blocks)) return PIPNET_ERR_ARG;
  hipLaunchKernelGGL(colormap_kernel, dim3(blocks), dim3(TPB), 0, (hipStream_t)stream, normalized, lut, total,
                     reinterpret_cast<uint32_t*>(out));
  PIPNET_CHECK_LAUNCH();
  return PIPNET_OK;
}
