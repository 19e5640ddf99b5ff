// Shared by the prototype heads (head.hip) and the explanation kernels (explain.hip): the
// wave-per-pixel geometry, the per-pixel softmax body and the zero-fill launch.
#pragma once
#include "common.hpp"

namespace {
// Zero-fill by a kernel rather than a memset call: the launch is captured as an ordinary
// kernel node when the stream is being recorded into a HIP graph (count_pipnet_amd.graph); a
// memset issued during capture was observed NOT to take effect on replay.
// Two ranges per launch (the fused head zeroes pooled and its arrival tickets together).
__global__ __launch_bounds__(256) void zero_u32_kernel(uint32_t* __restrict__ p, int64_t n, uint32_t* __restrict__ p2,
                                                       int64_t n2) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n + n2; i += (int64_t)gridDim.x * 256) {
    if (i < n) p[i] = 0u;
    else p2[i - n] = 0u;
  }
}
inline bool zero_fill(void* p, int64_t n_u32, hipStream_t s, void* p2 = nullptr, int64_t n2_u32 = 0) {
  const int64_t n = n_u32 + (p2 ? n2_u32 : 0);
  const int64_t blocks = (n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024;
  hipLaunchKernelGGL(zero_u32_kernel, dim3((unsigned)(blocks > 0 ? blocks : 1)), dim3(256), 0, s,
                     reinterpret_cast<uint32_t*>(p), n_u32, reinterpret_cast<uint32_t*>(p2), p2 ? n2_u32 : 0);
  return hipGetLastError() == hipSuccess;
}

constexpr int HEAD_THREADS = 256;
constexpr int PIX_PER_BLOCK = 32;

// nn.Softmax(dim=1) of one pixel by one wave: lane l holds channels l, l + 64, ... (NJ per lane).
// Leaves v[j] = exp(x_j - max) (0 for channels >= P) and returns 1 / sum; the softmax value is
// v[j] * inv.  The one copy of this arithmetic: softmax_pool_kernel (head.hip) and
// pool_argmax_kernel (explain.hip) both call it, so their proto / pooled bits cannot drift apart.
template <int NJ, typename T>
PIPNET_DEV float softmax_pixel(const T* __restrict__ feat, int64_t base, int P, int lane, float (&v)[NJ]) {
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = lane + 64 * j;
    v[j] = c < P ? (float)feat[base + c] : -INFINITY;
    m = fmaxf(m, v[j]);
  }
  m = wave_max(m);
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = lane + 64 * j;
    v[j] = c < P ? expf(v[j] - m) : 0.f;
    s += v[j];
  }
  return 1.0f / wave_sum(s);
}

inline int nj_bucket(int P) {
  const int nj = (P + 63) / 64;
  if (nj <= 1) return 1;
  if (nj <= 2) return 2;
  if (nj <= 4) return 4;
  if (nj <= 8) return 8;
  if (nj <= 12) return 12;
  if (nj <= 16) return 16;
  if (nj <= 32) return 32;
  return -1;
}
}  // namespace

#define PIPNET_NJ_SWITCH(NJV, CALL) \
  switch (NJV) {                    \
    case 1: CALL(1); break;         \
    case 2: CALL(2); break;         \
    case 4: CALL(4); break;         \
    case 8: CALL(8); break;         \
    case 12: CALL(12); break;       \
    case 16: CALL(16); break;       \
    case 32: CALL(32); break;       \
    default: return PIPNET_ERR_ARG; \
  }
