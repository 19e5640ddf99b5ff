// Data-parallel training (count_pipnet_amd/dist_train.py): the gradient arena's pack.
//
// Every rank's gradients cross ranks in ONE all-reduce over a flat fp32 arena.  The backward leaves one tensor per
// parameter (about 180 for a ConvNeXt-tiny suffix); pack_tensors_kernel gathers them into their arena slots in one
// launch instead of one copy per tensor.  Memory-bound: each element is read once and written once.
#include "common.hpp"

namespace {

constexpr int PACK_T = 256, PACK_BX = 64;      // 64 workgroups stride through one tensor; blockIdx.y = tensor

// table [n][3] int64: source address, arena offset in floats (a multiple of 4, so every slot starts on 16 bytes),
// element count.  A slot is the count rounded up to a multiple of 4; its padding is written as 0 (the all-reduce
// then adds zeros).  16-byte loads and stores where the source is 16-byte aligned, element by element otherwise.
__global__ __launch_bounds__(PACK_T) void pack_tensors_kernel(const int64_t* __restrict__ table,
                                                              float* __restrict__ arena) {
  const int64_t* row = table + 3 * (int64_t)blockIdx.y;
  const float* __restrict__ src = reinterpret_cast<const float*>(static_cast<uintptr_t>(row[0]));
  float* __restrict__ dst = arena + row[1];
  const int64_t n = row[2], n4 = n >> 2, slot = (n + 3) & ~(int64_t)3;
  const int64_t tid = (int64_t)blockIdx.x * PACK_T + threadIdx.x, stride = (int64_t)gridDim.x * PACK_T;
  if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0) {
    for (int64_t i = tid; i < n4; i += stride) st4(dst + 4 * i, ld4(src + 4 * i));
    const int64_t i = 4 * n4 + tid;            // the last, partial vector and the slot's padding
    if (i < slot) dst[i] = i < n ? src[i] : 0.f;
  } else {
    for (int64_t i = tid; i < slot; i += stride) dst[i] = i < n ? src[i] : 0.f;
  }
}

}  // namespace

extern "C" int pipnet_pack_tensors_f32(const int64_t* table, int n, float* arena, void* stream) {
  if (n < 0 || n > 65535 || !table || !arena) return PIPNET_ERR_ARG;
  if (!aligned16(arena)) return PIPNET_ERR_ALIGN;
  if (n == 0) return PIPNET_OK;
  hipLaunchKernelGGL(pack_tensors_kernel, dim3(PACK_BX, (unsigned)n), dim3(PACK_T), 0, (hipStream_t)stream, table,
                     arena);
  PIPNET_CHECK_LAUNCH();
  return PIPNET_OK;
}
