// Stand-alone host check of the augmentation entries' planning and argument validation
// (csrc/augment_ops.hip), for a sanitizer build on the CPU -- no kernel is launched:
/*   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined
          -fsanitize=address,undefined -I include tools/augment_plan_check.cpp
          count_pipnet_amd/csrc/augment_ops.hip -o augment_plan_check && ./augment_plan_check
     (the unprefixed -fsanitize reaches the link step; the compiler ignores it for the device) */
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pipnet_amd.h"

static int failures = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);       \
      ++failures;                                                 \
    }                                                             \
  } while (0)

int main() {
  int k1 = 0, k2 = 0;
  int64_t ws = 0;
  // plan: taps and workspace of ragged batches, from one pixel to a 31x downscale
  const std::vector<std::vector<int32_t>> batches = {
      {375, 500, 500, 375}, {1, 1}, {37, 45, 64, 64, 50, 90, 90, 50, 33, 200}, {7000, 3}, {}};
  for (const auto& sizes : batches) {
    const int B = (int)sizes.size() / 2;
    for (int S1 : {1, 12, 64, 232, 272}) {
      for (int S2 : {1, 4, 40, 228, 232}) {
        EXPECT(pipnet_augment_geometry_plan(sizes.data(), B, S1, S2, &k1, &k2, &ws) == PIPNET_OK);
        EXPECT(k1 >= 3 && k2 >= 3 && ws >= 0 && ws % 4 == 0);
        const int64_t ints = (int64_t)B * 2 * S1 * (2 + k1) + (int64_t)B * 2 * S2 * (2 + k2) + (int64_t)B * (8 + 2 * S1);
        EXPECT(ws >= ints * 4 + (int64_t)B * S1 * S1 * 3);
        for (int b = 0; b < B; ++b) {      // a row holds every tap of its axis: ceil(scale) * 2 + 1
          const int need = (sizes[2 * b] + S1 - 1) / S1 * 2 + 1;
          EXPECT(k1 >= need);
        }
        EXPECT(k2 >= (S1 + S2 - 1) / S2 * 2 + 1);
      }
    }
  }
  const int32_t bad[2] = {0, 5};
  EXPECT(pipnet_augment_geometry_plan(bad, 1, 64, 40, &k1, &k2, &ws) == PIPNET_ERR_ARG);
  EXPECT(pipnet_augment_geometry_plan(nullptr, 1, 64, 40, &k1, &k2, &ws) == PIPNET_ERR_ARG);
  EXPECT(pipnet_augment_geometry_plan(bad, -1, 64, 40, &k1, &k2, &ws) == PIPNET_ERR_ARG);
  EXPECT(pipnet_augment_geometry_plan(bad, 1, 0, 40, &k1, &k2, &ws) == PIPNET_ERR_ARG);
  EXPECT(pipnet_augment_geometry_plan(bad, 1, 64, 9000, &k1, &k2, &ws) == PIPNET_ERR_ARG);
  EXPECT(pipnet_augment_geometry_plan(bad, 1, 64, 40, nullptr, &k2, &ws) == PIPNET_ERR_ARG);

  // entries: every rejection happens before any HIP call; an empty batch is a no-op
  const float m[3] = {0.5f, 0.5f, 0.5f};
  void* p = reinterpret_cast<void*>(16);
  auto u8 = static_cast<uint8_t*>(p);
  EXPECT(pipnet_augment_geometry_rgb8(nullptr, nullptr, nullptr, nullptr, 0, 64, 40, 3, 5, nullptr, nullptr, nullptr) == PIPNET_OK);
  EXPECT(pipnet_augment_geometry_rgb8(nullptr, nullptr, nullptr, nullptr, 2, 64, 40, 3, 5, nullptr, nullptr, nullptr) == PIPNET_ERR_ARG);
  EXPECT(pipnet_augment_geometry_rgb8(u8, (const int64_t*)p, (const int32_t*)p, (const double*)p, 2, 64, 40, 3, 3,
                                      (int32_t*)p, u8, nullptr) == PIPNET_ERR_ARG);      // kmax2 < taps of 64 -> 40
  EXPECT(pipnet_augment_geometry_rgb8(u8, (const int64_t*)p, (const int32_t*)p, (const double*)p, 2, 64, 0, 3, 5,
                                      (int32_t*)p, u8, nullptr) == PIPNET_ERR_ARG);
  EXPECT(pipnet_augment_geometry_rgb8(u8, (const int64_t*)p, (const int32_t*)p, (const double*)p, 20000, 8192, 40, 3, 411,
                                      (int32_t*)p, u8, nullptr) == PIPNET_ERR_ARG);      // pixel index past 2^29
  EXPECT(pipnet_augment_view_rgb8(nullptr, nullptr, 2, 0, 40, 32, 0, m, m, 0.1f, 1, nullptr, nullptr, nullptr) == PIPNET_OK);
  EXPECT(pipnet_augment_view_rgb8(nullptr, nullptr, 2, 3, 40, 32, 0, m, m, 0.1f, 1, nullptr, nullptr, nullptr) == PIPNET_ERR_ARG);
  EXPECT(pipnet_augment_view_rgb8(u8, (const double*)p, 0, 3, 40, 32, 0, m, m, 0.1f, 1, nullptr, (float*)p, nullptr) == PIPNET_ERR_ARG);
  EXPECT(pipnet_augment_view_rgb8(u8, (const double*)p, 2, 3, 40, 41, 0, m, m, 0.1f, 1, nullptr, (float*)p, nullptr) == PIPNET_ERR_ARG);
  EXPECT(pipnet_augment_view_rgb8(u8, (const double*)p, 2, 3, 40, 32, 0, nullptr, m, 0.1f, 1, nullptr, (float*)p, nullptr) == PIPNET_ERR_ARG);
  EXPECT(pipnet_augment_view_rgb8(u8, (const double*)p, 2, 3, 8000, 4000, 0, m, m, 0.1f, 1, nullptr, (float*)p, nullptr) == PIPNET_ERR_ARG);
  std::printf(failures ? "%d check(s) failed\n" : "augment_plan_check: all checks passed\n", failures);
  return failures ? 1 : 0;
}
