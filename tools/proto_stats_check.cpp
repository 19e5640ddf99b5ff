// Stand-alone host check of the argument validation of the prototype-statistics entries
// (csrc/proto_stats.hip), for a sanitizer build on the CPU -- no kernel is launched: every call
// here must be rejected before any HIP call.
/*   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined
          -fsanitize=address,undefined -I include tools/proto_stats_check.cpp
          count_pipnet_amd/csrc/proto_stats.hip -o proto_stats_check && ./proto_stats_check
     (the unprefixed -fsanitize reaches the link step; the compiler ignores it for the device) */
#include <cstdint>
#include <cstdio>

#include "pipnet_amd.h"

static int failures = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);       \
      ++failures;                                                 \
    }                                                             \
  } while (0)

struct Args {
  const float* act;
  int64_t lda;
  const int64_t* labels;
  int B, P, K;
  const float* edges;
  int NB;
  int64_t *n_class, *n_ge, *n_gt;
  double *total, *total_gt;
  float* vmax;
  int32_t* hist;
  int64_t* bad;
};

static int update(const Args& a) {
  return pipnet_proto_stats_update_f32(a.act, a.lda, a.labels, a.B, a.P, a.K, 0.01f, a.edges, a.NB, a.n_class, a.n_ge,
                                       a.n_gt, a.total, a.total_gt, a.vmax, a.hist, a.bad, nullptr);
}

int main() {
  void* p = reinterpret_cast<void*>(16);        // never dereferenced: every call below is rejected on the host
  const Args good = {(const float*)p, 768, (const int64_t*)p, 64, 768, 200, (const float*)p, 50,
                     (int64_t*)p, (int64_t*)p, (int64_t*)p, (double*)p, (double*)p, (float*)p, (int32_t*)p, (int64_t*)p};
  Args a = good;
  a.B = 0;
  EXPECT(update(a) == PIPNET_ERR_ARG);
  a = good, a.B = -3;
  EXPECT(update(a) == PIPNET_ERR_ARG);
  a = good, a.P = 0;
  EXPECT(update(a) == PIPNET_ERR_ARG);
  a = good, a.K = 0;
  EXPECT(update(a) == PIPNET_ERR_ARG);
  a = good, a.K = -1;
  EXPECT(update(a) == PIPNET_ERR_ARG);
  a = good, a.lda = 767;
  EXPECT(update(a) == PIPNET_ERR_ARG);
  a = good, a.lda = -768;
  EXPECT(update(a) == PIPNET_ERR_ARG);
  a = good, a.NB = PIPNET_PROTO_STATS_MAX_BINS + 1;
  EXPECT(update(a) == PIPNET_ERR_ARG);
  a = good, a.NB = -1;
  EXPECT(update(a) == PIPNET_ERR_ARG);
  a = good, a.P = 2147483647, a.lda = 2147483647;      // column blocks would overflow int
  EXPECT(update(a) == PIPNET_ERR_ARG);
  a = good, a.act = nullptr;
  EXPECT(update(a) == PIPNET_ERR_ARG);
  a = good, a.labels = nullptr;
  EXPECT(update(a) == PIPNET_ERR_ARG);
  a = good, a.n_class = nullptr;
  EXPECT(update(a) == PIPNET_ERR_ARG);
  a = good, a.n_ge = nullptr;
  EXPECT(update(a) == PIPNET_ERR_ARG);
  a = good, a.n_gt = nullptr;
  EXPECT(update(a) == PIPNET_ERR_ARG);
  a = good, a.total = nullptr;
  EXPECT(update(a) == PIPNET_ERR_ARG);
  a = good, a.total_gt = nullptr;
  EXPECT(update(a) == PIPNET_ERR_ARG);
  a = good, a.vmax = nullptr;
  EXPECT(update(a) == PIPNET_ERR_ARG);
  a = good, a.bad = nullptr;
  EXPECT(update(a) == PIPNET_ERR_ARG);
  a = good, a.edges = nullptr;                         // a histogram needs its edges and its bins
  EXPECT(update(a) == PIPNET_ERR_ARG);
  a = good, a.hist = nullptr;
  EXPECT(update(a) == PIPNET_ERR_ARG);

  EXPECT(pipnet_colsum_accum_f64(nullptr, 48, 4, 48, (double*)p, nullptr) == PIPNET_ERR_ARG);
  EXPECT(pipnet_colsum_accum_f64((const float*)p, 48, 4, 48, nullptr, nullptr) == PIPNET_ERR_ARG);
  EXPECT(pipnet_colsum_accum_f64((const float*)p, 48, 0, 48, (double*)p, nullptr) == PIPNET_ERR_ARG);
  EXPECT(pipnet_colsum_accum_f64((const float*)p, 48, 4, 0, (double*)p, nullptr) == PIPNET_ERR_ARG);
  EXPECT(pipnet_colsum_accum_f64((const float*)p, 47, 4, 48, (double*)p, nullptr) == PIPNET_ERR_ARG);
  EXPECT(pipnet_colsum_accum_f64((const float*)p, 2147483647, 4, 2147483647, (double*)p, nullptr) == PIPNET_ERR_ARG);
  std::printf(failures ? "%d check(s) failed\n" : "proto_stats_check: all checks passed\n", failures);
  return failures ? 1 : 0;
}
