// Stand-alone host check of the part-purity entries (csrc/part_purity.hip), for a sanitizer build
// on the CPU -- no kernel is launched: every entry call here must be rejected before any HIP call,
// and the shared row function (csrc/part_purity_row.hpp) runs on the host on planted border and
// fold cases.
/*   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined
          -fsanitize=address,undefined -I include tools/part_purity_check.cpp
          count_pipnet_amd/csrc/part_purity.hip -o part_purity_check && ./part_purity_check
     (the unprefixed -fsanitize reaches the link step; the compiler ignores it for the device) */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../count_pipnet_amd/csrc/part_purity_row.hpp"
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
  const float* pooled;
  int64_t lda;
  const int32_t* loc;
  const uint8_t* relevant;
  const int64_t* index;
  int B, P, k, H, W, image_size, skip;
  const double* xy;
  const uint8_t* vis;
  const int32_t* size;
  int64_t N;
  const int32_t* merged;
  const uint8_t* is_left;
  const int32_t* pair_index;
  int Q, M;
  int64_t *n, *hits;
  uint64_t* first_key;
  int64_t *rows, *bad;
};

static int update(const Args& a) {
  return pipnet_part_purity_update(a.pooled, a.lda, a.loc, a.relevant, a.B, a.P, 0, 0.5, a.H, a.W, a.image_size, a.skip,
                                   1, a.xy, a.vis, a.size, a.N, a.merged, a.is_left, a.pair_index, a.Q, a.M, a.n,
                                   a.hits, a.first_key, a.rows, a.bad, nullptr);
}

static int rows(const Args& a) {
  return pipnet_part_purity_rows(a.index, a.loc, a.relevant, a.P, a.k, a.H, a.W, a.image_size, a.skip, 1, a.xy, a.vis,
                                 a.size, a.N, a.merged, a.is_left, a.pair_index, a.Q, a.M, a.n, a.hits, a.first_key,
                                 a.rows, a.bad, nullptr);
}

template <class F>
static void shared_rejections(const Args& good, F call) {
  Args a = good;
  a.P = 0;
  EXPECT(call(a) == PIPNET_ERR_ARG);
  a = good, a.P = 2147483647, a.lda = 2147483647, a.B = 1;      // column blocks would overflow int
  EXPECT(call(a) == PIPNET_ERR_ARG);
  a = good, a.H = 0;
  EXPECT(call(a) == PIPNET_ERR_ARG);
  a = good, a.W = -1;
  EXPECT(call(a) == PIPNET_ERR_ARG);
  a = good, a.H = 65536, a.W = 65536;                           // H * W overflows int
  EXPECT(call(a) == PIPNET_ERR_ARG);
  a = good, a.image_size = 31;
  EXPECT(call(a) == PIPNET_ERR_ARG);
  a = good, a.skip = -1;
  EXPECT(call(a) == PIPNET_ERR_ARG);
  a = good, a.skip = 2147483647;                                // index * skip overflows int
  EXPECT(call(a) == PIPNET_ERR_ARG);
  a = good, a.N = 0;
  EXPECT(call(a) == PIPNET_ERR_ARG);
  a = good, a.Q = 0;
  EXPECT(call(a) == PIPNET_ERR_ARG);
  a = good, a.Q = PIPNET_PART_PURITY_MAX_PARTS + 1, a.M = 12;
  EXPECT(call(a) == PIPNET_ERR_ARG);
  a = good, a.M = 0;
  EXPECT(call(a) == PIPNET_ERR_ARG);
  a = good, a.M = a.Q + 1;
  EXPECT(call(a) == PIPNET_ERR_ARG);
  a = good, a.loc = nullptr;
  EXPECT(call(a) == PIPNET_ERR_ARG);
  a = good, a.relevant = nullptr;
  EXPECT(call(a) == PIPNET_ERR_ARG);
  a = good, a.xy = nullptr;
  EXPECT(call(a) == PIPNET_ERR_ARG);
  a = good, a.vis = nullptr;
  EXPECT(call(a) == PIPNET_ERR_ARG);
  a = good, a.size = nullptr;
  EXPECT(call(a) == PIPNET_ERR_ARG);
  a = good, a.merged = nullptr;
  EXPECT(call(a) == PIPNET_ERR_ARG);
  a = good, a.is_left = nullptr;
  EXPECT(call(a) == PIPNET_ERR_ARG);
  a = good, a.pair_index = nullptr;
  EXPECT(call(a) == PIPNET_ERR_ARG);
  a = good, a.n = nullptr;
  EXPECT(call(a) == PIPNET_ERR_ARG);
  a = good, a.hits = nullptr;
  EXPECT(call(a) == PIPNET_ERR_ARG);
  a = good, a.first_key = nullptr;
  EXPECT(call(a) == PIPNET_ERR_ARG);
  a = good, a.rows = nullptr;
  EXPECT(call(a) == PIPNET_ERR_ARG);
  a = good, a.bad = nullptr;
  EXPECT(call(a) == PIPNET_ERR_ARG);
}

static void check_arguments() {
  void* p = reinterpret_cast<void*>(16);        // never dereferenced: every call below is rejected on the host
  const Args good = {(const float*)p, 768, (const int32_t*)p, (const uint8_t*)p, (const int64_t*)p, 64, 768, 10, 26, 26,
                     224, 8, (const double*)p, (const uint8_t*)p, (const int32_t*)p, 11788, (const int32_t*)p,
                     (const uint8_t*)p, (const int32_t*)p, 15, 12, (int64_t*)p, (int64_t*)p, (uint64_t*)p, (int64_t*)p,
                     (int64_t*)p};
  shared_rejections(good, update);
  shared_rejections(good, rows);
  Args a = good;
  a.B = 0;
  EXPECT(update(a) == PIPNET_ERR_ARG);
  a = good, a.B = -2;
  EXPECT(update(a) == PIPNET_ERR_ARG);
  a = good, a.lda = 767;
  EXPECT(update(a) == PIPNET_ERR_ARG);
  a = good, a.lda = -768;
  EXPECT(update(a) == PIPNET_ERR_ARG);
  a = good, a.B = 65536, a.P = 32768, a.lda = 32768;            // B * P = 2^31 overflows int32
  EXPECT(update(a) == PIPNET_ERR_ARG);
  a = good, a.pooled = nullptr;
  EXPECT(update(a) == PIPNET_ERR_ARG);
  a = good, a.k = 0;
  EXPECT(rows(a) == PIPNET_ERR_ARG);
  a = good, a.k = 33;
  EXPECT(rows(a) == PIPNET_ERR_ARG);
  a = good, a.index = nullptr;
  EXPECT(rows(a) == PIPNET_ERR_ARG);

  auto finish = [&](const int64_t* n, const int64_t* hits, const uint64_t* key, const int64_t* rws, int P, int M,
                    void* out) {
    return pipnet_part_purity_finish(n, hits, key, rws, P, M, (uint8_t*)out, (double*)out, (int32_t*)out, (int64_t*)out,
                                     (int32_t*)out, (int64_t*)out, (double*)out, (double*)out, nullptr);
  };
  const int64_t* i64 = (const int64_t*)p;
  const uint64_t* u64 = (const uint64_t*)p;
  EXPECT(finish(nullptr, i64, u64, i64, 768, 12, p) == PIPNET_ERR_ARG);
  EXPECT(finish(i64, nullptr, u64, i64, 768, 12, p) == PIPNET_ERR_ARG);
  EXPECT(finish(i64, i64, nullptr, i64, 768, 12, p) == PIPNET_ERR_ARG);
  EXPECT(finish(i64, i64, u64, nullptr, 768, 12, p) == PIPNET_ERR_ARG);
  EXPECT(finish(i64, i64, u64, i64, 768, 12, nullptr) == PIPNET_ERR_ARG);
  EXPECT(finish(i64, i64, u64, i64, 0, 12, p) == PIPNET_ERR_ARG);
  EXPECT(finish(i64, i64, u64, i64, 768, 0, p) == PIPNET_ERR_ARG);
  EXPECT(finish(i64, i64, u64, i64, 768, PIPNET_PART_PURITY_MAX_PARTS + 1, p) == PIPNET_ERR_ARG);
  EXPECT(finish(i64, i64, u64, i64, 2147483647, 12, p) == PIPNET_ERR_ARG);
  EXPECT(pipnet_part_purity_finish(i64, i64, u64, i64, 768, 12, (uint8_t*)p, (double*)p, (int32_t*)p, nullptr,
                                   (int32_t*)p, (int64_t*)p, (double*)p, (double*)p, nullptr) == PIPNET_ERR_ARG);
}

// Q = 5 ids: 0 "left eye", 1 "crown", 2 "right eye", 3 "left leg", 4 "right leg"; M = 3 merged parts
// (crown 0, eye 1, leg 2); pairs in file order: (0, 2) then (3, 4).
struct Rows {
  int32_t merged[5] = {1, 0, 1, 2, 2};
  uint8_t is_left[5] = {1, 0, 0, 1, 0};
  int32_t pair_index[5] = {0, 0, 0, 1, 0};
  PpFold fold{merged, is_left, pair_index, 5, 3};
  std::vector<int64_t> n = std::vector<int64_t>(3, 0), hits = std::vector<int64_t>(3, 0);
  std::vector<uint64_t> key = std::vector<uint64_t>(3, PP_NO_KEY);
  void row(const PpGeom& g, const double* xy, const uint8_t* vis, int w, int h, int loc, uint64_t ord) {
    pp_row(g, fold, xy, vis, w, h, loc, ord, n.data(), hits.data(), key.data());
  }
};

static void check_patch() {
  int h0, h1, w0, w1;
  const PpGeom g8{8, 8, 64, 5, 0};              // skip = round(32 / 7)
  pp_patch(g8, 0, h0, h1, w0, w1);
  EXPECT(h0 == 0 && h1 == 32 && w0 == 0 && w1 == 32);
  pp_patch(g8, 6 * 8 + 7, h0, h1, w0, w1);      // row 6: 30..62; last column: clamped to the border
  EXPECT(h0 == 30 && h1 == 62 && w0 == 32 && w1 == 64);
  const PpGeom g26{26, 26, 224, 8, 1};          // the small-stride rule
  pp_patch(g26, 0, h0, h1, w0, w1);
  EXPECT(h0 == 0 && h1 == 32 && w0 == 0 && w1 == 32);
  pp_patch(g26, 1 * 26 + 2, h0, h1, w0, w1);
  EXPECT(h0 == 4 && h1 == 36 && w0 == 12 && w1 == 44);
  pp_patch(g26, 24 * 26 + 25, h0, h1, w0, w1);  // row 24: 188..220; column 25: 196 - 4 .. 224
  EXPECT(h0 == 188 && h1 == 220 && w0 == 192 && w1 == 224);
  const PpGeom g1{1, 1, 32, 0, 0};
  pp_patch(g1, 0, h0, h1, w0, w1);
  EXPECT(h0 == 0 && h1 == 32 && w0 == 0 && w1 == 32);
}

static void check_rows() {
  // a 100 x 48 image under an 8 x 8 map at 64 pixels; loc 9 = (1, 1): patch rows / cols 5..37, scaled
  // to y in [48/64 * 5, 48/64 * 37] = [3.75, 27.75], x in [100/64 * 5, 100/64 * 37] = [7.8125, 57.8125]
  const PpGeom g{8, 8, 64, 5, 0};
  const double top = (48 / 64.0) * 5, bottom = (48 / 64.0) * 37, left = (100 / 64.0) * 5, right = (100 / 64.0) * 37;
  const uint8_t crown_only[5] = {0, 1, 0, 0, 0};
  struct { double x, y; bool in; } cases[] = {
      {30, top, true},  {30, std::nextafter(top, 0.0), false},    {30, bottom, true}, {30, std::nextafter(bottom, 1e9), false},
      {left, 10, true}, {std::nextafter(left, 0.0), 10, false}, {right, 10, true},  {std::nextafter(right, 1e9), 10, false}};
  for (auto& c : cases) {                       // the closed comparisons, border by border
    Rows r;
    const double xy[10] = {0, 0, c.x, c.y, 0, 0, 0, 0, 0, 0};
    r.row(g, xy, crown_only, 100, 48, 9, 0);
    EXPECT(r.n[0] == 1 && r.hits[0] == (c.in ? 1 : 0) && r.key[0] == 1 && r.n[1] == 0 && r.key[1] == PP_NO_KEY);
  }
  // the fold: left eye in the patch, right eye outside
  const double xy[10] = {30, 10, 500, 500, 90, 40, 30, 12, 90, 44};
  Rows r;
  const uint8_t left_only[5] = {1, 0, 0, 0, 0};
  r.row(g, xy, left_only, 100, 48, 9, 2);       // the eye through the left member: slot Q + 0
  EXPECT(r.n[1] == 1 && r.hits[1] == 1 && r.key[1] == ((2ull << 6) | 5));
  const uint8_t right_only[5] = {0, 0, 1, 0, 0};
  r.row(g, xy, right_only, 100, 48, 9, 3);      // later row: visible, not in the patch; the key stays
  EXPECT(r.n[1] == 2 && r.hits[1] == 1 && r.key[1] == ((2ull << 6) | 5));
  const uint8_t both[5] = {1, 0, 1, 1, 1};
  r.row(g, xy, both, 100, 48, 9, 1);            // an earlier ordinal: own slot 2; one hit per row and part
  EXPECT(r.n[1] == 3 && r.hits[1] == 2 && r.key[1] == ((1ull << 6) | 2));
  EXPECT(r.n[2] == 1 && r.hits[2] == 1 && r.key[2] == ((1ull << 6) | 4));      // leg: right id visible -> slot 4
  const uint8_t left_leg[5] = {0, 0, 0, 1, 0};
  Rows s;
  s.row(g, xy, left_leg, 100, 48, 9, 0);        // second pair through its left member: slot Q + 1
  EXPECT(s.n[2] == 1 && s.hits[2] == 1 && s.key[2] == 6 && s.n[0] == 0 && s.n[1] == 0);
  const uint8_t none[5] = {0, 0, 0, 0, 0};
  s.row(g, xy, none, 100, 48, 9, 1);            // no visible part: nothing changes
  EXPECT(s.n[0] == 0 && s.n[1] == 0 && s.n[2] == 1);
  Rows t;                                       // a merged index outside [0, M) in the table is passed over
  t.merged[1] = 7;
  t.row(g, xy, crown_only, 100, 48, 9, 0);
  EXPECT(t.n[0] == 0 && t.n[1] == 0 && t.n[2] == 0);
}

int main() {
  check_arguments();
  check_patch();
  check_rows();
  std::printf(failures ? "%d check(s) failed\n" : "part_purity_check: all checks passed\n", failures);
  return failures ? 1 : 0;
}
