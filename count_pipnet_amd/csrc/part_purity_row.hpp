// The row function of the part-purity evaluation (util/eval_cub_csv.py:62-118): one row =
// (prototype, image, latent location of the prototype's maximum).  Shared by the kernels of
// part_purity.hip and the stand-alone host check (tools/part_purity_check.cpp), nothing else.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PP_HD __host__ __device__ inline
#else
#define PP_HD inline
#endif

constexpr int PP_PATCH = 32;               // util/func.py get_patch_size: 32 pixels whatever the backbone
constexpr int PP_KEY_SLOT_BITS = 6;        // first_key = ordinal << 6 | slot, slot < 2 Q <= 64
constexpr uint64_t PP_NO_KEY = ~0ull;

struct PpGeom {
  int H, W;                                // latent map
  int image_size, skip;                    // util/func.py get_patch_size
  int small_map;                           // the 26 x 26 small-stride rule of get_img_coordinates
};

struct PpFold {
  const int32_t* merged;                   // [Q] index of the merged part, 0 .. M-1
  const uint8_t* is_left;                  // [Q] the id is folded into its right partner
  const int32_t* pair_index;               // [Q] index of a left id's pair, in pair order (others: not read)
  int Q, M;
};

// One axis of util/vis_pipnet.py get_img_coordinates (:1162-1193) for the 3-D map shape (P, H, W)
// eval_cub_csv.py hands it: i the latent index, n the axis length (the clamp to the image border),
// last = W - 1 (the small-stride rule tests both axes against the last column).
PP_HD void pp_axis(const PpGeom& g, int i, int n, int& lo, int& hi) {
  if (g.small_map) {
    lo = (i - 1) * g.skip + 4;
    lo = lo < 0 ? 0 : lo;
    if (!(i < g.W - 1)) lo -= 4;
    hi = lo + PP_PATCH;
  } else {
    lo = i * g.skip;
    hi = i * g.skip + PP_PATCH;
    hi = hi > g.image_size ? g.image_size : hi;
  }
  if (i == n - 1) hi = g.image_size;
  if (hi == g.image_size) lo = g.image_size - PP_PATCH;
}

PP_HD void pp_patch(const PpGeom& g, int loc, int& h0, int& h1, int& w0, int& w1) {
  pp_axis(g, loc / g.W, g.H, h0, h1);
  pp_axis(g, loc % g.W, g.W, w0, w1);
}

// Merge one row into the state of its prototype (n, hits, first_key: the prototype's [M] slices,
// entry m at index m * stride).  xy [Q,2] fp64 (x, y), vis [Q], width / height: the image's
// annotations.  ord: the row ordinal.
// Geometry in fp64 as the reference writes it: (orig / float(image_size)) * coordinate -- a
// divide, then a multiply; closed comparisons.
PP_HD void pp_row(const PpGeom& g, const PpFold& f, const double* xy, const uint8_t* vis, int width, int height,
                  int loc, uint64_t ord, int64_t* n, int64_t* hits, uint64_t* first_key, int stride = 1) {
  int h0, h1, w0, w1;
  pp_patch(g, loc, h0, h1, w0, w1);
  const double sh = (double)height / (double)g.image_size;
  const double sw = (double)width / (double)g.image_size;
  const double hmin = sh * (double)h0, hmax = sh * (double)h1;
  const double wmin = sw * (double)w0, wmax = sw * (double)w1;
  uint32_t seen = 0, hit = 0;              // merged parts present / hit in this row (M <= 32)
  for (int q = 0; q < f.Q; ++q) {
    if (!vis[q]) continue;
    const int m = f.merged[q];
    if ((unsigned)m >= (unsigned)f.M) continue;
    const int at = m * stride;
    const double x = xy[2 * q], y = xy[2 * q + 1];
    const bool in = y >= hmin && y <= hmax && x >= wmin && x <= wmax;
    int slot = q;                          // own id: its position among the image's parts
    if (f.is_left[q]) {                    // through the left partner: after every own id, in pair order
      const int pi = f.pair_index[q];
      slot = f.Q + ((unsigned)pi < (unsigned)f.Q ? pi : f.Q - 1);
    }
    const uint64_t key = (ord << PP_KEY_SLOT_BITS) | (uint64_t)slot;
    const uint32_t bit = 1u << m;
    if (!(seen & bit)) {
      seen |= bit;
      n[at] += 1;
    }
    if (key < first_key[at]) first_key[at] = key;
    if (in && !(hit & bit)) {
      hit |= bit;
      hits[at] += 1;
    }
  }
}
