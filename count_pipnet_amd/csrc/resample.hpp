// Pillow's ImagingResample(BILINEAR) for 8-bit RGB, restated (oracle/input_ref.py): the
// coefficient rows and the two-pass integer resample of one output pixel.  Shared by the
// evaluation transform (input_ops.hip) and the training augmentation (augment_ops.hip), so
// both resize with the same arithmetic.
#pragma once
#include "common.hpp"

namespace pipnet_resample {

constexpr int PREC = 22;   // PRECISION_BITS = 32 - 8 - 2

__host__ __device__ inline int ksize_for(int in_size, int out_size) {
  const double scale = (double)((float)in_size - 0.0f) / out_size;
  const double support = scale < 1.0 ? 1.0 : scale;
  return (int)ceil(support) * 2 + 1;
}

__device__ inline double triangle(double x) {
  if (x < 0.0) x = -x;
  return x < 1.0 ? 1.0 - x : 0.0;
}

// Table row = (xmin, n, k[0..kmax)) for output coordinate xx of an axis resized in_size ->
// out_size: precompute_coeffs (triangle filter, support max(scale, 1)) in double, normalised,
// then 22-bit fixed point rounded half away from zero (normalize_coeffs_8bpc).
__device__ inline void coeff_row(int in_size, int out_size, int xx, int kmax, int32_t* __restrict__ row) {
#pragma clang fp contract(off)
  const double scale = (double)((float)in_size - 0.0f) / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;
  const double center = 0.0 + (xx + 0.5) * scale;
  const double ss = 1.0 / filterscale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  if (xmax > kmax) xmax = kmax;    // cannot happen (kmax >= ksize); keeps the row in bounds
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) ww += triangle(((double)(x + xmin) - center + 0.5) * ss);
  for (int x = 0; x < kmax; ++x) {
    int32_t q = 0;
    if (x < xmax) {
      double w = triangle(((double)(x + xmin) - center + 0.5) * ss);
      if (ww != 0.0) w /= ww;
      const double f = w * (double)(1 << PREC);
      q = w < 0 ? (int32_t)(-0.5 + f) : (int32_t)(0.5 + f);
    }
    row[2 + x] = q;
  }
  row[0] = xmin;
  row[1] = xmax;
}

__device__ inline int clip8(int ss) {
  const int v = ss >> PREC;            // arithmetic shift, as Pillow's clip8 lookup
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// Output pixel (y, x) of the h x w HWC image `img` resized to out_h x out_w; tv / th are the
// vertical row y and the horizontal row x of the coefficient table.  Two separable passes, each
// clip8((1 << 21) + sum(u8 * k) >> 22): horizontal first, vertical first for very tall images
// that shrink vertically (h > 100 w, out_h < h), a pass skipped when its axis keeps its size.
// The first pass is recomputed per output pixel (no intermediate image).
__device__ inline void resample_pixel(const uint8_t* __restrict__ img, int h, int w, int out_h, int out_w,
                                      const int32_t* __restrict__ tv, const int32_t* __restrict__ th, int y, int x,
                                      int (&c3)[3]) {
  const bool need_h = w != out_w, need_v = h != out_h;
  if (!need_h && !need_v) {
    const uint8_t* p = img + ((int64_t)y * w + x) * 3;
    c3[0] = p[0], c3[1] = p[1], c3[2] = p[2];
  } else if (!need_v) {                  // horizontal pass only
    const int xmin = th[0], n = th[1];
    const uint8_t* p = img + ((int64_t)y * w + xmin) * 3;
    int a0 = 1 << (PREC - 1), a1 = a0, a2 = a0;
    for (int t = 0; t < n; ++t) {
      const int k = th[2 + t];
      a0 += p[3 * t] * k, a1 += p[3 * t + 1] * k, a2 += p[3 * t + 2] * k;
    }
    c3[0] = clip8(a0), c3[1] = clip8(a1), c3[2] = clip8(a2);
  } else if (!need_h) {                  // vertical pass only
    const int ymin = tv[0], n = tv[1];
    int a0 = 1 << (PREC - 1), a1 = a0, a2 = a0;
    for (int s = 0; s < n; ++s) {
      const uint8_t* p = img + ((int64_t)(ymin + s) * w + x) * 3;
      const int k = tv[2 + s];
      a0 += p[0] * k, a1 += p[1] * k, a2 += p[2] * k;
    }
    c3[0] = clip8(a0), c3[1] = clip8(a1), c3[2] = clip8(a2);
  } else if (h > 100 * w && out_h < h) {   // Pillow: vertical pass first for very tall images
    const int ymin = tv[0], nv = tv[1], xmin = th[0], nh = th[1];
    int a0 = 1 << (PREC - 1), a1 = a0, a2 = a0;
    for (int t = 0; t < nh; ++t) {
      int v0 = 1 << (PREC - 1), v1 = v0, v2 = v0;
      for (int s = 0; s < nv; ++s) {
        const uint8_t* p = img + ((int64_t)(ymin + s) * w + xmin + t) * 3;
        const int k = tv[2 + s];
        v0 += p[0] * k, v1 += p[1] * k, v2 += p[2] * k;
      }
      const int k = th[2 + t];
      a0 += clip8(v0) * k, a1 += clip8(v1) * k, a2 += clip8(v2) * k;
    }
    c3[0] = clip8(a0), c3[1] = clip8(a1), c3[2] = clip8(a2);
  } else {                                // horizontal pass first (the common case)
    const int ymin = tv[0], nv = tv[1], xmin = th[0], nh = th[1];
    int a0 = 1 << (PREC - 1), a1 = a0, a2 = a0;
    for (int s = 0; s < nv; ++s) {
      const uint8_t* p = img + ((int64_t)(ymin + s) * w + xmin) * 3;
      int v0 = 1 << (PREC - 1), v1 = v0, v2 = v0;
      for (int t = 0; t < nh; ++t) {
        const int k = th[2 + t];
        v0 += p[3 * t] * k, v1 += p[3 * t + 1] * k, v2 += p[3 * t + 2] * k;
      }
      const int k = tv[2 + s];
      a0 += clip8(v0) * k, a1 += clip8(v1) * k, a2 += clip8(v2) * k;
    }
    c3[0] = clip8(a0), c3[1] = clip8(a1), c3[2] = clip8(a2);
  }
}

}  // namespace pipnet_resample
