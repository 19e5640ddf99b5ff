// Two-view training augmentation on the GPU: the reference's TwoAugSupervisedDataset
// (util/data.py:596-617) with the transforms of every get_* family (util/data.py:261-594),
// applied to a ragged batch of decoded RGB images.  The random parameters are drawn on the host
// (count_pipnet_amd/augment.py); the pixel arithmetic below restates Pillow 12.2.0's, so for the
// same parameters the uint8 images and the fp32 views are bit-identical to the reference's
// (tests/augment_ref.py is the numpy restatement, pinned against live Pillow).
//
// transform1 (once per image) = pipnet_augment_geometry_rgb8:
//   Resize((S1, S1)) -> [Image.transform(AFFINE, NEAREST, fill) | Image.rotate] -> [hflip]
//   -> RandomResizedCrop = crop(box).resize((S2, S2), BILINEAR)                 -> [B,S2,S2,3] u8
//   The first resize writes an S1 x S1 uint8 intermediate (resample.hpp, as the evaluation
//   transform).  Warp and flip are index maps, so they are composed into the tap fetch of the
//   second resample, whose coefficients are those of an image of the crop's size and whose taps
//   therefore stay inside the crop window.
// transform2 (once per view) = pipnet_augment_view_rgb8:
//   [colour op 1] -> [colour op 2] -> RandomCrop(s) at (i, j) -> [Grayscale(3)] -> ToTensor
//   -> [+ noise] -> Normalize                                                   -> [V,B,3,s,s] fp32
//   One workgroup per (view, image, slice of output rows): LDS histograms of the whole S2 x S2
//   image where the operation needs them (Contrast: mean of L; AutoContrast, Equalize:
//   per-channel histograms; as second operation: of the first operation's output), a 3 x 256
//   LUT per operation, then the windowed apply with coalesced fp32 plane stores.
#include "philox.hpp"
#include "resample.hpp"

namespace {

using namespace pipnet_resample;

constexpr int GP = PIPNET_AUG_GEOM_PARAMS;   // path, m0..m5, fill, flip, crop top, left, height, width
constexpr int VP = PIPNET_AUG_VIEW_PARAMS;   // op1, param1, op2, param2, crop top, left, noise flag, noise id
enum { OP_IDENTITY = 0, OP_BRIGHTNESS, OP_COLOR, OP_CONTRAST, OP_SHARPNESS, OP_POSTERIZE, OP_SOLARIZE,
       OP_AUTOCONTRAST, OP_EQUALIZE };
enum { WARP_NONE = 0, WARP_FIXED = 1, WARP_DOUBLE = 2 };

PIPNET_DEV int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
PIPNET_DEV int to_int(double v) {            // saturating (int)v: a wild parameter cannot be UB
  return v >= 2147483647.0 ? 2147483647 : (v <= -2147483648.0 ? (int)-2147483648LL : (int)v);
}

// The crop window of image b, clamped into the S1 x S1 image.
PIPNET_DEV void crop_box(const double* __restrict__ gp, int S1, int& ci, int& cj, int& ch, int& cw) {
  ci = clampi(to_int(gp[9]), 0, S1 - 1);
  cj = clampi(to_int(gp[10]), 0, S1 - 1);
  ch = clampi(to_int(gp[11]), 1, S1 - ci);
  cw = clampi(to_int(gp[12]), 1, S1 - cj);
}

// ---- geometry ---------------------------------------------------------------------------

// Coefficient rows of both resamples.  Rows [0, B*2*S1): sizes[b] -> S1 x S1 (kmax1 taps);
// rows after them: crop (ch, cw) of image b -> S2 x S2 (kmax2 taps).  Vertical rows first.
__global__ __launch_bounds__(256) void aug_coeffs_kernel(const int32_t* __restrict__ sizes,
                                                         const double* __restrict__ gparams, int B, int S1, int S2,
                                                         int kmax1, int kmax2, int32_t* __restrict__ table1,
                                                         int32_t* __restrict__ table2) {
  int i = blockIdx.x * 256 + threadIdx.x;
  const int n1 = B * 2 * S1, n2 = B * 2 * S2;
  if (i < n1) {
    const int b = i / (2 * S1), r = i - b * 2 * S1;
    const bool vert = r < S1;
    coeff_row(sizes[2 * b + (vert ? 0 : 1)], S1, vert ? r : r - S1, kmax1, table1 + (int64_t)i * (2 + kmax1));
  } else if (i < n1 + n2) {
    i -= n1;
    const int b = i / (2 * S2), r = i - b * 2 * S2;
    const bool vert = r < S2;
    int ci, cj, ch, cw;
    crop_box(gparams + (int64_t)b * GP, S1, ci, cj, ch, cw);
    coeff_row(vert ? ch : cw, S2, vert ? r : r - S2, kmax2, table2 + (int64_t)i * (2 + kmax2));
  }
}

// Per image: the 16.16 fixed-point matrix a0..a5 (Pillow's affine_fixed) and, on the double
// path only (the others never read them), the input coordinate of every output row / column
// (affine_transform with m1 == m3 == 0: COORD(xo), xo += m0 -- accumulated by repeated addition
// as Pillow does).  One thread per (image, axis).
// Layout per image: [8 + 2*S1] int32 = a0..a5, pad, pad, yin[S1], xin[S1].
__global__ __launch_bounds__(64) void aug_warp_prep_kernel(const double* __restrict__ gparams, int B, int S1,
                                                           int32_t* __restrict__ warp) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= 2 * B) return;
  const int b = t >> 1, axis = t & 1;        // 0: rows (m3 m4 m5), 1: columns (m0 m1 m2)
  const double* gp = gparams + (int64_t)b * GP;
  int32_t* w = warp + (int64_t)b * (8 + 2 * S1);
  const double ma = gp[axis ? 1 : 4], mb = gp[axis ? 2 : 5], mc = gp[axis ? 3 : 6];
  const double diag = axis ? ma : mb;        // m0 / m4
  int32_t* a = w + (axis ? 0 : 3);
  a[0] = to_int(floor(ma * 65536.0 + 0.5));
  a[1] = to_int(floor(mb * 65536.0 + 0.5));
  a[2] = to_int(floor((mc + 0.5 * ma + 0.5 * mb) * 65536.0 + 0.5));
  w[6 + axis] = 0;
  if (to_int(gp[0]) != WARP_DOUBLE) return;
  int32_t* tab = w + 8 + (axis ? S1 : 0);
  double o = mc + diag * 0.5;
  for (int k = 0; k < S1; ++k) {
    tab[k] = o < 0.0 ? -1 : to_int(o);
    o += diag;
  }
}

// First resize: image b (h x w) -> S1 x S1 uint8 HWC.  One thread per output pixel.
__global__ __launch_bounds__(256) void aug_resize_u8_kernel(const uint8_t* __restrict__ pix,
                                                            const int64_t* __restrict__ offsets,
                                                            const int32_t* __restrict__ sizes, int B, int S1, int kmax,
                                                            const int32_t* __restrict__ table,
                                                            uint8_t* __restrict__ mid) {
  const int64_t plane = (int64_t)S1 * S1;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * plane) return;
  const int b = (int)(i / plane);
  const int rem = (int)(i - (int64_t)b * plane);
  const int y = rem / S1, x = rem - y * S1;
  const int rs = 2 + kmax;
  const int32_t* tv = table + ((int64_t)b * 2 * S1 + y) * rs;
  const int32_t* th = table + ((int64_t)b * 2 * S1 + S1 + x) * rs;
  int c3[3];
  resample_pixel(pix + offsets[b], sizes[2 * b], sizes[2 * b + 1], S1, S1, tv, th, y, x, c3);
  uint8_t* q = mid + i * 3;
  q[0] = (uint8_t)c3[0], q[1] = (uint8_t)c3[1], q[2] = (uint8_t)c3[2];
}

struct Warp {
  const uint8_t* img;     // S1 x S1 x 3 resized image
  const int32_t* tab;     // aug_warp_prep_kernel's row of this image
  int S1, path, fill, flip;
};

// Pixel (y, x) of hflip(warp(img)): both are index maps (NEAREST), out-of-image reads the fill.
PIPNET_DEV void fetch(const Warp& w, int y, int x, int (&c)[3]) {
  if (w.flip) x = w.S1 - 1 - x;
  int xin = x, yin = y;
  if (w.path == WARP_FIXED) {
    const int32_t* a = w.tab;
    xin = (int32_t)((int64_t)a[2] + (int64_t)x * a[0] + (int64_t)y * a[1]) >> 16;
    yin = (int32_t)((int64_t)a[5] + (int64_t)x * a[3] + (int64_t)y * a[4]) >> 16;
  } else if (w.path == WARP_DOUBLE) {
    yin = w.tab[8 + y];
    xin = w.tab[8 + w.S1 + x];
  }
  if (xin < 0 || xin >= w.S1 || yin < 0 || yin >= w.S1) {
    c[0] = c[1] = c[2] = w.fill;
  } else {
    const uint8_t* p = w.img + ((int64_t)yin * w.S1 + xin) * 3;
    c[0] = p[0], c[1] = p[1], c[2] = p[2];
  }
}

// Second resample: crop(box).resize((S2, S2), BILINEAR) of hflip(warp(mid)), horizontal pass
// first, a pass skipped when the crop already has that size.  One thread per output pixel.
__global__ __launch_bounds__(256) void aug_geometry_kernel(const uint8_t* __restrict__ mid,
                                                           const double* __restrict__ gparams,
                                                           const int32_t* __restrict__ warp, int B, int S1, int S2,
                                                           int kmax, const int32_t* __restrict__ table,
                                                           uint8_t* __restrict__ out) {
  const int64_t plane = (int64_t)S2 * S2;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * plane) return;
  const int b = (int)(i / plane);
  const int rem = (int)(i - (int64_t)b * plane);
  const int y = rem / S2, x = rem - y * S2;
  const double* gp = gparams + (int64_t)b * GP;
  int ci, cj, ch, cw;
  crop_box(gp, S1, ci, cj, ch, cw);
  Warp w;
  w.img = mid + (int64_t)b * S1 * S1 * 3;
  w.tab = warp + (int64_t)b * (8 + 2 * S1);
  w.S1 = S1;
  w.path = to_int(gp[0]);
  w.fill = clampi(to_int(gp[7]), 0, 255);
  w.flip = gp[8] != 0.0;
  const int rs = 2 + kmax;
  const int32_t* tv = table + ((int64_t)b * 2 * S2 + y) * rs;
  const int32_t* th = table + ((int64_t)b * 2 * S2 + S2 + x) * rs;
  const bool need_h = cw != S2, need_v = ch != S2;
  // taps in crop coordinates: [ymin, ymin + nv) x [xmin, xmin + nh), unit weight when skipped
  const int ymin = need_v ? tv[0] : y, nv = need_v ? tv[1] : 1;
  const int xmin = need_h ? th[0] : x, nh = need_h ? th[1] : 1;
  int c[3], a0 = 1 << (PREC - 1), a1 = a0, a2 = a0;
  for (int s = 0; s < nv; ++s) {
    int v0, v1, v2;
    if (need_h) {
      v0 = v1 = v2 = 1 << (PREC - 1);
      for (int t = 0; t < nh; ++t) {
        fetch(w, ci + ymin + s, cj + xmin + t, c);
        const int k = th[2 + t];
        v0 += c[0] * k, v1 += c[1] * k, v2 += c[2] * k;
      }
      v0 = clip8(v0), v1 = clip8(v1), v2 = clip8(v2);
    } else {
      fetch(w, ci + ymin + s, cj + x, c);
      v0 = c[0], v1 = c[1], v2 = c[2];
    }
    if (need_v) {
      const int k = tv[2 + s];
      a0 += v0 * k, a1 += v1 * k, a2 += v2 * k;
    } else {
      a0 = v0, a1 = v1, a2 = v2;
    }
  }
  if (need_v) a0 = clip8(a0), a1 = clip8(a1), a2 = clip8(a2);
  uint8_t* q = out + i * 3;
  q[0] = (uint8_t)a0, q[1] = (uint8_t)a1, q[2] = (uint8_t)a2;
}

// ---- views ------------------------------------------------------------------------------

PIPNET_DEV int luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// Image.blend(degenerate d, image p, factor f) for one 8-bit sample (libImaging/Blend.c).
PIPNET_DEV int blend8(int d, int p, float f) {
#pragma clang fp contract(off)
  const float t = (float)d + f * (float)(p - d);
  if (f >= 0.0f && f <= 1.0f) return (int)t;
  return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

// ImageFilter.SMOOTH at (y, x), channel k: 3x3 kernel [[1,1,1],[1,5,1],[1,1,1]] / 13 in fp32,
// + 0.5 and truncated; the one-pixel border is copied.
PIPNET_DEV int smooth8(const uint8_t* __restrict__ img, int S, int y, int x, int k) {
#pragma clang fp contract(off)
  const uint8_t* p = img + ((int64_t)y * S + x) * 3 + k;
  if (y == 0 || x == 0 || y == S - 1 || x == S - 1) return p[0];
  const int rs = S * 3;
  float ss = 0.0f;
  ss += (float)p[-rs - 3] + (float)p[-rs] + (float)p[-rs + 3];
  ss += (float)p[-3] + 5.0f * (float)p[0] + (float)p[3];
  ss += (float)p[rs - 3] + (float)p[rs] + (float)p[rs + 3];
  const float v = floorf(ss / 13.0f + 0.5f);
  return v <= 0.0f ? 0 : (v >= 255.0f ? 255 : (int)v);
}

PIPNET_DEV bool needs_stats(int op) { return op == OP_CONTRAST || op == OP_AUTOCONTRAST || op == OP_EQUALIZE; }
PIPNET_DEV bool uses_lut(int op) {
  return op == OP_BRIGHTNESS || op == OP_CONTRAST || (op >= OP_POSTERIZE && op <= OP_EQUALIZE);
}

// First operation at pixel (y, x) of the S x S image.
PIPNET_DEV void apply_first(const uint8_t* __restrict__ img, int S, int y, int x, int op, float f,
                            const uint8_t* lut, int (&c)[3]) {
  const uint8_t* p = img + ((int64_t)y * S + x) * 3;
  c[0] = p[0], c[1] = p[1], c[2] = p[2];
  if (op == OP_COLOR) {
    const int l = luma(c[0], c[1], c[2]);
    c[0] = blend8(l, c[0], f), c[1] = blend8(l, c[1], f), c[2] = blend8(l, c[2], f);
  } else if (op == OP_SHARPNESS) {
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = blend8(smooth8(img, S, y, x, k), c[k], f);
  } else if (uses_lut(op)) {
    c[0] = lut[c[0]], c[1] = lut[256 + c[1]], c[2] = lut[512 + c[2]];
  }
}

// Second operation on the first one's output (never Sharpness: it would need neighbours of it).
PIPNET_DEV void apply_second(int op, float f, const uint8_t* lut, int (&c)[3]) {
  if (op == OP_COLOR) {
    const int l = luma(c[0], c[1], c[2]);
    c[0] = blend8(l, c[0], f), c[1] = blend8(l, c[1], f), c[2] = blend8(l, c[2], f);
  } else if (uses_lut(op)) {
    c[0] = lut[c[0]], c[1] = lut[256 + c[1]], c[2] = lut[512 + c[2]];
  }
}

// LUT entry i of channel k for a per-channel operation; hist = [R, G, B, L][256] of the
// operation's input over the whole image (only read where needs_stats(op)), npix its pixels.
PIPNET_DEV int lut_entry(int op, double param, const uint32_t* hist, int npix, int k, int i) {
#pragma clang fp contract(off)
  const uint32_t* h = hist + 256 * k;
  switch (op) {
    case OP_BRIGHTNESS:
      return blend8(0, i, (float)param);
    case OP_CONTRAST: {                       // degenerate = int(ImageStat(L).mean + 0.5)
      double sum = 0.0;
      for (int j = 0; j < 256; ++j) sum += (double)j * (double)hist[768 + j];
      return blend8((int)(sum / (double)npix + 0.5), i, (float)param);
    }
    case OP_POSTERIZE: {
      const int bits = clampi(to_int(param), 0, 8);
      return i & ~((1 << (8 - bits)) - 1) & 255;
    }
    case OP_SOLARIZE:
      return (double)i < param ? i : 255 - i;
    case OP_AUTOCONTRAST: {
      int lo = 0, hi = 255;
      while (lo < 255 && !h[lo]) ++lo;
      while (hi > 0 && !h[hi]) --hi;
      if (hi <= lo) return i;
      const double scale = 255.0 / (double)(hi - lo);
      const double off = (double)(-lo) * scale;
      const int v = (int)((double)i * scale + off);
      return clampi(v, 0, 255);
    }
    case OP_EQUALIZE: {
      int nonempty = 0, last = 0;
      int64_t total = 0, before = 0;
      for (int j = 0; j < 256; ++j) {
        if (h[j]) ++nonempty, last = j;
        total += h[j];
        if (j < i) before += h[j];
      }
      if (nonempty <= 1) return i;
      const int64_t step = (total - h[last]) / 255;
      if (step == 0) return i;
      const int64_t v = (step / 2 + before) / step;
      return v > 255 ? 255 : (int)v;
    }
    default:
      return i;
  }
}

constexpr int VIEW_THREADS = 1024;

__global__ __launch_bounds__(VIEW_THREADS) void aug_view_kernel(
    const uint8_t* __restrict__ imgs, const double* __restrict__ vparams, int B, int S2, int s, int gray, float m0,
    float m1, float m2, float s0, float s1, float s2, float noise_std, uint64_t seed,
    const float* __restrict__ noise, float* __restrict__ out) {
  __shared__ uint32_t hist[4 * 256];
  __shared__ uint8_t lut1[3 * 256], lut2[3 * 256];
  const int vb = blockIdx.x;                 // view * B + image
  const int b = vb % B;
  const int tid = threadIdx.x;
  const double* vp = vparams + (int64_t)vb * VP;
  const uint8_t* img = imgs + (int64_t)b * S2 * S2 * 3;
  const int op1 = to_int(vp[0]), op2 = to_int(vp[2]);
  const double p1 = vp[1], p2 = vp[3];
  const float f1 = (float)p1, f2 = (float)p2;
  const int npix = S2 * S2;

  if (needs_stats(op1)) {                    // uniform per workgroup
    for (int i = tid; i < 4 * 256; i += VIEW_THREADS) hist[i] = 0;
    __syncthreads();
    for (int i = tid; i < npix; i += VIEW_THREADS) {
      const uint8_t* p = img + (int64_t)i * 3;
      if (op1 == OP_CONTRAST) {
        atomicAdd(&hist[768 + luma(p[0], p[1], p[2])], 1u);
      } else {
        atomicAdd(&hist[p[0]], 1u);
        atomicAdd(&hist[256 + p[1]], 1u);
        atomicAdd(&hist[512 + p[2]], 1u);
      }
    }
    __syncthreads();
  }
  if (uses_lut(op1))
    for (int i = tid; i < 768; i += VIEW_THREADS) lut1[i] = (uint8_t)lut_entry(op1, p1, hist, npix, i >> 8, i & 255);
  __syncthreads();
  if (needs_stats(op2)) {
    for (int i = tid; i < 4 * 256; i += VIEW_THREADS) hist[i] = 0;
    __syncthreads();
    for (int i = tid; i < npix; i += VIEW_THREADS) {
      int c[3];
      const int y = i / S2;
      apply_first(img, S2, y, i - y * S2, op1, f1, lut1, c);
      if (op2 == OP_CONTRAST) {
        atomicAdd(&hist[768 + luma(c[0], c[1], c[2])], 1u);
      } else {
        atomicAdd(&hist[c[0]], 1u);
        atomicAdd(&hist[256 + c[1]], 1u);
        atomicAdd(&hist[512 + c[2]], 1u);
      }
    }
    __syncthreads();
  }
  if (uses_lut(op2))
    for (int i = tid; i < 768; i += VIEW_THREADS) lut2[i] = (uint8_t)lut_entry(op2, p2, hist, npix, i >> 8, i & 255);
  __syncthreads();

  const int ci = clampi(to_int(vp[4]), 0, S2 - s), cj = clampi(to_int(vp[5]), 0, S2 - s);
  const bool noisy = vp[6] != 0.0;
  // Philox block per (view, image id, pixel): the draw does not depend on the batch an image is in
  const uint64_t view = (uint64_t)(vb / B);
  const uint64_t ctr0 = (view << 56) | ((uint64_t)(uint32_t)to_int(vp[7]) << 24);
  const int plane = s * s;
  float* o = out + (int64_t)vb * 3 * plane;
  const float* nz = noise ? noise + (int64_t)vb * 3 * plane : nullptr;
  // this workgroup's rows of the window (the statistics above are recomputed per slice: the
  // S2 x S2 image is L2-resident, and most operations need none)
  const int row0 = (int)((int64_t)s * blockIdx.y / gridDim.y), row1 = (int)((int64_t)s * (blockIdx.y + 1) / gridDim.y);
  for (int i = row0 * s + tid; i < row1 * s; i += VIEW_THREADS) {
#pragma clang fp contract(off)
    const int y = i / s, x = i - y * s;
    int c[3];
    apply_first(img, S2, ci + y, cj + x, op1, f1, lut1, c);
    apply_second(op2, f2, lut2, c);
    if (gray) c[0] = c[1] = c[2] = luma(c[0], c[1], c[2]);
    float v0 = (float)c[0] / 255.0f, v1 = (float)c[1] / 255.0f, v2 = (float)c[2] / 255.0f;
    if (noisy) {
      if (nz) {
        v0 += nz[i], v1 += nz[plane + i], v2 += nz[2 * plane + i];
      } else {                               // Box-Muller on the 24-bit uniforms of one block
        uint32_t r[4];
        philox4(seed, ctr0 + (uint64_t)i, r);
        const float k24 = 1.0f / 16777216.0f;
        const float ra = sqrtf(-2.0f * logf(((float)(r[0] >> 8) + 0.5f) * k24));
        const float rb = sqrtf(-2.0f * logf(((float)(r[2] >> 8) + 0.5f) * k24));
        const float ta = 6.28318530718f * (((float)(r[1] >> 8) + 0.5f) * k24);
        const float tb = 6.28318530718f * (((float)(r[3] >> 8) + 0.5f) * k24);
        v0 += noise_std * (ra * cosf(ta));
        v1 += noise_std * (ra * sinf(ta));
        v2 += noise_std * (rb * cosf(tb));
      }
    }
    o[i] = (v0 - m0) / s0;
    o[plane + i] = (v1 - m1) / s1;
    o[2 * plane + i] = (v2 - m2) / s2;
  }
}

}  // namespace

// Host-side planning, shared by the entry and its callers (no HIP call).
extern "C" int pipnet_augment_geometry_plan(const int32_t* sizes_host, int B, int S1, int S2, int* kmax1, int* kmax2,
                                            int64_t* workspace_bytes) {
  if (B < 0 || S1 <= 0 || S2 <= 0 || S1 > 8192 || S2 > 8192 || !kmax1 || !kmax2 || !workspace_bytes ||
      (B > 0 && !sizes_host))
    return PIPNET_ERR_ARG;
  int k1 = 3;
  for (int b = 0; b < B; ++b) {
    const int h = sizes_host[2 * b], w = sizes_host[2 * b + 1];
    if (h <= 0 || w <= 0) return PIPNET_ERR_ARG;
    const int kv = ksize_for(h, S1), kh = ksize_for(w, S1);
    k1 = kv > k1 ? kv : k1;
    k1 = kh > k1 ? kh : k1;
  }
  const int k2 = ksize_for(S1, S2) > 3 ? ksize_for(S1, S2) : 3;   // a crop is at most S1 wide
  *kmax1 = k1;
  *kmax2 = k2;
  const int64_t ints = (int64_t)B * 2 * S1 * (2 + k1) + (int64_t)B * 2 * S2 * (2 + k2) + (int64_t)B * (8 + 2 * S1);
  const int64_t mid = ((int64_t)B * S1 * S1 * 3 + 3) / 4 * 4;
  *workspace_bytes = ints * (int64_t)sizeof(int32_t) + mid;
  return PIPNET_OK;
}

extern "C" int pipnet_augment_geometry_rgb8(const uint8_t* pixels, const int64_t* offsets, const int32_t* sizes,
                                            const double* gparams, int B, int S1, int S2, int kmax1, int kmax2,
                                            int32_t* workspace, uint8_t* out_u8, void* stream) {
  if (B < 0 || S1 <= 0 || S2 <= 0 || S1 > 8192 || S2 > 8192 || kmax1 < 3 || kmax2 < 3) return PIPNET_ERR_ARG;
  if (kmax2 < ksize_for(S1, S2)) return PIPNET_ERR_ARG;
  if (B == 0) return PIPNET_OK;
  if (!pixels || !offsets || !sizes || !gparams || !workspace || !out_u8) return PIPNET_ERR_ARG;
  if ((int64_t)B * S1 * S1 >= ((int64_t)1 << 31) / 4 || (int64_t)B * S2 * S2 >= ((int64_t)1 << 31) / 4)
    return PIPNET_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  int32_t* table1 = workspace;
  int32_t* table2 = table1 + (int64_t)B * 2 * S1 * (2 + kmax1);
  int32_t* warp = table2 + (int64_t)B * 2 * S2 * (2 + kmax2);
  uint8_t* mid = reinterpret_cast<uint8_t*>(warp + (int64_t)B * (8 + 2 * S1));
  const int rows = B * 2 * (S1 + S2);
  hipLaunchKernelGGL(aug_coeffs_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, sizes, gparams, B, S1, S2, kmax1,
                     kmax2, table1, table2);
  PIPNET_CHECK_LAUNCH();
  hipLaunchKernelGGL(aug_warp_prep_kernel, dim3((2 * B + 63) / 64), dim3(64), 0, s, gparams, B, S1, warp);
  PIPNET_CHECK_LAUNCH();
  const int64_t n1 = (int64_t)B * S1 * S1, n2 = (int64_t)B * S2 * S2;
  hipLaunchKernelGGL(aug_resize_u8_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, s, pixels, offsets,
                     sizes, B, S1, kmax1, table1, mid);
  PIPNET_CHECK_LAUNCH();
  hipLaunchKernelGGL(aug_geometry_kernel, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, s, mid, gparams, warp, B,
                     S1, S2, kmax2, table2, out_u8);
  PIPNET_CHECK_LAUNCH();
  return PIPNET_OK;
}

extern "C" int pipnet_augment_view_rgb8(const uint8_t* images, const double* vparams, int V, int B, int S2, int s,
                                        int grayscale, const float* mean3, const float* std3, float noise_std,
                                        uint64_t seed, const float* noise, float* out, void* stream) {
  if (V < 1 || V > 128 || B < 0 || S2 <= 0 || S2 > 8192 || s <= 0 || s > S2 || !mean3 || !std3)
    return PIPNET_ERR_ARG;
  if (3 * (int64_t)s * s >= ((int64_t)1 << 24)) return PIPNET_ERR_ARG;      // the Philox counter's pixel field
  if (B == 0) return PIPNET_OK;
  if (!images || !vparams || !out) return PIPNET_ERR_ARG;
  if ((int64_t)V * B >= ((int64_t)1 << 31) - 1) return PIPNET_ERR_ARG;
  // row slices per (view, image) until about two workgroups per CU are in flight
  int slices = 1;
  while (slices < 8 && (int64_t)V * B * slices < 512 && slices * 2 <= s) slices *= 2;
  hipLaunchKernelGGL(aug_view_kernel, dim3((unsigned)(V * B), slices), dim3(VIEW_THREADS), 0, (hipStream_t)stream, images,
                     vparams, B, S2, s, grayscale ? 1 : 0, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2],
                     noise_std, seed, noise, out);
  PIPNET_CHECK_LAUNCH();
  return PIPNET_OK;
}
