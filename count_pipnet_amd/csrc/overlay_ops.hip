// Prototype feature-map overlays on the GPU: the arrays behind the *_overlay.png figures of util/vis_pipnet.py
// :454-475 (PIP-Net) and :1000-1021 (CountPIPNet).  Per entry (image b, prototype p) the reference runs, on the host,
//   scipy.ndimage.zoom(map, (S / h, S / w))  (order 3, mode 'constant', grid_mode False; float64 inside, float32 out)
//   mask = resized > 0.1;  overlay[y, x] = (*cmap(resized[y, x])[:3], 0.7) in a Python loop over the S * S pixels.
// The arithmetic contract (every operation, its order and its precision) is stated in include/pipnet_amd.h next to
// pipnet_map_overlay and restated in numpy in tests/overlay_ref.py; this file follows it operation for operation,
// with nothing contracted, so the results are those bits.
// overlay_kernel: one workgroup per (entry, band of `band` output rows).
//   1. the map (one channel of the NHWC tensor, stride P) goes into LDS as doubles, rows padded to an odd stride so
//      that the row pass below (lane r walks row r) spreads over the banks; the first band also writes `maps`
//      (and where no other output is asked for it is the only band and ends here: a gather of the maps);
//   2. the order-3 prefilter: one lane per column, then one lane per row -- a line is a sequential recursion, a
//      26 x 26 map costs two passes of 26 lanes, and every band redoes it rather than exchange 5 KB through memory;
//   3. one lane per output column keeps its four tap indices and weights in registers and walks the band's rows (the
//      row taps come from a small LDS table): 16 LDS doubles, 32 multiplications and 16 additions per pixel, the
//      float32 result into an LDS tile [band][S];
//   4. the band's pixels are one contiguous span of every output, so the stores are flat: 16 bytes per lane and
//      consecutive lanes on consecutive 16 bytes -- a lane writes half an overlay pixel (two doubles), four resized
//      floats, or four mask / colour bytes (S % 4 == 0 and aligned pointers; one element per lane otherwise, the
//      same values).  The overlay is 32 of the 38 bytes a pixel costs.
// Every byte offset is 64-bit.  Tap indices are clamped to the map, so no input can make the kernel leave LDS.
#include <cmath>

#include "common.hpp"

#pragma clang fp contract(off)

namespace pipnet_overlay {

constexpr int TPB = 256;
constexpr int MAX_BAND = 32;          // output rows per workgroup, halved until the LDS fits
constexpr int LUT_DOUBLES = 256 * 3;
constexpr int LDS_LIMIT = 64 * 1024;

struct Axis {                         // per-axis constants, computed on the host in doubles
  double zn;                          // pow(z, n - 1), libm
  double zoom;                        // (n - 1) / (S - 1)
};

// LDS bytes beside the coefficients: the colour table, the row-tap table (4 weights + 4 indices per row) and the tile
static inline int64_t side_bytes(int band, int S) {
  return (int64_t)LUT_DOUBLES * 8 + (int64_t)band * 4 * (8 + 4) + (int64_t)band * S * 4;
}

// the order-3 prefilter of one line c[0], c[st], ..., c[(n - 1) * st], in place
PIPNET_DEV void filter_line(double* c, int n, int st, double z, double gain, double zn) {
#pragma clang fp contract(off)
  for (int i = 0; i < n; ++i) c[i * st] *= gain;
  double c0 = c[0] + zn * c[(n - 1) * st];
  double zi = z;
  for (int i = 1; i < n - 1; ++i) {
    c0 += zi * (c[i * st] + zn * c[(n - 1 - i) * st]);
    zi *= z;
  }
  c0 /= 1.0 - zn * zn;
  c[0] = c0;
  double run = c0;
  for (int i = 1; i < n; ++i) {              // causal
    run = c[i * st] + z * run;
    c[i * st] = run;
  }
  run = (z * c[(n - 2) * st] + c[(n - 1) * st]) * z / (z * z - 1.0);
  c[(n - 1) * st] = run;
  for (int i = n - 2; i >= 0; --i) {         // anticausal
    run = z * (run - c[i * st]);
    c[i * st] = run;
  }
}

// the four taps of output coordinate i on an axis of n samples: indices mirrored once, cubic B-spline weights
PIPNET_DEV void taps(int i, int n, double zoom, int idx[4], double wt[4]) {
#pragma clang fp contract(off)
  const double x = (double)i * zoom;
  const double f = floor(x);
  const double y = x - f;
  const double t = 1.0 - y;
  wt[0] = t * t * t / 6.0;
  wt[1] = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0;
  wt[2] = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0;
  wt[3] = 1.0 - wt[0] - wt[1] - wt[2];
  const int f0 = (int)f - 1;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    int k = f0 + a;
    if (k < 0) k = -k;
    if (k >= n) k = 2 * (n - 1) - k;
    idx[a] = min(max(k, 0), n - 1);          // in the contract the mirror already lands inside
  }
}

PIPNET_DEV bool above(float r) { return r > 0.1f; }

// min(trunc(r * 256f), 255) on the mask, 0 off it
PIPNET_DEV int colour_of(float r) {
  if (!above(r)) return 0;
  const float s = r * 256.0f;
  return s >= 255.0f ? 255 : (int)s;
}

__global__ __launch_bounds__(TPB) void overlay_kernel(const float* __restrict__ proto, int B, int h, int w, int P,
                                                      const int32_t* __restrict__ items,
                                                      const double* __restrict__ lut, int S, double alpha, double z,
                                                      double gain, Axis ay, Axis ax, float* __restrict__ maps,
                                                      float* __restrict__ resized, uint8_t* __restrict__ mask,
                                                      uint8_t* __restrict__ colour, double* __restrict__ overlay,
                                                      int band, int bands, int ws, int vec) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* coef = reinterpret_cast<double*>(smem);                  // [h][ws], rounded up to 16 bytes
  double* lutd = coef + ((h * ws + 1) & ~1);                       // [256][3]
  double* wyt = lutd + LUT_DOUBLES;                                // [band][4]
  int* iyt = reinterpret_cast<int*>(wyt + band * 4);               // [band][4]
  float* tile = reinterpret_cast<float*>(iyt + band * 4);          // [band][S]
  const int tid = threadIdx.x;
  const int item = blockIdx.x / bands;
  const int bi = blockIdx.x - item * bands;
  const int b = items[(int64_t)item * 2], p = items[(int64_t)item * 2 + 1];
  if (b < 0 || b >= B || p < 0 || p >= P) return;                  // the whole workgroup: nothing written
  const int y0 = bi * band, rows = min(band, S - y0);

  const float* src = proto + (int64_t)b * h * w * P + p;
  float* mdst = (maps && bi == 0) ? maps + (int64_t)item * h * w : nullptr;
  for (int i = tid; i < h * w; i += TPB) {
    const int r = i / w, c = i - r * w;
    const float v = src[(int64_t)i * P];
    coef[r * ws + c] = (double)v;
    if (mdst) mdst[i] = v;
  }
  if (overlay)
    for (int i = tid; i < LUT_DOUBLES; i += TPB) lutd[i] = lut[i];
  if (!resized && !mask && !colour && !overlay) return;            // only the maps were asked for (one band then)
  if (tid < rows) {
    int idx[4];
    double wt[4];
    taps(y0 + tid, h, ay.zoom, idx, wt);
#pragma unroll
    for (int a = 0; a < 4; ++a) wyt[tid * 4 + a] = wt[a], iyt[tid * 4 + a] = idx[a] * ws;
  }
  __syncthreads();
  for (int c = tid; c < w; c += TPB) filter_line(coef + c, h, ws, z, gain, ay.zn);       // axis 0: the columns
  __syncthreads();
  for (int r = tid; r < h; r += TPB) filter_line(coef + r * ws, w, 1, z, gain, ax.zn);   // axis 1: the rows
  __syncthreads();

  for (int x = tid; x < S; x += TPB) {
    int ix[4];
    double wx[4];
    taps(x, w, ax.zoom, ix, wx);
    for (int yy = 0; yy < rows; ++yy) {
      double s = 0.0;
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const double* row = coef + iyt[yy * 4 + a];
        const double wa = wyt[yy * 4 + a];
#pragma unroll
        for (int bb = 0; bb < 4; ++bb) {
          double v = row[ix[bb]];
          v *= wa;
          v *= wx[bb];
          s += v;
        }
      }
      tile[yy * S + x] = (float)s;
    }
  }
  __syncthreads();

  const int npix = rows * S;
  const int64_t base = (int64_t)item * S * S + (int64_t)y0 * S;     // first pixel of the band in every output
  if (vec) {                          // S % 4 == 0: npix and base are multiples of 4
    for (int i = tid; i < (npix >> 2); i += TPB) {
      const f32x4 r4 = *reinterpret_cast<const f32x4*>(tile + 4 * i);
      if (resized) *reinterpret_cast<f32x4*>(resized + base + 4 * i) = r4;
      if (mask)
        *reinterpret_cast<uint32_t*>(mask + base + 4 * i) = (uint32_t)above(r4.x) | ((uint32_t)above(r4.y) << 8) |
                                                              ((uint32_t)above(r4.z) << 16) |
                                                              ((uint32_t)above(r4.w) << 24);
      if (colour)
        *reinterpret_cast<uint32_t*>(colour + base + 4 * i) =
            (uint32_t)colour_of(r4.x) | ((uint32_t)colour_of(r4.y) << 8) | ((uint32_t)colour_of(r4.z) << 16) |
            ((uint32_t)colour_of(r4.w) << 24);
    }
  } else {
    for (int i = tid; i < npix; i += TPB) {
      const float r = tile[i];
      if (resized) resized[base + i] = r;
      if (mask) mask[base + i] = (uint8_t)above(r);
      if (colour) colour[base + i] = (uint8_t)colour_of(r);
    }
  }
  if (overlay) {                      // half a pixel per lane: 16 bytes, consecutive lanes on consecutive 16 bytes
    typedef double f64x2 __attribute__((ext_vector_type(2)));
    f64x2* dst = reinterpret_cast<f64x2*>(overlay + base * 4);
    for (int j = tid; j < 2 * npix; j += TPB) {
      const float r = tile[j >> 1];
      f64x2 v = {0.0, 0.0};
      if (above(r)) {
        const double* e = lutd + colour_of(r) * 3;
        if (j & 1) v.x = e[2], v.y = alpha;
        else v.x = e[0], v.y = e[1];
      }
      dst[j] = v;
    }
  }
}

}  // namespace pipnet_overlay

extern "C" int pipnet_map_overlay(const float* proto, int B, int h, int w, int P, const int32_t* items, int N,
                                  const double* lut, int S, double alpha, float* maps, float* resized, uint8_t* mask,
                                  uint8_t* colour, double* overlay, void* stream) {
#pragma clang fp contract(off)
  using namespace pipnet_overlay;
  if (B < 0 || N < 0 || P <= 0 || h < 3 || w < 3 || S < 2) return PIPNET_ERR_ARG;
  if ((int64_t)S * S >= ((int64_t)1 << 29)) return PIPNET_ERR_ARG;
  const int ws = w | 1;                                                         // odd row stride, in doubles
  const int64_t coef_bytes = (((int64_t)h * ws + 1) & ~(int64_t)1) * 8;         // a multiple of 16: the tile stays aligned
  int band = MAX_BAND;
  while (band > 1 && coef_bytes + side_bytes(band, S) > LDS_LIMIT) band >>= 1;
  const int64_t lds = coef_bytes + side_bytes(band, S);
  if (lds > LDS_LIMIT) return PIPNET_ERR_ARG;
  if (N == 0) return PIPNET_OK;
  if (!proto || !items || !lut || B == 0) return PIPNET_ERR_ARG;
  if (!aligned16(overlay) || !aligned16(lut)) return PIPNET_ERR_ARG;            // NULL is aligned
  const bool pictures = resized || mask || colour || overlay;
  const int bands = pictures ? (S + band - 1) / band : 1;                       // the maps alone: one workgroup each
  if ((int64_t)N * bands >= ((int64_t)1 << 24)) return PIPNET_ERR_ARG;           // a grid holds < 2^32 threads
  const uintptr_t bytes4 = reinterpret_cast<uintptr_t>(mask) | reinterpret_cast<uintptr_t>(colour);
  const int vec = S % 4 == 0 && aligned16(resized) && (bytes4 & 3u) == 0;
  const double z = sqrt(3.0) - 2.0;
  const double gain = (1.0 - z) * (1.0 - 1.0 / z);
  const Axis ay = {pow(z, (double)(h - 1)), (double)(h - 1) / (double)(S - 1)};
  const Axis ax = {pow(z, (double)(w - 1)), (double)(w - 1) / (double)(S - 1)};
  hipLaunchKernelGGL(overlay_kernel, dim3((unsigned)((int64_t)N * bands)), dim3(TPB), (size_t)lds,
                     (hipStream_t)stream, proto, B, h, w, P, items, lut, S, alpha, z, gain, ay, ax, maps, resized,
                     mask, colour, overlay, band, bands, ws, vec);
  PIPNET_CHECK_LAUNCH();
  return PIPNET_OK;
}
