// Prototype similarity heatmaps on the GPU: the heatmap_p{p}.png pixels of util/visualize_prediction.py:92-100.
// Per entry (image b, prototype p, frame f) the reference runs, on the host and at batch size 1,
//   ToPILImage (m.mul(255).byte()) -> Pillow resize(BICUBIC) -> ToTensor -> applyColorMap(uint8(255 * .))
//   -> 0.2 * heat / 255 + 0.6 * frame (float32) -> plt.imsave(vmin=0, vmax=1) ((v * 255).astype(uint8)).
// All of it is integer and float32 arithmetic, restated here bit for bit:
//   1. q = sat8(trunc(m * 255f))                                    one channel of the NHWC map, stride P;
//   2. Pillow's ImagingResample(BICUBIC) of the 8-bit band q to S x S: horizontal pass over the map rows into a
//      uint8 intermediate, then the vertical pass, each clip8(((1 << 21) + sum(u8 * k)) >> 22) with the 22-bit
//      coefficient rows the host built in doubles (kernels.bicubic_rows: the filter needs no fp64 here); a pass
//      whose axis keeps its size is skipped;
//   3. uint8(255 * (r / 255f)) is r for all 256 bytes, so the table index is the resized byte;
//   4. v = fl(fl(w_heat * fl(lut[r][c] / 255f)) + fl(w_img * fl(frame[c] / 255f))), nothing contracted;
//   5. byte = sat8(trunc(fl(v * 255f))).
// heatmap_kernel: one workgroup per (entry, band of BAND output rows).  The map rows the band needs are quantised
// into LDS (a gather of one channel), the horizontal pass fills an LDS [rows][S] byte tile, and after the barrier
// every lane takes four consecutive output pixels: one LDS dword per vertical tap, 12 frame bytes in, 12 bytes
// out (S % 4 == 0 and 4-byte aligned images), or one output byte per lane otherwise -- consecutive lanes on
// consecutive bytes of an output row either way.  Both terms of step 4 have 256 values each way, so the
// workgroup tabulates fl(w_heat * fl(e / 255f)) per table entry and fl(w_img * fl(b / 255f)) per frame byte in
// LDS once (the same float32 operations, done 1024 times instead of six per pixel).
// The coefficient rows come from device memory: every index read from them is clamped to the LDS window, so a
// wrong table gives wrong pixels, never an access outside the map, the tile or the images.  Every byte offset
// is 64-bit.
#include "common.hpp"

namespace pipnet_heatmap {

constexpr int TPB = 256;
constexpr int BAND = 16;           // output rows per workgroup
// Map rows a band can need.  Row y reads [int(c - 1.5), int(c + 2.5)) with c = (y + 0.5) * scale, so a band from
// centre c0 to c1 = c0 + (BAND - 1) * scale spans int(c1 + 2.5) - int(c0 - 1.5) <= 19 rows for scale < 1 (scale == 1
// skips the pass and reads BAND rows).  The window holds three rows more than that; the kernel clamps to it anyway.
constexpr int WIN = BAND + 6;
constexpr int TAPS = 5;            // coefficients per row: 2 * support + 1 for an upscale
constexpr int ROW = 2 + TAPS;      // (xmin, n, k[0..TAPS))
constexpr int PREC = 22;           // Pillow's PRECISION_BITS = 32 - 8 - 2
constexpr int TABLE_BYTES = (256 * 3 + 256) * (int)sizeof(float);
constexpr int LDS_LIMIT = 64 * 1024;

struct __attribute__((packed, aligned(4))) Bytes12 {
  uint32_t w[3];
};

PIPNET_DEV int clip8(int ss) {
  const int v = ss >> PREC;            // arithmetic shift, as Pillow's clip8 lookup
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// uint8(trunc(s)) of torch's .byte() / numpy's astype(uint8) for 0 <= s < 256, saturated beyond; NaN gives 0
PIPNET_DEV int sat8(float s) { return s >= 255.0f ? 255 : (s > 0.0f ? (int)s : 0); }

PIPNET_DEV int blend(const float* __restrict__ lutf, const float* __restrict__ frf, int r, int c, int frame_byte) {
#pragma clang fp contract(off)
  const float v = lutf[r * 3 + c] + frf[frame_byte];
  return sat8(v * 255.0f);
}

__global__ __launch_bounds__(TPB) void heatmap_kernel(const float* __restrict__ proto, int B, int h, int w, int P,
                                                      const uint8_t* __restrict__ frames, int F, int S,
                                                      const int32_t* __restrict__ items,
                                                      const uint8_t* __restrict__ lut,
                                                      const int32_t* __restrict__ rows_h,
                                                      const int32_t* __restrict__ rows_v, float w_heat, float w_img,
                                                      uint8_t* __restrict__ out, uint8_t* __restrict__ resized,
                                                      int bands, int wq, int sq, int vec) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* lutf = reinterpret_cast<float*>(smem);                    // [256][3] fl(w_heat * fl(e / 255f))
  float* frf = lutf + 256 * 3;                                     // [256]    fl(w_img * fl(b / 255f))
  uint8_t* tile = reinterpret_cast<uint8_t*>(frf + 256);           // [WIN][sq] after the horizontal pass
  uint8_t* qbuf = tile + WIN * sq;                                 // [WIN][wq] the quantised map rows
  const int tid = threadIdx.x;
  const int item = blockIdx.x / bands;
  const int band = blockIdx.x - item * bands;
  const int32_t* it = items + (int64_t)item * 3;
  const int b = it[0], p = it[1], f = it[2];
  if (b < 0 || b >= B || p < 0 || p >= P || f < 0 || f >= F) return;        // the whole workgroup: nothing written
  const int y0 = band * BAND, y1 = min(y0 + BAND, S);
  const bool need_h = w != S, need_v = h != S;

  // the map rows [lo, lo + rows) this band reads, never more than WIN and never past the map
  int lo = y0, rows = y1 - y0;
  if (need_v) {
    lo = min(max(rows_v[y0 * ROW], 0), h);
    const int last = rows_v[(y1 - 1) * ROW] + rows_v[(y1 - 1) * ROW + 1];
    rows = min(max(last, lo), min(h, lo + WIN)) - lo;
  }

  {  // the two blend tables: 256 threads, one entry each
    frf[tid] = w_img * ((float)tid / 255.0f);
    const uint8_t* e = lut + 3 * tid;
    lutf[3 * tid] = w_heat * ((float)e[0] / 255.0f);
    lutf[3 * tid + 1] = w_heat * ((float)e[1] / 255.0f);
    lutf[3 * tid + 2] = w_heat * ((float)e[2] / 255.0f);
  }
  const float* src = proto + ((int64_t)b * h + lo) * w * P + p;
  for (int i = tid; i < rows * w; i += TPB) {
    const int r = i / w, c = i - r * w;
    qbuf[r * wq + c] = (uint8_t)sat8(src[(int64_t)i * P] * 255.0f);
  }
  __syncthreads();

  const uint8_t* t = qbuf;           // what the vertical pass reads
  int ts = wq;
  if (need_h) {
    for (int x = tid; x < S; x += TPB) {         // a lane keeps its column's coefficients and walks the rows
      const int32_t* k = rows_h + x * ROW;
      const int xmin = k[0];
      const int t0 = max(0, -xmin), t1 = min(min(k[1], TAPS), w - xmin);
      int kk[TAPS];
#pragma unroll
      for (int j = 0; j < TAPS; ++j) kk[j] = k[2 + j];
      for (int r = 0; r < rows; ++r) {
        int acc = 1 << (PREC - 1);
#pragma unroll
        for (int j = 0; j < TAPS; ++j)
          if (j >= t0 && j < t1) acc += qbuf[r * wq + xmin + j] * kk[j];
        tile[r * sq + x] = (uint8_t)clip8(acc);
      }
    }
    __syncthreads();
    t = tile;
    ts = sq;
  }

  const int64_t image = (int64_t)S * S;
  const uint8_t* frame = frames + (int64_t)f * image * 3;
  uint8_t* dst = out + (int64_t)item * image * 3;
  uint8_t* rdst = resized ? resized + (int64_t)item * image : nullptr;
  if (vec) {                        // four pixels per lane: S % 4 == 0, every image 4-byte aligned
    const int groups = S >> 2;
    for (int i = tid; i < (y1 - y0) * groups; i += TPB) {
      const int yy = i / groups, x = (i - yy * groups) << 2, y = y0 + yy;
      uint32_t r4;
      if (need_v) {
        const int32_t* k = rows_v + y * ROW;
        const int r0 = k[0] - lo;
        const int s0 = max(0, -r0), s1 = min(min(k[1], TAPS), rows - r0);
        int a0 = 1 << (PREC - 1), a1 = a0, a2 = a0, a3 = a0;
        for (int s = s0; s < s1; ++s) {
          const uint32_t q4 = *reinterpret_cast<const uint32_t*>(t + (r0 + s) * ts + x);
          const int kk = k[2 + s];
          a0 += (int)(q4 & 255u) * kk, a1 += (int)((q4 >> 8) & 255u) * kk;
          a2 += (int)((q4 >> 16) & 255u) * kk, a3 += (int)(q4 >> 24) * kk;
        }
        r4 = (uint32_t)clip8(a0) | ((uint32_t)clip8(a1) << 8) | ((uint32_t)clip8(a2) << 16) |
             ((uint32_t)clip8(a3) << 24);
      } else {
        r4 = *reinterpret_cast<const uint32_t*>(t + yy * ts + x);
      }
      const int64_t at = ((int64_t)y * S + x) * 3;
      const Bytes12 in = *reinterpret_cast<const Bytes12*>(frame + at);
      Bytes12 o;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        uint32_t word = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int byte = 4 * d + e;                    // byte of the 12: pixel byte / 3, channel byte % 3
          const int r = (r4 >> (8 * (byte / 3))) & 255u;
          word |= (uint32_t)blend(lutf, frf, r, byte % 3, (in.w[d] >> (8 * e)) & 255u) << (8 * e);
        }
        o.w[d] = word;
      }
      *reinterpret_cast<Bytes12*>(dst + at) = o;
      if (rdst) *reinterpret_cast<uint32_t*>(rdst + (int64_t)y * S + x) = r4;
    }
  } else {                          // one output byte per lane
    const int rb = S * 3;
    for (int i = tid; i < (y1 - y0) * rb; i += TPB) {
      const int yy = i / rb, bx = i - yy * rb, y = y0 + yy;
      const int x = bx / 3, c = bx - 3 * x;
      int r;
      if (need_v) {
        const int32_t* k = rows_v + y * ROW;
        const int r0 = k[0] - lo;
        const int s0 = max(0, -r0), s1 = min(min(k[1], TAPS), rows - r0);
        int acc = 1 << (PREC - 1);
        for (int s = s0; s < s1; ++s) acc += t[(r0 + s) * ts + x] * k[2 + s];
        r = clip8(acc);
      } else {
        r = t[yy * ts + x];
      }
      const int64_t at = (int64_t)y * rb + bx;
      dst[at] = (uint8_t)blend(lutf, frf, r, c, frame[at]);
      if (rdst && c == 0) rdst[(int64_t)y * S + x] = (uint8_t)r;
    }
  }
}

}  // namespace pipnet_heatmap

extern "C" int pipnet_heatmap_rgb8(const float* proto, int B, int h, int w, int P, const uint8_t* frames, int F, int S,
                                   const int32_t* items, int N, const uint8_t* lut, const int32_t* rows_h,
                                   const int32_t* rows_v, float w_heat, float w_img, uint8_t* out, uint8_t* resized,
                                   void* stream) {
  using namespace pipnet_heatmap;
  if (B < 0 || F < 0 || N < 0 || h <= 0 || w <= 0 || P <= 0 || S <= 0) return PIPNET_ERR_ARG;
  if (h > S || w > S) return PIPNET_ERR_ARG;                                   // upscale only: TAPS coefficients
  if ((int64_t)S * S >= ((int64_t)1 << 31) / 4) return PIPNET_ERR_ARG;
  const int sq = (S + 15) & ~15, wq = (w + 15) & ~15;                          // LDS rows, 16-byte multiples
  const int64_t lds = TABLE_BYTES + (int64_t)WIN * (sq + wq);
  if (lds > LDS_LIMIT) return PIPNET_ERR_ARG;
  if (N == 0) return PIPNET_OK;
  if (!proto || !frames || !items || !lut || !rows_h || !rows_v || !out || B == 0 || F == 0) return PIPNET_ERR_ARG;
  const int bands = (S + BAND - 1) / BAND;
  if ((int64_t)N * bands >= ((int64_t)1 << 24)) return PIPNET_ERR_ARG;               // a grid holds < 2^32 threads
  const uintptr_t align = reinterpret_cast<uintptr_t>(frames) | reinterpret_cast<uintptr_t>(out) |
                          reinterpret_cast<uintptr_t>(resized);
  const int vec = S % 4 == 0 && (align & 3u) == 0;
  hipLaunchKernelGGL(heatmap_kernel, dim3((unsigned)((int64_t)N * bands)), dim3(TPB), (size_t)lds,
                     (hipStream_t)stream, proto, B, h, w, P, frames, F, S, items, lut, rows_h, rows_v, w_heat, w_img,
                     out, resized, bands, wq, sq, vec);
  PIPNET_CHECK_LAUNCH();
  return PIPNET_OK;
}
