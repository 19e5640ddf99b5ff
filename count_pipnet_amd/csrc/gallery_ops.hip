// Explanation images on the GPU: the pixel half of util/vis_pipnet.py's prototype grids
// (:298-319, :836-849: crop the patch of every shown entry, torchvision make_grid, crop) and of
// util/visualize_prediction.py:80-88 (the patch and the outlined frame of every kept prototype).
// The frames are the uint8 HWC images pipnet_resize_normalize_rgb8 already writes (Pillow's
// resize, bit for bit), ToTensor -> mul(255).byte() is the identity on uint8, so both halves are
// integer copies:
//   * patch_compose_kernel: one workgroup per item copies a window of a frame to a cell of a
//     canvas (a grid, or a patch slot), rows of 3-byte pixels.  A cell starts at any byte
//     alignment (x * 3 with odd canvas widths), source and destination rows are not aligned
//     alike, and an item is ~3 KB: plain byte loads and stores, consecutive lanes on consecutive
//     bytes of a row.  It clips to the frame (Python slice semantics) and to the canvas;
//   * draw_rects_kernel: one thread per output pixel copies the frame or writes the outline
//     colour, by the rule ImageDraw.rectangle(outline=, width=) follows for boxes at least
//     2 * width + 1 pixels wide and tall (tests/test_gallery_cpu.py holds it against Pillow).
// Every byte offset is 64-bit.
#include "common.hpp"

namespace {

constexpr int ITEM = 8;   // (frame, h0, h1, w0, w1, canvas, y, x)

__global__ __launch_bounds__(256) void patch_compose_kernel(const uint8_t* __restrict__ frames, int F, int fh, int fw,
                                                            const int32_t* __restrict__ items,
                                                            uint8_t* __restrict__ canvases, int C, int ch, int cw) {
  const int32_t* it = items + (int64_t)blockIdx.x * ITEM;
  const int f = it[0], h0 = it[1], w0 = it[3], c = it[5], y = it[6], x = it[7];
  if (f < 0 || f >= F || c < 0 || c >= C || h0 < 0 || w0 < 0 || y < 0 || x < 0) return;
  int rows = min(it[2], fh) - h0, cols = min(it[4], fw) - w0;      // the slice h0:h1, w0:w1 of the frame
  rows = min(rows, ch - y);                                         // and never past the canvas
  cols = min(cols, cw - x);
  if (rows <= 0 || cols <= 0) return;
  const uint8_t* src = frames + (((int64_t)f * fh + h0) * fw + w0) * 3;
  uint8_t* dst = canvases + (((int64_t)c * ch + y) * cw + x) * 3;
  const int rb = cols * 3;                                          // bytes of one row of the window
  const int64_t sstride = (int64_t)fw * 3, dstride = (int64_t)cw * 3;
  const int64_t total = (int64_t)rows * rb;
  for (int64_t i = threadIdx.x; i < total; i += 256) {
    const int r = (int)(i / rb);
    const int b = (int)(i - (int64_t)r * rb);
    dst[r * dstride + b] = src[r * sstride + b];
  }
}

__global__ __launch_bounds__(256) void draw_rects_kernel(const uint8_t* __restrict__ frames, int F, int fh, int fw,
                                                         const int32_t* __restrict__ src,
                                                         const int32_t* __restrict__ rects, int N, int width,
                                                         int cr, int cg, int cb, uint8_t* __restrict__ out) {
  const int64_t plane = (int64_t)fh * fw;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)N * plane) return;
  const int n = (int)(i / plane);
  const int rem = (int)(i - (int64_t)n * plane);
  const int y = rem / fw;
  const int x = rem - y * fw;
  const int f = src[n];
  if (f < 0 || f >= F) return;
  const int x0 = rects[4 * n], y0 = rects[4 * n + 1], x1 = rects[4 * n + 2], y1 = rects[4 * n + 3];
  const bool line = x >= x0 && x <= x1 && y >= y0 && y <= y1 &&
                    (x < x0 + width || x > x1 - width || y < y0 + width || y > y1 - width);
  const uint8_t* p = frames + ((int64_t)f * plane + rem) * 3;
  uint8_t* q = out + i * 3;
  q[0] = line ? (uint8_t)cr : p[0];
  q[1] = line ? (uint8_t)cg : p[1];
  q[2] = line ? (uint8_t)cb : p[2];
}

}  // namespace

extern "C" int pipnet_patch_compose_rgb8(const uint8_t* frames, int F, int fh, int fw, const int32_t* items, int N,
                                         uint8_t* canvases, int C, int ch, int cw, void* stream) {
  if (F < 0 || C < 0 || N < 0 || fh <= 0 || fw <= 0 || ch <= 0 || cw <= 0) return PIPNET_ERR_ARG;
  if ((int64_t)fh * fw >= ((int64_t)1 << 31) / 4 || (int64_t)ch * cw >= ((int64_t)1 << 31) / 4) return PIPNET_ERR_ARG;
  if (N == 0) return PIPNET_OK;
  if (!frames || !items || !canvases || F == 0 || C == 0) return PIPNET_ERR_ARG;
  hipLaunchKernelGGL(patch_compose_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, frames, F, fh, fw,
                     items, canvases, C, ch, cw);
  PIPNET_CHECK_LAUNCH();
  return PIPNET_OK;
}

extern "C" int pipnet_draw_rects_rgb8(const uint8_t* frames, int F, int fh, int fw, const int32_t* src,
                                      const int32_t* rects, int N, int width, int r, int g, int b, uint8_t* out,
                                      void* stream) {
  if (F < 0 || N < 0 || fh <= 0 || fw <= 0 || width < 1 || r < 0 || r > 255 || g < 0 || g > 255 || b < 0 || b > 255)
    return PIPNET_ERR_ARG;
  if ((int64_t)fh * fw >= ((int64_t)1 << 31) / 4) return PIPNET_ERR_ARG;
  if (N == 0) return PIPNET_OK;
  if (!frames || !src || !rects || !out || F == 0) return PIPNET_ERR_ARG;
  const int64_t blocks = ((int64_t)N * fh * fw + 255) / 256;
  if (blocks >= ((int64_t)1 << 31)) return PIPNET_ERR_ARG;
  hipLaunchKernelGGL(draw_rects_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, frames, F, fh, fw,
                     src, rects, N, width, r, g, b, out);
  PIPNET_CHECK_LAUNCH();
  return PIPNET_OK;
}
