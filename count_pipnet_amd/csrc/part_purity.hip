// Prototype part purity (util/eval_cub_csv.py), streamed on the device.
//
// The reference writes one CSV row per (prototype, image) from batch-1 forwards, then re-reads the
// CSV, opens every image for its size and loops over nested dicts.  Everything it reports reduces,
// per (prototype p, merged part m), to three integers: n (rows in which a member of m is visible),
// hits (those rows in which a visible member lies in the patch) and first_key (row ordinal and
// slot at which the dict key of m was inserted: the dict's iteration order decides the ties).
//
// Determinism, as in proto_stats.hip: every prototype's [p, :] state has ONE owner thread, which
// walks the batch's images (or the top-k slots) in order with plain loads and stores.  The state
// is integer, so it is exact, and it is bitwise independent of how the dataset is cut into
// batches; no atomic touches it (the `bad` counter is an integer atomic: exact in any order).
//
// Update kernel.  Thread = one prototype column, so pooled / loc reads are coalesced.  Firing is
// sparse (pooled > threshold on a relevant prototype), and the state is touched only by threads
// that fire: at its first row of the call a thread fetches its [M] state into its LDS column
// (3 M independent loads: one round trip), every row then updates LDS, and the column is written
// back once at the end.  Updating global memory row by row instead is a chain of dependent L2
// round trips (three per visible part) on the slowest lane of each wave: 318 us per batch of
// 64 x 768 at 2 % firing against 238 us (profiles/part_purity/part_purity.txt).  An image's
// annotations are the same for the whole workgroup: a chunk of PP_CHUNK images is staged in LDS,
// and only when some thread of the workgroup fires in that chunk (a workgroup-uniform vote), so a
// chunk with no row costs its pooled / loc loads only (19 us for the whole batch).
// What is left is the row function itself: a wave runs it once for every image on which any of
// its 64 lanes fires (at 2 % that is nearly every image), and one run is a serial walk over the
// parts with dependent LDS reads, about 3.7 us, on one wave per workgroup.
#include <limits.h>
#include <math.h>

#include "common.hpp"
#include "part_purity_row.hpp"

namespace {

constexpr int PP_THREADS = 64;
constexpr int PP_CHUNK = 8;
constexpr int PP_MAXQ = PIPNET_PART_PURITY_MAX_PARTS;
static_assert(2 * PP_MAXQ <= (1 << PP_KEY_SLOT_BITS), "a slot must fit the key's low bits");
static_assert(PP_MAXQ <= 32, "the row function keeps the merged parts of a row in 32-bit masks");

struct PpTable {
  const double* xy;                        // [N,Q,2]
  const uint8_t* vis;                      // [N,Q]
  const int32_t* size;                     // [N,2] width, height
  int64_t N;
};

struct PpState {
  int64_t* n;                              // [P,M]
  int64_t* hits;                           // [P,M]
  unsigned long long* first_key;           // [P,M]
  int64_t* rows;                           // [P]
  unsigned long long* bad;                 // [1]
};

struct PpUpdateArgs {
  const float* pooled;
  const int32_t* loc;
  const uint8_t* relevant;
  int64_t lda, i0;
  double threshold;
  int B, P;
  PpGeom g;
  PpFold f;
  PpTable t;
  PpState s;
};

__global__ __launch_bounds__(PP_THREADS) void part_purity_update_kernel(PpUpdateArgs a) {
  __shared__ double s_xy[PP_CHUNK][PP_MAXQ * 2];
  __shared__ uint8_t s_vis[PP_CHUNK][PP_MAXQ];
  __shared__ int s_wh[PP_CHUNK][2];
  __shared__ int s_merged[PP_MAXQ], s_pair[PP_MAXQ];
  __shared__ uint8_t s_left[PP_MAXQ];
  __shared__ int64_t s_n[PP_MAXQ][PP_THREADS], s_hits[PP_MAXQ][PP_THREADS];      // [m][thread]: no bank conflict
  __shared__ unsigned long long s_key[PP_MAXQ][PP_THREADS];
  const int tid = threadIdx.x;
  const int Q = a.f.Q;
  if (blockIdx.x == 0) {                   // dataset indices outside the table: counted once per batch
    unsigned long long c = 0;
    for (int b = tid; b < a.B; b += PP_THREADS) c += a.i0 + b < 0 || a.i0 + b >= a.t.N;
    if (c) atomicAdd(a.s.bad, c);
  }
  for (int q = tid; q < Q; q += PP_THREADS) {
    s_merged[q] = a.f.merged[q];
    s_pair[q] = a.f.pair_index[q];
    s_left[q] = a.f.is_left[q];
  }
  PpFold f = a.f;
  f.merged = s_merged;
  f.pair_index = s_pair;
  f.is_left = s_left;
  const int p = blockIdx.x * PP_THREADS + tid;
  const bool active = p < a.P && a.relevant[p < a.P ? p : 0] != 0;
  const int pc = p < a.P ? p : a.P - 1;    // idle lanes read the last column, and vote
  int64_t* n = a.s.n + (int64_t)pc * f.M;
  int64_t* hits = a.s.hits + (int64_t)pc * f.M;
  unsigned long long* key = a.s.first_key + (int64_t)pc * f.M;
  int64_t nrows = 0;
  bool loaded = false;                     // this thread's state column is in LDS

  for (int b0 = 0; b0 < a.B; b0 += PP_CHUNK) {
    float v[PP_CHUNK];
    int l[PP_CHUNK];
    unsigned fire = 0;
#pragma unroll
    for (int u = 0; u < PP_CHUNK; ++u) {
      const int b = b0 + u < a.B ? b0 + u : a.B - 1;           // the tail repeats the last image, masked below
      v[u] = a.pooled[(int64_t)b * a.lda + pc];
      l[u] = a.loc[(int64_t)b * a.P + pc];
    }
#pragma unroll
    for (int u = 0; u < PP_CHUNK; ++u) {
      const int64_t i = a.i0 + b0 + u;
      const bool ok = active && b0 + u < a.B && i >= 0 && i < a.t.N && (double)v[u] > a.threshold;
      fire |= ok ? 1u << u : 0u;
    }
    if (!__syncthreads_or(fire != 0)) continue;                // workgroup-uniform: nobody fires in this chunk
    for (int e = tid; e < PP_CHUNK * Q; e += PP_THREADS) {
      const int u = e / Q, q = e - u * Q;
      const int64_t i = a.i0 + b0 + u;
      const bool in = b0 + u < a.B && i >= 0 && i < a.t.N;
      s_xy[u][2 * q] = in ? a.t.xy[(i * Q + q) * 2] : 0.0;
      s_xy[u][2 * q + 1] = in ? a.t.xy[(i * Q + q) * 2 + 1] : 0.0;
      s_vis[u][q] = in ? a.t.vis[i * Q + q] : 0;
      if (q == 0) {
        s_wh[u][0] = in ? a.t.size[2 * i] : 0;
        s_wh[u][1] = in ? a.t.size[2 * i + 1] : 0;
      }
    }
    if (fire && !loaded) {
      for (int m = 0; m < f.M; ++m) {
        s_n[m][tid] = n[m];
        s_hits[m][tid] = hits[m];
        s_key[m][tid] = key[m];
      }
      loaded = true;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < PP_CHUNK; ++u) {
      if (!(fire >> u & 1u)) continue;
      ++nrows;
      pp_row(a.g, f, s_xy[u], s_vis[u], s_wh[u][0], s_wh[u][1], l[u], (uint64_t)(a.i0 + b0 + u), &s_n[0][tid],
             &s_hits[0][tid], reinterpret_cast<uint64_t*>(&s_key[0][tid]), PP_THREADS);
    }
    __syncthreads();                                           // the staging buffers are rewritten next chunk
  }
  if (!loaded) return;                                         // after the last barrier
  for (int m = 0; m < f.M; ++m) {
    n[m] = s_n[m][tid];
    hits[m] = s_hits[m][tid];
    key[m] = s_key[m][tid];
  }
  a.s.rows[pc] += nrows;
}

struct PpRowsArgs {
  const int64_t* index;                    // [P,k]
  const int32_t* loc;                      // [P,k]
  const uint8_t* relevant;
  int P, k;
  PpGeom g;
  PpFold f;
  PpTable t;
  PpState s;
};

__global__ __launch_bounds__(PP_THREADS) void part_purity_rows_kernel(PpRowsArgs a) {
  const int p = blockIdx.x * PP_THREADS + threadIdx.x;
  if (p >= a.P || !a.relevant[p]) return;
  const int Q = a.f.Q, M = a.f.M;
  int64_t nrows = 0;
  unsigned long long nbad = 0;
  for (int j = 0; j < a.k; ++j) {          // slot order = row order
    const int64_t i = a.index[(int64_t)p * a.k + j];
    if (i < 0) continue;                   // an empty slot
    if (i >= a.t.N) {
      ++nbad;
      continue;
    }
    ++nrows;
    pp_row(a.g, a.f, a.t.xy + i * Q * 2, a.t.vis + i * Q, a.t.size[2 * i], a.t.size[2 * i + 1],
           a.loc[(int64_t)p * a.k + j], (uint64_t)j, a.s.n + (int64_t)p * M, a.s.hits + (int64_t)p * M,
           reinterpret_cast<uint64_t*>(a.s.first_key) + (int64_t)p * M);
  }
  if (nrows) a.s.rows[p] += nrows;
  if (nbad) atomicAdd(a.s.bad, nbad);
}

struct PpFinishArgs {
  const int64_t* n;
  const int64_t* hits;
  const unsigned long long* first_key;
  const int64_t* rows;
  int P, M;
  uint8_t* in_csv;
  double* max_purity;
  int32_t* max_part;
  int64_t* max_sum;
  int32_t* most_part;
  int64_t* most_sum;
  double* most_purity;
  double* purity;                          // [P,M]
};

// The per-prototype loop of eval_cub_csv.py:131-165 over the parts in dict order = ascending
// first_key (a repeated-minimum walk: M <= 32).
__global__ __launch_bounds__(PP_THREADS) void part_purity_finish_kernel(PpFinishArgs a) {
  const int p = blockIdx.x * PP_THREADS + threadIdx.x;
  if (p >= a.P) return;
  const int M = a.M;
  const int64_t* n = a.n + (int64_t)p * M;
  const int64_t* hits = a.hits + (int64_t)p * M;
  const unsigned long long* key = a.first_key + (int64_t)p * M;
  for (int m = 0; m < M; ++m) a.purity[(int64_t)p * M + m] = n[m] > 0 ? (double)hits[m] / (double)n[m] : (double)NAN;
  double max_purity = 0.0, most_purity = 0.0;
  int max_part = -1, most_part = -1;
  int64_t max_sum = 0, most_sum = 0;
  unsigned long long prev = 0;
  bool first = true;
  for (int step = 0; step < M; ++step) {
    int best = -1;
    unsigned long long bk = PP_NO_KEY;
    for (int m = 0; m < M; ++m) {
      const unsigned long long k = key[m];
      if (k == PP_NO_KEY || n[m] <= 0) continue;
      if (!first && k <= prev) continue;   // keys are distinct: (ordinal, slot) names one insertion
      if (k < bk) {
        bk = k;
        best = m;
      }
    }
    if (best < 0) break;
    prev = bk;
    first = false;
    const double pur = (double)hits[best] / (double)n[best];
    const int64_t s = hits[best];
    if (pur > max_purity) {
      max_purity = pur, max_part = best, max_sum = s;
    } else if (pur == max_purity) {
      if (pur == 0.0 || s > max_sum) max_purity = pur, max_part = best, max_sum = s;
    }
    if (s > most_sum) most_part = best, most_sum = s, most_purity = pur;
  }
  a.in_csv[p] = a.rows[p] > 0;
  a.max_purity[p] = max_purity;
  a.max_part[p] = max_part;
  a.max_sum[p] = max_sum;
  a.most_part[p] = most_part;
  a.most_sum[p] = most_sum;
  a.most_purity[p] = most_purity;
}

bool pp_geometry_ok(int H, int W, int image_size, int skip) {
  return H >= 1 && W >= 1 && image_size >= PP_PATCH && skip >= 0 && (int64_t)H * W <= INT_MAX &&
         (int64_t)(H > W ? H : W) * skip <= INT_MAX - PP_PATCH - 4;
}

bool pp_table_ok(const double* xy, const uint8_t* vis, const int32_t* size, int64_t N, const int32_t* merged,
                 const uint8_t* is_left, const int32_t* pair_index, int Q, int M) {
  return xy && vis && size && merged && is_left && pair_index && N >= 1 && Q >= 1 && Q <= PP_MAXQ && M >= 1 && M <= Q;
}

}  // namespace

extern "C" int pipnet_part_purity_update(const float* pooled, int64_t lda, const int32_t* loc, const uint8_t* relevant,
                                         int B, int P, int64_t i0, double threshold, int H, int W, int image_size,
                                         int skip, int small_map, const double* xy, const uint8_t* vis,
                                         const int32_t* size, int64_t N, const int32_t* merged, const uint8_t* is_left,
                                         const int32_t* pair_index, int Q, int M, int64_t* n, int64_t* hits,
                                         uint64_t* first_key, int64_t* rows, int64_t* bad, void* stream) {
  if (B < 1 || P < 1 || lda < (int64_t)P || (int64_t)B * P > INT_MAX || P > INT_MAX - PP_THREADS) return PIPNET_ERR_ARG;
  if (!pooled || !loc || !relevant || !n || !hits || !first_key || !rows || !bad) return PIPNET_ERR_ARG;
  if (!pp_geometry_ok(H, W, image_size, skip)) return PIPNET_ERR_ARG;
  if (!pp_table_ok(xy, vis, size, N, merged, is_left, pair_index, Q, M)) return PIPNET_ERR_ARG;
  PpUpdateArgs a;
  a.pooled = pooled;
  a.loc = loc;
  a.relevant = relevant;
  a.lda = lda;
  a.i0 = i0;
  a.threshold = threshold;
  a.B = B;
  a.P = P;
  a.g = PpGeom{H, W, image_size, skip, small_map != 0};
  a.f = PpFold{merged, is_left, pair_index, Q, M};
  a.t = PpTable{xy, vis, size, N};
  a.s = PpState{n, hits, reinterpret_cast<unsigned long long*>(first_key), rows,
                reinterpret_cast<unsigned long long*>(bad)};
  hipLaunchKernelGGL(part_purity_update_kernel, dim3((P + PP_THREADS - 1) / PP_THREADS), dim3(PP_THREADS), 0,
                     (hipStream_t)stream, a);
  PIPNET_CHECK_LAUNCH();
  return PIPNET_OK;
}

extern "C" int pipnet_part_purity_rows(const int64_t* index, const int32_t* loc, const uint8_t* relevant, int P, int k,
                                       int H, int W, int image_size, int skip, int small_map, const double* xy,
                                       const uint8_t* vis, const int32_t* size, int64_t N, const int32_t* merged,
                                       const uint8_t* is_left, const int32_t* pair_index, int Q, int M, int64_t* n,
                                       int64_t* hits, uint64_t* first_key, int64_t* rows, int64_t* bad, void* stream) {
  if (P < 1 || k < 1 || k > 32 || P > INT_MAX - PP_THREADS) return PIPNET_ERR_ARG;
  if (!index || !loc || !relevant || !n || !hits || !first_key || !rows || !bad) return PIPNET_ERR_ARG;
  if (!pp_geometry_ok(H, W, image_size, skip)) return PIPNET_ERR_ARG;
  if (!pp_table_ok(xy, vis, size, N, merged, is_left, pair_index, Q, M)) return PIPNET_ERR_ARG;
  PpRowsArgs a;
  a.index = index;
  a.loc = loc;
  a.relevant = relevant;
  a.P = P;
  a.k = k;
  a.g = PpGeom{H, W, image_size, skip, small_map != 0};
  a.f = PpFold{merged, is_left, pair_index, Q, M};
  a.t = PpTable{xy, vis, size, N};
  a.s = PpState{n, hits, reinterpret_cast<unsigned long long*>(first_key), rows,
                reinterpret_cast<unsigned long long*>(bad)};
  hipLaunchKernelGGL(part_purity_rows_kernel, dim3((P + PP_THREADS - 1) / PP_THREADS), dim3(PP_THREADS), 0,
                     (hipStream_t)stream, a);
  PIPNET_CHECK_LAUNCH();
  return PIPNET_OK;
}

extern "C" int pipnet_part_purity_finish(const int64_t* n, const int64_t* hits, const uint64_t* first_key,
                                         const int64_t* rows, int P, int M, uint8_t* in_csv, double* max_purity,
                                         int32_t* max_part, int64_t* max_sum, int32_t* most_part, int64_t* most_sum,
                                         double* most_purity, double* purity, void* stream) {
  if (P < 1 || M < 1 || M > PP_MAXQ || P > INT_MAX - PP_THREADS) return PIPNET_ERR_ARG;
  if (!n || !hits || !first_key || !rows || !in_csv || !max_purity || !max_part || !max_sum || !most_part ||
      !most_sum || !most_purity || !purity)
    return PIPNET_ERR_ARG;
  PpFinishArgs a;
  a.n = n;
  a.hits = hits;
  a.first_key = reinterpret_cast<const unsigned long long*>(first_key);
  a.rows = rows;
  a.P = P;
  a.M = M;
  a.in_csv = in_csv;
  a.max_purity = max_purity;
  a.max_part = max_part;
  a.max_sum = max_sum;
  a.most_part = most_part;
  a.most_sum = most_sum;
  a.most_purity = most_purity;
  a.purity = purity;
  hipLaunchKernelGGL(part_purity_finish_kernel, dim3((P + PP_THREADS - 1) / PP_THREADS), dim3(PP_THREADS), 0,
                     (hipStream_t)stream, a);
  PIPNET_CHECK_LAUNCH();
  return PIPNET_OK;
}
