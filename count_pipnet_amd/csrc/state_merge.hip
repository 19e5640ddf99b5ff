// Merges of the per-rank states of the dataset passes (prototype top-k, class-conditional
// statistics, part purity) after one all-gather per pass: W states in, one state out, equal to
// the state one process reaches over the whole dataset ("Sharded passes").
//
// Every entry point reads the W states through the pointer to rank 0's field and ONE byte stride
// between consecutive ranks, common to all fields: that is a gathered buffer of W packed states
// (all_gather_into_tensor), field f of rank r at field_f + r * stride.  The output state is
// separate memory.  As in proto_stats.hip / part_purity.hip every output entry has one owner
// thread that reads its W inputs with plain loads, in rank order, and stores once: no atomic, no
// cross-thread sum, so the fp64 sums are the rank-ordered chain ((s_0 + s_1) + s_2) + ... and
// everything else (integer sums, maxima, unsigned minima, the k best of a union) does not depend
// on any order at all.  One launch per merge, nothing waits for the device.
#include <limits.h>
#include <math.h>

#include "common.hpp"

namespace {

constexpr int SM_THREADS = 256;
constexpr int SM_MAX_BLOCKS = 4096;        // grid-stride above it
constexpr int TM_THREADS = 64;
constexpr int TM_MAX_K = PIPNET_TOPK_MAX_K;
constexpr int TM_MAX_W = PIPNET_STATE_MERGE_MAX_RANKS;

template <typename T>
PIPNET_DEV const T* at_rank(const T* p, int r, int64_t stride) {
  return reinterpret_cast<const T*>(reinterpret_cast<const char*>(p) + (int64_t)r * stride);
}

static inline int sm_blocks(int64_t n) {
  const int64_t b = (n + SM_THREADS - 1) / SM_THREADS;
  return (int)(b < 1 ? 1 : (b > SM_MAX_BLOCKS ? SM_MAX_BLOCKS : b));
}

static inline bool stride_ok(int64_t stride, int W) { return W == 1 || (stride > 0 && stride % 8 == 0); }

// ---- top-k: a W-way merge of sorted lists ---------------------------------------------------------
// One thread per (group, prototype).  Each rank's list is sorted by (score descending, dataset
// index ascending) and holds the k best of its block in that order, so the k best of the union are
// the first k of the W-way merge.  The thread keeps one head (score, index), one position and one
// length per rank in LDS ([rank][thread], 14 KB per workgroup, conflict-free) -- held in registers,
// 16 ranks of heads and their addresses spilled to scratch -- and takes, k times, the best head.
struct TmArgs {
  const float* score;      // [W][G, P, k]
  const int64_t* index;
  const int32_t* loc;
  const int32_t* fill;     // [W][G, P]
  const int64_t* abstained;  // [W][1]
  float* o_score;
  int64_t* o_index;
  int32_t* o_loc;
  int32_t* o_fill;
  int64_t* o_abstained;
  int64_t stride;
  int W, GP, k;
};

__global__ __launch_bounds__(TM_THREADS) void topk_merge_kernel(TmArgs a) {
  __shared__ float sS[TM_MAX_W][TM_THREADS];         // head score of rank r, [rank][thread]: 4 KB
  __shared__ int64_t sI[TM_MAX_W][TM_THREADS];       // head dataset index: 8 KB
  __shared__ unsigned char sPos[TM_MAX_W][TM_THREADS], sCnt[TM_MAX_W][TM_THREADS];     // k <= 32 fits a byte
  const int tid = threadIdx.x;
  const int t = blockIdx.x * TM_THREADS + tid;
  if (t == 0) {
    int64_t s = 0;
    for (int r = 0; r < a.W; ++r) s += *at_rank(a.abstained, r, a.stride);
    *a.o_abstained = s;
  }
  if (t >= a.GP) return;                             // no barrier below: a thread only touches its own column
  const int k = a.k;
  const int64_t base = (int64_t)t * k;
  int total = 0;
  for (int r = 0; r < a.W; ++r) {
    int n = at_rank(a.fill, r, a.stride)[t];
    n = n < 0 ? 0 : (n > k ? k : n);                 // a corrupt fill count must not index past the slots
    sCnt[r][tid] = (unsigned char)n;
    sPos[r][tid] = 0;
    total += n;
    if (n > 0) {
      sS[r][tid] = at_rank(a.score, r, a.stride)[base];
      sI[r][tid] = at_rank(a.index, r, a.stride)[base];
    }
  }
  const int fill = total < k ? total : k;
  for (int j = 0; j < fill; ++j) {                   // fill <= total: some rank still has a head
    int best = -1;
    float bs = 0.f;
    int64_t bi = 0;
    for (int r = 0; r < a.W; ++r) {
      if (sPos[r][tid] >= sCnt[r][tid]) continue;
      const float s = sS[r][tid];
      const int64_t i = sI[r][tid];
      if (best < 0 || s > bs || (s == bs && i < bi)) {
        best = r;
        bs = s;
        bi = i;
      }
    }
    if (best < 0) break;                             // cannot happen; never index a rank that is not there
    const int bpos = sPos[best][tid];
    sPos[best][tid] = (unsigned char)(bpos + 1);
    if (bpos + 1 < sCnt[best][tid]) {
      sS[best][tid] = at_rank(a.score, best, a.stride)[base + bpos + 1];
      sI[best][tid] = at_rank(a.index, best, a.stride)[base + bpos + 1];
    }
    a.o_score[base + j] = bs;
    a.o_index[base + j] = bi;
    a.o_loc[base + j] = at_rank(a.loc, best, a.stride)[base + bpos];
  }
  for (int j = fill; j < k; ++j) {
    a.o_score[base + j] = 0.f;
    a.o_index[base + j] = -1;
    a.o_loc[base + j] = -1;
  }
  a.o_fill[t] = fill;
}

// ---- statistics -------------------------------------------------------------------------------------
struct SmArgs {
  const int64_t* n_class;
  const int64_t* n_ge;
  const int64_t* n_gt;
  const double* total;
  const double* total_gt;
  const float* vmax;
  const int32_t* hist;
  const int64_t* bad;
  int64_t* o_n_class;
  int64_t* o_n_ge;
  int64_t* o_n_gt;
  double* o_total;
  double* o_total_gt;
  float* o_vmax;
  int32_t* o_hist;
  int64_t* o_bad;
  int64_t stride, KP, KPNB;
  int W, K;
};

template <typename T>
PIPNET_DEV T rank_sum(const T* p, int64_t i, int W, int64_t stride) {
  T s = at_rank(p, 0, stride)[i];
  for (int r = 1; r < W; ++r) s += at_rank(p, r, stride)[i];      // r = 0 .. W-1: the rank-ordered chain
  return s;
}

__global__ __launch_bounds__(SM_THREADS) void proto_stats_merge_kernel(SmArgs a) {
  const int64_t t0 = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * SM_THREADS;
  const int64_t n = a.KPNB > a.KP ? a.KPNB : a.KP;                // K <= KP: P >= 1
  for (int64_t i = t0; i < n; i += step) {
    if (i < a.KPNB) a.o_hist[i] = rank_sum(a.hist, i, a.W, a.stride);
    if (i < a.KP) {
      a.o_n_ge[i] = rank_sum(a.n_ge, i, a.W, a.stride);
      a.o_n_gt[i] = rank_sum(a.n_gt, i, a.W, a.stride);
      a.o_total[i] = rank_sum(a.total, i, a.W, a.stride);
      a.o_total_gt[i] = rank_sum(a.total_gt, i, a.W, a.stride);
      float m = at_rank(a.vmax, 0, a.stride)[i];
      for (int r = 1; r < a.W; ++r) m = fmaxf(m, at_rank(a.vmax, r, a.stride)[i]);
      a.o_vmax[i] = m;
    }
    if (i < a.K) a.o_n_class[i] = rank_sum(a.n_class, i, a.W, a.stride);
    if (i == 0) *a.o_bad = rank_sum(a.bad, 0, a.W, a.stride);
  }
}

__global__ __launch_bounds__(SM_THREADS) void colsum_merge_f64_kernel(const double* acc, int64_t stride, int W, int D,
                                                                       double* out) {
  const int d = blockIdx.x * SM_THREADS + threadIdx.x;
  if (d < D) out[d] = rank_sum(acc, d, W, stride);
}

// ---- part purity ------------------------------------------------------------------------------------
struct PmArgs {
  const int64_t* n;
  const int64_t* hits;
  const unsigned long long* first_key;
  const int64_t* rows;
  const int64_t* bad;
  int64_t* o_n;
  int64_t* o_hits;
  unsigned long long* o_first_key;
  int64_t* o_rows;
  int64_t* o_bad;
  int64_t stride, PM;
  int W, P;
};

__global__ __launch_bounds__(SM_THREADS) void part_purity_merge_kernel(PmArgs a) {
  const int64_t t0 = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * SM_THREADS;
  for (int64_t i = t0; i < a.PM; i += step) {                     // P <= PM: M >= 1
    a.o_n[i] = rank_sum(a.n, i, a.W, a.stride);
    a.o_hits[i] = rank_sum(a.hits, i, a.W, a.stride);
    unsigned long long key = at_rank(a.first_key, 0, a.stride)[i];
    for (int r = 1; r < a.W; ++r) {
      const unsigned long long other = at_rank(a.first_key, r, a.stride)[i];
      key = other < key ? other : key;                            // unsigned: all ones is "never inserted"
    }
    a.o_first_key[i] = key;
    if (i < a.P) a.o_rows[i] = rank_sum(a.rows, i, a.W, a.stride);
    if (i == 0) *a.o_bad = rank_sum(a.bad, 0, a.W, a.stride);
  }
}

}  // namespace

extern "C" int pipnet_topk_merge(const float* score, const int64_t* index, const int32_t* loc, const int32_t* fill,
                                 const int64_t* abstained, int64_t rank_stride, int W, int G, int P, int k,
                                 float* out_score, int64_t* out_index, int32_t* out_loc, int32_t* out_fill,
                                 int64_t* out_abstained, void* stream) {
  if (W < 1 || W > TM_MAX_W || G < 1 || P < 1 || k < 1 || k > TM_MAX_K) return PIPNET_ERR_ARG;
  if ((int64_t)G * P > INT_MAX - TM_THREADS || !stride_ok(rank_stride, W)) return PIPNET_ERR_ARG;
  if (!score || !index || !loc || !fill || !abstained || !out_score || !out_index || !out_loc || !out_fill ||
      !out_abstained)
    return PIPNET_ERR_ARG;
  TmArgs a;
  a.score = score;
  a.index = index;
  a.loc = loc;
  a.fill = fill;
  a.abstained = abstained;
  a.o_score = out_score;
  a.o_index = out_index;
  a.o_loc = out_loc;
  a.o_fill = out_fill;
  a.o_abstained = out_abstained;
  a.stride = rank_stride;
  a.W = W;
  a.GP = G * P;
  a.k = k;
  hipLaunchKernelGGL(topk_merge_kernel, dim3((a.GP + TM_THREADS - 1) / TM_THREADS), dim3(TM_THREADS), 0,
                     (hipStream_t)stream, a);
  PIPNET_CHECK_LAUNCH();
  return PIPNET_OK;
}

extern "C" int pipnet_proto_stats_merge(const int64_t* n_class, const int64_t* n_ge, const int64_t* n_gt,
                                        const double* total, const double* total_gt, const float* vmax,
                                        const int32_t* hist, const int64_t* bad, int64_t rank_stride, int W, int K,
                                        int P, int NB, int64_t* out_n_class, int64_t* out_n_ge, int64_t* out_n_gt,
                                        double* out_total, double* out_total_gt, float* out_vmax, int32_t* out_hist,
                                        int64_t* out_bad, void* stream) {
  if (W < 1 || W > TM_MAX_W || K < 1 || P < 1 || NB < 0 || NB > PIPNET_PROTO_STATS_MAX_BINS) return PIPNET_ERR_ARG;
  if (!stride_ok(rank_stride, W)) return PIPNET_ERR_ARG;
  if (!n_class || !n_ge || !n_gt || !total || !total_gt || !vmax || !bad) return PIPNET_ERR_ARG;
  if (!out_n_class || !out_n_ge || !out_n_gt || !out_total || !out_total_gt || !out_vmax || !out_bad)
    return PIPNET_ERR_ARG;
  if (NB > 0 && (!hist || !out_hist)) return PIPNET_ERR_ARG;
  SmArgs a;
  a.n_class = n_class;
  a.n_ge = n_ge;
  a.n_gt = n_gt;
  a.total = total;
  a.total_gt = total_gt;
  a.vmax = vmax;
  a.hist = hist;
  a.bad = bad;
  a.o_n_class = out_n_class;
  a.o_n_ge = out_n_ge;
  a.o_n_gt = out_n_gt;
  a.o_total = out_total;
  a.o_total_gt = out_total_gt;
  a.o_vmax = out_vmax;
  a.o_hist = out_hist;
  a.o_bad = out_bad;
  a.stride = rank_stride;
  a.KP = (int64_t)K * P;
  a.KPNB = a.KP * NB;
  a.W = W;
  a.K = K;
  hipLaunchKernelGGL(proto_stats_merge_kernel, dim3(sm_blocks(a.KPNB > a.KP ? a.KPNB : a.KP)), dim3(SM_THREADS), 0,
                     (hipStream_t)stream, a);
  PIPNET_CHECK_LAUNCH();
  return PIPNET_OK;
}

extern "C" int pipnet_colsum_merge_f64(const double* acc, int64_t rank_stride, int W, int D, double* out,
                                       void* stream) {
  if (W < 1 || W > TM_MAX_W || D < 1 || D > INT_MAX - SM_THREADS || !stride_ok(rank_stride, W)) return PIPNET_ERR_ARG;
  if (!acc || !out) return PIPNET_ERR_ARG;
  hipLaunchKernelGGL(colsum_merge_f64_kernel, dim3((D + SM_THREADS - 1) / SM_THREADS), dim3(SM_THREADS), 0,
                     (hipStream_t)stream, acc, rank_stride, W, D, out);
  PIPNET_CHECK_LAUNCH();
  return PIPNET_OK;
}

extern "C" int pipnet_part_purity_merge(const int64_t* n, const int64_t* hits, const uint64_t* first_key,
                                        const int64_t* rows, const int64_t* bad, int64_t rank_stride, int W, int P,
                                        int M, int64_t* out_n, int64_t* out_hits, uint64_t* out_first_key,
                                        int64_t* out_rows, int64_t* out_bad, void* stream) {
  if (W < 1 || W > TM_MAX_W || P < 1 || M < 1 || M > PIPNET_PART_PURITY_MAX_PARTS) return PIPNET_ERR_ARG;
  if (!stride_ok(rank_stride, W)) return PIPNET_ERR_ARG;
  if (!n || !hits || !first_key || !rows || !bad || !out_n || !out_hits || !out_first_key || !out_rows || !out_bad)
    return PIPNET_ERR_ARG;
  PmArgs a;
  a.n = n;
  a.hits = hits;
  a.first_key = reinterpret_cast<const unsigned long long*>(first_key);
  a.rows = rows;
  a.bad = bad;
  a.o_n = out_n;
  a.o_hits = out_hits;
  a.o_first_key = reinterpret_cast<unsigned long long*>(out_first_key);
  a.o_rows = out_rows;
  a.o_bad = out_bad;
  a.stride = rank_stride;
  a.PM = (int64_t)P * M;
  a.W = W;
  a.P = P;
  hipLaunchKernelGGL(part_purity_merge_kernel, dim3(sm_blocks(a.PM)), dim3(SM_THREADS), 0, (hipStream_t)stream, a);
  PIPNET_CHECK_LAUNCH();
  return PIPNET_OK;
}
