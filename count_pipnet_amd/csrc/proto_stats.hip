// Class-conditional prototype activation statistics (util/histograms.py; the dataset statistic
// behind CountPIPNet's virtual weights, pipnet/count_pipnet.py:226-321), streamed on the device.
//
// The reference concatenates every batch's pooled activations on the host and then loops in
// Python over prototypes x classes with boolean masks.  Everything it reports reduces to a few
// counters and sums per (class, prototype); pipnet_proto_stats_update_f32 merges one batch into
// them.  Determinism is the design constraint: every (class k, prototype p) entry of the state
// has ONE owner thread, which walks the batch's images in order, so the counters and both fp64
// sums are accumulated in dataset order whatever the batch size -- no floating-point atomic, no
// cross-thread sum.
//
// Work spreading.  Thread = one prototype column; grid.y partitions the classes (k % parts), so
// a batch of many classes is walked by `parts` workgroups per column block, each skipping the
// images of the other partitions.  Inside a thread the state of the CURRENT class lives in
// registers over a run of equal labels: it is loaded when the run begins and stored when it ends
// (or the batch does), so a long same-class run is a register chain, not a chain of dependent
// global read-modify-writes (an L2 round trip of 200+ cycles each).  The histogram keeps one
// pending (bin, count) pair the same way.  Labels are wave-uniform (one address for all lanes);
// activations and labels are fetched PS_CHUNK images ahead of their use.
// Measured on an MI355X at batch 64 (profiles/proto_stats/proto_stats.txt): the class partitions
// take the kernel from 70 to 25 us at P = 768, K = 200 and from 52 to 25 us at P = 2048, K = 9; a
// no-return integer atomic in place of the histogram's load + store changed nothing (+-3 us).
#include <limits.h>
#include <math.h>

#include "common.hpp"

namespace {

constexpr int PS_THREADS = 64;
constexpr int PS_CHUNK = 8;
#ifndef PS_MAX_PARTS_DEF
#define PS_MAX_PARTS_DEF 16                // -DPS_MAX_PARTS_DEF=1: no class partitions (A/B builds, tools/bench_proto_stats.py)
#endif
constexpr int PS_MAX_PARTS = PS_MAX_PARTS_DEF;
constexpr int PS_TARGET_BLOCKS = 256;      // one workgroup per CU is plenty for [B,P] of a batch

struct PsArgs {
  const float* act;
  const int64_t* labels;
  const float* edges;
  int64_t* n_class;
  int64_t* n_ge;
  int64_t* n_gt;
  double* total;
  double* total_gt;
  float* vmax;
  int32_t* hist;
  unsigned long long* bad;
  int64_t lda;
  int B, P, K, NB;
  float thr;
};

// Bin of v among the ascending edges e[0..nb]: the largest i < nb with e[i] <= v (so v == e[nb]
// lands in the last bin), or -1 outside [e[0], e[nb]] and for NaN.
PIPNET_DEV int ps_bin(const float* e, int nb, float v) {
  if (!(v >= e[0] && v <= e[nb])) return -1;
  int lo = 0, hi = nb;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (e[mid] <= v) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(PS_THREADS) void proto_stats_update_kernel(PsArgs a) {
  __shared__ float s_edges[PIPNET_PROTO_STATS_MAX_BINS + 1];
  const int tid = threadIdx.x;
  const int part = blockIdx.y, parts = gridDim.y;
  const int NB = a.NB;
  if (blockIdx.x == gridDim.x - 1) {
    // the counting workgroup of this class partition: n_class (one owner thread per class) and,
    // in partition 0, the labels outside [0, K)
    for (int k = part + parts * tid; k < a.K; k += parts * PS_THREADS) {
      int64_t c = 0;
      for (int b = 0; b < a.B; ++b) c += a.labels[b] == (int64_t)k;
      if (c) a.n_class[k] += c;
    }
    if (part == 0) {
      unsigned long long c = 0;
      for (int b = tid; b < a.B; b += PS_THREADS) c += a.labels[b] < 0 || a.labels[b] >= (int64_t)a.K;
      if (c) atomicAdd(a.bad, c);         // an integer count: exact in any order
    }
    return;
  }
  for (int i = tid; i <= NB && NB > 0; i += PS_THREADS) s_edges[i] = a.edges[i];
  __syncthreads();
  const int p = blockIdx.x * PS_THREADS + tid;
  if (p >= a.P) return;

  int cur = -1;                           // class whose (cur, p) state is held in registers
  int64_t nge = 0, ngt = 0;
  double tot = 0.0, totgt = 0.0;
  float vmx = -INFINITY;
  int hbin = -1, hcnt = 0;                // pending histogram increments of (cur, p)
  int64_t at = 0;                         // cur * P + p

  auto flush_hist = [&]() {
    if (hcnt) a.hist[at * NB + hbin] += hcnt;
    hcnt = 0;
    hbin = -1;
  };
  auto flush = [&]() {
    if (cur < 0) return;
    flush_hist();
    a.n_ge[at] = nge;
    a.n_gt[at] = ngt;
    a.total[at] = tot;
    a.total_gt[at] = totgt;
    a.vmax[at] = vmx;
  };

  for (int b0 = 0; b0 < a.B; b0 += PS_CHUNK) {
    float v[PS_CHUNK];
    int kk[PS_CHUNK];
#pragma unroll
    for (int u = 0; u < PS_CHUNK; ++u) {
      const int b = b0 + u < a.B ? b0 + u : a.B - 1;           // the tail repeats the last image, skipped below
      v[u] = a.act[(int64_t)b * a.lda + p];
      const int64_t l = a.labels[b];
      const bool mine = b0 + u < a.B && l >= 0 && l < (int64_t)a.K && (unsigned)l % (unsigned)parts == (unsigned)part;
      kk[u] = mine ? (int)l : -1;
    }
#pragma unroll
    for (int u = 0; u < PS_CHUNK; ++u) {
      const int k = kk[u];
      if (k < 0) continue;                // another partition's class, a bad label, or the tail
      if (k != cur) {
        flush();
        cur = k;
        at = (int64_t)k * a.P + p;
        nge = a.n_ge[at];
        ngt = a.n_gt[at];
        tot = a.total[at];
        totgt = a.total_gt[at];
        vmx = a.vmax[at];
      }
      const float x = v[u];
      nge += x >= a.thr;
      tot += (double)x;
      vmx = fmaxf(vmx, x);
      if (x > a.thr) {
        ++ngt;
        totgt += (double)x;
        if (NB > 0) {
          const int bin = ps_bin(s_edges, NB, x);
          if (bin >= 0) {
            if (bin != hbin) {
              flush_hist();
              hbin = bin;
            }
            ++hcnt;
          }
        }
      }
    }
  }
  flush();
}

__global__ __launch_bounds__(PS_THREADS) void colsum_accum_f64_kernel(const float* __restrict__ x, int64_t ldx, int B,
                                                                       int D, double* __restrict__ acc) {
  const int d = blockIdx.x * PS_THREADS + threadIdx.x;
  if (d >= D) return;
  double s = acc[d];
  for (int b0 = 0; b0 < B; b0 += PS_CHUNK) {
    float v[PS_CHUNK];
#pragma unroll
    for (int u = 0; u < PS_CHUNK; ++u) v[u] = x[(int64_t)(b0 + u < B ? b0 + u : B - 1) * ldx + d];
#pragma unroll
    for (int u = 0; u < PS_CHUNK; ++u)
      if (b0 + u < B) s += (double)v[u];  // image order: one chain of fp64 adds
  }
  acc[d] = s;
}

}  // namespace

extern "C" int pipnet_proto_stats_update_f32(const float* act, int64_t lda, const int64_t* labels, int B, int P, int K,
                                             float thr, const float* edges, int NB, int64_t* n_class, int64_t* n_ge,
                                             int64_t* n_gt, double* total, double* total_gt, float* vmax, int32_t* hist,
                                             int64_t* bad, void* stream) {
  if (B < 1 || P < 1 || K < 1 || lda < (int64_t)P || NB < 0 || NB > PIPNET_PROTO_STATS_MAX_BINS) return PIPNET_ERR_ARG;
  if (P > INT_MAX - PS_THREADS) return PIPNET_ERR_ARG;
  if (!act || !labels || !n_class || !n_ge || !n_gt || !total || !total_gt || !vmax || !bad) return PIPNET_ERR_ARG;
  if (NB > 0 && (!edges || !hist)) return PIPNET_ERR_ARG;
  PsArgs a;
  a.act = act;
  a.labels = labels;
  a.edges = edges;
  a.n_class = n_class;
  a.n_ge = n_ge;
  a.n_gt = n_gt;
  a.total = total;
  a.total_gt = total_gt;
  a.vmax = vmax;
  a.hist = hist;
  a.bad = reinterpret_cast<unsigned long long*>(bad);
  a.lda = lda;
  a.B = B;
  a.P = P;
  a.K = K;
  a.NB = NB;
  a.thr = thr;
  // class partitions: enough workgroups for about one per CU, never more partitions than classes
  // (the result does not depend on the number: ownership and image order hold for any)
  const int colblocks = (P + PS_THREADS - 1) / PS_THREADS;
  int parts = PS_TARGET_BLOCKS / colblocks;
  parts = parts < 1 ? 1 : (parts > PS_MAX_PARTS ? PS_MAX_PARTS : parts);
  parts = parts > K ? K : parts;
  hipLaunchKernelGGL(proto_stats_update_kernel, dim3(colblocks + 1, parts), dim3(PS_THREADS), 0, (hipStream_t)stream, a);
  PIPNET_CHECK_LAUNCH();
  return PIPNET_OK;
}

extern "C" int pipnet_colsum_accum_f64(const float* x, int64_t ldx, int B, int D, double* acc, void* stream) {
  if (B < 1 || D < 1 || ldx < (int64_t)D || D > INT_MAX - PS_THREADS) return PIPNET_ERR_ARG;
  if (!x || !acc) return PIPNET_ERR_ARG;
  hipLaunchKernelGGL(colsum_accum_f64_kernel, dim3((D + PS_THREADS - 1) / PS_THREADS), dim3(PS_THREADS), 0,
                     (hipStream_t)stream, x, ldx, B, D, acc);
  PIPNET_CHECK_LAUNCH();
  return PIPNET_OK;
}
