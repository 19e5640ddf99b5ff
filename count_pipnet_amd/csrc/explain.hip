// Prototype explanations on gfx950 -- "which patch activates each prototype most", the top-k pass
// of util/vis_pipnet.py:187-275 / :652-755 kept on the device:
//   * pool_argmax   per-patch softmax + spatial max-pool + the LOCATION of the max, proto map
//                   optional (the explain pass of PIP-Net never reads it)
//   * map_argmax    the same location rule on a stored fp32 NHWC map (CountPIPNet's 0/1 Gumbel
//                   map, the bf16 head's fp32 proto map)
//   * topk_update   streaming per-(group, prototype) top-k over the dataset + abstain count
//   * local_explain per image: the top classes and, for each, the prototypes that contribute to it
//                   (util/visualize_prediction.py:63-75, :139-154)
// Location rule = the reference's two-step max (vis_pipnet.py:235-238):
//   max_h, h_idx = torch.max(map, dim=0); max_w, w_idx = torch.max(max_h, dim=0)
// torch.max returns the first index among equal maxima, so of all pixels holding the map's
// maximum the winner is the one with the smallest w, then the smallest h in that column: the
// smallest column-major rank r = w * H + h.  Every comparison below is on (value, rank).
#include <limits.h>

#include "common.hpp"
#include "head_common.hpp"

namespace {

constexpr uint32_t NO_RANK = 0xFFFFFFFFu;

// (value >= 0, rank) as one 64-bit key whose unsigned order is (value ascending, rank descending):
// non-negative floats order like their bit patterns, so the maximum key is the largest value at
// the smallest rank.  Key 0 (a zeroed workspace) is below every real key.
PIPNET_DEV unsigned long long pack_key(float v, uint32_t rank) {
  return ((unsigned long long)__float_as_uint(v) << 32) | (unsigned long long)(NO_RANK - rank);
}

PIPNET_DEV bool better(float v, uint32_t r, float bv, uint32_t br) { return v > bv || (v == bv && r < br); }

// rank w * H + h -> h * W + w; a rank no pixel has (nothing compared greater: NaN maps) -> 0
PIPNET_DEV int32_t rank_to_loc(uint32_t rank, int H, int W) {
  if (rank >= (uint32_t)(H * W)) return 0;
  const int w = (int)(rank / (uint32_t)H);
  const int h = (int)rank - w * H;
  return h * W + w;
}

// softmax_pool_kernel<NJ, 0> (head.hip) -- same grid, same wave-per-pixel loop, the same
// softmax_pixel arithmetic -- that also tracks where each channel's maximum sits.  A lane keeps a
// running (value, rank) per channel; the workgroup's four waves combine through LDS as packed keys
// and the workgroups of an image through one 64-bit atomicMax per channel on key[B, P] (zero on
// entry).  The maximum of a set does not depend on the order it is taken in, so the value half of
// the final key is bit for bit the pooled value of pipnet_softmax_pool_f32.  WRITE: store proto.
template <int NJ, bool WRITE>
__global__ __launch_bounds__(HEAD_THREADS) void pool_argmax_kernel(const float* __restrict__ feat, int H, int W, int P,
                                                                   float* __restrict__ proto,
                                                                   unsigned long long* __restrict__ key) {
  __shared__ unsigned long long red[HEAD_THREADS / 64][NJ * 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int b = blockIdx.y;
  const int HW = H * W;
  const int pix0 = blockIdx.x * PIX_PER_BLOCK;
  float bv[NJ];
  uint32_t br[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    bv[j] = 0.f;          // softmax outputs are >= 0; (0, NO_RANK) packs below every real key
    br[j] = NO_RANK;
  }
  for (int pi = wv; pi < PIX_PER_BLOCK; pi += HEAD_THREADS / 64) {
    const int pix = pix0 + pi;
    if (pix >= HW) break;
    const int h = pix / W;
    const uint32_t rank = (uint32_t)((pix - h * W) * H + h);
    const int64_t base = ((int64_t)b * HW + pix) * P;
    float v[NJ];
    const float inv = softmax_pixel<NJ>(feat, base, P, lane, v);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = lane + 64 * j;
      if (c < P) {
        const float yv = v[j] * inv;
        if constexpr (WRITE) __builtin_nontemporal_store(yv, proto + base + c);   // written once
        if (better(yv, rank, bv[j], br[j])) {
          bv[j] = yv;
          br[j] = rank;
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) red[wv][lane + 64 * j] = pack_key(bv[j], br[j]);
  __syncthreads();
  for (int c = threadIdx.x; c < P; c += HEAD_THREADS) {
    unsigned long long r = red[0][c];
#pragma unroll
    for (int w = 1; w < HEAD_THREADS / 64; ++w) r = red[w][c] > r ? red[w][c] : r;
    atomicMax(key + (int64_t)b * P + c, r);
  }
}

__global__ __launch_bounds__(256) void argmax_unpack_kernel(const unsigned long long* __restrict__ key, int64_t n,
                                                            int H, int W, float* __restrict__ pooled,
                                                            int32_t* __restrict__ loc) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const unsigned long long k = key[i];
    pooled[i] = __uint_as_float((uint32_t)(k >> 32));
    loc[i] = rank_to_loc(NO_RANK - (uint32_t)k, H, W);
  }
}

// Location + value of the maximum of a stored map, any sign: one workgroup owns 64 channels of
// one image and walks all its pixels (wave w the pixels w, w + 4, ...: every load instruction is a
// coalesced 256-B row segment), so the result needs no scratch and no atomics.  NaN entries never
// compare greater and are passed over.
constexpr int MAP_UNROLL = 4;
__global__ __launch_bounds__(HEAD_THREADS) void map_argmax_kernel(const float* __restrict__ map, int H, int W, int P,
                                                                  float* __restrict__ val, int32_t* __restrict__ loc) {
  __shared__ float red_v[HEAD_THREADS / 64][64];
  __shared__ uint32_t red_r[HEAD_THREADS / 64][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int b = blockIdx.y;
  const int c = blockIdx.x * 64 + lane;
  const int HW = H * W;
  float bv = -INFINITY;
  uint32_t br = NO_RANK;
  if (c < P) {
    const float* src = map + (int64_t)b * HW * P + c;
#pragma unroll MAP_UNROLL
    for (int pix = wv; pix < HW; pix += HEAD_THREADS / 64) {
      const float x = src[(int64_t)pix * P];
      const int h = pix / W;
      const uint32_t rank = (uint32_t)((pix - h * W) * H + h);
      if (better(x, rank, bv, br)) {
        bv = x;
        br = rank;
      }
    }
  }
  red_v[wv][lane] = bv;
  red_r[wv][lane] = br;
  __syncthreads();
  if (wv == 0 && c < P) {
#pragma unroll
    for (int w = 1; w < HEAD_THREADS / 64; ++w)
      if (better(red_v[w][lane], red_r[w][lane], bv, br)) {
        bv = red_v[w][lane];
        br = red_r[w][lane];
      }
    val[(int64_t)b * P + c] = bv;
    loc[(int64_t)b * P + c] = rank_to_loc(br, H, W);
  }
}

// Streaming top-k.  One thread owns the k slots of one (group, prototype) and takes the batch's
// images in index order, which is the reference's loop (vis_pipnet.py:248-274, :724-754) verbatim:
// accept when the list is short or the score beats the last entry, then a stable descending sort
// -- the newcomer sits at the end before the sort, so it lands behind every entry of equal score.
// Done here as an insertion from the end that stops at the first entry >= the score.  By
// induction the list is always the k best by (score descending, dataset index ascending).
// Blocks past the (group, prototype) range count the abstained images (amax(out) == 0,
// vis_pipnet.py:217-219) into one device int64; torch.amax propagates NaN, so a row holding a NaN
// is not abstained, whatever else it holds.
struct TopkArgs {
  const float* score;      // [B, P]
  const int32_t* loc;      // [B, P]
  const int32_t* group;    // [B] or null (every image in group 0); an id outside [0, G) skips the image
  const float* out;        // [B, K] logits or null
  float* st_score;         // [G, P, k]
  int64_t* st_index;       // [G, P, k]
  int32_t* st_loc;         // [G, P, k]
  int32_t* st_fill;        // [G, P]
  unsigned long long* abstained;
  int64_t i0;
  int B, P, G, K, k, use_min;
  float min_score;
};

// 64 threads per workgroup: a thread's k slots live in LDS for the call ([slot][thread], 32 KB at
// k = 32) -- read from the state once, updated there, written back once -- and the batch's scores
// are fetched TOPK_CHUNK at a time before they are looked at, so the call costs a few memory round
// trips, not one per image: it sits between two batches' forwards on the caller's stream.  A slot
// filled in this call keeps the image's number in the batch (as -2 - b) in place of its location,
// which is fetched with the others at write-back.  The abstain blocks take TOPK_ROWS images each,
// one wave reading a row of logits 64 columns at a time.
constexpr int TOPK_THREADS = 64;
constexpr int TOPK_MAX_K = PIPNET_TOPK_MAX_K;
constexpr int TOPK_CHUNK = 8;
constexpr int TOPK_ROWS = 8;

__global__ __launch_bounds__(TOPK_THREADS) void topk_update_kernel(TopkArgs a) {
  __shared__ float sS[TOPK_MAX_K][TOPK_THREADS];
  __shared__ int64_t sI[TOPK_MAX_K][TOPK_THREADS];
  __shared__ int32_t sL[TOPK_MAX_K][TOPK_THREADS];
  const int tid = threadIdx.x;
  const int state_blocks = (a.G * a.P + TOPK_THREADS - 1) / TOPK_THREADS;
  if ((int)blockIdx.x >= state_blocks) {
    const int b0 = ((int)blockIdx.x - state_blocks) * TOPK_ROWS;
    int cnt = 0;
#pragma unroll
    for (int r = 0; r < TOPK_ROWS; ++r) {
      const int b = b0 + r;
      float m = -INFINITY;
      bool nan = false;                             // fmaxf drops a NaN, torch.amax keeps it: NaN == 0 is false
      if (b < a.B)
        for (int j = tid; j < a.K; j += TOPK_THREADS) {
          const float x = a.out[(int64_t)b * a.K + j];
          nan |= x != x;
          m = fmaxf(m, x);
        }
      m = wave_max(m);
      cnt += b < a.B && m == 0.f && !__any(nan);
    }
    if (tid == 0 && cnt) atomicAdd(a.abstained, (unsigned long long)cnt);
    return;
  }
  const int t = blockIdx.x * TOPK_THREADS + tid;
  if (t >= a.G * a.P) return;
  const int g = t / a.P, p = t - g * a.P;
  const int k = a.k;
  float* S = a.st_score + (int64_t)t * k;
  int64_t* I = a.st_index + (int64_t)t * k;
  int32_t* L = a.st_loc + (int64_t)t * k;
  int n = a.st_fill[t];
  n = n < 0 ? 0 : (n > k ? k : n);                 // a corrupt fill count must not index past the slots
#pragma unroll 8
  for (int j = 0; j < n; ++j) {
    sS[j][tid] = S[j];
    sI[j][tid] = I[j];
    sL[j][tid] = L[j] < -1 ? -1 : L[j];          // locations are >= 0: nothing stored can pass for a marker
  }
  float last = n > 0 ? sS[n - 1][tid] : 0.f;
  bool changed = false;
  for (int b0 = 0; b0 < a.B; b0 += TOPK_CHUNK) {
    float sc[TOPK_CHUNK];
    int gr[TOPK_CHUNK];
#pragma unroll
    for (int u = 0; u < TOPK_CHUNK; ++u) {
      const int b = b0 + u < a.B ? b0 + u : a.B - 1;         // the tail repeats the last image, skipped below
      sc[u] = a.score[(int64_t)b * a.P + p];
      gr[u] = a.group ? a.group[b] : 0;
    }
#pragma unroll
    for (int u = 0; u < TOPK_CHUNK; ++u) {
      const int b = b0 + u;
      const float s = sc[u];
      if (b >= a.B || gr[u] != g) continue;
      if (a.use_min && s < a.min_score) continue;
      if (n == k && !(s > last)) continue;
      int pos = n < k ? n : k - 1;
      while (pos > 0 && sS[pos - 1][tid] < s) {
        sS[pos][tid] = sS[pos - 1][tid];
        sI[pos][tid] = sI[pos - 1][tid];
        sL[pos][tid] = sL[pos - 1][tid];
        --pos;
      }
      sS[pos][tid] = s;
      sI[pos][tid] = a.i0 + b;
      sL[pos][tid] = -2 - b;
      if (n < k) ++n;
      last = sS[n - 1][tid];
      changed = true;
    }
  }
  if (!changed) return;
#pragma unroll 8
  for (int j = 0; j < n; ++j) {
    const int32_t l = sL[j][tid];
    S[j] = sS[j][tid];
    I[j] = sI[j][tid];
    L[j] = l <= -2 ? a.loc[(int64_t)(-2 - l) * a.P + p] : l;
  }
  a.st_fill[t] = n;
}

}  // namespace

extern "C" int pipnet_softmax_pool_argmax_f32(const float* feat, int B, int H, int W, int P, float* proto,
                                              float* pooled, int32_t* loc, void* workspace, void* stream) {
  if (B < 0 || B > 65535 || H <= 0 || W <= 0 || P <= 0 || (int64_t)H * W > INT_MAX) return PIPNET_ERR_ARG;   // B: grid.y
  const int nj = nj_bucket(P);
  if (nj < 0) return PIPNET_ERR_ARG;
  if (B == 0) return PIPNET_OK;                      // an empty batch: its tensors' data pointers are null
  if (!feat || !pooled || !loc || !workspace) return PIPNET_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(workspace) & 7u) return PIPNET_ERR_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = (int64_t)B * P;
  unsigned long long* key = reinterpret_cast<unsigned long long*>(workspace);
  if (!zero_fill(key, 2 * n, s)) return PIPNET_ERR_LAUNCH;
  const int HW = H * W;
  const dim3 grid((HW + PIX_PER_BLOCK - 1) / PIX_PER_BLOCK, B);
#define PA_CALL(N)                                                                                              \
  if (proto) hipLaunchKernelGGL((pool_argmax_kernel<N, true>), grid, dim3(HEAD_THREADS), 0, s, feat, H, W, P, proto, key); \
  else hipLaunchKernelGGL((pool_argmax_kernel<N, false>), grid, dim3(HEAD_THREADS), 0, s, feat, H, W, P, proto, key);
  PIPNET_NJ_SWITCH(nj, PA_CALL)
#undef PA_CALL
  PIPNET_CHECK_LAUNCH();
  const int64_t blocks = (n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024;
  hipLaunchKernelGGL(argmax_unpack_kernel, dim3((unsigned)blocks), dim3(256), 0, s, key, n, H, W, pooled, loc);
  PIPNET_CHECK_LAUNCH();
  return PIPNET_OK;
}

extern "C" int pipnet_map_argmax_f32(const float* map, int B, int H, int W, int P, float* val, int32_t* loc,
                                     void* stream) {
  if (B < 0 || B > 65535 || H <= 0 || W <= 0 || P <= 0 || (int64_t)H * W > INT_MAX) return PIPNET_ERR_ARG;   // B: grid.y
  if (B == 0) return PIPNET_OK;
  if (!map || !val || !loc) return PIPNET_ERR_ARG;
  hipLaunchKernelGGL(map_argmax_kernel, dim3((P + 63) / 64, B), dim3(HEAD_THREADS), 0, (hipStream_t)stream, map, H, W,
                     P, val, loc);
  PIPNET_CHECK_LAUNCH();
  return PIPNET_OK;
}

extern "C" int pipnet_topk_update(const float* score, const int32_t* loc, int B, int P, int64_t i0,
                                  const int32_t* group, int G, int use_min, float min_score, const float* out, int K,
                                  int k, float* st_score, int64_t* st_index, int32_t* st_loc, int32_t* st_fill,
                                  int64_t* abstained, void* stream) {
  if (B < 0 || P <= 0 || G <= 0 || k < 1 || k > TOPK_MAX_K || (int64_t)G * P > INT_MAX - TOPK_THREADS) return PIPNET_ERR_ARG;
  if (out && (K <= 0 || !abstained)) return PIPNET_ERR_ARG;
  if (B == 0) return PIPNET_OK;                      // an empty batch: score / loc may be null
  if (!score || !loc || !st_score || !st_index || !st_loc || !st_fill) return PIPNET_ERR_ARG;
  TopkArgs a;
  a.score = score;
  a.loc = loc;
  a.group = group;
  a.out = out;
  a.st_score = st_score;
  a.st_index = st_index;
  a.st_loc = st_loc;
  a.st_fill = st_fill;
  a.abstained = reinterpret_cast<unsigned long long*>(abstained);
  a.i0 = i0;
  a.B = B;
  a.P = P;
  a.G = G;
  a.K = K;
  a.k = k;
  a.use_min = use_min != 0;
  a.min_score = min_score;
  const int blocks = (G * P + TOPK_THREADS - 1) / TOPK_THREADS + (out ? (B + TOPK_ROWS - 1) / TOPK_ROWS : 0);
  hipLaunchKernelGGL(topk_update_kernel, dim3(blocks), dim3(TOPK_THREADS), 0, (hipStream_t)stream, a);
  PIPNET_CHECK_LAUNCH();
  return PIPNET_OK;
}

// ---- local explanations (util/visualize_prediction.py:63-75, :139-154) --------------------------
// Per image: classes by logit descending, prototypes by pooled score descending (both with the
// lower index first among equals: a stable descending sort), and for each of the C best classes
// the prototypes p with |pooled[p] * W[c, p]| > min_abs, in prototype order.
namespace {

constexpr int LX_THREADS = 256;
constexpr int LX_MAX = PIPNET_LOCAL_EXPLAIN_MAX;        // prototypes / classes per image: the head's largest nj_bucket

// float -> uint32 whose unsigned order is the float order (-0 made +0 first: equal values must
// share their bits, the index half of the key breaks the tie); order_value is the inverse.
PIPNET_DEV uint32_t order_bits(float v) {
  if (v == 0.f) v = 0.f;
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
PIPNET_DEV float order_value(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o); }

// (value, index) as one key: descending key order = value descending, then index ascending.  No
// real key is 0 (that needs index 0xFFFFFFFF), so 0 pads a sort to a power of two at its end.
PIPNET_DEV unsigned long long order_key(float v, int index) {
  return ((unsigned long long)order_bits(v) << 32) | (unsigned long long)(~(uint32_t)index);
}
PIPNET_DEV int key_index(unsigned long long k) { return (int)(~(uint32_t)k); }

// Descending bitonic sort of key[0, n2) in LDS by the whole workgroup, n2 a power of two.  Keys
// are distinct (apart from the zero pads), so the result is the one total order whatever the
// values: NaN bit patterns sort somewhere and nothing depends on a float comparison.
PIPNET_DEV void sort_desc(unsigned long long* key, int n2) {
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < n2; i += LX_THREADS) {
        const int l = i ^ j;
        if (l > i) {
          const unsigned long long a = key[i], b = key[l];
          if ((i & k) == 0 ? a < b : a > b) {
            key[i] = b;
            key[l] = a;
          }
        }
      }
      __syncthreads();
    }
}

PIPNET_DEV int next_pow2(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

// One workgroup per image.  (1) the prototypes with a non-zero score (a zero score makes a zero
// product, never kept for min_abs >= 0) are compacted into LDS as keys -- wave ballot + prefix
// over the waves' counts, 256 prototypes a round -- and sorted over the next power of two of
// their number, not of P; (2) the K class keys are sorted the same way; (3) one wave per class
// rank walks the sorted active list 64 entries at a time: gather W[c, p], the keep test on the
// fp64 product (exact for two fp32 factors, so the decision is the reference's Python-float one),
// ballot, and store at slot (kept so far + lanes below) while that is < M.  Every output element
// is written here: kept slots, then the (-1, 0, 0, 0, -1) padding.
__global__ __launch_bounds__(LX_THREADS) void local_explain_kernel(
    const float* __restrict__ pooled, const int32_t* __restrict__ loc, const float* __restrict__ out,
    const float* __restrict__ W, int64_t ldw, int P, int K, int C, int M, double min_abs, int32_t* __restrict__ cls,
    float* __restrict__ cls_logit, int32_t* __restrict__ n_out, int32_t* __restrict__ e_proto,
    float* __restrict__ e_sim, float* __restrict__ e_w, float* __restrict__ e_simw, int32_t* __restrict__ e_loc) {
  __shared__ unsigned long long pkey[LX_MAX];
  __shared__ unsigned long long ckey[LX_MAX];
  __shared__ int wave_cnt[LX_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t b = blockIdx.x;
  const float* score = pooled + b * P;
  const float* logit = out + b * K;

  int na = 0;                                         // active prototypes so far (uniform)
  for (int p0 = 0; p0 < P; p0 += LX_THREADS) {
    const int p = p0 + tid;
    const float v = p < P ? score[p] : 0.f;
    const bool active = v != 0.f;                     // NaN is active; its product is never kept
    const unsigned long long mask = __ballot(active);
    if (lane == 0) wave_cnt[wv] = __popcll(mask);
    __syncthreads();
    int base = na, total = 0;
#pragma unroll
    for (int w = 0; w < LX_THREADS / 64; ++w) {
      if (w < wv) base += wave_cnt[w];
      total += wave_cnt[w];
    }
    if (active) pkey[base + __popcll(mask & ((1ull << lane) - 1ull))] = order_key(v, p);
    na += total;
    __syncthreads();                                  // wave_cnt is rewritten next round
  }
  const int na2 = next_pow2(na), k2 = next_pow2(K);
  for (int i = na + tid; i < na2; i += LX_THREADS) pkey[i] = 0ull;
  for (int i = tid; i < k2; i += LX_THREADS) ckey[i] = i < K ? order_key(logit[i], i) : 0ull;
  __syncthreads();
  sort_desc(pkey, na2);
  sort_desc(ckey, k2);

  for (int r = wv; r < C; r += LX_THREADS / 64) {
    const int c = key_index(ckey[r]);
    const float* wrow = W + (int64_t)c * ldw;
    const int64_t row = b * C + r;
    const int64_t e0 = row * M;
    int kept = 0;
    for (int i0 = 0; i0 < na; i0 += 64) {
      const int i = i0 + lane;
      bool keep = false;
      int p = 0;
      float s = 0.f, w = 0.f;
      double sw = 0.0;
      if (i < na) {
        const unsigned long long k = pkey[i];
        p = key_index(k);
        s = order_value((uint32_t)(k >> 32));
        w = wrow[p];
        sw = (double)s * (double)w;
        keep = fabs(sw) > min_abs;
      }
      const unsigned long long mask = __ballot(keep);
      const int slot = kept + __popcll(mask & ((1ull << lane) - 1ull));
      if (keep && slot < M) {
        e_proto[e0 + slot] = p;
        e_sim[e0 + slot] = s;
        e_w[e0 + slot] = w;
        e_simw[e0 + slot] = (float)sw;
        e_loc[e0 + slot] = loc[b * P + p];
      }
      kept += __popcll(mask);
    }
    for (int j = (kept < M ? kept : M) + lane; j < M; j += 64) {
      e_proto[e0 + j] = -1;
      e_sim[e0 + j] = 0.f;
      e_w[e0 + j] = 0.f;
      e_simw[e0 + j] = 0.f;
      e_loc[e0 + j] = -1;
    }
    if (lane == 0) {
      cls[row] = c;
      cls_logit[row] = logit[c];
      n_out[row] = kept;
    }
  }
}

}  // namespace

extern "C" int pipnet_local_explain_f32(const float* pooled, const int32_t* loc, const float* out, const float* W,
                                        int64_t ldw, int B, int P, int K, int C, int M, double min_abs, int32_t* cls,
                                        float* cls_logit, int32_t* n, int32_t* e_proto, float* e_sim, float* e_w,
                                        float* e_simw, int32_t* e_loc, void* stream) {
  if (B < 0 || P < 1 || P > LX_MAX || K < 1 || K > LX_MAX || C < 1 || C > K || M < 1 || ldw < P) return PIPNET_ERR_ARG;
  if (!(min_abs >= 0.0)) return PIPNET_ERR_ARG;      // a NaN threshold as well
  if (!pooled || !loc || !out || !W || !cls || !cls_logit || !n || !e_proto || !e_sim || !e_w || !e_simw || !e_loc)
    return PIPNET_ERR_ARG;
  if (B == 0) return PIPNET_OK;
  hipLaunchKernelGGL(local_explain_kernel, dim3(B), dim3(LX_THREADS), 0, (hipStream_t)stream, pooled, loc, out, W, ldw,
                     P, K, C, M, min_abs, cls, cls_logit, n, e_proto, e_sim, e_w, e_simw, e_loc);
  PIPNET_CHECK_LAUNCH();
  return PIPNET_OK;
}
