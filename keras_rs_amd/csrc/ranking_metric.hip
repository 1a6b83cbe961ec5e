// K10 -- ranking metrics: DCG, NDCG, MAP, MRR, P@k and R@k of keras_rs.metrics from one sort of each list.
//
// Replaces RankingMetric.update_state (ranking_metric.py:159-209), sort_by_scores / get_list_weights / compute_dcg
// (ranking_metrics_utils.py) and the six compute_metric methods.  The reference sorts once per metric (twice for
// NDCG) through argsort + take_along_axis + top_k + gathers, each a launch with a [batch, list] intermediate; here a
// list is sorted once in LDS and every requested metric is a sum (or max) over its sorted items.
//
//   * ranking_metric_kernel    stage A.  Builds one 64-bit key per item,
//                                key = hi32 << 32 | r20 << 12 | (4095 - index),
//                                hi32 = order_key(score) for a valid item, 1 for an invalid one (order_key of a real
//                                value is >= 0x007fffff), r20 = the top 20 bits of tie_hash(seed, draw, row, index)
//                                when ties are shuffled and 0 otherwise; padding slots carry key 0.  A descending
//                                bitonic sort of the keys in LDS is the rank order.  Labels and weights stay in LDS
//                                in item order and are fetched through the index in the key.  NDCG's ideal DCG sorts
//                                the same list a second time on order_key(w * gain).
//   * metric_accumulate_kernel stage B: per-list weights (get_list_weights), the batch-wide default weight, DCG's
//                                division by its weight, and the Mean update of every metric's {total, count};
//                                advances the draw counter.  One workgroup up to 1024 lists; above, the same sums
//                                over several workgroups in three launches (metric_*_partials_kernel,
//                                metric_state_update_kernel).
//
// Packing, sort, reductions and the scan are krs_list.h's.  Sums run in a fixed order (a thread's items in rank
// order, then seg_all_reduce's butterflies): no atomics, bit-identical from call to call.  Nothing waits for the host.
#include "krs_list.h"

namespace krs {
namespace {

constexpr int kThreads = kListThreads;
constexpr int kMaxList = KRS_RANK_MAX_LIST;
constexpr int kMaxSpecs = KRS_METRIC_MAX_SPECS;
constexpr int kEpt = kMaxList / kThreads;   // sorted positions per thread, at most
constexpr int kWaves = kListWaves;
// reduction slots of stage A: one per spec, then sum w gain, sum gain, sum w rel, sum rel, sum w, number of valid items
constexpr int kSumWG = kMaxSpecs, kSumG = kMaxSpecs + 1, kSumWR = kMaxSpecs + 2, kSumR = kMaxSpecs + 3,
              kSumW = kMaxSpecs + 4, kNValid = kMaxSpecs + 5, kSlots = kMaxSpecs + 6;
static_assert(kMaxList == 4096, "the key keeps the item index in 12 bits");

struct Specs {
  int n;
  int kind[kMaxSpecs];
  int k[kMaxSpecs];   // min(k, L)
};
struct States {
  float* p[kMaxSpecs];
};

__device__ __forceinline__ bool is_dcg_kind(int kind) { return kind == KRS_METRIC_DCG || kind == KRS_METRIC_NDCG; }
__device__ __forceinline__ float divide_no_nan(float a, float b) { return b == 0.0f ? 0.0f : a / b; }

// the finalizer of splitmix64 (Steele, Lea, Flood 2014; Vigna's public-domain constants)
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// counter-based tie hash: salt = mix64(seed ^ mix64(draw + 0x9E3779B97F4A7C15)), hash = mix64(salt + (row << 12 | index))
__device__ __forceinline__ uint64_t tie_salt(uint64_t seed, uint64_t draw) {
  return mix64(seed ^ mix64(draw + 0x9E3779B97F4A7C15ull));
}
__device__ __forceinline__ uint32_t tie_r20(uint64_t salt, int64_t row, int index) {
  return (uint32_t)(mix64(salt + (((uint64_t)row << 12) | (uint64_t)index)) >> 44);
}

__device__ __forceinline__ float rank_discount(const float* __restrict__ discount, int discount_len, int r1) {
  if (discount) return r1 <= discount_len ? discount[r1 - 1] : 0.0f;
  return 1.0f / log2f(1.0f + (float)r1);
}

template <typename T>
__global__ __launch_bounds__(kThreads, 8) void ranking_metric_kernel(
    const T* __restrict__ scores, int64_t ld, const float* __restrict__ labels, const uint8_t* __restrict__ mask,
    const float* __restrict__ weights, int64_t w_row_stride, int64_t w_item_stride, float weight,
    const float* __restrict__ gain, const float* __restrict__ discount, int discount_len, int shuffle, uint64_t seed,
    const int64_t* __restrict__ draw, Specs sp, int64_t batch, int L,
    float* __restrict__ values, float* __restrict__ sums, int32_t* __restrict__ order) {
  __shared__ uint64_t keys[kMaxList];
  __shared__ float ys[kMaxList];      // label in item order, 0 for an invalid item
  __shared__ float ws[kMaxList];      // weight in item order, 0 for an invalid item
  __shared__ float red[kSlots][kWaves];
  __shared__ int ibuf[kWaves];
  const ListPack lp(L);
  const int P = lp.P, tpl = lp.tpl, ept = lp.ept;
  const int lgP = __ffs(P) - 1;
  const int64_t row0 = lp.row0();
  const int n_slots = lp.n_slots();
  const uint64_t salt = shuffle ? tie_salt(seed, draw ? (uint64_t)*draw : 0ull) : 0ull;

  bool need_map = false, need_dcg = false, need_ndcg = false;
  unsigned max_mask = 0;
#pragma unroll
  for (int j = 0; j < kMaxSpecs; ++j)
    if (j < sp.n) {
      need_map |= sp.kind[j] == KRS_METRIC_MAP;
      need_dcg |= is_dcg_kind(sp.kind[j]);
      need_ndcg |= sp.kind[j] == KRS_METRIC_NDCG;
      if (sp.kind[j] == KRS_METRIC_MRR) max_mask |= 1u << j;
    }

  for (int i = threadIdx.x; i < n_slots; i += kThreads) {
    const int q = i >> lgP, k = i & (P - 1);
    const int64_t row = row0 + q;
    uint64_t key = 0;   // padding: below every item
    float y = 0.0f, w = 0.0f;
    if (k < L && row < batch) {
      const int64_t o = row * L + k;
      const float s = load1(&scores[row * ld + k]);
      const float yy = labels[o];
      const float ww = weights ? weights[row * w_row_stride + k * w_item_stride] : weight;
      const bool valid = yy >= 0.0f && (!mask || mask[o]) && ww > 0.0f;
      y = valid ? yy : 0.0f;
      w = valid ? ww : 0.0f;
      const uint32_t hi = valid ? order_key(s) : 1u;
      const uint32_t r20 = shuffle ? tie_r20(salt, row, k) : 0u;
      key = ((uint64_t)hi << 32) | ((uint64_t)r20 << 12) | (uint64_t)(4095 - k);
    }
    keys[i] = key;
    ys[i] = y;
    ws[i] = w;
  }
  __syncthreads();
  bitonic_sort(keys, n_slots, P, 0);

  const int q = lp.q(), u = lp.u();
  const int64_t row = row0 + q;
  const bool live = row < batch;
  const uint64_t* lk = keys + q * P + u * ept;   // this thread's ranks u*ept + 1 .. u*ept + ept
  const float* ly = ys + q * P;
  const float* lw = ws + q * P;
  float acc[kSlots];
#pragma unroll
  for (int j = 0; j < kSlots; ++j) acc[j] = 0.0f;
  int idx[kEpt], cnt = 0;
  float rel[kEpt], wv[kEpt], gv[kEpt];
#pragma unroll
  for (int c = 0; c < kEpt; ++c) {
    idx[c] = -1;
    rel[c] = wv[c] = gv[c] = 0.0f;
    if (c < ept) {
      const uint64_t key = lk[c];
      if (key != 0) {   // (a list past the batch holds padding only)
        const int i = 4095 - (int)(key & 4095u);
        idx[c] = i;
        const float y = ly[i];
        wv[c] = lw[i];
        rel[c] = y >= 1.0f ? 1.0f : 0.0f;
        gv[c] = gain ? gain[row * L + i] : exp2f(y) - 1.0f;
        cnt += y >= 1.0f ? 1 : 0;
        acc[kSumWG] += wv[c] * gv[c];
        acc[kSumG] += gv[c];
        acc[kSumWR] += wv[c] * rel[c];
        acc[kSumR] += rel[c];
        acc[kSumW] += wv[c];
        acc[kNValid] += (uint32_t)(key >> 32) != 1u ? 1.0f : 0.0f;
        if (order) order[row * L + u * ept + c] = i;
      }
    }
  }
  int cum = need_map ? seg_exclusive_scan(ibuf, cnt, tpl) : 0;
#pragma unroll
  for (int c = 0; c < kEpt; ++c) {
    if (idx[c] < 0) continue;
    const int r1 = u * ept + c + 1;
    const float rank = (float)r1;
    cum += rel[c] != 0.0f ? 1 : 0;
    const float d = need_dcg ? rank_discount(discount, discount_len, r1) : 0.0f;
#pragma unroll
    for (int j = 0; j < kMaxSpecs; ++j) {
      if (j >= sp.n || r1 > sp.k[j]) continue;
      switch (sp.kind[j]) {
        case KRS_METRIC_DCG:
        case KRS_METRIC_NDCG: acc[j] += wv[c] * (gv[c] * d); break;
        case KRS_METRIC_MAP: acc[j] += ((float)cum / rank) * (wv[c] * rel[c]); break;
        case KRS_METRIC_MRR: acc[j] = fmaxf(acc[j], rel[c] * (1.0f / rank)); break;
        default: acc[j] += rel[c]; break;   // precision, recall
      }
    }
  }
  seg_all_reduce<kSlots>(red, acc, max_mask, tpl);

  float vals[kMaxSpecs];
#pragma unroll
  for (int j = 0; j < kMaxSpecs; ++j) {
    vals[j] = acc[j];
    if (j < sp.n) {
      if (sp.kind[j] == KRS_METRIC_MAP) vals[j] = divide_no_nan(acc[j], acc[kSumWR]);
      else if (sp.kind[j] == KRS_METRIC_PRECISION) vals[j] = divide_no_nan(acc[j], fminf((float)sp.k[j], acc[kNValid]));
      else if (sp.kind[j] == KRS_METRIC_RECALL) vals[j] = divide_no_nan(acc[j], acc[kSumR]);
    }
  }

  if (need_ndcg) {
    // the ideal order: w * gain descending (ties contribute equal terms, so the index alone breaks them)
    __syncthreads();   // (every thread has read its keys)
    for (int i = threadIdx.x; i < n_slots; i += kThreads) {
      const int qq = i >> lgP, k = i & (P - 1);
      const int64_t r = row0 + qq;
      uint64_t key = 0;
      if (k < L && r < batch) {
        const float g = gain ? gain[r * L + k] : exp2f(ys[i]) - 1.0f;
        key = ((uint64_t)order_key(ws[i] * g) << 32) | (uint64_t)(4095 - k);
      }
      keys[i] = key;
    }
    __syncthreads();
    bitonic_sort(keys, n_slots, P, 0);
    float ideal[kMaxSpecs];
#pragma unroll
    for (int j = 0; j < kMaxSpecs; ++j) ideal[j] = 0.0f;
#pragma unroll
    for (int c = 0; c < kEpt; ++c) {
      if (c >= ept) continue;
      const uint64_t key = lk[c];
      if (key == 0) continue;
      const int i = 4095 - (int)(key & 4095u);
      const int r1 = u * ept + c + 1;
      const float w = lw[i];
      const float g = gain ? gain[row * L + i] : exp2f(ly[i]) - 1.0f;
      const float d = rank_discount(discount, discount_len, r1);
#pragma unroll
      for (int j = 0; j < kMaxSpecs; ++j)
        if (j < sp.n && sp.kind[j] == KRS_METRIC_NDCG && r1 <= sp.k[j]) ideal[j] += w * (g * d);
    }
    seg_all_reduce<kMaxSpecs>(red, ideal, 0u, tpl);
#pragma unroll
    for (int j = 0; j < kMaxSpecs; ++j)
      if (j < sp.n && sp.kind[j] == KRS_METRIC_NDCG) vals[j] = divide_no_nan(vals[j], ideal[j]);
  }

  if (!live || u != 0) return;
#pragma unroll
  for (int j = 0; j < kMaxSpecs; ++j)
    if (j < sp.n) values[(int64_t)j * batch + row] = vals[j];
  sums[row] = acc[kSumWG];
  sums[batch + row] = acc[kSumG];
  sums[2 * batch + row] = acc[kSumWR];
  sums[3 * batch + row] = acc[kSumR];
  sums[4 * batch + row] = acc[kSumW];
}

// get_list_weights for one list: 0 without weight, sum(w relevance) / sum(relevance) with relevance, else the default
__device__ __forceinline__ float list_weight(float swr, float sr, float sw, float avg) {
  if (!(sw > 0.0f)) return 0.0f;
  return sr > 0.0f ? divide_no_nan(swr, sr) : avg;
}

// stage B, pass 1 over the lists first, first + stride, ...: per relevance definition (gain; label >= 1) the sum of
// sum(w relevance) / sum(relevance) and the number of lists with weight and relevance
__device__ __forceinline__ void default_weight_sums(const float* __restrict__ sums, int64_t batch, int64_t first,
                                                    int64_t stride, float (&s)[4]) {
  const float* swg = sums;
  const float* sg = sums + batch;
  const float* swr = sums + 2 * batch;
  const float* sr = sums + 3 * batch;
  const float* sw = sums + 4 * batch;
#pragma unroll 4
  for (int64_t b = first; b < batch; b += stride) {
    const bool has_w = sw[b] > 0.0f;
    s[0] += divide_no_nan(swg[b], sg[b]);
    s[1] += has_w && sg[b] > 0.0f ? 1.0f : 0.0f;
    s[2] += divide_no_nan(swr[b], sr[b]);
    s[3] += has_w && sr[b] > 0.0f ? 1.0f : 0.0f;
  }
}

// stage B, pass 2 over the same lists: every list's weight, DCG's division by it, and per spec the sums of
// value * weight (t[2 j]) and weight (t[2 j + 1])
__device__ __forceinline__ void mean_update_sums(const float* __restrict__ values, const float* __restrict__ sums,
                                                 const Specs& sp, int64_t batch, int64_t first, int64_t stride,
                                                 const float (&s)[4], float* __restrict__ out_values,
                                                 float* __restrict__ out_weights, float (&t)[2 * kMaxSpecs]) {
  const float* swg = sums;
  const float* sg = sums + batch;
  const float* swr = sums + 2 * batch;
  const float* sr = sums + 3 * batch;
  const float* sw = sums + 4 * batch;
  const float avg_g = s[1] > 0.0f ? s[0] / s[1] : 1.0f;
  const float avg_r = s[3] > 0.0f ? s[2] / s[3] : 1.0f;
#pragma unroll 1
  for (int64_t b = first; b < batch; b += stride) {
    const float wg = list_weight(swg[b], sg[b], sw[b], avg_g);
    const float wr = list_weight(swr[b], sr[b], sw[b], avg_r);
#pragma unroll
    for (int j = 0; j < kMaxSpecs; ++j) {
      if (j >= sp.n) continue;
      const float w = is_dcg_kind(sp.kind[j]) ? wg : wr;
      float v = values[(int64_t)j * batch + b];
      if (sp.kind[j] == KRS_METRIC_DCG) v = divide_no_nan(v, w);
      t[2 * j] += v * w;
      t[2 * j + 1] += w;
      if (out_values) out_values[(int64_t)j * batch + b] = v;
      if (out_weights) out_weights[(int64_t)j * batch + b] = w;
    }
  }
}

// the whole of stage B in one workgroup: the route for batch <= kThreads
__global__ __launch_bounds__(kThreads) void metric_accumulate_kernel(const float* __restrict__ values,
                                                                     const float* __restrict__ sums, Specs sp,
                                                                     int64_t batch, States st,
                                                                     float* __restrict__ out_values,
                                                                     float* __restrict__ out_weights,
                                                                     int64_t* __restrict__ draw) {
  __shared__ float red[2 * kMaxSpecs][kWaves];
  float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  default_weight_sums(sums, batch, threadIdx.x, kThreads, s);
  seg_all_reduce<4>(red, s, 0u, kThreads);
  float t[2 * kMaxSpecs];
#pragma unroll
  for (int j = 0; j < 2 * kMaxSpecs; ++j) t[j] = 0.0f;
  mean_update_sums(values, sums, sp, batch, threadIdx.x, kThreads, s, out_values, out_weights, t);
  seg_all_reduce<2 * kMaxSpecs>(red, t, 0u, kThreads);
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int j = 0; j < kMaxSpecs; ++j)
    if (j < sp.n) {
      float* state = st.p[j];
      state[0] += t[2 * j];
      state[1] += t[2 * j + 1];
    }
  if (draw) *draw = *draw + 1;
}

// Stage B over several workgroups, for batch > kThreads (one workgroup takes 3.6 ns per list: 233 us at 65 536
// lists).  Three launches, each workgroup g on the lists g * kThreads + thread, + gridDim.x * kThreads, ...:
//   metric_weight_partials_kernel  pass 1; partial[g][0..3]
//   metric_mean_partials_kernel    every workgroup adds the partials of pass 1 in the order of g, then pass 2 on its
//                                  lists; partial2[g][0..15]
//   metric_state_update_kernel     thread j adds column j of partial2 in the order of g into its state word
// Every sum has a fixed order and nothing is atomic, as in the one-workgroup route.
constexpr int kAccMaxGroups = 256;
constexpr int kAccPartials = 4 + 2 * kMaxSpecs;   // floats of workspace per workgroup

__global__ __launch_bounds__(kThreads) void metric_weight_partials_kernel(const float* __restrict__ sums,
                                                                          int64_t batch, float* __restrict__ ws) {
  __shared__ float red[4][kWaves];
  float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  default_weight_sums(sums, batch, (int64_t)blockIdx.x * kThreads + threadIdx.x, (int64_t)gridDim.x * kThreads, s);
  seg_all_reduce<4>(red, s, 0u, kThreads);
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int c = 0; c < 4; ++c) ws[blockIdx.x * kAccPartials + c] = s[c];
}

__global__ __launch_bounds__(kThreads) void metric_mean_partials_kernel(const float* __restrict__ values,
                                                                        const float* __restrict__ sums, Specs sp,
                                                                        int64_t batch, float* ws,
                                                                        float* __restrict__ out_values,
                                                                        float* __restrict__ out_weights) {
  __shared__ float red[2 * kMaxSpecs][kWaves];
  float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int g = 0; g < (int)gridDim.x; ++g) {
#pragma unroll
    for (int c = 0; c < 4; ++c) s[c] += ws[g * kAccPartials + c];
  }
  float t[2 * kMaxSpecs];
#pragma unroll
  for (int j = 0; j < 2 * kMaxSpecs; ++j) t[j] = 0.0f;
  mean_update_sums(values, sums, sp, batch, (int64_t)blockIdx.x * kThreads + threadIdx.x,
                   (int64_t)gridDim.x * kThreads, s, out_values, out_weights, t);
  seg_all_reduce<2 * kMaxSpecs>(red, t, 0u, kThreads);
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int j = 0; j < 2 * kMaxSpecs; ++j) ws[blockIdx.x * kAccPartials + 4 + j] = t[j];
}

__global__ __launch_bounds__(64) void metric_state_update_kernel(const float* __restrict__ ws, int groups, Specs sp,
                                                                  States st, int64_t* __restrict__ draw) {
  const int j = threadIdx.x;
  if (j < 2 * sp.n) {
    float a = 0.0f;
    for (int g = 0; g < groups; ++g) a += ws[g * kAccPartials + 4 + j];
    float* word = nullptr;
#pragma unroll
    for (int m = 0; m < kMaxSpecs; ++m)
      if (m == (j >> 1)) word = st.p[m] + (j & 1);
    *word += a;
  }
  if (j == 0 && draw) *draw = *draw + 1;
}

int acc_groups(int64_t batch) {
  const int64_t g = ceil_div(batch, (int64_t)kThreads);
  return (int)(g < kAccMaxGroups ? g : kAccMaxGroups);
}

int fill_specs(const char* what, const int* kinds, const int* ks, int n_specs, int L, Specs* sp) {
  KRS_REQUIRE(n_specs >= 1 && n_specs <= kMaxSpecs, "%s: %d metric specs outside the supported 1..%d "
              "(KRS_METRIC_MAX_SPECS)", what, n_specs, kMaxSpecs);
  KRS_REQUIRE(kinds, "%s: null kinds", what);
  sp->n = n_specs;
  for (int j = 0; j < kMaxSpecs; ++j) {
    sp->kind[j] = j < n_specs ? kinds[j] : 0;
    sp->k[j] = j < n_specs ? (ks && ks[j] > 0 && ks[j] < L ? ks[j] : L) : 0;
    KRS_REQUIRE(sp->kind[j] >= KRS_METRIC_DCG && sp->kind[j] <= KRS_METRIC_RECALL, "%s: bad metric kind %d", what,
                sp->kind[j]);
  }
  return KRS_OK;
}

}  // namespace
}  // namespace krs

extern "C" int krs_ranking_metrics(const void* scores, int64_t ld, int dtype, const float* labels, const uint8_t* mask,
                                   const float* weights, int64_t weights_row_stride,
                                   int64_t weights_item_stride, float weight, const float* gain,
                                   const float* discount, int64_t discount_len, int shuffle_ties, uint64_t seed,
                                   const int64_t* draw,
                                   const int* kinds, const int* ks, int n_specs, int64_t batch, int64_t list,
                                   float* values, float* sums, int32_t* order, void* stream) {
  using namespace krs;
  const char* what = "krs_ranking_metrics";
  int rc = check_lists(what, ld, dtype, batch, list);
  if (rc != KRS_OK) return rc;
  const int L = (int)list;
  Specs sp;
  rc = fill_specs(what, kinds, ks, n_specs, L, &sp);
  if (rc != KRS_OK) return rc;
  KRS_REQUIRE(!weights || (weights_row_stride >= 0 && (weights_item_stride == 0 || weights_item_stride == 1) &&
                           weights_row_stride >= weights_item_stride * list),
              "%s: weights strides (%lld, %lld) are neither [batch, list] nor one weight per list", what,
              (long long)weights_row_stride, (long long)weights_item_stride);
  if (discount)
    for (int j = 0; j < sp.n; ++j)
      KRS_REQUIRE(!(sp.kind[j] == KRS_METRIC_DCG || sp.kind[j] == KRS_METRIC_NDCG) || discount_len >= sp.k[j],
                  "%s: %lld discounts for k = %d", what, (long long)discount_len, sp.k[j]);
  KRS_REQUIRE(batch == 0 || (scores && labels && values && sums), "%s: null argument", what);
  if (batch == 0) return KRS_OK;
  const dim3 grid = ListPack(L).grid(batch);
  const int dlen = discount ? (int)(discount_len < kMaxList ? discount_len : kMaxList) : 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == KRS_BF16)
    hipLaunchKernelGGL(ranking_metric_kernel<uint16_t>, grid, dim3(kThreads), 0, st,
                       reinterpret_cast<const uint16_t*>(scores), ld, labels, mask, weights, weights_row_stride,
                       weights_item_stride, weight, gain, discount, dlen,
                       shuffle_ties != 0, seed, draw, sp, batch, L, values, sums, order);
  else
    hipLaunchKernelGGL(ranking_metric_kernel<float>, grid, dim3(kThreads), 0, st,
                       reinterpret_cast<const float*>(scores), ld, labels, mask, weights, weights_row_stride,
                       weights_item_stride, weight, gain, discount, dlen,
                       shuffle_ties != 0, seed, draw, sp, batch, L, values, sums, order);
  KRS_CHECK_LAUNCH(what);
  return KRS_OK;
}

extern "C" size_t krs_ranking_metrics_accumulate_workspace_bytes(int64_t batch) {
  using namespace krs;
  return batch <= kThreads ? 0 : (size_t)acc_groups(batch) * kAccPartials * sizeof(float);
}

extern "C" int krs_ranking_metrics_accumulate(const float* values, const float* sums, const int* kinds, int n_specs,
                                              int64_t batch, float* const* states, float* out_values,
                                              float* out_weights, int64_t* draw, void* workspace,
                                              size_t workspace_bytes, void* stream) {
  using namespace krs;
  const char* what = "krs_ranking_metrics_accumulate";
  Specs sp;
  const int rc = fill_specs(what, kinds, nullptr, n_specs, 1, &sp);
  if (rc != KRS_OK) return rc;
  KRS_REQUIRE(batch >= 0, "%s: negative batch", what);
  KRS_REQUIRE(states && (batch == 0 || (values && sums)), "%s: null argument", what);
  States st;
  for (int j = 0; j < kMaxSpecs; ++j) {
    st.p[j] = j < n_specs ? states[j] : nullptr;
    KRS_REQUIRE(j >= n_specs || st.p[j], "%s: null state %d", what, j);
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (batch <= kThreads) {
    hipLaunchKernelGGL(metric_accumulate_kernel, dim3(1), dim3(kThreads), 0, s, values, sums, sp, batch, st,
                       out_values, out_weights, draw);
    KRS_CHECK_LAUNCH(what);
    return KRS_OK;
  }
  const size_t need = krs_ranking_metrics_accumulate_workspace_bytes(batch);
  if (!workspace || workspace_bytes < need)
    return fail(KRS_ERR_WORKSPACE, "%s: needs %zu workspace bytes, got %zu", what, need, workspace_bytes);
  const int groups = acc_groups(batch);
  float* ws = static_cast<float*>(workspace);
  hipLaunchKernelGGL(metric_weight_partials_kernel, dim3(groups), dim3(kThreads), 0, s, sums, batch, ws);
  KRS_CHECK_LAUNCH(what);
  hipLaunchKernelGGL(metric_mean_partials_kernel, dim3(groups), dim3(kThreads), 0, s, values, sums, sp, batch, ws,
                     out_values, out_weights);
  KRS_CHECK_LAUNCH(what);
  hipLaunchKernelGGL(metric_state_update_kernel, dim3(1), dim3(64), 0, s, ws, groups, sp, st, draw);
  KRS_CHECK_LAUNCH(what);
  return KRS_OK;
}
