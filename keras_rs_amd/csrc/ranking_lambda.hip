// K28 -- LambdaRank pair weights on the pairwise ranking losses: K9's hinge / logistic / soft zero-one loss and logit
// gradient with every pair weighted by how far swapping its two items would move DCG (include/krs.h, K28).
//
// The weight of a pair depends on the two items' ranks by score, so a list is sorted here before its pairs are walked:
//
//   1. sort      pair_key(order_key(s), index) of every item, several lists to a workgroup (ListPack), in LDS.  An
//                invalid item carries the key 0 (below every score, above the padding, which is the whole pair 0).
//   2. records   position p of a list receives {s, y, g, G} of the item of rank p + 1: s out of the key itself, the
//                others gathered through the key's index.  The valid items are then the prefix [0, n_valid), the pair
//                walk tests no validity, and the discount of an item is a function of its position alone.
//   3. tables    D_cut (and smooth_fraction * R when SMOOTH) once per workgroup in LDS, shared by all of its lists: no
//                log in the pair walk, D_cut[j] is a broadcast read.
//   4. ideal DCG (normalized) the gains of the valid prefix sorted in the key buffer, which is dead by then, their
//                first min(topn, n_valid) multiplied by the table and summed in a fixed order; G <- G / Z.
//   5. pairs     a pair with both ranks beyond topn weighs nothing.  Walk A: the thread of every position walks
//                j in [0, min(topn, n_valid)).  Walk B, only when topn < list: the tail j in [topn, n_valid) of each
//                row p < topn is split over the lanes of one wave (of the list's tpl lanes when those are fewer) and
//                summed by a butterfly, so the long rows cost n_valid / 64 steps each and not n_valid steps of a wave
//                with topn lanes alive.  2 * n_valid * topn pairs a list in place of n_valid^2.
//   6. write     back to item order through the index each thread kept from its keys.
//
// One owner per output, no atomics, fixed summation orders: repeated calls are bit-identical.  No host synchronisation.
#include "krs_list.h"
#include "ranking_lambda_plan.h"

namespace krs {
namespace {

constexpr int kThreads = kListThreads;
constexpr int kEpt = KRS_RANK_MAX_LIST / kThreads;   // positions per thread, at most
static_assert(lambda_rank::kThreads == kListThreads && lambda_rank::kMaxList == KRS_RANK_MAX_LIST, "plan constants");

struct LambdaArgs {
  const void* logits;
  int64_t ld;
  const float* labels;
  const uint8_t* mask;
  const float* gain;       // NULL = 2^y - 1
  const float* discount;   // NULL = 1 / log2(1 + r); entry r - 1 is D(r)
  const float* g;
  float g_scale, inv_t, sigma;
  int topn;                // 1 .. L
  int normalized;
  int64_t batch;
  int L;
  float* item_loss;
  void* dlogits;
};

// K9's pair_term (ranking_loss.hip), restated: phi and phi' of one pair as autodiff differentiates the reference's
// expression (relu'(0) = abs'(0) = 0)
template <int KIND>
__device__ __forceinline__ void pair_term(float x, float& phi, float& dphi) {
  if constexpr (KIND == KRS_RANK_HINGE) {
    const float h = 1.0f - x;
    phi = fmaxf(h, 0.0f);
    dphi = h > 0.0f ? -1.0f : 0.0f;
  } else if constexpr (KIND == KRS_RANK_LOGISTIC) {
    const float e = __expf(-fabsf(x));
    const float r = __builtin_amdgcn_rcpf(1.0f + e);
    phi = fmaxf(-x, 0.0f) + __logf(1.0f + e);
    dphi = x > 0.0f ? -e * r : (x < 0.0f ? -r : 0.0f);
  } else {  // KRS_RANK_SOFT_ZERO_ONE
    const float e = __expf(-fabsf(x));
    const float r = __builtin_amdgcn_rcpf(1.0f + e);
    phi = x > 0.0f ? e * r : r;
    dphi = -e * r * r;
  }
}

// the float an order_key was made from (-0 comes back as +0, every NaN as one NaN)
__device__ __forceinline__ float key_value(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__device__ __forceinline__ float table_discount(const float* __restrict__ discount, int i) {
  return discount ? discount[i] : 1.0f / log2f(2.0f + (float)i);   // D(i + 1), K10's default
}

// One ordered pair (k, j) of rank positions seen from k: at most one of (k, j), (j, k) carries I(y > y'), and lambda is
// symmetric.  me / o = {s, y, g, G}; dk / dj = D_cut of the two positions; rtab[d] = smooth_fraction * R(d).
template <int KIND, bool SMOOTH>
__device__ __forceinline__ void lambda_pair(const float4 me, float dk, int k, const float4 o, float dj, int j,
                                            const float* rtab, float one_minus_sigma, float inv_t, float& loss,
                                            float& gsum, float& grad) {
  const bool gt = me.y > o.y, lt = o.y > me.y;
  const float d = me.x - o.x;
  const float x = (gt ? d : -d) * inv_t;
  float phi, dphi;
  pair_term<KIND>(x, phi, dphi);
  float w = fabsf(dk - dj);
  if constexpr (SMOOTH) w = fmaf(one_minus_sigma, w, rtab[k > j ? k - j : j - k]);
  const float lam = fabsf(me.w - o.w) * w;
  loss += gt ? lam * phi : 0.0f;
  gsum += gt ? lam * dphi : 0.0f;
  grad -= lt ? o.z * (lam * dphi) : 0.0f;
}

template <int KIND, bool SMOOTH, typename T>
__global__ __launch_bounds__(kThreads) void lambda_pairwise_kernel(const LambdaArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float red[1][kListWaves];
  const int L = a.L;
  const lambda_rank::Layout lay = lambda_rank::layout(L, SMOOTH);
  uint64_t* keys = reinterpret_cast<uint64_t*>(smem + lay.keys);
  float4* recs = reinterpret_cast<float4*>(smem + lay.recs);
  float* dcut = reinterpret_cast<float*>(smem + lay.dcut);
  float* rtab = reinterpret_cast<float*>(smem + lay.rtab);   // (SMOOTH only: not allocated otherwise)
  const T* logits = reinterpret_cast<const T*>(a.logits);
  T* dlogits = reinterpret_cast<T*>(a.dlogits);
  const ListPack lp(L);
  const int P = lp.P, tpl = lp.tpl, ept = lp.ept;
  const int64_t row0 = lp.row0();
  const int n_slots = lp.n_slots();
  const int topn = a.topn;

  // 1. keys and tables
  for (int i = threadIdx.x; i < n_slots; i += kThreads) {
    const int q = i / P, k = i - q * P;
    const int64_t row = row0 + q;
    uint64_t key = 0;   // padding: below every real pair
    if (k < L && row < a.batch) {
      const int64_t o = row * L + k;
      const bool valid = a.labels[o] >= 0.0f && (!a.mask || a.mask[o]);
      key = pair_key(valid ? order_key(load1(&logits[row * a.ld + k])) : 0u, (uint32_t)k);   // (a real order_key is > 0)
    }
    keys[i] = key;
  }
  for (int p = threadIdx.x; p < L; p += kThreads) {
    dcut[p] = p < topn ? table_discount(a.discount, p) : 0.0f;
    if constexpr (SMOOTH)
      rtab[p] = p == 0 ? 0.0f : a.sigma * fabsf(table_discount(a.discount, p - 1) - table_discount(a.discount, p));
  }
  __syncthreads();
  bitonic_sort(keys, n_slots, P, 0);

  // 2. records in rank order; this thread's positions are u, u + tpl, ..
  const int q = lp.q(), u = lp.u();
  const int64_t row = row0 + q;
  uint64_t* lkeys = keys + q * P;
  float4* list = recs + q * P;
  int idx[kEpt];
  float cnt[1] = {0.0f};
#pragma unroll
  for (int c = 0; c < kEpt; ++c) {
    idx[c] = -1;
    if (c >= ept) continue;
    const uint64_t key = lkeys[u + c * tpl];
    if (key == 0) continue;   // padding, or a list beyond the batch
    idx[c] = (int)pair_index(key);
    if ((key >> 32) == 0) continue;   // invalid: no rank, no pairs
    const int64_t o = row * L + idx[c];
    const float y = a.labels[o];
    list[u + c * tpl] = make_float4(key_value((uint32_t)(key >> 32)), y, a.g ? a.g_scale * a.g[o] : a.g_scale,
                                    a.gain ? a.gain[o] : exp2f(y) - 1.0f);
    cnt[0] += 1.0f;
  }
  seg_all_reduce<1>(red, cnt, 0u, tpl);
  const int nv = (int)cnt[0];
  const int ncut = topn < nv ? topn : nv;
  __syncthreads();   // the records are complete and the keys are dead

  // 4. ideal DCG
  if (a.normalized) {
#pragma unroll
    for (int c = 0; c < kEpt; ++c) {
      const int p = u + c * tpl;
      if (c < ept) lkeys[p] = p < nv ? pair_key(order_key(list[p].w), (uint32_t)p) : 0;
    }
    __syncthreads();
    bitonic_sort(keys, n_slots, P, 0);
    float z[1] = {0.0f};
#pragma unroll
    for (int c = 0; c < kEpt; ++c) {
      const int p = u + c * tpl;
      if (c < ept && p < ncut) z[0] += key_value((uint32_t)(lkeys[p] >> 32)) * dcut[p];
    }
    seg_all_reduce<1>(red, z, 0u, tpl);
    const float ideal = z[0];
#pragma unroll
    for (int c = 0; c < kEpt; ++c) {
      const int p = u + c * tpl;
      if (c < ept && p < nv) list[p].w = ideal > 0.0f ? list[p].w / ideal : 0.0f;
    }
    __syncthreads();   // the scaled gains are in place and the gain keys are dead
  }

  // 5. walk A: every position against the first min(topn, n_valid)
  const float oms = 1.0f - a.sigma;
  float loss[kEpt], grad[kEpt];
#pragma unroll
  for (int c = 0; c < kEpt; ++c) {
    loss[c] = 0.0f, grad[c] = 0.0f;
    const int k = u + c * tpl;
    if (c >= ept || k >= nv) continue;
    const float4 me = list[k];
    const float dk = dcut[k];
    float gsum = 0.0f;
#pragma unroll 4
    for (int j = 0; j < ncut; ++j)
      lambda_pair<KIND, SMOOTH>(me, dk, k, list[j], dcut[j], j, rtab, oms, a.inv_t, loss[c], gsum, grad[c]);
    grad[c] = me.z * gsum + grad[c];
  }
  // walk B: the tails of the rows below topn.  Row p belongs to group p mod ng of its list, a group being w lanes.
  if (topn < L) {   // (uniform over the workgroup; n_valid <= topn leaves every tail empty)
    const int w = tpl < 64 ? tpl : 64, ng = tpl / w, lane = u & (w - 1);
    float2* tails = reinterpret_cast<float2*>(lkeys);
    for (int p = u / w; p < topn; p += ng) {   // (the same trips for every lane of a wave)
      float v[3] = {0.0f, 0.0f, 0.0f};
      float gk = 0.0f;
      if (p < ncut) {
        const float4 me = list[p];
        const float dk = dcut[p];
        gk = me.z;
#pragma unroll 4
        for (int j = topn + lane; j < nv; j += w)
          lambda_pair<KIND, SMOOTH>(me, dk, p, list[j], 0.0f, j, rtab, oms, a.inv_t, v[0], v[1], v[2]);
      }
#pragma unroll
      for (int i = 0; i < 3; ++i)
        for (int o = 1; o < w; o <<= 1) v[i] += __shfl_xor(v[i], o);
      if (lane == 0 && p < ncut) tails[p] = make_float2(v[0], gk * v[1] + v[2]);
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < kEpt; ++c) {
      const int k = u + c * tpl;
      if (c < ept && k < ncut) {
        const float2 t = tails[k];
        loss[c] += t.x;
        grad[c] += t.y;
      }
    }
  }

  // 6. back to item order
#pragma unroll
  for (int c = 0; c < kEpt; ++c) {
    if (idx[c] < 0) continue;
    const int64_t o = row * L + idx[c];
    if (a.item_loss) a.item_loss[o] = loss[c];
    if (dlogits) store1(&dlogits[o], a.inv_t * grad[c]);
  }
}

template <int KIND, bool SMOOTH, typename T>
int launch_one(const LambdaArgs& a, hipStream_t st) {
  auto kern = lambda_pairwise_kernel<KIND, SMOOTH, T>;
  static bool raised = false;   // once per build, to the longest list's LDS: no runtime call is left for a captured step
  if (!raised) {
    KRS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lambda_rank::layout(lambda_rank::kMaxList, SMOOTH).total));
    raised = true;
  }
  const size_t lds = (size_t)lambda_rank::layout(a.L, SMOOTH).total;
  hipLaunchKernelGGL(kern, ListPack(a.L).grid(a.batch), dim3(kThreads), lds, st, a);
  KRS_CHECK_LAUNCH("krs_pairwise_lambda_loss");
  return KRS_OK;
}

template <int KIND>
int launch_kind(const LambdaArgs& a, int dtype, hipStream_t st) {
  const bool smooth = a.sigma > 0.0f;
  if (dtype == KRS_BF16) return smooth ? launch_one<KIND, true, uint16_t>(a, st) : launch_one<KIND, false, uint16_t>(a, st);
  return smooth ? launch_one<KIND, true, float>(a, st) : launch_one<KIND, false, float>(a, st);
}

}  // namespace
}  // namespace krs

extern "C" int krs_pairwise_lambda_loss(int kind, const void* logits, int64_t ld, int dtype, const float* labels,
                                        const uint8_t* mask, const float* gain, const float* discount,
                                        int64_t discount_len, int64_t topn, int normalized, float smooth_fraction,
                                        const float* g, float g_scale, float inv_temperature, int64_t batch,
                                        int64_t list, float* item_loss, void* dlogits, void* stream) {
  using namespace krs;
  const char* what = "krs_pairwise_lambda_loss";
  const int rc = check_lists(what, ld, dtype, batch, list);
  if (rc != KRS_OK) return rc;
  KRS_REQUIRE(kind != KRS_RANK_MSE, "%s: lambda weights are not defined for KRS_RANK_MSE", what);
  KRS_REQUIRE(kind >= KRS_RANK_HINGE && kind <= KRS_RANK_SOFT_ZERO_ONE, "%s: bad loss kind %d", what, kind);
  KRS_REQUIRE(inv_temperature > 0.0f, "%s: inverse temperature must be positive", what);
  KRS_REQUIRE(item_loss || dlogits, "%s: neither the loss nor the gradient is wanted", what);
  KRS_REQUIRE(batch == 0 || (logits && labels), "%s: null argument", what);
  KRS_REQUIRE(smooth_fraction >= 0.0f && smooth_fraction <= 1.0f, "%s: smooth_fraction %g outside [0, 1]", what,
              (double)smooth_fraction);
  KRS_REQUIRE(topn >= 0, "%s: negative topn", what);
  const int64_t need = list + (smooth_fraction > 0.0f ? 1 : 0);
  KRS_REQUIRE(!discount || discount_len >= need, "%s: %lld discounts for a list of %lld (%lld needed%s)", what,
              (long long)discount_len, (long long)list, (long long)need,
              smooth_fraction > 0.0f ? ": list + 1 with smooth_fraction > 0" : "");
  if (batch == 0) return KRS_OK;
  LambdaArgs a;
  a.logits = logits, a.ld = ld, a.labels = labels, a.mask = mask, a.gain = gain, a.discount = discount, a.g = g;
  a.g_scale = g_scale, a.inv_t = inv_temperature, a.sigma = smooth_fraction;
  a.topn = (int)(topn == 0 || topn > list ? list : topn);
  a.normalized = normalized != 0;
  a.batch = batch, a.L = (int)list, a.item_loss = item_loss, a.dlogits = dlogits;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  switch (kind) {
    case KRS_RANK_HINGE: return launch_kind<KRS_RANK_HINGE>(a, dtype, st);
    case KRS_RANK_LOGISTIC: return launch_kind<KRS_RANK_LOGISTIC>(a, dtype, st);
    default: return launch_kind<KRS_RANK_SOFT_ZERO_ONE>(a, dtype, st);
  }
}
