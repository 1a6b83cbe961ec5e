// K9 -- ranking losses: the pairwise losses and ListMLE of keras_rs.losses, loss and logit gradient in one pass.
//
// Replaces PairwiseLoss.compute_unreduced_loss / call (pairwise_loss.py, pairwise_loss_utils.py:pairwise_comparison),
// PairwiseMeanSquaredError.compute_unreduced_loss (pairwise_mean_squared_error.py) and
// ListMLELoss.compute_unreduced_loss (list_mle_loss.py:70-150).  The reference builds several (batch, list, list)
// tensors per call; here a list is staged in LDS once and its pairs are walked on chip.
//
//   * pairwise_kernel   one record {s, y', g} per item in LDS (y' = NaN marks an invalid item, so y'_k > y'_j is the
//                       pair weight I(y_k > y_j) valid_k valid_j); lane k walks j and accumulates
//                         l_k    = sum_j w_kj phi(x_kj),                       x_kj = (s_k - s_j) / T
//                         dl/ds_k = (1/T) [g_k sum_j w_kj phi'(x_kj) - sum_j g_j w_jk phi'(x_jk)]
//                       At most one of (k, j), (j, k) carries weight, so each ordered pair costs one phi / phi'.
//                       Mean squared error (symmetric weight valid_k valid_j, k != j, no temperature):
//                         l_k = sum_j w_kj d_kj^2,  d_kj = (y_k - y_j) - (s_k - s_j)
//                         dl/ds_k = -2 sum_j w_kj d_kj (g_k + g_j)
//   * listmle_kernel    sorts each list in LDS on pair_key (label descending, index ascending; invalid items
//                       carry the label -1e9 as in the reference), then one reverse scan for the normalisers
//                       E_r = sum_{q >= r} exp(z_q - m) and one forward scan for the closed-form gradient.
//
// Packing, sort, reductions and scans are krs_list.h's.  No atomics and fixed summation orders: repeated calls are
// bit-identical.  No host synchronisation: a call can be captured into a HIP graph.
#include "krs_list.h"

namespace krs {
namespace {

constexpr int kThreads = kListThreads;
constexpr int kMaxList = KRS_RANK_MAX_LIST;
constexpr float kListMleEps = 1e-10f;   // list_mle_loss.py: self._epsilon
constexpr float kListMleMasked = -1e9f; // list_mle_loss.py: the label / logit of an invalid item

// ---- pairwise --------------------------------------------------------------------------------------------------------
// phi and phi' of one weighted ordered pair, as autodiff differentiates the reference's expression (relu'(0) = 0,
// abs'(0) = 0): hinge relu(1 - x); logistic relu(-x) + log(1 + exp(-|x|)); soft zero-one
// where(x > 0, 1 - sigmoid(x), sigmoid(-x)).
template <int KIND>
__device__ __forceinline__ void pair_term(float x, float& phi, float& dphi) {
  if constexpr (KIND == KRS_RANK_HINGE) {
    const float h = 1.0f - x;
    phi = fmaxf(h, 0.0f);
    dphi = h > 0.0f ? -1.0f : 0.0f;
  } else if constexpr (KIND == KRS_RANK_LOGISTIC) {
    const float e = __expf(-fabsf(x));          // shared by phi and phi'
    const float r = __builtin_amdgcn_rcpf(1.0f + e);
    phi = fmaxf(-x, 0.0f) + __logf(1.0f + e);
    dphi = x > 0.0f ? -e * r : (x < 0.0f ? -r : 0.0f);
  } else {  // KRS_RANK_SOFT_ZERO_ONE
    const float e = __expf(-fabsf(x));
    const float r = __builtin_amdgcn_rcpf(1.0f + e);   // sigmoid(|x|)
    phi = x > 0.0f ? e * r : r;                        // sigmoid(-x)
    dphi = -e * r * r;                                 // -sigmoid(x) sigmoid(-x)
  }
}

template <int KIND, typename T>
__global__ __launch_bounds__(kThreads) void pairwise_kernel(const T* __restrict__ logits, int64_t ld,
                                                            const float* __restrict__ labels,
                                                            const uint8_t* __restrict__ mask,
                                                            const float* __restrict__ g, float g_scale, float inv_t,
                                                            int64_t batch, int L, float* __restrict__ item_loss,
                                                            T* __restrict__ dlogits) {
  __shared__ float4 sm[kMaxList];   // {s, y' (NaN = invalid), g, unused}
  // ListPack's tpl and lpb (the host launches by it), written out: taken from the struct, the same pair loop measured
  // 1-2 % slower at (256, 2048).  Items are packed L, not P, apart: nothing is sorted here.
  const int tpl = L >= kThreads ? kThreads : pow2_at_least(L);   // threads per list
  const int lpb = kThreads / tpl;                                  // lists per workgroup
  const int64_t row0 = (int64_t)blockIdx.x * lpb;
  const int n_items = lpb * L;
  for (int i = threadIdx.x; i < n_items; i += kThreads) {
    const int q = i / L, k = i - q * L;
    const int64_t row = row0 + q;
    if (row >= batch) break;
    const int64_t o = row * L + k;
    const float s = load1(&logits[row * ld + k]);
    const float y = labels[o];
    const bool valid = y >= 0.0f && (!mask || mask[o]);
    const float gv = valid ? (g ? g_scale * g[o] : g_scale) : 0.0f;
    sm[i] = make_float4(s, valid ? y : quiet_nan(), gv, 0.0f);
  }
  __syncthreads();
  const int q = threadIdx.x / tpl, u = threadIdx.x - q * tpl;
  const int64_t row = row0 + q;
  if (row >= batch) return;
  const float4* list = sm + q * L;
  for (int k = u; k < L; k += tpl) {
    const float4 me = list[k];
    float loss = 0.0f, grad = 0.0f;
    if constexpr (KIND == KRS_RANK_MSE) {
      if (me.y == me.y) {
#pragma unroll 4
        for (int j = 0; j < L; ++j) {
          const float4 o = list[j];
          const float d = (me.y - o.y) - (me.x - o.x);
          const bool w = o.y == o.y;                 // j valid (j == k adds d = 0)
          loss += w ? d * d : 0.0f;
          grad += w ? d * (me.z + o.z) : 0.0f;
        }
      }
      grad *= -2.0f;
    } else {
      float gsum = 0.0f;   // sum_j w_kj phi'(x_kj), scaled by g_k at the end
#pragma unroll 4
      for (int j = 0; j < L; ++j) {
        const float4 o = list[j];
        const bool gt = me.y > o.y, lt = o.y > me.y;
        const float d = me.x - o.x;
        const float x = (gt ? d : -d) * inv_t;     // argument of the weighted one of (k, j), (j, k)
        float phi, dphi;
        pair_term<KIND>(x, phi, dphi);
        loss += gt ? phi : 0.0f;
        gsum += gt ? dphi : 0.0f;
        grad -= lt ? o.z * dphi : 0.0f;
      }
      grad = inv_t * (me.z * gsum + grad);
    }
    const int64_t o = row * L + k;
    if (item_loss) item_loss[o] = loss;
    if (dlogits) store1(&dlogits[o], grad);
  }
}

// ---- ListMLE -----------------------------------------------------------------------------------------------------------
constexpr int kEpt = kMaxList / kThreads;   // sorted positions per thread, at most

template <typename T>
__global__ __launch_bounds__(kThreads) void listmle_kernel(const T* __restrict__ logits, int64_t ld,
                                                           const float* __restrict__ labels,
                                                           const uint8_t* __restrict__ mask,
                                                           const float* __restrict__ g, float g_scale, float inv_t,
                                                           int64_t batch, int L, float* __restrict__ list_loss,
                                                           T* __restrict__ dlogits) {
  __shared__ uint64_t keys[kMaxList];
  __shared__ float z[kMaxList];     // s / T in item order
  __shared__ float buf[kThreads / kListWaves][kListWaves];   // scans use all of it, reductions its first rows
  const ListPack lp(L);
  const int P = lp.P, tpl = lp.tpl, ept = lp.ept;
  const int64_t row0 = lp.row0();
  const int n_slots = lp.n_slots();
  for (int i = threadIdx.x; i < n_slots; i += kThreads) {
    const int q = i / P, k = i - q * P;
    const int64_t row = row0 + q;
    uint64_t key = 0;                          // padding: below every real pair
    if (k < L && row < batch) {
      const int64_t o = row * L + k;
      const float y = labels[o];
      const bool valid = y >= 0.0f && (!mask || mask[o]);
      key = pair_key(order_key(valid ? y : kListMleMasked), (uint32_t)k);
      z[q * L + k] = load1(&logits[row * ld + k]) * inv_t;
    }
    keys[i] = key;
  }
  __syncthreads();
  bitonic_sort(keys, n_slots, P, 0);

  const int q = lp.q(), u = lp.u();
  const int64_t row = row0 + q;
  const bool live = row < batch;
  const uint64_t* lk = keys + q * P + u * ept;   // this thread's sorted positions u*ept .. u*ept + ept - 1
  const float* lz = z + q * L;
  // valid: a label >= 0 has the top bit of its order key set; -1e9 (invalid) and padding do not
  bool valid[kEpt];
  float zr[kEpt];
  float top2[2] = {-__builtin_inff(), 0.0f};   // {max z, number of valid items}
#pragma unroll
  for (int c = 0; c < kEpt; ++c) {
    valid[c] = false;
    zr[c] = 0.0f;
    if (c < ept && live) {
      const uint64_t key = lk[c];
      valid[c] = (key >> 63) != 0;
      if (valid[c]) {
        zr[c] = lz[pair_index(key)];
        top2[0] = fmaxf(top2[0], zr[c]);
        top2[1] += 1.0f;
      }
    }
  }
  seg_all_reduce<2>(buf, top2, 1u, tpl);
  const float m_raw = top2[0];
  const bool any_valid = top2[1] > 0.0f;
  const float m = any_valid ? m_raw : 0.0f;
  // ties of the maximum share its gradient (autodiff of max)
  float ties[1] = {0.0f}, ez[kEpt];
  bool top[kEpt];
#pragma unroll
  for (int c = 0; c < kEpt; ++c) {
    top[c] = valid[c] && zr[c] == m_raw;
    ties[0] += top[c] ? 1.0f : 0.0f;
    zr[c] = zr[c] - m;                          // sorted_logits - raw_max
    ez[c] = valid[c] ? expf(zr[c]) : 0.0f;
  }
  seg_all_reduce<1>(buf, ties, 0u, tpl);
  const float n_ties = ties[0];
  // E_r: suffix sums of exp, fixed order (within a thread from its last position down, then across threads)
  float tsum = 0.0f;
#pragma unroll
  for (int c = kEpt - 1; c >= 0; --c) tsum += ez[c];
  float* sbuf = &buf[0][0];
  seg_scan<true, false>(sbuf, tsum, u, tpl);
  float acc = u + 1 < tpl ? sbuf[threadIdx.x + 1] : 0.0f;
  float inv[kEpt], tot[2] = {0.0f, 0.0f}, isum = 0.0f;   // tot: {loss, dl/dm = sum_r eps / (E_r + eps)}
#pragma unroll
  for (int c = kEpt - 1; c >= 0; --c) {
    acc += ez[c];
    const float den = acc + kListMleEps;
    inv[c] = valid[c] ? 1.0f / den : 0.0f;
    if (valid[c]) {
      tot[0] += logf(den) - zr[c];
      tot[1] += kListMleEps * inv[c];
    }
  }
  // prefix sums of 1 / (E_r + eps)
#pragma unroll
  for (int c = 0; c < kEpt; ++c) isum += inv[c];
  seg_scan<false, false>(sbuf, isum, u, tpl);
  float pre = u > 0 ? sbuf[threadIdx.x - 1] : 0.0f;
  seg_all_reduce<2>(buf, tot, 0u, tpl);   // (its leading barrier follows the read of sbuf)
  const float loss = tot[0], dmax = tot[1];
  if (!live) return;
  const float gl = any_valid ? (g ? g_scale * g[row] : g_scale) * inv_t : 0.0f;
  if (u == 0 && list_loss) list_loss[row] = any_valid ? loss : 0.0f;
  if (!dlogits) return;
#pragma unroll
  for (int c = 0; c < kEpt; ++c) {
    if (c >= ept) break;
    const uint64_t key = lk[c];
    if (key == 0) continue;                     // padding
    pre += inv[c];
    float d = 0.0f;
    if (valid[c]) {
      d = ez[c] * pre - 1.0f;
      if (top[c]) d += dmax / n_ties;
    }
    store1(&dlogits[row * L + pair_index(key)], gl * d);
  }
}

template <typename T>
void launch_pairwise(int kind, dim3 grid, hipStream_t st, const void* logits, int64_t ld, const float* labels,
                     const uint8_t* mask, const float* g, float g_scale, float inv_t, int64_t batch, int L,
                     float* item_loss, void* dlogits) {
  const T* x = reinterpret_cast<const T*>(logits);
  T* dx = reinterpret_cast<T*>(dlogits);
#define KRS_PAIRWISE_LAUNCH(K)                                                                                  \
  hipLaunchKernelGGL((pairwise_kernel<K, T>), grid, dim3(kThreads), 0, st, x, ld, labels, mask, g, g_scale, inv_t, \
                     batch, L, item_loss, dx)
  switch (kind) {
    case KRS_RANK_HINGE: KRS_PAIRWISE_LAUNCH(KRS_RANK_HINGE); break;
    case KRS_RANK_LOGISTIC: KRS_PAIRWISE_LAUNCH(KRS_RANK_LOGISTIC); break;
    case KRS_RANK_SOFT_ZERO_ONE: KRS_PAIRWISE_LAUNCH(KRS_RANK_SOFT_ZERO_ONE); break;
    default: KRS_PAIRWISE_LAUNCH(KRS_RANK_MSE); break;
  }
#undef KRS_PAIRWISE_LAUNCH
}

int check_common(const char* what, const void* logits, int64_t ld, int dtype, const float* labels, float inv_t,
                 int64_t batch, int64_t list, const void* loss, const void* dlogits) {
  const int rc = check_lists(what, ld, dtype, batch, list);
  if (rc != KRS_OK) return rc;
  KRS_REQUIRE(inv_t > 0.0f, "%s: inverse temperature must be positive", what);
  KRS_REQUIRE(loss || dlogits, "%s: neither the loss nor the gradient is wanted", what);
  KRS_REQUIRE(batch == 0 || (logits && labels), "%s: null argument", what);
  return KRS_OK;
}

}  // namespace
}  // namespace krs

extern "C" int krs_pairwise_loss(int kind, const void* logits, int64_t ld, int dtype, const float* labels,
                                 const uint8_t* mask, const float* g, float g_scale, float inv_temperature,
                                 int64_t batch, int64_t list, float* item_loss, void* dlogits, void* stream) {
  using namespace krs;
  const int rc = check_common("krs_pairwise_loss", logits, ld, dtype, labels, inv_temperature, batch, list, item_loss,
                              dlogits);
  if (rc != KRS_OK) return rc;
  KRS_REQUIRE(kind >= KRS_RANK_HINGE && kind <= KRS_RANK_MSE, "krs_pairwise_loss: bad loss kind %d", kind);
  if (batch == 0) return KRS_OK;
  const int L = (int)list;
  const dim3 grid = ListPack(L).grid(batch);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == KRS_BF16)
    launch_pairwise<uint16_t>(kind, grid, st, logits, ld, labels, mask, g, g_scale, inv_temperature, batch, L,
                              item_loss, dlogits);
  else
    launch_pairwise<float>(kind, grid, st, logits, ld, labels, mask, g, g_scale, inv_temperature, batch, L, item_loss,
                           dlogits);
  KRS_CHECK_LAUNCH("krs_pairwise_loss");
  return KRS_OK;
}

extern "C" int krs_listmle_loss(const void* logits, int64_t ld, int dtype, const float* labels, const uint8_t* mask,
                                const float* g, float g_scale, float inv_temperature, int64_t batch, int64_t list,
                                float* list_loss, void* dlogits, void* stream) {
  using namespace krs;
  const int rc = check_common("krs_listmle_loss", logits, ld, dtype, labels, inv_temperature, batch, list, list_loss,
                              dlogits);
  if (rc != KRS_OK) return rc;
  if (batch == 0) return KRS_OK;
  const int L = (int)list;
  const dim3 grid = ListPack(L).grid(batch);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == KRS_BF16)
    hipLaunchKernelGGL(listmle_kernel<uint16_t>, grid, dim3(kThreads), 0, st,
                       reinterpret_cast<const uint16_t*>(logits), ld, labels, mask, g, g_scale, inv_temperature, batch,
                       L, list_loss, reinterpret_cast<uint16_t*>(dlogits));
  else
    hipLaunchKernelGGL(listmle_kernel<float>, grid, dim3(kThreads), 0, st, reinterpret_cast<const float*>(logits), ld,
                       labels, mask, g, g_scale, inv_temperature, batch, L, list_loss,
                       reinterpret_cast<float*>(dlogits));
  KRS_CHECK_LAUNCH("krs_listmle_loss");
  return KRS_OK;
}
