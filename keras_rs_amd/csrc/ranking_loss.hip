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
//   * listmle_kernel    sorts each list in LDS on the K8 pair key (label descending, index ascending; invalid items
//                       carry the label -1e9 as in the reference), then one reverse scan for the normalisers
//                       E_r = sum_{q >= r} exp(z_q - m) and one forward scan for the closed-form gradient.
//
// Lists of up to kThreads items are packed several per workgroup (all lists of a launch share L, so every
// workgroup runs one uniform schedule); longer lists take a workgroup each.  No atomics and fixed summation orders:
// repeated calls are bit-identical.  No host synchronisation: a call can be captured into a HIP graph.
#include "krs_common.h"

namespace krs {
namespace {

constexpr int kThreads = 1024;
constexpr int kMaxList = KRS_RANK_MAX_LIST;
constexpr float kListMleEps = 1e-10f;   // list_mle_loss.py: self._epsilon
constexpr float kListMleMasked = -1e9f; // list_mle_loss.py: the label / logit of an invalid item

__device__ __forceinline__ int pow2_at_least(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

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
  const int tpl = L >= kThreads ? kThreads : pow2_at_least(L);   // threads per list
  const int lpb = kThreads / tpl;                                  // lists per workgroup
  const int64_t row0 = (int64_t)blockIdx.x * lpb;
  const int n_items = lpb * L;
  for (int i = threadIdx.x; i < n_items; i += kThreads) {
    const int q = i / L, k = i - q * L;
    const int64_t row = row0 + q;
    if (row >= batch) break;
    const int64_t o = row * L + k;
    float s;
    if constexpr (sizeof(T) == 2) s = bf16_to_f32(logits[row * ld + k]);
    else s = logits[row * ld + k];
    const float y = labels[o];
    const bool valid = y >= 0.0f && (!mask || mask[o]);
    const float gv = valid ? (g ? g_scale * g[o] : g_scale) : 0.0f;
    sm[i] = make_float4(s, valid ? y : __uint_as_float(0x7fc00000u), gv, 0.0f);
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
    if (dlogits) {
      if constexpr (sizeof(T) == 2) dlogits[o] = f32_to_bf16(grad);
      else dlogits[o] = grad;
    }
  }
}

// ---- ListMLE -----------------------------------------------------------------------------------------------------------
// inclusive scan (reverse: suffix) of v over the tpl threads of each list; every thread of the workgroup calls it
template <bool REVERSE, bool MAX>
__device__ __forceinline__ float seg_scan(float* buf, float v, int u, int tpl) {
  __syncthreads();   // (the previous scan's results have been read)
  buf[threadIdx.x] = v;
  __syncthreads();
  for (int o = 1; o < tpl; o <<= 1) {
    const bool has = REVERSE ? u + o < tpl : u >= o;
    if (has) {
      const float w = buf[REVERSE ? threadIdx.x + o : threadIdx.x - o];
      v = MAX ? fmaxf(v, w) : v + w;
    }
    __syncthreads();
    buf[threadIdx.x] = v;
    __syncthreads();
  }
  return v;
}

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
  __shared__ float buf[kThreads];
  const int P = pow2_at_least(L);
  const int tpl = P >= kThreads ? kThreads : P;
  const int ept = P / tpl;
  const int lpb = kThreads / tpl;
  const int64_t row0 = (int64_t)blockIdx.x * lpb;
  const int n_slots = lpb * P;
  for (int i = threadIdx.x; i < n_slots; i += kThreads) {
    const int q = i / P, k = i - q * P;
    const int64_t row = row0 + q;
    uint64_t key = 0;                          // padding: below every real pair
    if (k < L && row < batch) {
      const int64_t o = row * L + k;
      float s;
      if constexpr (sizeof(T) == 2) s = bf16_to_f32(logits[row * ld + k]);
      else s = logits[row * ld + k];
      const float y = labels[o];
      const bool valid = y >= 0.0f && (!mask || mask[o]);
      key = ((uint64_t)order_key(valid ? y : kListMleMasked) << 32) | (uint32_t)~(uint32_t)k;
      z[q * L + k] = s * inv_t;
    }
    keys[i] = key;
  }
  __syncthreads();
  // bitonic sort of each P-long segment, descending
  for (int kk = 2; kk <= P; kk <<= 1)
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int p = threadIdx.x; p < n_slots / 2; p += kThreads) {
        const int e = ((p & ~(j - 1)) << 1) | (p & (j - 1));
        const uint64_t a = keys[e], b = keys[e + j];
        const bool desc = ((e & (P - 1)) & kk) == 0;
        if (desc ? a < b : a > b) {
          keys[e] = b;
          keys[e + j] = a;
        }
      }
      __syncthreads();
    }

  const int q = threadIdx.x / tpl, u = threadIdx.x - q * tpl;
  const int64_t row = row0 + q;
  const bool live = row < batch;
  const uint64_t* lk = keys + q * P + u * ept;   // this thread's sorted positions u*ept .. u*ept + ept - 1
  const float* lz = z + q * L;
  // valid: a label >= 0 has the top bit of its order key set; -1e9 (invalid) and padding do not
  bool valid[kEpt];
  float zr[kEpt];
  float zmax = -__builtin_inff(), nvalid = 0.0f;
#pragma unroll
  for (int c = 0; c < kEpt; ++c) {
    valid[c] = false;
    zr[c] = 0.0f;
    if (c < ept && live) {
      const uint64_t key = lk[c];
      valid[c] = (key >> 63) != 0;
      if (valid[c]) {
        zr[c] = lz[~(uint32_t)key];
        zmax = fmaxf(zmax, zr[c]);
        nvalid += 1.0f;
      }
    }
  }
  const int last = threadIdx.x - u + tpl - 1;    // the thread holding a list's inclusive total
  seg_scan<false, true>(buf, zmax, u, tpl);
  const float m_raw = buf[last];
  seg_scan<false, false>(buf, nvalid, u, tpl);
  const bool any_valid = buf[last] > 0.0f;
  const float m = any_valid ? m_raw : 0.0f;
  // ties of the maximum share its gradient (autodiff of max)
  float ties = 0.0f, ez[kEpt];
  bool top[kEpt];
#pragma unroll
  for (int c = 0; c < kEpt; ++c) {
    top[c] = valid[c] && zr[c] == m_raw;
    ties += top[c] ? 1.0f : 0.0f;
    zr[c] = zr[c] - m;                          // sorted_logits - raw_max
    ez[c] = valid[c] ? expf(zr[c]) : 0.0f;
  }
  seg_scan<false, false>(buf, ties, u, tpl);
  const float n_ties = buf[last];
  // E_r: suffix sums of exp, fixed order (within a thread from its last position down, then across threads)
  float tsum = 0.0f;
#pragma unroll
  for (int c = kEpt - 1; c >= 0; --c) tsum += ez[c];
  seg_scan<true, false>(buf, tsum, u, tpl);
  float acc = u + 1 < tpl ? buf[threadIdx.x + 1] : 0.0f;
  float inv[kEpt], lsum = 0.0f, esum = 0.0f, isum = 0.0f;
#pragma unroll
  for (int c = kEpt - 1; c >= 0; --c) {
    acc += ez[c];
    const float den = acc + kListMleEps;
    inv[c] = valid[c] ? 1.0f / den : 0.0f;
    if (valid[c]) {
      lsum += logf(den) - zr[c];
      esum += kListMleEps * inv[c];
    }
  }
  // prefix sums of 1 / (E_r + eps)
#pragma unroll
  for (int c = 0; c < kEpt; ++c) isum += inv[c];
  seg_scan<false, false>(buf, isum, u, tpl);
  float pre = u > 0 ? buf[threadIdx.x - 1] : 0.0f;
  seg_scan<false, false>(buf, lsum, u, tpl);
  const float loss = buf[last];
  seg_scan<false, false>(buf, esum, u, tpl);
  const float dmax = buf[last];   // dl/dm = sum_r eps / (E_r + eps)
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
    const int64_t o = row * L + ~(uint32_t)key;
    if constexpr (sizeof(T) == 2) dlogits[o] = f32_to_bf16(gl * d);
    else dlogits[o] = gl * d;
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
  KRS_REQUIRE(list >= 1 && list <= kMaxList, "%s: list length %lld outside the supported 1..%d (KRS_RANK_MAX_LIST)",
              what, (long long)list, kMaxList);
  KRS_REQUIRE(batch >= 0, "%s: negative batch", what);
  KRS_REQUIRE(ld >= list, "%s: ld %lld below the list length %lld", what, (long long)ld, (long long)list);
  KRS_REQUIRE(dtype == KRS_F32 || dtype == KRS_BF16, "%s: bad dtype", what);
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
  int tpl = 1;
  while (tpl < L && tpl < kThreads) tpl <<= 1;
  const int lpb = kThreads / tpl;
  const dim3 grid((unsigned)ceil_div(batch, lpb));
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
  int P = 1;
  while (P < L) P <<= 1;
  const int lpb = P >= kThreads ? 1 : kThreads / P;
  const dim3 grid((unsigned)ceil_div(batch, lpb));
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
