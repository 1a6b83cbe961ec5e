// K11 -- the retrieval training head: row softmax cross-entropy with its logit gradient in one launch, and the two
// logit corrections that precede it (keras_rs.layers.SamplingProbabilityCorrection, RemoveAccidentalHits).
//
// Replaces keras.losses.CategoricalCrossentropy(from_logits=True) / SparseCategoricalCrossentropy as the reference's
// retrieval examples use them (examples/sequential_retrieval.py:344-360: scores = q c^T, labels = eye(B)),
// sampling_probability_correction.py:56-58 and remove_accidental_hits.py:84-97.
//
//   * softmax_xent_kernel   y' = y (1 - ls) + ls / N (dense labels, or one-hot of label_index), then per row
//                             m = max_j x_j,  Z = sum_j exp(x_j - m),  S = sum_j y'_j,  A = sum_j y'_j (m - x_j)
//                             loss = A + S log Z                       (= sum_j y'_j ((m - x_j) + log Z))
//                             dlogits_j = g (S exp(x_j - m) / Z - y'_j)
//                           Every thread keeps online statistics {m_t, Z_t, S_t, A_t} of its own elements (when m_t
//                           rises by d, Z_t scales by exp(-d) and A_t gains S_t d: every term stays non-negative, no
//                           m S - sum y' x cancellation), the row's threads combine them, and a second walk writes the
//                           gradient.
//   * sampling_correction_kernel      out = x - log(min(max(p, eps), 1)), probs row = logits row mod p_rows
//   * remove_accidental_hits_kernel   pos = first argmax of the row's labels, dup_j = (ids_j == ids_pos),
//                                     out_j = x_j + (dup_j - y_j) * value with every operation rounded on its own
//
// Layout: rows of up to kThreads columns are packed as krs_list.h's ListPack packs lists, one element per thread, the
// row held in registers.  Longer rows take a workgroup each:
//   - cols <= kStageCols = 9216: the row's logits and smoothed labels are staged in LDS as fp32 while the statistics
//     are taken (2 x 36 KiB + 192 B of partials = 73,920 B per workgroup; two workgroups, 147,840 B, fit the CU's
//     160 KiB, and 1024 threads at <= 64 VGPRs leave both resident), so HBM sees logits and labels once;
//   - cols > kStageCols: two streams over the row, statistics first and then the gradient.
// 16-byte loads and stores (4 fp32 / 8 bf16 logits, 4 labels) when every pointer and leading dimension involved is
// 16-byte aligned, scalar accesses otherwise and for a row's last cols % 8 (bf16) or cols % 4 elements.
// Reductions: lane butterflies within a wave, then the wave partials of a row added through LDS in wave order.  No
// atomics, a fixed summation order: repeated calls are bit-identical.  No host synchronisation and no allocation: a
// call can be captured into a HIP graph.
#include "krs_list.h"

namespace krs {
namespace {

constexpr int kThreads = kListThreads;
constexpr int kWaves = kListWaves;
constexpr int kStageCols = 9216;
constexpr float kNegInf = -__builtin_inff();

// 16 bytes of T (kVec<T> elements) at p, which is 16-byte aligned
template <typename T>
constexpr int kVec = 16 / (int)sizeof(T);
template <typename T>
__device__ __forceinline__ void load_vec(const T* p, float (&v)[kVec<T>]) {
  if constexpr (sizeof(T) == 2) {
    const uint4 r = *reinterpret_cast<const uint4*>(p);
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = __uint_as_float(w[i] << 16);
      v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
  } else {
    const float4 r = *reinterpret_cast<const float4*>(p);
    v[0] = r.x, v[1] = r.y, v[2] = r.z, v[3] = r.w;
  }
}
template <typename T>
__device__ __forceinline__ void store_vec(T* p, const float (&v)[kVec<T>]) {
  if constexpr (sizeof(T) == 2) {
    *reinterpret_cast<uint4*>(p) = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]),
                                              pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
  } else {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  }
}
template <int N>
__device__ __forceinline__ void load_f32(const float* p, float (&v)[N]) {
#pragma unroll
  for (int i = 0; i < N; i += 4) {
    const float4 r = *reinterpret_cast<const float4*>(p + i);
    v[i] = r.x, v[i + 1] = r.y, v[i + 2] = r.z, v[i + 3] = r.w;
  }
}
template <int N>
__device__ __forceinline__ void store_f32(float* p, const float (&v)[N]) {
#pragma unroll
  for (int i = 0; i < N; i += 4) *reinterpret_cast<float4*>(p + i) = make_float4(v[i], v[i + 1], v[i + 2], v[i + 3]);
}

// All-reduce of K values over the `tpr` threads of a row (tpr a power of two, rows aligned to it; tpr and the call
// are uniform over the workgroup).  Lane butterflies up to the wave; beyond it the row's wave partials go through
// `red` [K][kWaves] and every thread adds them in wave order, ((a + b) + c) + d: seg_all_reduce's butterfly over the
// partials would change low bits of the loss and the gradient for rows of four waves or more.
template <bool MAX, int K>
__device__ __forceinline__ void row_all_reduce(float (&v)[K], float* red, int tpr) {
  const int width = tpr < 64 ? tpr : 64;
  for (int o = 1; o < width; o <<= 1) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float w = __shfl_xor(v[k], o, 64);
      v[k] = MAX ? fmaxf(v[k], w) : v[k] + w;
    }
  }
  if (tpr > 64) {
    const int wave = threadIdx.x >> 6;
    __syncthreads();   // (the previous reduction's partials have been read)
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int k = 0; k < K; ++k) red[k * kWaves + wave] = v[k];
    }
    __syncthreads();
    const int wpr = tpr >> 6, w0 = (wave / wpr) * wpr;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float a = red[k * kWaves + w0];
      for (int i = 1; i < wpr; ++i) a = MAX ? fmaxf(a, red[k * kWaves + w0 + i]) : a + red[k * kWaves + w0 + i];
      v[k] = a;
    }
  }
}

// ---- softmax cross-entropy ------------------------------------------------------------------------------------------
struct RowStats {
  float m = kNegInf, z = 0.0f, s = 0.0f, a = 0.0f;
  // raises the running maximum to at least `top` (the largest of the elements about to be added)
  __device__ __forceinline__ void lift(float top) {
    const float mn = fmaxf(m, top);
    if (mn > m) {
      z *= __expf(m - mn);                 // exp(-inf) = 0 on the first lift, where z is 0 anyway
      if (m > kNegInf) a += s * (mn - m);
      m = mn;
    }
  }
  __device__ __forceinline__ void add(float x, float y) {
    z += __expf(x - m);
    s += y;
    a += y * (m - x);
  }
};

template <typename T, bool SPARSE>
__global__ __launch_bounds__(kThreads) void softmax_xent_kernel(const T* __restrict__ logits, int64_t ldx,
                                                                const float* __restrict__ labels, int64_t ldl,
                                                                const int32_t* __restrict__ label_index, float ls,
                                                                const float* __restrict__ g, float g_scale,
                                                                int64_t rows, int cols, int vec_ok,
                                                                float* __restrict__ row_loss, T* __restrict__ dlogits,
                                                                int64_t ldd) {
  constexpr int V = kVec<T>;
  __shared__ __attribute__((aligned(16))) float sx[kStageCols];
  __shared__ __attribute__((aligned(16))) float sy[SPARSE ? 4 : kStageCols];
  __shared__ float red[3 * kWaves];
  const float keep = 1.0f - ls, spread = ls / (float)cols;
  const bool packed = cols <= kThreads;
  // ListPack's tpl and lpb (the host launches by it), written out: with tpr a constant on the staged and streamed
  // paths the kernel measured 1-2 % faster at (8192, 8192) than with the struct's.
  int tpr = kThreads;
  if (packed) tpr = pow2_at_least(cols);
  const int rpb = kThreads / tpr;
  const int q = threadIdx.x / tpr, u = threadIdx.x - q * tpr;
  const int64_t row = (int64_t)blockIdx.x * rpb + q;
  const bool live = row < rows;
  const bool staged = !packed && cols <= kStageCols;
  const T* x = logits + (live ? row : 0) * ldx;
  const float* yrow = SPARSE ? nullptr : labels + (live ? row : 0) * ldl;
  int hot = -1;
  bool bad = false;
  if (SPARSE && live) {
    hot = label_index[row];
    bad = hot < 0 || hot >= cols;
  }
  auto smooth = [&](float y) { return y * keep + spread; };
  auto label_at = [&](int j) { return smooth(SPARSE ? (j == hot ? 1.0f : 0.0f) : yrow[j]); };

  // ---- statistics ----
  RowStats st;
  float x0 = 0.0f, y0 = 0.0f;          // the packed path's one element
  const int nvec = (!packed && vec_ok) ? cols / V : 0;
  if (packed) {
    if (live && u < cols) {
      x0 = load1(x + u);
      y0 = label_at(u);
      st.lift(x0);
      st.add(x0, y0);
    }
  } else {
    for (int c = u; c < nvec; c += kThreads) {
      const int j = c * V;
      float xv[V], yv[V];
      load_vec(x + j, xv);
      if constexpr (SPARSE) {
#pragma unroll
        for (int i = 0; i < V; ++i) yv[i] = j + i == hot ? 1.0f : 0.0f;
      } else {
        load_f32(yrow + j, yv);
      }
      float top = xv[0];
#pragma unroll
      for (int i = 0; i < V; ++i) {
        yv[i] = smooth(yv[i]);
        top = fmaxf(top, xv[i]);
      }
      st.lift(top);
#pragma unroll
      for (int i = 0; i < V; ++i) st.add(xv[i], yv[i]);
      if (staged) {
        store_f32(sx + j, xv);
        if constexpr (!SPARSE) store_f32(sy + j, yv);
      }
    }
    for (int j = nvec * V + u; j < cols; j += kThreads) {   // (a thread reads back from LDS only what it stored)
      const float xs = load1(x + j), ys = label_at(j);
      st.lift(xs);
      st.add(xs, ys);
      if (staged) {
        sx[j] = xs;
        if constexpr (!SPARSE) sy[j] = ys;
      }
    }
  }
  float mx[1] = {st.m};
  row_all_reduce<true, 1>(mx, red, tpr);
  const float m = mx[0];
  float sums[3] = {st.z * __expf(st.m - m), st.s, st.m > kNegInf ? st.a + st.s * (m - st.m) : 0.0f};
  row_all_reduce<false, 3>(sums, red, tpr);
  if (!live) return;
  const float Z = sums[0], S = sums[1];
  if (u == 0 && row_loss) row_loss[row] = bad ? quiet_nan() : sums[2] + S * logf(Z);
  if (!dlogits) return;

  // ---- gradient ----
  // (expf, not the fast intrinsic: the latter flushes a subnormal exp(x - m) to zero, and S / Z may be far above 1)
  const float gr = bad ? quiet_nan() : (g ? g_scale * g[row] : g_scale);
  const float c = gr * (S / Z);
  T* dx = dlogits + row * ldd;
  if (packed) {
    if (u < cols) store1(dx + u, c * expf(x0 - m) - gr * y0);
    return;
  }
  for (int cidx = u; cidx < nvec; cidx += kThreads) {
    const int j = cidx * V;
    float xv[V], yv[V];
    if (staged) {
      load_f32(sx + j, xv);
      if constexpr (!SPARSE) load_f32(sy + j, yv);
    } else {
      load_vec(x + j, xv);
      if constexpr (!SPARSE) {
        load_f32(yrow + j, yv);
#pragma unroll
        for (int i = 0; i < V; ++i) yv[i] = smooth(yv[i]);
      }
    }
    if constexpr (SPARSE) {
#pragma unroll
      for (int i = 0; i < V; ++i) yv[i] = smooth(j + i == hot ? 1.0f : 0.0f);
    }
#pragma unroll
    for (int i = 0; i < V; ++i) xv[i] = c * expf(xv[i] - m) - gr * yv[i];
    store_vec(dx + j, xv);
  }
  for (int j = nvec * V + u; j < cols; j += kThreads) {
    const float xs = staged ? sx[j] : load1(x + j);
    const float ys = (staged && !SPARSE) ? sy[j] : label_at(j);
    store1(dx + j, c * expf(xs - m) - gr * ys);
  }
}

// ---- sampling probability correction --------------------------------------------------------------------------------
// one chunk of kVec<T> columns per thread
template <typename T>
__global__ __launch_bounds__(256) void sampling_correction_kernel(const T* __restrict__ logits, int64_t ldx,
                                                                  const float* __restrict__ probs, int64_t p_rows,
                                                                  float eps, int64_t rows, int cols, int vec_ok,
                                                                  T* __restrict__ out, int64_t ldo) {
  constexpr int V = kVec<T>;
  const int cpr = (cols + V - 1) / V;   // chunks per row
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= rows * cpr) return;
  const int64_t row = t / cpr;
  const int j = (int)(t - row * cpr) * V;
  const T* x = logits + row * ldx + j;
  const float* p = probs + (row % p_rows) * cols + j;
  T* o = out + row * ldo + j;
  if (vec_ok && j + V <= cols) {
    float xv[V], pv[V];
    load_vec(x, xv);
    load_f32(p, pv);
#pragma unroll
    for (int i = 0; i < V; ++i) xv[i] = xv[i] - logf(fminf(fmaxf(pv[i], eps), 1.0f));
    store_vec(o, xv);
  } else {
    const int n = cols - j < V ? cols - j : V;
    for (int i = 0; i < n; ++i) store1(o + i, load1(x + i) - logf(fminf(fmaxf(p[i], eps), 1.0f)));
  }
}

// ---- remove accidental hits -------------------------------------------------------------------------------------------
template <typename T, typename I>
__global__ __launch_bounds__(kThreads) void remove_accidental_hits_kernel(const T* __restrict__ logits, int64_t ldx,
                                                                          const float* __restrict__ labels,
                                                                          int64_t ldl, const I* __restrict__ ids,
                                                                          int64_t id_rows, float value, int64_t rows,
                                                                          int cols, T* __restrict__ out, int64_t ldo) {
  __shared__ unsigned long long red[kWaves];
  const ListPack lp(cols);
  const int tpr = lp.tpl;
  const int u = lp.u();
  const int64_t row = lp.row0() + lp.q();
  const bool live = row < rows;
  const float* y = labels + (live ? row : 0) * ldl;
  // first index of the largest label: the largest (order key, ~index) pair; 0 (no element) is below every pair
  unsigned long long best = 0;
  if (live)
    for (int j = u; j < cols; j += tpr) {
      const unsigned long long key = pair_key(order_key(y[j]), (uint32_t)j);
      best = key > best ? key : best;
    }
  const int width = tpr < 64 ? tpr : 64;
  for (int o = 1; o < width; o <<= 1) {
    const unsigned long long w = __shfl_xor(best, o, 64);
    best = w > best ? w : best;
  }
  if (tpr > 64) {   // (uniform over the workgroup) the partials of the row's waves
    const int wave = threadIdx.x >> 6, wpr = tpr >> 6, w0 = (wave / wpr) * wpr;
    if ((threadIdx.x & 63) == 0) red[wave] = best;
    __syncthreads();
    best = red[w0];
    for (int i = 1; i < wpr; ++i) best = red[w0 + i] > best ? red[w0 + i] : best;
  }
  if (!live) return;
  const int pos = (int)pair_index(best);         // < cols: every live row has cols >= 1 elements
  const I* idr = ids + (row % id_rows) * cols;
  const I id_pos = idr[pos];
  const T* x = logits + row * ldx;
  T* o = out + row * ldo;
  for (int j = u; j < cols; j += tpr) {
    const float dup = idr[j] == id_pos ? 1.0f : 0.0f;
    store1(o + j, __fadd_rn(load1(x + j), __fmul_rn(__fsub_rn(dup, y[j]), value)));
  }
}

inline int rows_per_block(int64_t cols) { return ListPack((int)cols).lpb; }   // (cols <= 2^30)

int check_matrix(const char* what, const void* logits, int64_t ld, int dtype, int64_t rows, int64_t cols) {
  KRS_REQUIRE(rows >= 0, "%s: negative row count", what);
  KRS_REQUIRE(cols >= 1 && cols <= (1ll << 30), "%s: %lld columns outside the supported 1..2^30", what,
              (long long)cols);
  KRS_REQUIRE(dtype == KRS_F32 || dtype == KRS_BF16, "%s: bad dtype %d", what, dtype);
  KRS_REQUIRE(ld >= cols, "%s: ld %lld below the column count %lld", what, (long long)ld, (long long)cols);
  KRS_REQUIRE(ceil_div(rows, rows_per_block(cols)) <= 0x7fffffff, "%s: too many rows", what);
  KRS_REQUIRE(rows == 0 || logits, "%s: null logits", what);
  return KRS_OK;
}

template <typename T>
void launch_xent(dim3 grid, hipStream_t st, const void* logits, int64_t ld, const float* labels, int64_t ldl,
                 const int32_t* label_index, float ls, const float* g, float g_scale, int64_t rows, int cols,
                 float* row_loss, void* dlogits, int64_t ldd) {
  constexpr int V = kVec<T>;
  const T* x = reinterpret_cast<const T*>(logits);
  T* dx = reinterpret_cast<T*>(dlogits);
  const int vec_ok = aligned16(x) && ld % V == 0 && (!labels || (aligned16(labels) && ldl % 4 == 0)) &&
                     (!dx || (aligned16(dx) && ldd % V == 0));
  if (label_index)
    hipLaunchKernelGGL((softmax_xent_kernel<T, true>), grid, dim3(kThreads), 0, st, x, ld, labels, ldl, label_index,
                       ls, g, g_scale, rows, cols, vec_ok, row_loss, dx, ldd);
  else
    hipLaunchKernelGGL((softmax_xent_kernel<T, false>), grid, dim3(kThreads), 0, st, x, ld, labels, ldl, label_index,
                       ls, g, g_scale, rows, cols, vec_ok, row_loss, dx, ldd);
}

template <typename T>
void launch_correction(hipStream_t st, const void* logits, int64_t ld, const float* probs, int64_t p_rows, float eps,
                       int64_t rows, int cols, void* out, int64_t ldo) {
  constexpr int V = kVec<T>;
  const int vec_ok = aligned16(logits) && ld % V == 0 && aligned16(out) && ldo % V == 0 && aligned16(probs) &&
                     cols % 4 == 0;
  const int64_t chunks = rows * ceil_div(cols, V);
  hipLaunchKernelGGL(sampling_correction_kernel<T>, dim3((unsigned)ceil_div(chunks, 256)), dim3(256), 0, st,
                     reinterpret_cast<const T*>(logits), ld, probs, p_rows, eps, rows, cols, vec_ok,
                     reinterpret_cast<T*>(out), ldo);
}

template <typename T, typename I>
void launch_hits(dim3 grid, hipStream_t st, const void* logits, int64_t ld, const float* labels, int64_t ldl,
                 const void* ids, int64_t id_rows, float value, int64_t rows, int cols, void* out, int64_t ldo) {
  hipLaunchKernelGGL((remove_accidental_hits_kernel<T, I>), grid, dim3(kThreads), 0, st,
                     reinterpret_cast<const T*>(logits), ld, labels, ldl, reinterpret_cast<const I*>(ids), id_rows,
                     value, rows, cols, reinterpret_cast<T*>(out), ldo);
}

}  // namespace
}  // namespace krs

extern "C" int krs_softmax_xent(const void* logits, int64_t ld, int dtype, const float* labels, int64_t ld_labels,
                                const int32_t* label_index, float label_smoothing, const float* g, float g_scale,
                                int64_t rows, int64_t cols, float* row_loss, void* dlogits, int64_t ld_dlogits,
                                void* stream) {
  using namespace krs;
  const char* what = "krs_softmax_xent";
  const int rc = check_matrix(what, logits, ld, dtype, rows, cols);
  if (rc != KRS_OK) return rc;
  KRS_REQUIRE(label_smoothing >= 0.0f && label_smoothing < 1.0f, "%s: label_smoothing %g outside [0, 1)", what,
              (double)label_smoothing);
  KRS_REQUIRE((labels != nullptr) != (label_index != nullptr),
              "%s: exactly one of labels and label_index must be given", what);
  KRS_REQUIRE(!labels || ld_labels >= cols, "%s: ld_labels %lld below the column count %lld", what,
              (long long)ld_labels, (long long)cols);
  KRS_REQUIRE(row_loss || dlogits, "%s: neither the loss nor the gradient is wanted", what);
  KRS_REQUIRE(!dlogits || ld_dlogits >= cols, "%s: ld_dlogits %lld below the column count %lld", what,
              (long long)ld_dlogits, (long long)cols);
  if (rows == 0) return KRS_OK;
  const dim3 grid((unsigned)ceil_div(rows, rows_per_block(cols)));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == KRS_BF16)
    launch_xent<uint16_t>(grid, st, logits, ld, labels, ld_labels, label_index, label_smoothing, g, g_scale, rows,
                          (int)cols, row_loss, dlogits, ld_dlogits);
  else
    launch_xent<float>(grid, st, logits, ld, labels, ld_labels, label_index, label_smoothing, g, g_scale, rows,
                       (int)cols, row_loss, dlogits, ld_dlogits);
  KRS_CHECK_LAUNCH(what);
  return KRS_OK;
}

extern "C" int krs_sampling_correction(const void* logits, int64_t ld, int dtype, const float* probs, int64_t p_rows,
                                       float epsilon, int64_t rows, int64_t cols, void* out, int64_t ld_out,
                                       void* stream) {
  using namespace krs;
  const char* what = "krs_sampling_correction";
  const int rc = check_matrix(what, logits, ld, dtype, rows, cols);
  if (rc != KRS_OK) return rc;
  KRS_REQUIRE(p_rows >= 1, "%s: p_rows %lld must be at least 1", what, (long long)p_rows);
  KRS_REQUIRE(ld_out >= cols, "%s: ld_out %lld below the column count %lld", what, (long long)ld_out,
              (long long)cols);
  KRS_REQUIRE(rows == 0 || (probs && out), "%s: null argument", what);
  KRS_REQUIRE(ceil_div(rows * ceil_div(cols, 4), 256) <= 0x7fffffff, "%s: too many elements for one launch", what);
  if (rows == 0) return KRS_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == KRS_BF16) launch_correction<uint16_t>(st, logits, ld, probs, p_rows, epsilon, rows, (int)cols, out, ld_out);
  else launch_correction<float>(st, logits, ld, probs, p_rows, epsilon, rows, (int)cols, out, ld_out);
  KRS_CHECK_LAUNCH(what);
  return KRS_OK;
}

extern "C" int krs_remove_accidental_hits(const void* logits, int64_t ld, int dtype, const float* labels,
                                          int64_t ld_labels, const void* ids, int id_dtype, int64_t id_rows,
                                          float value, int64_t rows, int64_t cols, void* out, int64_t ld_out,
                                          void* stream) {
  using namespace krs;
  const char* what = "krs_remove_accidental_hits";
  const int rc = check_matrix(what, logits, ld, dtype, rows, cols);
  if (rc != KRS_OK) return rc;
  KRS_REQUIRE(id_dtype == KRS_I32 || id_dtype == KRS_I64, "%s: bad id dtype %d", what, id_dtype);
  KRS_REQUIRE(id_rows >= 1, "%s: id_rows %lld must be at least 1", what, (long long)id_rows);
  KRS_REQUIRE(ld_labels >= cols && ld_out >= cols, "%s: a leading dimension is below the column count %lld", what,
              (long long)cols);
  KRS_REQUIRE(rows == 0 || (labels && ids && out), "%s: null argument", what);
  if (rows == 0) return KRS_OK;
  const dim3 grid((unsigned)ceil_div(rows, rows_per_block(cols)));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool bf = dtype == KRS_BF16, i64 = id_dtype == KRS_I64;
  if (bf && i64) launch_hits<uint16_t, int64_t>(grid, st, logits, ld, labels, ld_labels, ids, id_rows, value, rows, (int)cols, out, ld_out);
  else if (bf) launch_hits<uint16_t, int32_t>(grid, st, logits, ld, labels, ld_labels, ids, id_rows, value, rows, (int)cols, out, ld_out);
  else if (i64) launch_hits<float, int64_t>(grid, st, logits, ld, labels, ld_labels, ids, id_rows, value, rows, (int)cols, out, ld_out);
  else launch_hits<float, int32_t>(grid, st, logits, ld, labels, ld_labels, ids, id_rows, value, rows, (int)cols, out, ld_out);
  KRS_CHECK_LAUNCH(what);
  return KRS_OK;
}
