// K24 -- the regression head: MSE / MAE / Huber loss with its Keras reduction, the gradient to the predictions and the
// batch sums of the regression metrics, from ONE read of the predictions.
//
// Replaces keras.losses.MeanSquaredError / MeanAbsoluteError / Huber and the update of
// keras.metrics.RootMeanSquaredError / MeanSquaredError / MeanAbsoluteError as the reference's rating examples compile
// them (examples/basic_ranking.py, listwise_ranking.py, multi_task.py: loss = MeanSquaredError(),
// metrics = [RootMeanSquaredError()]).  The contract -- the fp32 operation order of an element, a row and the gradient,
// the reductions and the summation order -- is include/krs.h's (K24) and is restated in numpy by
// tests/regression_restatement.py; nothing here may be contracted into an fma:
#pragma clang fp contract(off)
//
// K7's scheme (loss.hip) at full width: per-thread sums over a fixed stride, a fixed-order halving tree in LDS per
// workgroup, one partial per workgroup and sum added in workgroup order -- by the main kernel itself when one workgroup
// does all the work, by regression_finish_kernel otherwise.  No float atomics, no host wait.  The gradient's row
// coefficient k_b needs no row sum, so a row's columns are walked once; MEAN_WITH_SAMPLE_WEIGHT needs W = sum w before
// the first gradient, which regression_wsum_kernel takes from the b weights alone (each workgroup of the main kernel
// then adds the W partials in workgroup order: the same bits in every workgroup).
//
// Two builds per dtype (regression_plan.h chooses): the vector build for the contiguous [b, 1] rating head moves 16
// bytes per lane (4 fp32 / 8 bf16 rows an item), the element build walks any [b, c] with any strides and bases.
#include "krs_common.h"
#include "regression_plan.h"

namespace krs {
namespace {

constexpr int kThreads = KRS_REGRESSION_THREADS;
constexpr int kSums = regr::kSums;

struct Args {
  const void* pred;
  const float* target;
  const float* w;
  const float* g;
  float* loss;          // [b] under NONE, [1] otherwise, or NULL
  void* dpred;
  float* sums;          // [3] or NULL
  const float* w_partials;   // W pass ran: its w_blocks partials
  float* partials;      // [kSums][gridDim.x], used when gridDim.x > 1
  int64_t ldp, ldt, ldd, b, items;
  int c, tail, w_blocks;
  int kind, reduction;
  float delta, g_scale, phi, count;   // phi: 1 / float(b) where the reduction divides by the batch size, else 1
};

// one correctly rounded fp32 division: what hipcc makes of `/` (v_div_scale / v_div_fmas / v_div_fixup), kept in one
// place because the contract counts on it
__device__ __forceinline__ float div_rn(float x, float y) { return x / y; }

__device__ __forceinline__ float sign_of(float e) { return e != e ? e : (float)(e > 0.0f) - (float)(e < 0.0f); }

// one element: f (the loss term), d (f'), q = e * e, a = |e|
struct Element {
  float f, d, q, a;
};
__device__ __forceinline__ Element element(float p, float y, int kind, float delta) {
  const float e = p - y;
  const float q = e * e, a = fabsf(e), sg = sign_of(e);
  const bool mse = kind == KRS_REGRESSION_MSE, mae = kind == KRS_REGRESSION_MAE, inside = a <= delta;
  Element el;
  el.f = mse ? q : mae ? a : inside ? 0.5f * q : delta * a - 0.5f * (delta * delta);
  el.d = mse ? e + e : mae ? sg : inside ? e : delta * sg;
  el.q = q, el.a = a;
  return el;
}

// s_b of krs.h from the row's weight (1 without weights)
__device__ __forceinline__ float row_share(const Args& a, bool by_w, float W, float wb) {
  if (by_w) return W != 0.0f ? div_rn(wb, W) : 0.0f;
  return a.w ? wb * a.phi : a.phi;
}

// adds a finished row to the thread's sums; returns t_b
__device__ __forceinline__ float row_sums(const Args& a, float cf, float r, float q, float ab, float wb,
                                          float& st, float& sq, float& sa, float& sw) {
  const float v = div_rn(r, cf);
  const float t = a.w ? wb * v : v;
  const bool weighted = a.w != nullptr;
  st += t;
  sq += weighted ? wb * div_rn(q, cf) : q;
  sa += weighted ? wb * div_rn(ab, cf) : ab;
  sw += wb;                                   // (read only with weights)
  return t;
}

// the outputs of a call from the four totals
__device__ __forceinline__ void finalize(const Args& a, float W, float t, float q, float ab, float w) {
  if (a.loss && a.reduction != KRS_REGRESSION_NONE) {
    if (a.w_partials) a.loss[0] = W != 0.0f ? div_rn(t, W) : 0.0f;
    else a.loss[0] = t * a.phi;
  }
  if (a.sums) {
    a.sums[0] = q;
    a.sums[1] = ab;
    a.sums[2] = a.w ? w : a.count;
  }
}

// one row of c columns through element accesses
template <typename T>
__device__ __forceinline__ void walk_row(const Args& a, int64_t row, float cf, bool by_w, float W,
                                         float& st, float& sq, float& sa, float& sw) {
  const T* p = reinterpret_cast<const T*>(a.pred) + row * a.ldp;
  const float* y = a.target + row * a.ldt;
  T* dp = a.dpred ? reinterpret_cast<T*>(a.dpred) + row * a.ldd : nullptr;
  const float wb = a.w ? a.w[row] : 1.0f;
  float k = 0.0f;
  if (dp) k = div_rn((a.g ? a.g[row] : a.g_scale) * row_share(a, by_w, W, wb), cf);
  float r = 0.0f, q = 0.0f, ab = 0.0f;
  for (int j = 0; j < a.c; ++j) {
    const Element el = element(load1(p + j), y[j], a.kind, a.delta);
    r += el.f, q += el.q, ab += el.a;
    if (dp) store1(dp + j, k * el.d);
  }
  const float t = row_sums(a, cf, r, q, ab, wb, st, sq, sa, sw);
  if (a.loss && a.reduction == KRS_REGRESSION_NONE) a.loss[row] = t;
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

template <typename T, bool VEC>
__global__ __launch_bounds__(kThreads) void regression_kernel(const Args a) {
  constexpr int V = VEC ? 16 / (int)sizeof(T) : 1;
  __shared__ float part[kSums][kThreads];
  __shared__ float w_total;
  const bool by_w = a.w_partials != nullptr;
  float W = 0.0f;
  if (by_w) {
    if (threadIdx.x == 0) {
      float s = 0.0f;
      for (int j = 0; j < a.w_blocks; ++j) s += a.w_partials[j];     // workgroup order
      w_total = s;
    }
    __syncthreads();
    W = w_total;
  }
  const float cf = (float)a.c;
  float st = 0.0f, sq = 0.0f, sa = 0.0f, sw = 0.0f;      // this thread's share of T, sum q, sum a, sum w
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t it = (int64_t)blockIdx.x * kThreads + threadIdx.x; it < a.items; it += stride) {
    if constexpr (VEC) {       // V rows of one column, every stride 1
      const int64_t r0 = it * V;
      float p[V], y[V], wv[V], gv[V], out[V];
      if constexpr (sizeof(T) == 2) {
        const uint4 raw = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(a.pred) + r0);
        const uint32_t u[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          p[2 * i] = __uint_as_float(u[i] << 16);
          p[2 * i + 1] = __uint_as_float(u[i] & 0xffff0000u);
        }
      } else {
        load_f32(reinterpret_cast<const float*>(a.pred) + r0, p);
      }
      load_f32(a.target + r0, y);
      if (a.w) load_f32(a.w + r0, wv);
      if (a.g) load_f32(a.g + r0, gv);
#pragma unroll
      for (int i = 0; i < V; ++i) {
        const float wb = a.w ? wv[i] : 1.0f;
        const Element el = element(p[i], y[i], a.kind, a.delta);
        if (a.dpred) {
          const float k = div_rn((a.g ? gv[i] : a.g_scale) * row_share(a, by_w, W, wb), cf);
          p[i] = k * el.d;
        }
        out[i] = row_sums(a, cf, 0.0f + el.f, 0.0f + el.q, 0.0f + el.a, wb, st, sq, sa, sw);
      }
      if (a.dpred) {
        if constexpr (sizeof(T) == 2)
          *reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(a.dpred) + r0) =
              make_uint4(pack_bf16x2(p[0], p[1]), pack_bf16x2(p[2], p[3]), pack_bf16x2(p[4], p[5]),
                         pack_bf16x2(p[6], p[7]));
        else
          store_f32(reinterpret_cast<float*>(a.dpred) + r0, p);
      }
      if (a.loss && a.reduction == KRS_REGRESSION_NONE) store_f32(a.loss + r0, out);
    } else {
      walk_row<T>(a, it, cf, by_w, W, st, sq, sa, sw);
    }
  }
  if (VEC && blockIdx.x == 0 && (int)threadIdx.x < a.tail)      // the rows after the last full item
    walk_row<T>(a, a.items * V + threadIdx.x, cf, by_w, W, st, sq, sa, sw);

  part[0][threadIdx.x] = st, part[1][threadIdx.x] = sq, part[2][threadIdx.x] = sa, part[3][threadIdx.x] = sw;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
#pragma unroll
      for (int k = 0; k < kSums; ++k) part[k][threadIdx.x] += part[k][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (gridDim.x > 1) {
#pragma unroll
      for (int k = 0; k < kSums; ++k) a.partials[k * gridDim.x + blockIdx.x] = part[k][0];
    } else {
      finalize(a, W, part[0][0], part[1][0], part[2][0], part[3][0]);
    }
  }
}

// the partials of `blocks` > 1 workgroups added in workgroup order
__global__ __launch_bounds__(KRS_REGRESSION_MAX_BLOCKS) void regression_finish_kernel(const Args a, int blocks) {
  __shared__ float part[kSums][KRS_REGRESSION_MAX_BLOCKS];
  __shared__ float tot_s[kSums + 1];
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < kSums; ++k) part[k][t] = t < blocks ? a.partials[k * blocks + t] : 0.0f;
  __syncthreads();
  if (t < kSums) {
    float s = 0.0f;
    for (int j = 0; j < blocks; ++j) s += part[t][j];
    tot_s[t] = s;
  } else if (t == kSums) {
    float s = 0.0f;
    for (int j = 0; j < a.w_blocks; ++j) s += a.w_partials[j];
    tot_s[kSums] = s;
  }
  __syncthreads();
  if (t == 0) {
    finalize(a, tot_s[kSums], tot_s[0], tot_s[1], tot_s[2], tot_s[3]);
  }
}

// W pass: the element route's order over the b weights
__global__ __launch_bounds__(kThreads) void regression_wsum_kernel(const float* __restrict__ w, int64_t b,
                                                                   float* __restrict__ partials) {
  __shared__ float part[kThreads];
  float acc = 0.0f;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < b; i += (int64_t)gridDim.x * kThreads) acc += w[i];
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = part[0];
}

thread_local krs_regression_route g_route = {};

regr::Call call_of(int reduction, const void* pred, int64_t ld_pred, int dtype, const float* target, int64_t ld_target,
                   const float* sample_weight, int64_t b, int64_t c, const float* g, const float* loss,
                   const void* dpred, int64_t ld_dpred) {
  regr::Call call;
  call.reduction = reduction, call.dtype = dtype, call.b = b, call.c = c;
  call.ld_pred = ld_pred, call.ld_target = ld_target, call.ld_dpred = ld_dpred;
  call.pred = pred, call.target = target, call.weight = sample_weight, call.g = g, call.loss = loss, call.dpred = dpred;
  return call;
}

int refuse(const regr::Plan& pl, const regr::Call& c) {
  return fail(pl.status,
              "krs_regression_fwd_bwd: bad %s (reduction %d, dtype %d, b %lld, c %lld, ld_pred %lld, ld_target %lld, "
              "ld_dpred %lld, pred %p, target %p)",
              pl.why, c.reduction, c.dtype, (long long)c.b, (long long)c.c, (long long)c.ld_pred, (long long)c.ld_target,
              (long long)c.ld_dpred, c.pred, c.target);
}

}  // namespace
}  // namespace krs

extern "C" size_t krs_regression_workspace_bytes(int64_t b, int64_t c) { return krs::regr::workspace_bytes(b, c); }

extern "C" int krs_regression_last_route(krs_regression_route* route) {
  if (route) *route = krs::g_route;
  return krs::g_route.kernel;
}

extern "C" int krs_regression_plan_route(int reduction, const void* pred, int64_t ld_pred, int dtype,
                                         const float* target, int64_t ld_target, const float* sample_weight, int64_t b,
                                         int64_t c, const float* g, const float* loss, const void* dpred,
                                         int64_t ld_dpred, krs_regression_route* route) {
  using namespace krs;
  const regr::Call call = call_of(reduction, pred, ld_pred, dtype, target, ld_target, sample_weight, b, c, g, loss,
                                  dpred, ld_dpred);
  const regr::Plan pl = regr::plan(call);
  if (route) *route = pl.route;
  return pl.status == KRS_OK ? KRS_OK : refuse(pl, call);
}

extern "C" int krs_regression_fwd_bwd(int kind, float delta, int reduction, const void* pred, int64_t ld_pred, int dtype,
                                      const float* target, int64_t ld_target, const float* sample_weight, int64_t b,
                                      int64_t c, const float* g, float g_scale, float* loss, void* dpred,
                                      int64_t ld_dpred, float* sums, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  using namespace krs;
  const char* what = "krs_regression_fwd_bwd";
  g_route = {};
  KRS_REQUIRE(kind >= KRS_REGRESSION_MSE && kind <= KRS_REGRESSION_HUBER, "%s: bad kind %d", what, kind);
  KRS_REQUIRE(kind != KRS_REGRESSION_HUBER || delta > 0.0f, "%s: delta %g must be positive", what, (double)delta);
  const regr::Call call = call_of(reduction, pred, ld_pred, dtype, target, ld_target, sample_weight, b, c, g, loss,
                                  dpred, ld_dpred);
  const regr::Plan pl = regr::plan(call);
  if (pl.status != KRS_OK) return refuse(pl, call);
  if (b == 0) return KRS_OK;
  KRS_REQUIRE(loss || dpred || sums, "%s: null outputs: none of loss, dpred and sums is wanted", what);
  const size_t need = regr::workspace_bytes(b, c);
  if (!workspace || workspace_bytes < need)
    return fail(KRS_ERR_WORKSPACE, "%s: workspace of %zu bytes at %p, %zu needed", what, workspace_bytes, workspace,
                need);
  float* ws = reinterpret_cast<float*>(workspace);
  Args a = {};
  a.pred = pred, a.target = target, a.w = sample_weight, a.g = g, a.loss = loss, a.dpred = dpred, a.sums = sums;
  a.w_partials = pl.w_pass ? ws : nullptr;
  a.partials = ws + KRS_REGRESSION_MAX_BLOCKS;
  a.ldp = ld_pred, a.ldt = ld_target, a.ldd = ld_dpred, a.b = b, a.items = pl.items;
  a.c = (int)c, a.tail = (int)pl.tail, a.w_blocks = pl.w_blocks;
  a.kind = kind, a.reduction = reduction;
  a.delta = delta, a.g_scale = g_scale;
  const bool over_b = reduction == KRS_REGRESSION_SUM_OVER_BATCH_SIZE ||
                      (reduction == KRS_REGRESSION_MEAN_WITH_SAMPLE_WEIGHT && !sample_weight);
  a.phi = over_b ? 1.0f / (float)b : 1.0f;
  a.count = (float)(b * c);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (pl.w_pass)
    hipLaunchKernelGGL(regression_wsum_kernel, dim3(pl.w_blocks), dim3(kThreads), 0, st, sample_weight, b, ws);
  const dim3 grid(pl.route.blocks), block(kThreads);
  const bool vec = pl.route.kernel == KRS_REGRESSION_VEC;
  if (dtype == KRS_BF16) {
    if (vec) hipLaunchKernelGGL((regression_kernel<uint16_t, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((regression_kernel<uint16_t, false>), grid, block, 0, st, a);
  } else {
    if (vec) hipLaunchKernelGGL((regression_kernel<float, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((regression_kernel<float, false>), grid, block, 0, st, a);
  }
  if (pl.route.blocks > 1)
    hipLaunchKernelGGL(regression_finish_kernel, dim3(1), dim3(KRS_REGRESSION_MAX_BLOCKS), 0, st, a, pl.route.blocks);
  KRS_CHECK_LAUNCH(what);
  g_route = pl.route;
  return KRS_OK;
}
