// K22: fused residual add + dropout + layer norm over the rows of [n, d], forward and backward (the arithmetic is fixed
// in include/krs.h; ln_plan.h decides every route).
//
// A row is owned by lanes_per_row = 8, 16, 32 or 64 lanes of one wave and sits in fp32 registers from its one load to
// its stores: both statistics passes, the normalisation and, in the backward, the two row sums run on registers, with
// __shfl_xor inside the row's lanes.  A workgroup of 4 waves has 256 / lanes_per_row rows in flight and walks its
// contiguous block of rows pass by pass; gamma and beta are loaded once, before the first pass (a row of more than 1024
// columns, 32 or 64 registers a lane, loads them at their use instead: see HOIST).  On the vec route a lane
// moves 16 bytes per access (register k of lane t is column ((k / V) * lanes + t) * V + k % V, V = 8 bf16 or 4 fp32);
// on the element route register k is column k * lanes + t, so a wave still reads whole contiguous runs.
// The weight gradients never meet an atomic: a lane adds its columns over its rows, the row slots of a wave are folded
// with __shfl_xor, the four waves are added in wave order through LDS, and the workgroup writes one partial row; a
// second kernel adds the partial rows in workgroup order.
#include <atomic>

#include "krs_common.h"
#include "ln_plan.h"

namespace krs {
namespace {

constexpr int kThreads = ln::kThreads;

struct Drop {
  uint32_t on, thr, seed_lo, seed_hi;
  float inv_keep;
  const int64_t* draw;
};

struct FwdParams {
  const void* x;
  const void* res;
  const float* gamma;
  const float* beta;
  void* y;
  void* sum;
  float* mean;
  float* rstd;
  int64_t ldx, ldr, ldy, lds, n, rows_per_group;
  int d, lanes_log2;
  float eps;
  Drop drop;
};

struct BwdParams {
  const void* s;
  const void* dy;
  const void* dsum;
  const float* gamma;
  const float* mean;
  const float* rstd;
  void* dx;
  void* dres;
  float* part;   // [groups, 2, d]: dgamma then dbeta of each workgroup; NULL = no weight gradient is wanted
  int64_t lds, lddy, lddsum, lddx, lddres, n, rows_per_group;
  int d, lanes_log2;
  Drop drop;
};

template <typename T, bool VEC>
__device__ __forceinline__ int col_of(int k, int t, int lanes) {
  constexpr int V = VEC ? 16 / (int)sizeof(T) : 1;
  return ((k / V) * lanes + t) * V + k % V;
}

// The column offsets of a lane do not change from pass to pass, and the compiler would keep all of them (and the
// 64-bit addresses made from them) in registers across the row loop: at 32 or 64 columns a lane that alone overflows the
// register file.  Passing the lane's index through an empty asm at the top of a pass makes them per-pass values.
template <int EPL>
__device__ __forceinline__ int per_pass(int t) {
  if constexpr (EPL >= 32) asm volatile("" : "+v"(t));
  return t;
}

// the lane's EPL columns of one row as fp32; columns at or past d (d = 0: a row that does not exist) read as 0
template <typename T, bool VEC, int EPL>
__device__ __forceinline__ void load_row(const T* row, int t, int lanes, int d, float (&r)[EPL]) {
  if constexpr (VEC) {
    constexpr int V = 16 / (int)sizeof(T);
#pragma unroll
    for (int c = 0; c < EPL / V; ++c) {
      const int c0 = (c * lanes + t) * V;
      if (c0 < d) {
        if constexpr (sizeof(T) == 2) {
          const uint4 q = *reinterpret_cast<const uint4*>(row + c0);
          const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            r[c * 8 + 2 * i] = __uint_as_float(w[i] << 16);
            r[c * 8 + 2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
          }
        } else {
          const float4 q = *reinterpret_cast<const float4*>(row + c0);
          r[c * 4] = q.x, r[c * 4 + 1] = q.y, r[c * 4 + 2] = q.z, r[c * 4 + 3] = q.w;
        }
      } else {
#pragma unroll
        for (int i = 0; i < V; ++i) r[c * V + i] = 0.0f;
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      const int c = k * lanes + t;
      r[k] = c < d ? load1(row + c) : 0.0f;
    }
  }
}

// gamma / beta (fp32) in the column layout of a T row; `fill` where the vector is NULL or the column is past d
template <typename T, bool VEC, int EPL>
__device__ __forceinline__ void load_cols(const float* g, int t, int lanes, int d, float fill, float (&r)[EPL]) {
#pragma unroll
  for (int k = 0; k < EPL; ++k) r[k] = fill;
  if (!g) return;
  if constexpr (VEC) {
    constexpr int V = 16 / (int)sizeof(T);
#pragma unroll
    for (int c = 0; c < EPL / V; ++c) {
      const int c0 = (c * lanes + t) * V;
      if (c0 < d) {
#pragma unroll
        for (int v = 0; v < V / 4; ++v) {
          const float4 q = *reinterpret_cast<const float4*>(g + c0 + 4 * v);
          r[c * V + 4 * v] = q.x, r[c * V + 4 * v + 1] = q.y, r[c * V + 4 * v + 2] = q.z, r[c * V + 4 * v + 3] = q.w;
        }
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      const int c = k * lanes + t;
      if (c < d) r[k] = g[c];
    }
  }
}

template <typename T, bool VEC, int EPL>
__device__ __forceinline__ void store_row(T* row, int t, int lanes, int d, const float (&r)[EPL]) {
  if constexpr (VEC) {
    constexpr int V = 16 / (int)sizeof(T);
#pragma unroll
    for (int c = 0; c < EPL / V; ++c) {
      const int c0 = (c * lanes + t) * V;
      if (c0 < d) {
        if constexpr (sizeof(T) == 2) {
          uint4 q;
          q.x = pack_bf16x2(r[c * 8], r[c * 8 + 1]), q.y = pack_bf16x2(r[c * 8 + 2], r[c * 8 + 3]);
          q.z = pack_bf16x2(r[c * 8 + 4], r[c * 8 + 5]), q.w = pack_bf16x2(r[c * 8 + 6], r[c * 8 + 7]);
          *reinterpret_cast<uint4*>(row + c0) = q;
        } else {
          *reinterpret_cast<float4*>(row + c0) = make_float4(r[c * 4], r[c * 4 + 1], r[c * 4 + 2], r[c * 4 + 3]);
        }
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      const int c = k * lanes + t;
      if (c < d) store1(row + c, r[k]);
    }
  }
}

// what a store to T and a load back would leave (bf16: nearest even; fp32: nothing to do)
template <typename T, int EPL>
__device__ __forceinline__ void round_row(float (&r)[EPL]) {
  if constexpr (sizeof(T) == 2) {
#pragma unroll
    for (int k = 0; k < EPL; k += 2) {
      const uint32_t w = pack_bf16x2(r[k], r[k + 1]);
      r[k] = __uint_as_float(w << 16);
      r[k + 1] = __uint_as_float(w & 0xffff0000u);
    }
  }
}

__device__ __forceinline__ float row_sum(float v, int lanes) {
  for (int o = lanes >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ uint32_t row_hash_base(const Drop& dr, int64_t row) {
  const uint64_t draw = (uint64_t)*dr.draw;
  return ln::hash_base(dr.seed_lo, dr.seed_hi, (uint32_t)draw, (uint32_t)(draw >> 32), (uint32_t)row);
}

template <typename T, bool VEC, int EPL>
__global__ __launch_bounds__(kThreads) void ln_fwd_kernel(FwdParams p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lanes = EPL > 8 ? 64 : 1 << p.lanes_log2;   // (more than 8 columns a lane: the whole wave owns the row)
  const int t0 = lane & (lanes - 1), slot = lane >> p.lanes_log2;
  const int rows_per_wave = 64 >> p.lanes_log2;
  const int64_t row0 = (int64_t)blockIdx.x * p.rows_per_group;
  const int64_t row_end = row0 + p.rows_per_group < p.n ? row0 + p.rows_per_group : p.n;
  const bool stats = p.y != nullptr;
  const T* x = reinterpret_cast<const T*>(p.x);
  const T* res = reinterpret_cast<const T*>(p.res);
  // gamma and beta stay in registers over the passes where a lane holds 8 or 16 columns; a wider row loads them at
  // their use (from L1 / L2), or the row and they would not fit the register file together
  constexpr bool HOIST = EPL <= 16;
  float gam[EPL], bet[EPL];
  if (HOIST && stats) {
    load_cols<T, VEC, EPL>(p.gamma, t0, lanes, p.d, 1.0f, gam);
    load_cols<T, VEC, EPL>(p.beta, t0, lanes, p.d, 0.0f, bet);
  }
  for (int64_t r0 = row0; r0 < row_end; r0 += ln::kWaves * rows_per_wave) {
    const int64_t row = r0 + wave * rows_per_wave + slot;
    int t = per_pass<EPL>(t0);
    const bool active = row < row_end;
    const int d = active ? p.d : 0;
    float s[EPL];
    load_row<T, VEC, EPL>(x + row * p.ldx, t, lanes, d, s);
    if (res || p.drop.on) {
      float add[EPL];
      if (res) {
        load_row<T, VEC, EPL>(res + row * p.ldr, t, lanes, d, add);
      } else {
#pragma unroll
        for (int k = 0; k < EPL; ++k) add[k] = 0.0f;
      }
      if (p.drop.on) {
        const uint32_t base = row_hash_base(p.drop, row);
#pragma unroll
        for (int k = 0; k < EPL; ++k) {
          const bool keep = ln::mix32(base + (uint32_t)col_of<T, VEC>(k, t, lanes)) >= p.drop.thr;
          s[k] = __fmaf_rn(s[k], keep ? p.drop.inv_keep : 0.0f, add[k]);
        }
      } else {
#pragma unroll
        for (int k = 0; k < EPL; ++k) s[k] += add[k];
      }
      round_row<T, EPL>(s);
    }
    if (p.sum) store_row<T, VEC, EPL>(reinterpret_cast<T*>(p.sum) + row * p.lds, t, lanes, d, s);
    if (!stats) continue;
    float a = 0.0f;
#pragma unroll
    for (int k = 0; k < EPL; ++k) a += s[k];
    const float mean = row_sum(a, lanes) / (float)p.d;
    float v = 0.0f;
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      const float c = col_of<T, VEC>(k, t, lanes) < d ? s[k] - mean : 0.0f;
      s[k] = c;
      v = __fmaf_rn(c, c, v);
    }
    const float rstd = 1.0f / sqrtf(row_sum(v, lanes) / (float)p.d + p.eps);
    if constexpr (!HOIST) {
      load_cols<T, VEC, EPL>(p.gamma, t, lanes, p.d, 1.0f, gam);
      load_cols<T, VEC, EPL>(p.beta, t, lanes, p.d, 0.0f, bet);
    }
#pragma unroll
    for (int k = 0; k < EPL; ++k) s[k] = __fmaf_rn(gam[k], s[k] * rstd, bet[k]);
    store_row<T, VEC, EPL>(reinterpret_cast<T*>(p.y) + row * p.ldy, t, lanes, d, s);
    if (t == 0 && active) {
      if (p.mean) p.mean[row] = mean;
      if (p.rstd) p.rstd[row] = rstd;
    }
  }
}

template <typename T, bool VEC, int EPL>
__global__ __launch_bounds__(kThreads) void ln_bwd_kernel(BwdParams p) {
  __shared__ float red[2 * 64 * EPL];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lanes = EPL > 8 ? 64 : 1 << p.lanes_log2;   // (more than 8 columns a lane: the whole wave owns the row)
  const int t0 = lane & (lanes - 1), slot = lane >> p.lanes_log2;
  const int rows_per_wave = 64 >> p.lanes_log2;
  const int64_t row0 = (int64_t)blockIdx.x * p.rows_per_group;
  const int64_t row_end = row0 + p.rows_per_group < p.n ? row0 + p.rows_per_group : p.n;
  const T* sp = reinterpret_cast<const T*>(p.s);
  const T* dyp = reinterpret_cast<const T*>(p.dy);
  const T* dsp = reinterpret_cast<const T*>(p.dsum);
  constexpr bool HOIST = EPL <= 16;   // (as the forward)
  float gam[EPL], dg[EPL], db[EPL];
  if (HOIST && dyp) load_cols<T, VEC, EPL>(p.gamma, t0, lanes, p.d, 1.0f, gam);
#pragma unroll
  for (int k = 0; k < EPL; ++k) dg[k] = 0.0f, db[k] = 0.0f;
  for (int64_t r0 = row0; r0 < row_end; r0 += ln::kWaves * rows_per_wave) {
    const int64_t row = r0 + wave * rows_per_wave + slot;
    int t = per_pass<EPL>(t0);
    const bool active = row < row_end;
    const int d = active ? p.d : 0;
    float ds[EPL];
    if (dyp) {
      float xh[EPL];
      const float mean = active ? p.mean[row] : 0.0f, rstd = active ? p.rstd[row] : 0.0f;
      load_row<T, VEC, EPL>(sp + row * p.lds, t, lanes, d, xh);
      load_row<T, VEC, EPL>(dyp + row * p.lddy, t, lanes, d, ds);
      if constexpr (!HOIST) load_cols<T, VEC, EPL>(p.gamma, t, lanes, p.d, 1.0f, gam);
      float c1 = 0.0f, c2 = 0.0f;
#pragma unroll
      for (int k = 0; k < EPL; ++k) {
        xh[k] = (xh[k] - mean) * rstd;          // (a column past d: dy = 0 there, so it joins no sum)
        if (p.part) {
          dg[k] = __fmaf_rn(ds[k], xh[k], dg[k]);
          db[k] += ds[k];
        }
        ds[k] *= gam[k];
        c1 += ds[k];
        c2 = __fmaf_rn(ds[k], xh[k], c2);
      }
      c1 = row_sum(c1, lanes) / (float)p.d;
      c2 = row_sum(c2, lanes) / (float)p.d;
#pragma unroll
      for (int k = 0; k < EPL; ++k) ds[k] = rstd * (ds[k] - c1 - xh[k] * c2);
      if (dsp) {
        float add[EPL];
        load_row<T, VEC, EPL>(dsp + row * p.lddsum, t, lanes, d, add);
#pragma unroll
        for (int k = 0; k < EPL; ++k) ds[k] += add[k];
      }
    } else {
      load_row<T, VEC, EPL>(dsp + row * p.lddsum, t, lanes, d, ds);
    }
    t = per_pass<EPL>(t0);   // (the stores make their offsets again)
    if (p.dres) store_row<T, VEC, EPL>(reinterpret_cast<T*>(p.dres) + row * p.lddres, t, lanes, d, ds);
    if (p.dx) {
      if (p.drop.on) {
        const uint32_t base = row_hash_base(p.drop, row);
#pragma unroll
        for (int k = 0; k < EPL; ++k) {
          const bool keep = ln::mix32(base + (uint32_t)col_of<T, VEC>(k, t, lanes)) >= p.drop.thr;
          ds[k] *= keep ? p.drop.inv_keep : 0.0f;
        }
      }
      store_row<T, VEC, EPL>(reinterpret_cast<T*>(p.dx) + row * p.lddx, t, lanes, d, ds);
    }
  }
  if (!p.part) return;
  const int t = per_pass<EPL>(t0);
  // the row slots of a wave hold the same columns on lanes `lanes` apart
  for (int o = lanes; o < 64; o <<= 1) {
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      dg[k] += __shfl_xor(dg[k], o);
      db[k] += __shfl_xor(db[k], o);
    }
  }
  // ... and the four waves are added in wave order: wave w takes the sum so far from LDS and passes its own on
  for (int w = 0; w < ln::kWaves; ++w) {
    if (wave == w && slot == 0) {
#pragma unroll
      for (int k = 0; k < EPL; ++k) {
        const int i = k * lanes + t;
        if (w > 0) dg[k] += red[i], db[k] += red[64 * EPL + i];
        if (w + 1 < ln::kWaves) {
          red[i] = dg[k], red[64 * EPL + i] = db[k];
        } else {
          const int c = col_of<T, VEC>(k, t, lanes);
          if (c < p.d) {
            float* out = p.part + (int64_t)blockIdx.x * 2 * p.d;
            out[c] = dg[k], out[p.d + c] = db[k];
          }
        }
      }
    }
    if (w + 1 < ln::kWaves) __syncthreads();
  }
}

// dgamma (blockIdx.y 0) and dbeta (1) from the partial rows, 64 columns a workgroup: thread (q, c) adds the workgroups
// q, q + 4, ... of column c in ascending order, then the four q in order
__global__ __launch_bounds__(kThreads) void ln_wgrad_finish_kernel(const float* part, int64_t groups, int d, float* dgamma,
                                                                   float* dbeta) {
  __shared__ float red[kThreads];
  const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + c, which = blockIdx.y;
  float* out = which ? dbeta : dgamma;
  if (!out) return;
  float a = 0.0f;
  if (j < d)
    for (int64_t g = q; g < groups; g += 4) a += part[(g * 2 + which) * d + j];
  red[threadIdx.x] = a;
  __syncthreads();
  if (q == 0 && j < d) out[j] = ((red[c] + red[64 + c]) + red[128 + c]) + red[192 + c];
}

// ---- host ----
// (one record per process, not per thread, as K19's: the backward runs on an autograd thread)
std::atomic<uint32_t> g_route{0};
inline void set_route(int kernel, int lanes, int vec) {
  g_route.store((uint32_t)kernel << 16 | (uint32_t)lanes << 1 | (uint32_t)vec);
}

inline bool vec_ok(const void* p, int64_t ld, int chunk) { return !p || (aligned16(p) && ld % chunk == 0); }

template <typename P>
void fill_drop(P& p, float dropout_p, uint64_t seed, const int64_t* draw) {
  p.drop.on = dropout_p > 0.0f;
  p.drop.thr = ln::drop_threshold(dropout_p);
  p.drop.inv_keep = 1.0f / (1.0f - dropout_p);
  p.drop.seed_lo = (uint32_t)seed, p.drop.seed_hi = (uint32_t)(seed >> 32);
  p.drop.draw = p.drop.on ? draw : nullptr;
}

inline int log2_of(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

#define KRS_LN_LAUNCH(KERNEL, T_, VEC_)                                                                        \
  switch (pl.per_lane) {                                                                                       \
    case 8: hipLaunchKernelGGL((KERNEL<T_, VEC_, 8>), grid, block, 0, st, p); break;                           \
    case 16: hipLaunchKernelGGL((KERNEL<T_, VEC_, 16>), grid, block, 0, st, p); break;                         \
    case 32: hipLaunchKernelGGL((KERNEL<T_, VEC_, 32>), grid, block, 0, st, p); break;                         \
    default: hipLaunchKernelGGL((KERNEL<T_, VEC_, 64>), grid, block, 0, st, p); break;                         \
  }
#define KRS_LN_DISPATCH(KERNEL)                                                  \
  do {                                                                           \
    const dim3 grid((unsigned)pl.groups), block(kThreads);                       \
    if (dtype == KRS_BF16) {                                                     \
      if (pl.vec) { KRS_LN_LAUNCH(KERNEL, uint16_t, true) }                      \
      else { KRS_LN_LAUNCH(KERNEL, uint16_t, false) }                            \
    } else {                                                                     \
      if (pl.vec) { KRS_LN_LAUNCH(KERNEL, float, true) }                         \
      else { KRS_LN_LAUNCH(KERNEL, float, false) }                               \
    }                                                                            \
  } while (0)

int check_common(const char* what, int64_t n, int64_t d, int dtype, float dropout_p, const int64_t* draw, bool aligned,
                 ln::Plan& pl) {
  pl = ln::plan(n, d, dtype, aligned);
  if (pl.status == ln::kInvalid)
    return fail(KRS_ERR_INVALID, "%s: n=%lld d=%lld dtype=%d: needs %s", what, (long long)n, (long long)d, dtype, pl.why);
  KRS_REQUIRE(dropout_p >= 0.0f && dropout_p < 1.0f, "%s: dropout_p %g outside [0, 1)", what, (double)dropout_p);
  if (pl.status == ln::kUnsupported)
    return fail(KRS_ERR_UNSUPPORTED, "%s: n=%lld d=%lld: supported is %s", what, (long long)n, (long long)d, pl.why);
  if (pl.kernel == ln::kRouteNone) return KRS_OK;
  KRS_REQUIRE(dropout_p == 0.0f || draw, "%s: dropout needs the draw counter", what);
  return KRS_OK;
}

}  // namespace
}  // namespace krs

extern "C" size_t krs_ln_workspace_bytes(int64_t n, int64_t d) { return krs::ln::workspace_bytes(n, d); }

extern "C" int krs_ln_last_route(int* kernel, int* lanes_per_row, int* vec) {
  const uint32_t r = krs::g_route.load();
  if (kernel) *kernel = (int)(r >> 16);
  if (lanes_per_row) *lanes_per_row = (int)((r & 0xffffu) >> 1);
  if (vec) *vec = (int)(r & 1u);
  return (int)(r >> 16);
}

extern "C" int krs_ln_fwd(const void* x, int64_t ldx, const void* residual, int64_t ldr, const float* gamma,
                          const float* beta, int dtype, int64_t n, int64_t d, float eps, float dropout_p, uint64_t seed,
                          const int64_t* draw, void* y, int64_t ldy, void* sum, int64_t lds, float* mean, float* rstd,
                          void* stream) {
  using namespace krs;
  const char* what = "krs_ln_fwd";
  set_route(KRS_LN_NONE, 0, 0);
  const int chunk = dtype == KRS_BF16 ? 8 : 4;
  const bool aligned = vec_ok(x, ldx, chunk) && vec_ok(residual, ldr, chunk) && vec_ok(y, ldy, chunk) &&
                       vec_ok(sum, lds, chunk) && vec_ok(gamma, 0, chunk) && vec_ok(beta, 0, chunk);
  ln::Plan pl;
  const int rc = check_common(what, n, d, dtype, dropout_p, draw, aligned, pl);
  if (rc != KRS_OK) return rc;
  KRS_REQUIRE(eps >= 0.0f, "%s: eps %g is negative", what, (double)eps);
  KRS_REQUIRE(ldx >= d && (!residual || ldr >= d) && (!y || ldy >= d) && (!sum || lds >= d), "%s: row stride below d",
              what);
  if (pl.kernel == ln::kRouteNone) return KRS_OK;
  KRS_REQUIRE(x, "%s: null x", what);
  KRS_REQUIRE(y || sum, "%s: no output is wanted (y and sum are both null)", what);
  KRS_REQUIRE(y || (!mean && !rstd && !gamma && !beta), "%s: the add form (y null) takes no gamma, beta, mean or rstd",
              what);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  FwdParams p{};
  p.x = x, p.res = residual, p.gamma = gamma, p.beta = beta, p.y = y, p.sum = sum, p.mean = mean, p.rstd = rstd;
  p.ldx = ldx, p.ldr = ldr, p.ldy = ldy, p.lds = lds, p.n = n, p.rows_per_group = pl.rows_per_group;
  p.d = (int)d, p.lanes_log2 = log2_of(pl.lanes_per_row), p.eps = eps;
  fill_drop(p, dropout_p, seed, draw);
  KRS_LN_DISPATCH(ln_fwd_kernel);
  KRS_CHECK_LAUNCH("krs_ln_fwd kernel");
  set_route(pl.kernel, pl.lanes_per_row, pl.vec);
  return KRS_OK;
}

extern "C" int krs_ln_bwd(const void* s, int64_t lds, const void* dy, int64_t lddy, const void* dsum, int64_t lddsum,
                          const float* gamma, const float* mean, const float* rstd, int dtype, int64_t n, int64_t d,
                          float dropout_p, uint64_t seed, const int64_t* draw, void* dx, int64_t lddx, void* dres,
                          int64_t lddres, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                          void* stream) {
  using namespace krs;
  const char* what = "krs_ln_bwd";
  set_route(KRS_LN_NONE, 0, 0);
  const int chunk = dtype == KRS_BF16 ? 8 : 4;
  const bool aligned = vec_ok(dy ? s : nullptr, lds, chunk) && vec_ok(dy, lddy, chunk) && vec_ok(dsum, lddsum, chunk) &&
                       vec_ok(dx, lddx, chunk) && vec_ok(dres, lddres, chunk) && vec_ok(dy ? gamma : nullptr, 0, chunk);
  ln::Plan pl;
  const int rc = check_common(what, n, d, dtype, dropout_p, draw, aligned, pl);
  if (rc != KRS_OK) return rc;
  KRS_REQUIRE(dx || dres || dgamma || dbeta, "%s: no gradient is wanted", what);
  KRS_REQUIRE((!dy || (lds >= d && lddy >= d)) && (!dsum || lddsum >= d) && (!dx || lddx >= d) && (!dres || lddres >= d),
              "%s: row stride below d", what);
  if (pl.kernel == ln::kRouteNone) return KRS_OK;
  KRS_REQUIRE(dy || dsum, "%s: null dy and dsum (no gradient arrives)", what);
  KRS_REQUIRE(!dy || (s && mean && rstd), "%s: dy needs s, mean and rstd", what);
  KRS_REQUIRE(dy || (!dgamma && !dbeta), "%s: dgamma and dbeta need dy", what);
  const bool wgrad = dgamma || dbeta;
  const size_t need = wgrad ? ln::workspace_bytes(n, d) : 0;
  if (wgrad && (!workspace || workspace_bytes < need))
    return fail(KRS_ERR_WORKSPACE, "%s: needs %zu workspace bytes, got %zu", what, need, workspace_bytes);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  BwdParams p{};
  p.s = s, p.dy = dy, p.dsum = dsum, p.gamma = gamma, p.mean = mean, p.rstd = rstd, p.dx = dx, p.dres = dres;
  p.part = wgrad ? reinterpret_cast<float*>(workspace) : nullptr;
  p.lds = lds, p.lddy = lddy, p.lddsum = lddsum, p.lddx = lddx, p.lddres = lddres, p.n = n;
  p.rows_per_group = pl.rows_per_group, p.d = (int)d, p.lanes_log2 = log2_of(pl.lanes_per_row);
  fill_drop(p, dropout_p, seed, draw);
  KRS_LN_DISPATCH(ln_bwd_kernel);
  KRS_CHECK_LAUNCH("krs_ln_bwd kernel");
  if (wgrad) {
    hipLaunchKernelGGL(ln_wgrad_finish_kernel, dim3((unsigned)ceil_div(d, 64), 2), dim3(kThreads), 0, st, p.part,
                       pl.groups, (int)d, dgamma, dbeta);
    KRS_CHECK_LAUNCH("krs_ln_bwd weight-gradient sum");
  }
  set_route(pl.kernel, pl.lanes_per_row, pl.vec);
  return KRS_OK;
}
