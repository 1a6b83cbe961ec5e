// K16 -- int8 row-quantized embedding tables for inference: the row quantizer and the fused gather + pool on int8 rows.
//
// A quantized table is two arrays: [vocab, dim] int8 rows and one fp32 dequantization step per row (include/krs.h, K16).
// The lookup is K1's design (embed_bag_fwd.hip) at a byte per element:
//   * a row is read as 16-byte pieces, one piece = 16 elements per lane: a D = 128 row is 128 B = 8 lanes, so a wave64
//     carries 8 independent groups; every lane owns a fixed column slice and accumulates it in 16 fp32 registers;
//   * ids of a window are validated and parked in LDS with the last-of-bag flag (phase A), then the flat loop issues four
//     row loads per lane unconditionally (row 0 stands in for invalid and padding slots and is masked) and, WITH them,
//     the four 4-byte loads of step[id]: the step depends on the id alone, so it never waits for the row;
//   * per lookup the factor w * step is formed once, every element is then one sign-extending byte conversion and one
//     fused multiply-add.
// Algorithmic bytes per lookup: D + 4 (id) + 4 (step) (+4 with weights); per bag D*s_o + 4.
#include <cstdlib>

#include "embed_fwd_q8_plan.h"
#include "krs_common.h"
#include "krs_q8.h"

namespace krs {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Q8FwdParams {
  const krs_table* tables;   // weights: int8 rows, slot: the [vocab] steps
  const krs_feature* feats;
  int n_feats;
  const void* ids;
  int id64;
  const void* offsets;  // null = dense mode
  int off64;
  const float* weights;
  int batch;
  int dim;
  void* out;
  int64_t out_ld;
  int* err_flag;
  int bpg;  // bags per group
};

// the 16 int8 elements of a piece -> fp32 (element i is byte i: little endian, byte 0 of word 0 first)
__device__ __forceinline__ void unpack_i8x16(const u32x4& r, float (&f)[16]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t wd = r[j];
    f[4 * j + 0] = (float)(int8_t)(wd & 0xffu);
    f[4 * j + 1] = (float)(int8_t)((wd >> 8) & 0xffu);
    f[4 * j + 2] = (float)(int8_t)((wd >> 16) & 0xffu);
    f[4 * j + 3] = (float)(int8_t)(wd >> 24);
  }
}

// store 16 fp32 values as OT starting at element pointer `dst` (16-byte aligned when `aligned`), non-temporal: pooled
// rows are written once and read by the next kernel
template <typename OT>
__device__ __forceinline__ void store_piece16(OT* dst, const float (&v)[16], bool aligned) {
  if (!aligned) {
#pragma unroll
    for (int i = 0; i < 16; ++i) store1<OT>(dst + i, v[i]);
    return;
  }
  if constexpr (sizeof(OT) == 4) {
#pragma unroll
    for (int i = 0; i < 16; i += 4) {
      f32x4 t4 = {v[i], v[i + 1], v[i + 2], v[i + 3]};
      __builtin_nontemporal_store(t4, reinterpret_cast<f32x4*>(dst + i));
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16; i += 8) {
      u32x4 t4 = {pack_bf16x2(v[i], v[i + 1]), pack_bf16x2(v[i + 2], v[i + 3]), pack_bf16x2(v[i + 4], v[i + 5]),
                  pack_bf16x2(v[i + 6], v[i + 7])};
      __builtin_nontemporal_store(t4, reinterpret_cast<u32x4*>(dst + i));
    }
  }
}

// OT: output element (float | uint16_t = bf16), LPR: lanes per row.  The two phases per window of a group's lookup
// stream are embed_bag_fwd_vec's: A stages ids, flags (+ weights) in LDS with clamped, unpredicated loads and writes the
// empty bags; B is the flat loop over the staged window.
template <typename OT, int LPR, bool HAS_W>
__global__ __launch_bounds__(256) void embed_bag_fwd_q8_vec(const Q8FwdParams p) {
  constexpr int G = 64 / LPR;
  constexpr int N = 16;
  constexpr int kUnroll = 4;
  constexpr int WIN = 8 * LPR;  // ids per window per group (8 coalesced loads per lane)
  constexpr int MAXB = 16;      // bags per group (host keeps bpg <= 16)
  __shared__ int s_ids[4 * G * WIN];
  __shared__ int s_flag[4 * G * WIN];
  __shared__ float s_w[HAS_W ? 4 * G * WIN : 1];
  __shared__ int s_end[4 * G * (MAXB + 1)];

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int g = lane / LPR;
  const int sub = lane % LPR;

  const int bags_per_wave = G * p.bpg;
  const int waves_per_feat = (p.batch + bags_per_wave - 1) / bags_per_wave;
  const int64_t wave_unit = (int64_t)blockIdx.x * 4 + wave;
  if (wave_unit >= (int64_t)waves_per_feat * p.n_feats) return;
  const int f = __builtin_amdgcn_readfirstlane((int)(wave_unit / waves_per_feat));
  const int wave_b0 = __builtin_amdgcn_readfirstlane((int)(wave_unit - (int64_t)f * waves_per_feat)) * bags_per_wave;

  // wave-uniform descriptors (scalar loads)
  const krs_feature ft = p.feats[f];
  const krs_table tb = p.tables[ft.table];
  const int vocab = tb.vocab;
  const int comb = ft.combiner;
  const int64_t row_bytes = p.dim;
  const int row_pieces = p.dim >> 4;
  const bool col_live = sub < row_pieces;  // LPR is the next of 8 / 16 / 32 / 64 >= row_pieces
  const char* table = reinterpret_cast<const char*>(tb.weights) + (col_live ? sub : 0) * 16;
  typedef const __attribute__((address_space(1))) float* gstep_ptr;
  gstep_ptr steps = (gstep_ptr)tb.slot;

  const int b_lo = wave_b0 + g * p.bpg;
  const int b_hi = min(b_lo + p.bpg, p.batch);
  if (b_lo >= b_hi) return;  // whole groups only: the lanes of a live group stay together
  const int nb = b_hi - b_lo;

  int* ids_l = s_ids + (wave * G + g) * WIN;
  int* flag_l = s_flag + (wave * G + g) * WIN;
  float* w_l = s_w + (HAS_W ? (wave * G + g) * WIN : 0);
  int* end_l = s_end + (wave * G + g) * (MAXB + 1);  // end_l[b] = start of bag b, end_l[b+1] = its end

  // ---- stream bounds and bag boundaries (relative to the stream start) ----
  const bool dense = p.offsets == nullptr;
  const int64_t bag0 = (int64_t)f * p.batch + b_lo;
  int64_t qs;
  if (dense) {
    qs = ft.ids_base + (int64_t)b_lo * ft.hot;
    for (int b = sub; b <= nb; b += LPR) end_l[b] = b * ft.hot;
  } else {
    qs = ld_index(p.offsets, p.off64, bag0);
    for (int b = sub; b <= nb; b += LPR) end_l[b] = (int)(ld_index(p.offsets, p.off64, bag0 + b) - qs);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  const int len = end_l[nb];  // lookups in this group's stream

  OT* out = reinterpret_cast<OT*>(p.out) + ft.out_col + sub * N;
  const bool out_aligned = ((reinterpret_cast<uintptr_t>(out) | (uintptr_t)(p.out_ld * sizeof(OT))) & 15) == 0;

  // empty bags: zeros straight away -- the stream below never reaches them
  if (!dense || ft.hot == 0) {
    for (int b = 0; b < nb; ++b) {
      if (end_l[b + 1] == end_l[b]) {
        float z[N];
#pragma unroll
        for (int i = 0; i < N; ++i) z[i] = 0.0f;
        if (col_live) store_piece16<OT>(out + (int64_t)(b_lo + b) * p.out_ld, z, out_aligned);
      }
    }
  }

  float acc[N];
#pragma unroll
  for (int i = 0; i < N; ++i) acc[i] = 0.0f;
  float sw = 0.0f, sw2 = 0.0f;
  int oob = 0;

  auto flush = [&](int b) {
    const float den = comb == KRS_MEAN ? sw : (comb == KRS_SQRTN ? sqrtf(sw2) : 1.0f);
    float o[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      float v = acc[i];
      if (comb != KRS_SUM) v = den == 0.0f ? 0.0f : v / den;
      o[i] = v;
      acc[i] = 0.0f;
    }
    if (col_live) store_piece16<OT>(out + (int64_t)(b_lo + b) * p.out_ld, o, out_aligned);
    sw = 0.0f;
    sw2 = 0.0f;
  };

  for (int w0 = 0; w0 < len; w0 += WIN) {
    const int wn = min(WIN, len - w0);
    // ---- phase A: stage ids, flags (+ weights) of this window; addresses clamped, no predication ----
    int staged[8];
    if (p.id64) {
      const int64_t* src = reinterpret_cast<const int64_t*>(p.ids) + qs + w0;
      int64_t raw[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) raw[i] = src[min(sub + LPR * i, wn - 1)];
#pragma unroll
      for (int i = 0; i < 8; ++i) staged[i] = (raw[i] >= 0 && raw[i] < vocab) ? (int)raw[i] : -1;
    } else {
      const int32_t* src = reinterpret_cast<const int32_t*>(p.ids) + qs + w0;
      int raw[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) raw[i] = src[min(sub + LPR * i, wn - 1)];
#pragma unroll
      for (int i = 0; i < 8; ++i) staged[i] = (raw[i] >= 0 && raw[i] < vocab) ? raw[i] : -1;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      ids_l[sub + LPR * i] = staged[i];
      flag_l[sub + LPR * i] = 0;
      oob |= (staged[i] < 0) & (sub + LPR * i < wn);
    }
    if constexpr (HAS_W) {
      const float* src = p.weights + qs + w0;
      float raw[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) raw[i] = src[min(sub + LPR * i, wn - 1)];
#pragma unroll
      for (int i = 0; i < 8; ++i) w_l[sub + LPR * i] = raw[i];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // last lookup of every non-empty bag that ends inside this window
    for (int b = sub; b < nb; b += LPR) {
      const int e = end_l[b + 1];
      if (e > end_l[b] && e - 1 >= w0 && e - 1 < w0 + wn) flag_l[e - 1 - w0] = b + 1;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

    // ---- phase B: the flat loop over the staged window ----
    for (int wq = 0; wq < wn; wq += kUnroll) {
      int idc[kUnroll], flg[kUnroll];
      float wc[kUnroll], stp[kUnroll];
      u32x4 raw[kUnroll];
#pragma unroll
      for (int k = 0; k < kUnroll; ++k) {
        const int slot = min(wq + k, WIN - 1);
        const bool live = wq + k < wn;
        idc[k] = live ? ids_l[slot] : -1;
        flg[k] = live ? flag_l[slot] : 0;
        if constexpr (HAS_W) wc[k] = live ? w_l[slot] : 0.0f; else wc[k] = live ? 1.0f : 0.0f;
      }
#pragma unroll
      for (int k = 0; k < kUnroll; ++k) {
        const int row = idc[k] < 0 ? 0 : idc[k];
        // global address space made explicit: a generic pointer would become flat_load (+ lgkmcnt waits)
        typedef const __attribute__((address_space(1))) u32x4* gvec_ptr;
        raw[k] = *(gvec_ptr)(table + (int64_t)row * row_bytes);
        stp[k] = steps[row];     // with the row load, not behind it: it needs the id only
      }
#pragma unroll
      for (int k = 0; k < kUnroll; ++k) {
        sw += wc[k];
        sw2 = fmaf(wc[k], wc[k], sw2);
        float fv[N];
        unpack_i8x16(raw[k], fv);
        // the stand-in row's step may be anything (NaN included): selected away, not multiplied away
        const float ws = idc[k] >= 0 ? wc[k] * stp[k] : 0.0f;
#pragma unroll
        for (int i = 0; i < N; ++i) acc[i] = fmaf(ws, fv[i], acc[i]);
        if (flg[k]) flush(flg[k] - 1);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // window consumed before it is restaged
  }
  if (oob && p.err_flag) atomicOr(p.err_flag, KRS_FLAG_ID_OUT_OF_RANGE);  // any lane that staged a bad id
}

// Any dim / any alignment: one lpr-lane group per bag, one column per lane per pass (embed_bag_fwd_generic on int8 rows).
__global__ __launch_bounds__(256) void embed_bag_fwd_q8_generic(const Q8FwdParams p, int out_dtype, int lpr) {
  const int groups_per_block = 256 / lpr;
  const int64_t bag = (int64_t)blockIdx.x * groups_per_block + threadIdx.x / lpr;
  const int sub = threadIdx.x % lpr;
  if (bag >= (int64_t)p.n_feats * p.batch) return;
  const int f = (int)(bag / p.batch);
  const int b = (int)(bag - (int64_t)f * p.batch);
  const krs_feature ft = p.feats[f];
  const krs_table tb = p.tables[ft.table];
  const int8_t* rows = reinterpret_cast<const int8_t*>(tb.weights);
  int64_t s, e;
  if (p.offsets) {
    s = ld_index(p.offsets, p.off64, bag);
    e = ld_index(p.offsets, p.off64, bag + 1);
  } else {
    s = ft.ids_base + (int64_t)b * ft.hot;
    e = s + ft.hot;
  }
  float sw = 0.0f, sw2 = 0.0f;
  int oob = 0;
  for (int64_t q = s; q < e; ++q) {
    const float w = p.weights ? p.weights[q] : 1.0f;
    sw += w;
    sw2 = fmaf(w, w, sw2);
  }
  const int comb = ft.combiner;
  const float den = comb == KRS_MEAN ? sw : (comb == KRS_SQRTN ? sqrtf(sw2) : 1.0f);
  for (int c = sub; c < p.dim; c += lpr) {
    float acc = 0.0f;
    for (int64_t q = s; q < e; ++q) {
      const int64_t id = ld_index(p.ids, p.id64, q);
      if (id < 0 || id >= tb.vocab) {
        oob = 1;
        continue;
      }
      const float ws = (p.weights ? p.weights[q] : 1.0f) * tb.slot[id];
      acc = fmaf(ws, (float)rows[id * p.dim + c], acc);
    }
    if (comb != KRS_SUM) acc = den == 0.0f ? 0.0f : acc / den;
    st_elem(p.out, out_dtype, (int64_t)b * p.out_ld + ft.out_col + c, acc);
  }
  if (oob && p.err_flag && sub == 0) atomicOr(p.err_flag, KRS_FLAG_ID_OUT_OF_RANGE);
}

// ---- the quantizer (its arithmetic: nonfinite, row_scales, quantize1 of krs_q8.h) ------------------------------------------

// Rows of up to 16 * lanes elements, held in registers: a group of `lanes` lanes (a power of two, 1 .. 64) per row, 16
// elements per lane.  VEC: the lane's elements are [16 sub, 16 sub + 16), moved by 16-byte loads and one 16-byte store
// (dim % 16 == 0, aligned bases); otherwise element sub + lanes * i, one at a time.  The abs-max and the non-finite mark
// cross the group with xor shuffles, which never leave it.
template <typename TT, bool VEC>
__global__ __launch_bounds__(256) void quantize_rows_q8_reg(const TT* __restrict__ table, int64_t vocab, int dim,
                                                            int8_t* __restrict__ q, float* __restrict__ step, int* err_flag,
                                                            int lanes) {
  const int64_t row = (int64_t)blockIdx.x * (256 / lanes) + threadIdx.x / lanes;
  const int sub = threadIdx.x % lanes;
  const bool live = row < vocab;      // (the lanes of a group share the row: a group is live or not as a whole)
  const TT* src = table + (live ? row : 0) * dim;
  float x[16];
  if constexpr (VEC) {
    const bool mine = live && sub * 16 < dim;
    if constexpr (sizeof(TT) == 4) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4 v = mine ? *reinterpret_cast<const f32x4*>(src + sub * 16 + 4 * j) : f32x4{0, 0, 0, 0};
        x[4 * j] = v[0]; x[4 * j + 1] = v[1]; x[4 * j + 2] = v[2]; x[4 * j + 3] = v[3];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const u32x4 v = mine ? *reinterpret_cast<const u32x4*>(src + sub * 16 + 8 * j) : u32x4{0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          x[8 * j + 2 * i] = __uint_as_float(v[i] << 16);
          x[8 * j + 2 * i + 1] = __uint_as_float(v[i] & 0xffff0000u);
        }
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int c = sub + lanes * i;
      x[i] = live && c < dim ? load1<TT>(src + c) : 0.0f;
    }
  }
  float a = 0.0f;
  int bad = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    a = fmaxf(a, fabsf(x[i]));
    bad |= nonfinite(x[i]);
  }
  for (int off = lanes >> 1; off > 0; off >>= 1) {
    a = fmaxf(a, __shfl_xor(a, off, 64));
    bad |= __shfl_xor(bad, off, 64);
  }
  float inv, st;
  row_scales(a, inv, st);
  int qi[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) qi[i] = bad ? 0 : quantize1(x[i], inv);
  int8_t* dst = q + (live ? row : 0) * dim;
  if constexpr (VEC) {
    if (live && sub * 16 < dim) {
      u32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        o[j] = (uint32_t)(qi[4 * j] & 0xff) | ((uint32_t)(qi[4 * j + 1] & 0xff) << 8) |
               ((uint32_t)(qi[4 * j + 2] & 0xff) << 16) | ((uint32_t)(qi[4 * j + 3] & 0xff) << 24);
      *reinterpret_cast<u32x4*>(dst + sub * 16) = o;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int c = sub + lanes * i;
      if (live && c < dim) dst[c] = (int8_t)qi[i];
    }
  }
  if (live && sub == 0) {
    step[row] = bad ? 0.0f : st;
    if (bad && err_flag) atomicOr(err_flag, KRS_FLAG_NONFINITE_ROW);
  }
}

// Rows longer than 1024 elements: a wave per row, the row is read twice (the second read of a row this wave has just
// streamed comes from the cache).
__global__ __launch_bounds__(256) void quantize_rows_q8_long(const void* __restrict__ table, int table_dtype, int64_t vocab,
                                                             int dim, int8_t* __restrict__ q, float* __restrict__ step,
                                                             int* err_flag) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= vocab) return;      // wave-uniform
  const int64_t base = row * dim;
  float a = 0.0f;
  int bad = 0;
  for (int c = lane; c < dim; c += 64) {
    const float x = ld_elem(table, table_dtype, base + c);
    a = fmaxf(a, fabsf(x));
    bad |= nonfinite(x);
  }
  for (int off = 32; off > 0; off >>= 1) {
    a = fmaxf(a, __shfl_xor(a, off, 64));
    bad |= __shfl_xor(bad, off, 64);
  }
  float inv, st;
  row_scales(a, inv, st);
  for (int c = lane; c < dim; c += 64)
    q[base + c] = bad ? (int8_t)0 : (int8_t)quantize1(ld_elem(table, table_dtype, base + c), inv);
  if (lane == 0) {
    step[row] = bad ? 0.0f : st;
    if (bad && err_flag) atomicOr(err_flag, KRS_FLAG_NONFINITE_ROW);
  }
}

// where the calling thread's last krs_embed_bag_fwd_q8 ran: cleared when the entry starts, written when it has queued its
// kernel, so a refused call and an empty one leave "none"
thread_local krs_embed_fwd_route g_q8_route = {};
static_assert(q8plan::kMaxBpg == 16, "embed_bag_fwd_q8_vec stages MAXB = 16 bag ends per group");

// the argument checks the decision needs, then the call's plan (embed_fwd_q8_plan.h); a refused plan leaves its message
int q8_fwd_plan(int n_feats, const void* offsets, const float* weights, int64_t nnz, int batch, int dim, const void* out,
                int out_dtype, int64_t out_ld, q8plan::Q8FwdPlan& pl) {
  q8plan::Q8FwdCall call;
  call.n_feats = n_feats; call.batch = batch; call.dim = dim; call.nnz = nnz; call.out_ld = out_ld;
  call.out_dtype = out_dtype; call.has_offsets = offsets != nullptr; call.has_weights = weights != nullptr;
  call.out_addr = reinterpret_cast<uintptr_t>(out);
  pl = q8plan::plan_q8_fwd(call);
  if (pl.status != KRS_OK) return fail(pl.status, "embed_bag_fwd_q8: %s", pl.why);
  return KRS_OK;
}

template <typename OT, int LPR>
void launch_q8_lpr(const Q8FwdParams& p, const krs_embed_fwd_route& rt, hipStream_t st) {
  const dim3 grid((unsigned)rt.blocks), block(256);
  if (rt.has_w) hipLaunchKernelGGL((embed_bag_fwd_q8_vec<OT, LPR, true>), grid, block, 0, st, p);
  else hipLaunchKernelGGL((embed_bag_fwd_q8_vec<OT, LPR, false>), grid, block, 0, st, p);
}

template <typename OT>
void launch_q8_vec(const Q8FwdParams& p, const krs_embed_fwd_route& rt, hipStream_t st) {
  if (rt.lpr == 8) launch_q8_lpr<OT, 8>(p, rt, st);
  else if (rt.lpr == 16) launch_q8_lpr<OT, 16>(p, rt, st);
  else if (rt.lpr == 32) launch_q8_lpr<OT, 32>(p, rt, st);
  else launch_q8_lpr<OT, 64>(p, rt, st);
}

}  // namespace
}  // namespace krs

extern "C" int krs_embed_bag_fwd_q8(const krs_table* tables, const krs_feature* feats, int n_feats,
                                    const void* ids, int id_type, const void* offsets, int off_type,
                                    const float* weights, int64_t nnz, int batch, int dim,
                                    void* out, int out_dtype, int64_t out_ld, int* err_flag, void* stream) {
  using namespace krs;
  g_q8_route = krs_embed_fwd_route{};
  KRS_REQUIRE(tables && feats && out, "embed_bag_fwd_q8: null tables/feats/out");
  KRS_REQUIRE(ids || nnz == 0, "embed_bag_fwd_q8: null ids");
  q8plan::Q8FwdPlan pl;
  if (int rc = q8_fwd_plan(n_feats, offsets, weights, nnz, batch, dim, out, out_dtype, out_ld, pl)) return rc;
  KRS_REQUIRE((id_type == KRS_I32 || id_type == KRS_I64) && (off_type == KRS_I32 || off_type == KRS_I64),
              "embed_bag_fwd_q8: bad index type");
  const krs_embed_fwd_route& rt = pl.route;
  if (rt.kernel == KRS_EMBED_FWD_NONE) return KRS_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);

  Q8FwdParams p;
  p.tables = tables; p.feats = feats; p.n_feats = n_feats;
  p.ids = ids; p.id64 = id_type == KRS_I64;
  p.offsets = offsets; p.off64 = off_type == KRS_I64;
  p.weights = weights; p.batch = batch; p.dim = dim;
  p.out = out; p.out_ld = out_ld; p.err_flag = err_flag;
  p.bpg = rt.bpg;   // bags per group of embed_bag_fwd_q8_vec (the generic kernel does not read it)

  if (rt.kernel == KRS_EMBED_FWD_GENERIC) {
    hipLaunchKernelGGL(embed_bag_fwd_q8_generic, dim3((unsigned)rt.blocks), dim3(256), 0, st, p, out_dtype, rt.lpr);
    KRS_CHECK_LAUNCH("embed_bag_fwd_q8_generic");
  } else {
    if (out_dtype == KRS_F32) launch_q8_vec<float>(p, rt, st); else launch_q8_vec<uint16_t>(p, rt, st);
    KRS_CHECK_LAUNCH("embed_bag_fwd_q8_vec");
  }
  g_q8_route = rt;
  return KRS_OK;
}

extern "C" int krs_embed_bag_fwd_q8_plan_route(int n_feats, const void* offsets, const float* weights, int64_t nnz, int batch,
                                               int dim, const void* out, int out_dtype, int64_t out_ld,
                                               krs_embed_fwd_route* route) {
  krs::q8plan::Q8FwdPlan pl;
  const int rc = krs::q8_fwd_plan(n_feats, offsets, weights, nnz, batch, dim, out, out_dtype, out_ld, pl);
  if (route) *route = pl.route;
  return rc;
}

extern "C" int krs_embed_bag_fwd_q8_last_route(krs_embed_fwd_route* route) {
  if (route) *route = krs::g_q8_route;
  return krs::g_q8_route.kernel;
}

extern "C" int krs_quantize_rows_q8(const void* table, int table_dtype, int64_t vocab, int dim, int8_t* q, float* step,
                                    int* err_flag, void* stream) {
  using namespace krs;
  const q8plan::QuantizePlan pl = q8plan::plan_quantize(vocab, dim, table_dtype, reinterpret_cast<uintptr_t>(table),
                                                        reinterpret_cast<uintptr_t>(q), reinterpret_cast<uintptr_t>(step));
  if (pl.status != KRS_OK) return fail(pl.status, "quantize_rows_q8: %s", pl.why);
  if (pl.blocks == 0) return KRS_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)pl.blocks), block(256);
  if (pl.two_pass) {
    hipLaunchKernelGGL(quantize_rows_q8_long, grid, block, 0, st, table, table_dtype, vocab, dim, q, step, err_flag);
  } else if (table_dtype == KRS_F32) {
    const float* t = reinterpret_cast<const float*>(table);
    if (pl.vec) hipLaunchKernelGGL((quantize_rows_q8_reg<float, true>), grid, block, 0, st, t, vocab, dim, q, step, err_flag, pl.lanes);
    else hipLaunchKernelGGL((quantize_rows_q8_reg<float, false>), grid, block, 0, st, t, vocab, dim, q, step, err_flag, pl.lanes);
  } else {
    const uint16_t* t = reinterpret_cast<const uint16_t*>(table);
    if (pl.vec) hipLaunchKernelGGL((quantize_rows_q8_reg<uint16_t, true>), grid, block, 0, st, t, vocab, dim, q, step, err_flag, pl.lanes);
    else hipLaunchKernelGGL((quantize_rows_q8_reg<uint16_t, false>), grid, block, 0, st, t, vocab, dim, q, step, err_flag, pl.lanes);
  }
  KRS_CHECK_LAUNCH("quantize_rows_q8");
  return KRS_OK;
}
