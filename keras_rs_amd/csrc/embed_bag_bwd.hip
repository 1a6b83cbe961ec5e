// K2 -- index-scatter gradient of the fused embedding bag (backward of K1): the APPLY kernels.
//
// Replaces the autodiff of ops.take/multiply/sum (the dense [V, D] scatter-add
// restated by the reference at keras_rs/src/layers/embedding/jax/test_utils.py:395-417,
// summed per table over the features that share it, :450-468) and, in the fused
// forms, the per-table optimizer step of jax/test_utils.py:474-497.
//
// Plan (embed_bag_plan.hip; once per batch of ids, independent of the gradient values): the lookups sorted by global
//   table row, as (key, bag << 32 | position) pairs, equal keys in ascending position; the segment list (first sorted
//   position of every run of equal keys); the work items of the segments longer than kLongSeg lookups.  This file
//   reads them from the workspace laid out by krs_bag_plan.h and knows nothing else of the plan.
// Apply: a group of LPR lanes (one 16-byte piece of the gradient row per lane, as in K1) per
//   SEGMENT = per touched table row: it issues the loads of the row (and optimizer slots) it will
//   update, gathers and sums the segment's gradient rows, and writes the finished row once:
//   no atomics, one owner per row, contributions summed in ascending p
//   => run-to-run bit-identical.  The row write is the dense gradient row, the compact
//   (unique_rows, grads) entry, or the SGD / Adagrad / Adam / FTRL update of the table row in place.
//   Hot rows (segments longer than kLongSeg) are summed by whole workgroups in chunks of kChunk
//   lookups; rows spanning several chunks are finished from fp32 partial rows in chunk order.
//   Table / slot rows are read and written non-temporally (each is touched once per launch).
// Algorithmic bytes: bags*D*s_g + nnz*(4+8) + U*(2*D*s_t [+ 2*D*4 per slot plane]).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "krs_bag_plan.h"

// The apply kernels are instantiated per (gradient type, table type, lanes per row, optimizer, weights, scale): 3 dtype
// pairs x 4 widths x 7 kernels x 7 modes = ~590 kernels (round 4: ~1000 -- the round-1 per-segment kernel and the
// fp32-gradient / bf16-table pair are gone), the fast kernel (four of the seven) once per KRS_EMBED_OPT_APPLY_DEPTH value.  keras_rs_amd/build.py compiles this file four times, in parallel:
// KRS_BWD_PART 0 = the dense / sparse / SGD forms, 1 = Adagrad and row-wise Adagrad, 2 = Adam, 3 = FTRL
// (entry points outside a part are left out of it).  Undefined = the whole file in one object.
#ifndef KRS_BWD_PART
#define KRS_BWD_PART -1
#endif
#define KRS_BWD_HAS(part) (KRS_BWD_PART < 0 || KRS_BWD_PART == (part))

namespace krs {
extern int g_apply_depth;   // embed_bag_fwd.hip: krs_embed_set_option(KRS_EMBED_OPT_APPLY_DEPTH, v)
namespace {

// ---- apply ------------------------------------------------------------------
enum ApplyMode { kDense = 0, kSgd = 1, kAdagrad = 2, kSparse = 3, kAdam = 4, kFtrl = 5, kAdagradRow = 6 };
constexpr bool mode_is_fused(int m) { return m == kSgd || m == kAdagrad || m == kAdam || m == kFtrl || m == kAdagradRow; }
// full-size fp32 slot planes [V, D] of a mode (row-wise Adagrad keeps ONE fp32 per row instead: slot = [V])
constexpr int mode_slots(int m) { return m == kAdagrad ? 1 : ((m == kAdam || m == kFtrl) ? 2 : 0); }

// Row-wise Adagrad (opt-in, NOT the reference's rule: the FBGEMM / TorchRec "rowwise_adagrad" form without
// epsilon): acc[row] += mean_j g_j^2;  w_j -= lr * g_j / sqrt(acc[row]).  The exact form moves 2 x D x 4
// accumulator bytes per touched row (two thirds of K2's traffic at C3), this one 8.  `ss` = this lane's share of
// sum_j g_j^2; the group's lanes (LPR, a power of two, all active) add theirs by butterfly shuffles.
template <int LPR>
__device__ __forceinline__ float row_sumsq(float ss) {
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  return ss;
}

// optimizer constants shared by every table of a call (the learning rate is per table)
struct Hyper {
  float a, b, c, d;  // Adam: beta_1, beta_2, epsilon, bias-correction factor; FTRL: lr_power, l1, l2, beta
};

// One element of the fused row update; g = the row's summed gradient.  s0 / s1 = slot planes.
//   SGD / Adagrad: jax/test_utils.py:474-497.
//   Adam (lazy: touched rows only; keras.optimizers.Adam.update_step as named by
//     jax/config_conversion.py:256-265): alpha = lr * sqrt(1 - b2^t) / (1 - b1^t) (h.d carries the
//     factor), m += (g - m)(1 - b1), v += (g^2 - v)(1 - b2), w -= alpha * m / (sqrt(v) + eps).
//   FTRL (keras.optimizers.Ftrl.update_step, options of jax/config_conversion.py:266-283; no
//     l2 shrinkage): n' = n + g^2; z += g - (n'^-p - n^-p) / lr * w;
//     w = (clip(z, -l1, l1) - z) / (n'^-p / lr + 2 (l2 + beta / (2 lr))); n = n'.
template <int MODE>
__device__ __forceinline__ void row_update(float& w, float& s0, float& s1, float g, float lr, const Hyper& h) {
  if constexpr (MODE == kSgd) {
    w = w - lr * g;
  } else if constexpr (MODE == kAdagrad) {
    s0 = fmaf(g, g, s0);
    w = w - lr * g / sqrtf(s0);
  } else if constexpr (MODE == kAdam) {
    s0 = s0 + (g - s0) * (1.0f - h.a);
    s1 = s1 + (g * g - s1) * (1.0f - h.b);
    w = w - (lr * h.d) * s0 / (sqrtf(s1) + h.c);
  } else if constexpr (MODE == kFtrl) {
    const float n_new = s0 + g * g;
    // the default power -0.5 is an exactly rounded square root on both sides of the parity check
    const float pn = h.a == -0.5f ? sqrtf(n_new) : powf(n_new, -h.a);
    const float po = h.a == -0.5f ? sqrtf(s0) : powf(s0, -h.a);
    s1 = s1 + g - (pn - po) / lr * w;
    const float quad = pn / lr + 2.0f * (h.c + h.d / (2.0f * lr));
    const float zc = fminf(fmaxf(s1, -h.b), h.b);
    w = (zc - s1) / quad;
    s0 = n_new;
  }
}

struct ApplyParams {
  const krs_table* tables;  // dense: gradient buffers; fused: the tables themselves
  int n_tables;
  const krs_feature* feats;
  int n_feats;
  const float* weights;
  const float* bag_scale;
  const void* grad;
  int64_t grad_ld;
  int batch;
  int dim;
  int64_t nnz;
  const uint32_t* keys;
  const uint64_t* vals;
  const uint32_t* seg_start;   // first sorted position of every segment
  const uint32_t* n_seg;       // device scalar
  const uint32_t* n_long;      // device scalars: items, partial rows, multi-chunk segments
  const LongItem* long_list;
  const MultiSeg* multi_list;
  float* partials;
  int64_t* unique_rows;        // sparse
  float* row_grads;            // sparse
  Hyper hyper;                 // Adam / FTRL
  const float* hyper_d_dev;    // Adam: bias-correction factor read from device memory at run time (NULL: hyper.d)
};

// The constants a launch runs with: Adam's bias-correction factor comes from device memory when the caller keeps it there
// (krs_embed_bag_bwd_fused_adam_dyn: a step replayed from a HIP graph reads the value of THIS replay, not the capture's).
template <int MODE>
__device__ __forceinline__ Hyper live_hyper(const ApplyParams& p) {
  Hyper h = p.hyper;
  if constexpr (MODE == kAdam) {
    if (p.hyper_d_dev) h.d = *p.hyper_d_dev;
  }
  return h;
}

template <typename T>
struct Piece;  // 16 bytes of gradient elements
template <>
struct Piece<float> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void unpack(const uint4& r, float (&f)[4]) {
    f[0] = __uint_as_float(r.x); f[1] = __uint_as_float(r.y);
    f[2] = __uint_as_float(r.z); f[3] = __uint_as_float(r.w);
  }
};
template <>
struct Piece<uint16_t> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void unpack(const uint4& r, float (&f)[8]) {
    f[0] = __uint_as_float(r.x << 16); f[1] = __uint_as_float(r.x & 0xffff0000u);
    f[2] = __uint_as_float(r.y << 16); f[3] = __uint_as_float(r.y & 0xffff0000u);
    f[4] = __uint_as_float(r.z << 16); f[5] = __uint_as_float(r.z & 0xffff0000u);
    f[6] = __uint_as_float(r.w << 16); f[7] = __uint_as_float(r.w & 0xffff0000u);
  }
};

typedef float f32x4n __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4n __attribute__((ext_vector_type(4)));

// N consecutive elements <-> fp32; `aligned` = the address is a multiple of N*sizeof(TT)
// (<= 32 bytes), in which case the access is one or two wide vector instructions.
template <typename TT, int N>
__device__ __forceinline__ void load_elems(const TT* src, float (&f)[N], bool aligned = false) {
  if constexpr (sizeof(TT) == 4) {
    if (aligned) {
#pragma unroll
      for (int i = 0; i < N; i += 4) {
        const f32x4n v = __builtin_nontemporal_load(reinterpret_cast<const f32x4n*>(src + i));
        f[i] = v[0]; f[i + 1] = v[1]; f[i + 2] = v[2]; f[i + 3] = v[3];
      }
    } else {
#pragma unroll
      for (int i = 0; i < N; ++i) f[i] = src[i];
    }
  } else {
    if (aligned) {
      if constexpr (N == 8) {
        const u32x4n rr = __builtin_nontemporal_load(reinterpret_cast<const u32x4n*>(src));
        const uint4 r = make_uint4(rr[0], rr[1], rr[2], rr[3]);
        Piece<uint16_t>::unpack(r, f);
      } else {
        const uint2 r = *reinterpret_cast<const uint2*>(src);
        f[0] = __uint_as_float(r.x << 16); f[1] = __uint_as_float(r.x & 0xffff0000u);
        f[2] = __uint_as_float(r.y << 16); f[3] = __uint_as_float(r.y & 0xffff0000u);
      }
    } else {
#pragma unroll
      for (int i = 0; i < N; ++i) f[i] = bf16_to_f32(src[i]);
    }
  }
}
template <typename TT, int N>
__device__ __forceinline__ void store_elems(TT* dst, const float (&f)[N], bool aligned = false) {
  if constexpr (sizeof(TT) == 4) {
    if (aligned) {
#pragma unroll
      for (int i = 0; i < N; i += 4)
        __builtin_nontemporal_store(f32x4n{f[i], f[i + 1], f[i + 2], f[i + 3]}, reinterpret_cast<f32x4n*>(dst + i));
    } else {
#pragma unroll
      for (int i = 0; i < N; ++i) dst[i] = f[i];
    }
  } else {
    if (aligned) {
      if constexpr (N == 8)
        __builtin_nontemporal_store(u32x4n{pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]), pack_bf16x2(f[4], f[5]),
                                           pack_bf16x2(f[6], f[7])}, reinterpret_cast<u32x4n*>(dst));
      else
        *reinterpret_cast<uint2*>(dst) = make_uint2(pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]));
    } else {
#pragma unroll
      for (int i = 0; i < N; ++i) dst[i] = f32_to_bf16(f[i]);
    }
  }
}

constexpr int kLongUnroll = 4;   // ... and per group in the hot-row kernel, whose chunks are long
constexpr int kSegsPerGroup = 4;  // segments each group walks (amortises the descriptor prologue)
// ... per mode: the slot-less modes (SGD, dense, compact) keep fewer rows in flight per lane and run better with TWO
// (round 5, variant builds at the C3 shape: fused SGD 1297-1315 -> 1119 us multi-hot, 273 -> 260 us at L = 1; Adagrad is flat
// over 1 / 2 / 3 / 4 -- 2266 / 2301 / 2314 / 2282 us -- and 22 % slower with 8)
constexpr int segs_per_group(int mode) { return mode_slots(mode) == 0 && mode != kAdagradRow ? 2 : kSegsPerGroup; }
constexpr int kMaxLdsDesc = 512;  // features / tables whose descriptors are cached in LDS

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(1))) u32x4* gvec_ptr;

// ---- the per-segment kernel, written for memory-level parallelism (round 3) ---------------------------------
// GT: gradient element, TT: table element (fused modes), LPR lanes per row.  One group of LPR lanes per SEGMENT (run of
// equal keys = one table row); the plan's segment list makes the work dense.  Feature / table descriptors are cached in
// LDS per workgroup, so the dependent chain is seg_start -> vals -> (LDS) -> gradient rows; consecutive segments are
// consecutive table rows (the stream is sorted by row), so a workgroup's row updates are near-sequential in HBM.
// The round-1 kernel (`bag_apply_kernel`, deleted in round 5 after two rounds of A/B: 2336 -> 2305-2326 us Adagrad,
// 1383 -> 1312 us SGD, profiles/r3z_k1_k2_multihot.txt; bit-identical) compiled into a chain of dependent round trips: its run-time branches
// (aligned / unaligned access forms, optional weights and bag scales, descriptors in LDS or in memory) sit
// AROUND loads, and hipcc closes every such branch with `s_waitcnt vmcnt(0)` -- the ISA of the C3 instance had a
// full drain between the table-row load, each accumulator load and each gradient row: seven to eight serial
// round trips per segment, hidden only by occupancy (4.1 TB/s on the algorithmic bytes).  This kernel does the
// same arithmetic in the same order with NO branch around a load:
//   * every access is an under-aligned wide vector access (typedefs below: the HSA ABI runs the memory pipeline
//     in unaligned-access mode, a `global_load_dwordx4` needs no 16-byte alignment), so there is one access form;
//   * weights / bag scales / LDS descriptors are compile-time cases (the host picks the instance);
//   * invalid or out-of-range work is CLAMPED to a valid address and masked at the store, never skipped;
//   * the metadata of the group's segs_per_group(MODE) segments is fetched in two trips for all of them (bounds; key and
//     the first two values), and the segments are software-pipelined: the table row, accumulator row and the
//     first two gradient rows of segment i+1 are requested before segment i is consumed.
// Per group that is 2 + 1 trips for four segments instead of ~8 each.  Segments longer than two lookups finish
// in a loop of four gradient rows per trip (DEPTH 0) or from sixteen values fetched in one load (DEPTH > 0, below).  Results are bit-identical to the round-1 kernel (same fmaf chain in
// ascending position, same row_update).  Descriptor counts beyond the LDS cache (> 512 features or tables) and the
// one dtype pair no Keras policy produces (fp32 gradients into bf16 tables) take bag_apply_generic.
typedef u32x4 u32x4_ua __attribute__((aligned(2)));
typedef u32x2 u32x2_ua __attribute__((aligned(2)));

template <int W>
struct RawRow {   // W dwords of a row piece, as loaded
  uint32_t r[W];
};
// (table / slot pointers come out of descriptors, i.e. as generic pointers: accessed as such they become FLAT
//  instructions, which count on the LDS counter too and make hipcc fence them against every ds_read -- the
//  descriptors live in LDS -- so every access below goes through an explicit global-address-space pointer)
#define KRS_AS1 __attribute__((address_space(1)))
template <int W, bool NT>
__device__ __forceinline__ RawRow<W> raw_load(const void* src) {
  RawRow<W> o;
  if constexpr (W == 2) {
    const KRS_AS1 u32x2_ua* q = (const KRS_AS1 u32x2_ua*)src;
    const u32x2 v = NT ? __builtin_nontemporal_load(q) : *q;
    o.r[0] = v[0]; o.r[1] = v[1];
  } else {
#pragma unroll
    for (int i = 0; i < W / 4; ++i) {
      const KRS_AS1 u32x4_ua* q = (const KRS_AS1 u32x4_ua*)src + i;
      const u32x4 v = NT ? __builtin_nontemporal_load(q) : *q;
      o.r[4 * i] = v[0]; o.r[4 * i + 1] = v[1]; o.r[4 * i + 2] = v[2]; o.r[4 * i + 3] = v[3];
    }
  }
  return o;
}
template <int W>
__device__ __forceinline__ void raw_store_nt(void* dst, const RawRow<W>& o) {
  if constexpr (W == 2) {
    __builtin_nontemporal_store(u32x2{o.r[0], o.r[1]}, (KRS_AS1 u32x2_ua*)dst);
  } else {
#pragma unroll
    for (int i = 0; i < W / 4; ++i)
      __builtin_nontemporal_store(u32x4{o.r[4 * i], o.r[4 * i + 1], o.r[4 * i + 2], o.r[4 * i + 3]},
                                  (KRS_AS1 u32x4_ua*)dst + i);
  }
}
// N elements of type TT <-> fp32
template <typename TT, int N>
__device__ __forceinline__ void raw_to_f32(const RawRow<N * (int)sizeof(TT) / 4>& o, float (&f)[N]) {
  if constexpr (sizeof(TT) == 4) {
#pragma unroll
    for (int k = 0; k < N; ++k) f[k] = __uint_as_float(o.r[k]);
  } else {
#pragma unroll
    for (int k = 0; k < N / 2; ++k) {
      f[2 * k] = __uint_as_float(o.r[k] << 16);
      f[2 * k + 1] = __uint_as_float(o.r[k] & 0xffff0000u);
    }
  }
}
template <typename TT, int N>
__device__ __forceinline__ RawRow<N * (int)sizeof(TT) / 4> f32_to_raw(const float (&f)[N]) {
  RawRow<N * (int)sizeof(TT) / 4> o;
  if constexpr (sizeof(TT) == 4) {
#pragma unroll
    for (int k = 0; k < N; ++k) o.r[k] = __float_as_uint(f[k]);
  } else {
#pragma unroll
    for (int k = 0; k < N / 2; ++k) o.r[k] = pack_bf16x2(f[2 * k], f[2 * k + 1]);
  }
  return o;
}

constexpr int kFastFirst = 2;   // gradient rows requested with the row itself
constexpr int kFastMore = 4;    // ... and per trip of the remainder loop (DEPTH 0)
constexpr int kValsBlock = 16;  // values of a longer segment a group fetches in one trip (DEPTH > 0)

// DEPTH (krs_embed_set_option(KRS_EMBED_OPT_APPLY_DEPTH, v)): how the rest of a segment longer than kFastFirst is fetched.
//   0 = the remainder loop: per trip of kFastMore rows a `vals` load, then the gathers whose addresses it gives -- two
//       dependent round trips per four lookups, and a row of 6.6 lookups (the 100-per-bag table of C3) goes through
//       five of them where a one-lookup row goes through two.  The A/B switch and the reference of the bit-for-bit test.
//   4 (default) / 8 / 16 = the deep front.  The group's lanes fetch the segment's next kValsBlock values in ONE coalesced
//       load (lane k of sixteen takes position s0 + kFastFirst + k, clamped to the segment), requested together with
//       the row, its slots and its first two gradient rows; the lanes hand each other the values by a 16-wide shuffle,
//       DEPTH gradient rows (and their coefficients) are requested together, and the following block of values is
//       requested BEFORE this block's rows are consumed.  A segment of <= kFastFirst + DEPTH lookups costs ONE round
//       trip beyond the row's own.  Same bytes, same fmaf chain in ascending position, same masking of clamped slots:
//       bit-identical to DEPTH 0 in every mode (tests/test_embed_bag_bwd_depth_gpu.py).
//   Every wave runs the deep body: the one load it adds to a row of one or two lookups (a clamped, coalesced 8 bytes per
//   lane out of the line its first values came from) is not measurable on the one-hot tables.  What was measured and
//   dropped: a second instantiation without any remainder code for the waves whose segments are all short (93 VGPRs,
//   5 waves per SIMD) beside a deep-only one, each leaving the other's waves alone -- the waves that leave still cost
//   40 - 50 us per launch (descriptor fill, barrier, two trips), more than the split returns; and both bodies behind a
//   wave-uniform branch in one kernel, which hipcc allocates at 152 VGPRs (3 waves per SIMD) for DEPTH 4.
//   Registers / waves per SIMD (-Rpass-analysis=kernel-resource-usage, fused Adagrad, 16 lanes per row, no weights or
//   scales; no instance uses scratch):   DEPTH      0        4        8        16
//                                bf16 rows, bf16 gradients   118 / 4  128 / 4  150 / 3  168 / 3
//                                fp32 rows, fp32 gradients   108 / 4  124 / 4  128 / 4  211 / 2
//   Measured at C3 (profiles/k2_apply_depth_ab.txt): DEPTH 4 keeps the four waves of DEPTH 0 and takes the 100-per-bag
//   table from 572 to 480 us, the 2 ... 27-per-bag tables from 1544 to 1464, all 26 from 2255 to 2139, the one-hot
//   tables stay at 227; 8 and 16 pay for their rows in flight with a wave per SIMD and lose part of that again.
template <typename GT, typename TT, int LPR, int MODE, bool HAS_W, bool HAS_SCALE, int DEPTH>
__global__ __launch_bounds__(256) void bag_apply_fast_kernel(const ApplyParams p) {
  constexpr int N = Piece<GT>::N;
  constexpr int VW = LPR < kValsBlock ? LPR : kValsBlock;   // values per block: one per lane of a 16-lane (or narrower) group
  constexpr int DT = DEPTH < VW ? (DEPTH > 0 ? DEPTH : 1) : VW;   // gradient rows per trip of the deep front
  enum Rest { kRestLoop, kRestDeep };                             // how the body finishes segments longer than kFastFirst
  constexpr int S = segs_per_group(MODE);
  constexpr int WT = N * (int)sizeof(TT) / 4;   // dwords of a lane's table piece
  constexpr int WS = N;                         // ... of its fp32 slot piece
  constexpr bool kFused = mode_is_fused(MODE);
  constexpr int kSlots = mode_slots(MODE);
  __shared__ int s_fcol[kMaxLdsDesc];
  __shared__ int s_ftab[kMaxLdsDesc];
  __shared__ krs_table s_tab[kMaxLdsDesc];
  constexpr int GPB = 256 / LPR;
  const uint32_t n_seg = *p.n_seg;
  const Hyper hy = live_hyper<MODE>(p);
  const int64_t u_base = (int64_t)blockIdx.x * (GPB * S);
  if (u_base >= n_seg) return;
  for (int f = threadIdx.x; f < p.n_feats; f += 256) {
    s_fcol[f] = p.feats[f].out_col;
    s_ftab[f] = p.feats[f].table;
  }
  if constexpr (MODE != kSparse)
    for (int t = threadIdx.x; t < p.n_tables; t += 256) s_tab[t] = p.tables[t];
  __syncthreads();

  const int sub = threadIdx.x % LPR;
  const int row_pieces = (int)(((int64_t)p.dim * sizeof(GT)) >> 4);
  const bool col_live = sub < row_pieces;
  const int csub = col_live ? sub : 0;
  const char* grad = reinterpret_cast<const char*>(p.grad) + (int64_t)csub * 16;
  const uint32_t batch = (uint32_t)p.batch;

  // ---- trip 1: the bounds of the group's segments; trip 2: key and the first two values of each ----
  int64_t s0[S], e0[S];
  bool ok[S];
#pragma unroll
  for (int i = 0; i < S; ++i) {
    const int64_t u = u_base + (int64_t)i * GPB + threadIdx.x / LPR;
    ok[i] = u < n_seg;
    const int64_t uc = ok[i] ? u : (int64_t)n_seg - 1;
    const bool has_next = uc + 1 < n_seg;
    s0[i] = p.seg_start[uc];
    const int64_t nx = p.seg_start[has_next ? uc + 1 : uc];
    e0[i] = has_next ? nx : p.nnz;
  }
  uint32_t key[S];
  uint64_t va[S][kFastFirst];
#pragma unroll
  for (int i = 0; i < S; ++i) {
    key[i] = p.keys[s0[i]];
#pragma unroll
    for (int q = 0; q < kFastFirst; ++q) va[i][q] = p.vals[min(s0[i] + q, e0[i] - 1)];
  }
#pragma unroll
  for (int i = 0; i < S; ++i) {
    // the trailing run of invalid keys (out-of-range ids; the padded tail of a static-capacity exchange, whose
    // values were never written): nothing of it may become an address -- bag 0 / position 0 stand in
    if (key[i] == kInvalidKey) {
#pragma unroll
      for (int q = 0; q < kFastFirst; ++q) va[i][q] = 0;
    }
    ok[i] = ok[i] && key[i] != kInvalidKey && e0[i] - s0[i] <= kLongSeg;
  }

  // what a segment has in flight
  struct InFlight {
    krs_table tb;
    int64_t off, row;
    RawRow<WT> w;
    RawRow<WS> a, b;
    float a_row;
    u32x4 g[kFastFirst];
    float c[kFastFirst];
    uint64_t vx;   // kRestDeep: this lane's value of the segment's first block
  };
  const int subv = threadIdx.x % VW;
  auto grad_src = [&](uint32_t bag) {
    const uint32_t f = bag / batch;
    const uint32_t b = bag - f * batch;
    // (timing-only builds of round 4 read sample 0 everywhere / a feature-major slab here: gathers free -10 %, layout -1 %,
    //  profiles/r4y_k2_gather_cost.txt)
    return grad + ((int64_t)b * p.grad_ld + s_fcol[f]) * (int64_t)sizeof(GT);
  };
  auto coef_of = [&](uint64_t v) {
    float c = 1.0f;
    if constexpr (HAS_W) c = p.weights[(uint32_t)v];
    if constexpr (HAS_SCALE) c *= p.bag_scale[(uint32_t)(v >> 32)];
    return c;
  };
  auto issue = [&](auto rest_c, int i, InFlight& x) {
    constexpr int REST = decltype(rest_c)::value;
    x.tb = krs_table{};
    x.off = 0;
    x.row = 0;
    if constexpr (MODE != kSparse) {
      const uint32_t f0 = (uint32_t)(va[i][0] >> 32) / batch;
      x.tb = s_tab[s_ftab[f0]];
      // (a segment that is not this kernel's to finish still names a table: its row 0 stands in)
      x.row = ok[i] ? (int64_t)key[i] - x.tb.row_base : 0;
      x.off = x.row * p.dim + csub * N;
      if constexpr (kFused) x.w = raw_load<WT, true>(reinterpret_cast<const TT*>(x.tb.weights) + x.off);
      if constexpr (kSlots >= 1) x.a = raw_load<WS, true>(x.tb.slot + x.off);
      if constexpr (kSlots == 2) x.b = raw_load<WS, true>(x.tb.slot + (int64_t)x.tb.vocab * p.dim + x.off);
      if constexpr (MODE == kAdagradRow) x.a_row = *((const KRS_AS1 float*)x.tb.slot + x.row);
    }
#pragma unroll
    for (int q = 0; q < kFastFirst; ++q) {
      x.g[q] = *(const KRS_AS1 u32x4_ua*)grad_src((uint32_t)(va[i][q] >> 32));
      x.c[q] = coef_of(va[i][q]);
    }
    if constexpr (REST == kRestDeep) x.vx = p.vals[min(s0[i] + kFastFirst + subv, e0[i] - 1)];
  };
  auto consume = [&](auto rest_c, int i, const InFlight& x) {
    constexpr int REST = decltype(rest_c)::value;
    const int64_t u = u_base + (int64_t)i * GPB + threadIdx.x / LPR;
    float acc[N];
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.0f;
#pragma unroll
    for (int q = 0; q < kFastFirst; ++q) {
      if (s0[i] + q < e0[i]) {
        float gv[N];
        Piece<GT>::unpack(make_uint4(x.g[q].x, x.g[q].y, x.g[q].z, x.g[q].w), gv);
#pragma unroll
        for (int k = 0; k < N; ++k) acc[k] = fmaf(x.c[q], gv[k], acc[k]);
      }
    }
    // the rest of a longer segment, four gradient rows per trip (positions clamped, contributions masked)
    if constexpr (REST == kRestLoop) if (ok[i]) {
      for (int64_t j0 = s0[i] + kFastFirst; j0 < e0[i]; j0 += kFastMore) {
        uint64_t vv[kFastMore];
#pragma unroll
        for (int q = 0; q < kFastMore; ++q) vv[q] = p.vals[min(j0 + q, e0[i] - 1)];
        u32x4 raw[kFastMore];
        float cf[kFastMore];
#pragma unroll
        for (int q = 0; q < kFastMore; ++q) {
          raw[q] = *(const KRS_AS1 u32x4_ua*)grad_src((uint32_t)(vv[q] >> 32));
          cf[q] = coef_of(vv[q]);
        }
#pragma unroll
        for (int q = 0; q < kFastMore; ++q) {
          if (j0 + q < e0[i]) {
            float gv[N];
            Piece<GT>::unpack(make_uint4(raw[q].x, raw[q].y, raw[q].z, raw[q].w), gv);
#pragma unroll
            for (int k = 0; k < N; ++k) acc[k] = fmaf(cf[q], gv[k], acc[k]);
          }
        }
      }
    }
    // ... or the deep front: blocks of VW values, DT gradient rows per trip (the lanes of a group walk the same segment,
    // so every lane a shuffle reads from is active with it)
    if constexpr (REST == kRestDeep) if (ok[i]) {
      // (a segment of invalid keys is not ok: none of its values becomes an address; zeros stand in all the same)
      uint64_t mv = key[i] == kInvalidKey ? 0 : x.vx;
      for (int64_t jb = s0[i] + kFastFirst; jb < e0[i]; jb += VW) {
        const uint64_t mvn = p.vals[min(jb + VW + subv, e0[i] - 1)];   // the next block, before this one is consumed
#pragma unroll
        for (int t = 0; t < VW; t += DT) {
          if (jb + t < e0[i]) {
            u32x4 raw[DT];
            float cf[DT];
#pragma unroll
            for (int q = 0; q < DT; ++q) {
              const uint32_t bag = (uint32_t)__shfl((int)(uint32_t)(mv >> 32), t + q, VW);
              uint32_t pos = 0;
              if constexpr (HAS_W) pos = (uint32_t)__shfl((int)(uint32_t)mv, t + q, VW);
              raw[q] = *(const KRS_AS1 u32x4_ua*)grad_src(bag);
              cf[q] = coef_of(((uint64_t)bag << 32) | pos);
            }
#pragma unroll
            for (int q = 0; q < DT; ++q) {
              if (jb + t + q < e0[i]) {
                float gv[N];
                Piece<GT>::unpack(make_uint4(raw[q].x, raw[q].y, raw[q].z, raw[q].w), gv);
#pragma unroll
                for (int k = 0; k < N; ++k) acc[k] = fmaf(cf[q], gv[k], acc[k]);
              }
            }
          }
        }
        mv = mvn;
      }
    }
    if constexpr (MODE == kAdagradRow) {
      float ss = 0.0f;
      if (col_live) {
#pragma unroll
        for (int k = 0; k < N; ++k) ss = fmaf(acc[k], acc[k], ss);
      }
      ss = row_sumsq<LPR>(ss);      // every lane of the group takes part, whatever `ok` says
      const float a_new = x.a_row + ss / (float)p.dim;
      if (ok[i] && col_live) {
        float wv[N];
        raw_to_f32<TT, N>(x.w, wv);
        const float inv = a_new > 0.0f ? x.tb.lr / sqrtf(a_new) : 0.0f;  // untouched accumulator + zero gradient: leave the row
#pragma unroll
        for (int k = 0; k < N; ++k) wv[k] = wv[k] - inv * acc[k];
        raw_store_nt<WT>(reinterpret_cast<TT*>(x.tb.weights) + x.off, f32_to_raw<TT, N>(wv));
        if (sub == 0) *((KRS_AS1 float*)x.tb.slot + x.row) = a_new;
      }
      return;
    }
    if (!ok[i] || !col_live) return;
    if constexpr (MODE == kSparse) {
      if (sub == 0) p.unique_rows[u] = (int64_t)key[i];
      float* dst = p.row_grads + u * p.dim + sub * N;
#pragma unroll
      for (int k = 0; k < N; ++k) dst[k] = acc[k];
    } else if constexpr (MODE == kDense) {
      raw_store_nt<WS>(reinterpret_cast<float*>(x.tb.weights) + x.off, f32_to_raw<float, N>(acc));
    } else {
      float wv[N], av[N], bv[N];
      raw_to_f32<TT, N>(x.w, wv);
#pragma unroll
      for (int k = 0; k < N; ++k) { av[k] = 0.0f; bv[k] = 0.0f; }
      if constexpr (kSlots >= 1) raw_to_f32<float, N>(x.a, av);
      if constexpr (kSlots == 2) raw_to_f32<float, N>(x.b, bv);
#pragma unroll
      for (int k = 0; k < N; ++k) row_update<MODE>(wv[k], av[k], bv[k], acc[k], x.tb.lr, hy);
      if constexpr (kSlots >= 1) raw_store_nt<WS>(x.tb.slot + x.off, f32_to_raw<float, N>(av));
      if constexpr (kSlots == 2) raw_store_nt<WS>(x.tb.slot + (int64_t)x.tb.vocab * p.dim + x.off, f32_to_raw<float, N>(bv));
      raw_store_nt<WT>(reinterpret_cast<TT*>(x.tb.weights) + x.off, f32_to_raw<TT, N>(wv));
    }
  };

  auto run = [&](auto rest_c) {
    InFlight fl[2];
    issue(rest_c, 0, fl[0]);
#pragma unroll
    for (int i = 0; i < S; ++i) {
      if (i + 1 < S) issue(rest_c, i + 1, fl[(i + 1) & 1]);
      consume(rest_c, i, fl[i & 1]);
    }
  };
  if constexpr (DEPTH == 0) run(std::integral_constant<int, kRestLoop>{});
  else run(std::integral_constant<int, kRestDeep>{});
}

// Writes one finished row (summed gradient `tot` of segment u, this lane's N columns): dense
// gradient row, compact (unique_rows, grads) entry, or the fused optimizer update in place.
// Row-wise Adagrad: EVERY lane of the row's group calls (live = the lane holds columns of the row).
template <typename GT, typename TT, int MODE, int LPR = 1>
__device__ __forceinline__ void finish_row(const ApplyParams& p, uint32_t u, uint32_t key, int64_t s0, int sub,
                                           const float (&tot)[Piece<GT>::N], bool live = true) {
  constexpr int N = Piece<GT>::N;
  if constexpr (MODE == kAdagradRow) {
    const uint64_t v0 = p.vals[s0];
    const int f0 = (int)((uint32_t)(v0 >> 32) / (uint32_t)p.batch);
    const krs_table tb = p.tables[p.feats[f0].table];
    const int64_t row = (int64_t)key - tb.row_base;
    float ss = 0.0f;
    if (live) {
#pragma unroll
      for (int k = 0; k < N; ++k) ss = fmaf(tot[k], tot[k], ss);
    }
    ss = row_sumsq<LPR>(ss);
    const float a_new = tb.slot[row] + ss / (float)p.dim;
    if (live) {
      const int64_t off = row * p.dim + sub * N;
      const bool t_al = (reinterpret_cast<uintptr_t>(tb.weights) & 15) == 0;
      float wv[N];
      load_elems<TT, N>(reinterpret_cast<const TT*>(tb.weights) + off, wv, t_al);
      const float inv = a_new > 0.0f ? tb.lr / sqrtf(a_new) : 0.0f;  // untouched accumulator + zero gradient: leave the row
#pragma unroll
      for (int k = 0; k < N; ++k) wv[k] = wv[k] - inv * tot[k];
      store_elems<TT, N>(reinterpret_cast<TT*>(tb.weights) + off, wv, t_al);
      if (sub == 0) tb.slot[row] = a_new;
    }
  } else if constexpr (MODE == kSparse) {
    if (sub == 0) p.unique_rows[u] = (int64_t)key;
    float* dst = p.row_grads + (int64_t)u * p.dim + sub * N;
#pragma unroll
    for (int k = 0; k < N; ++k) dst[k] = tot[k];
  } else {
    const uint64_t v0 = p.vals[s0];
    const int f0 = (int)((uint32_t)(v0 >> 32) / (uint32_t)p.batch);
    const krs_table tb = p.tables[p.feats[f0].table];
    const int64_t off = ((int64_t)key - tb.row_base) * p.dim + sub * N;
    const bool t_al = ((reinterpret_cast<uintptr_t>(tb.weights) | reinterpret_cast<uintptr_t>(tb.slot)) & 15) == 0;
    if constexpr (MODE == kDense) {
      store_elems<float, N>(reinterpret_cast<float*>(tb.weights) + off, tot, t_al);
    } else {
      float wv[N], av[N], bv[N];
#pragma unroll
      for (int k = 0; k < N; ++k) { av[k] = 0.0f; bv[k] = 0.0f; }
      const int64_t plane = tb.vocab * p.dim;
      load_elems<TT, N>(reinterpret_cast<const TT*>(tb.weights) + off, wv, t_al);
      if constexpr (mode_slots(MODE) >= 1) load_elems<float, N>(tb.slot + off, av, t_al);
      if constexpr (mode_slots(MODE) == 2) load_elems<float, N>(tb.slot + plane + off, bv, t_al && plane % 4 == 0);
      const Hyper hy = live_hyper<MODE>(p);
#pragma unroll
      for (int k = 0; k < N; ++k) row_update<MODE>(wv[k], av[k], bv[k], tot[k], tb.lr, hy);
      if constexpr (mode_slots(MODE) >= 1) store_elems<float, N>(tb.slot + off, av, t_al);
      if constexpr (mode_slots(MODE) == 2) store_elems<float, N>(tb.slot + plane + off, bv, t_al && plane % 4 == 0);
      store_elems<TT, N>(reinterpret_cast<TT*>(tb.weights) + off, wv, t_al);
    }
  }
}

// Hot rows (segments longer than kLongSeg, e.g. power-law ids or tiny vocabularies): one
// workgroup per segment.  Its 256/LPR groups sum interleaved positions of the segment (four
// gradient rows in flight each), the partial rows meet in LDS and are added in a fixed order
// (group 0, 1, 2, ...), so the result stays run-to-run bit-identical.
template <typename GT, typename TT, int LPR, int MODE, bool HAS_W>
__global__ __launch_bounds__(256) void bag_apply_long_kernel(const ApplyParams p) {
  constexpr int N = Piece<GT>::N;
  constexpr int GPB = 256 / LPR;
  extern __shared__ __attribute__((aligned(16))) char smem_long[];
  float* part = reinterpret_cast<float*>(smem_long);  // [GPB][dim]
  const uint32_t n_long = *p.n_long;
  const uint32_t n_seg = *p.n_seg;
  const int g = threadIdx.x / LPR;
  const int sub = threadIdx.x % LPR;
  const int row_pieces = (int)(((int64_t)p.dim * sizeof(GT)) >> 4);
  const bool col_live = sub < row_pieces;
  const int csub = col_live ? sub : 0;
  const char* grad = reinterpret_cast<const char*>(p.grad) + (int64_t)csub * 16;
  const bool g_aligned = ((reinterpret_cast<uintptr_t>(p.grad) | (uintptr_t)(p.grad_ld * sizeof(GT))) & 15) == 0;
  for (uint32_t li = blockIdx.x; li < n_long; li += gridDim.x) {
    const LongItem item = p.long_list[li];
    const uint32_t u = item.seg;
    const int64_t s0 = p.seg_start[u];
    const int64_t seg_end = u + 1 < n_seg ? (int64_t)p.seg_start[u + 1] : p.nnz;
    const uint32_t key = p.keys[s0];
    if (key == kInvalidKey) continue;
    // this workgroup's piece of the segment
    const int64_t c0 = s0 + (int64_t)item.chunk * kChunk;
    const int64_t e0 = min(seg_end, c0 + kChunk);
    float acc[N];
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.0f;
    for (int64_t j0 = c0 + g; j0 < e0; j0 += (int64_t)GPB * kLongUnroll) {
      uint64_t vv[kLongUnroll];
#pragma unroll
      for (int q = 0; q < kLongUnroll; ++q) vv[q] = p.vals[min(j0 + (int64_t)q * GPB, e0 - 1)];
      float coef[kLongUnroll];
      u32x4 raw[kLongUnroll];
#pragma unroll
      for (int q = 0; q < kLongUnroll; ++q) {
        const uint32_t bag = (uint32_t)(vv[q] >> 32);
        const uint32_t pos = (uint32_t)vv[q];
        const int f = (int)(bag / (uint32_t)p.batch);
        const int b = (int)(bag - (uint32_t)f * (uint32_t)p.batch);
        float c = 1.0f;
        if constexpr (HAS_W) c = p.weights[pos];
        if (p.bag_scale) c *= p.bag_scale[bag];
        coef[q] = c;
        const char* src = grad + ((int64_t)b * p.grad_ld + p.feats[f].out_col) * (int64_t)sizeof(GT);
        if (g_aligned) {
          raw[q] = *(gvec_ptr)src;
        } else {
          const GT* e = reinterpret_cast<const GT*>(src);
          if constexpr (sizeof(GT) == 4) {
            raw[q] = u32x4{__float_as_uint(e[0]), __float_as_uint(e[1]), __float_as_uint(e[2]), __float_as_uint(e[3])};
          } else {
            raw[q] = u32x4{e[0] | ((uint32_t)e[1] << 16), e[2] | ((uint32_t)e[3] << 16),
                           e[4] | ((uint32_t)e[5] << 16), e[6] | ((uint32_t)e[7] << 16)};
          }
        }
      }
#pragma unroll
      for (int q = 0; q < kLongUnroll; ++q) {
        if (j0 + (int64_t)q * GPB < e0) {
          float gv[N];
          Piece<GT>::unpack(make_uint4(raw[q].x, raw[q].y, raw[q].z, raw[q].w), gv);
#pragma unroll
          for (int k = 0; k < N; ++k) acc[k] = fmaf(coef[q], gv[k], acc[k]);
        }
      }
    }
    if (col_live) {
#pragma unroll
      for (int k = 0; k < N; ++k) part[g * p.dim + sub * N + k] = acc[k];
    }
    __syncthreads();
    if (g == 0 && (col_live || MODE == kAdagradRow)) {
      float tot[N];
#pragma unroll
      for (int k = 0; k < N; ++k) tot[k] = 0.0f;
      if (col_live)
        for (int gg = 0; gg < GPB; ++gg)
#pragma unroll
          for (int k = 0; k < N; ++k) tot[k] += part[gg * p.dim + sub * N + k];
      if (item.partial != 0xffffffffu) {  // one of several chunks: the row is finished by bag_apply_finish_kernel
        if (col_live) {
          float* dst = p.partials + (int64_t)item.partial * (kPartialBytes / 4) + sub * N;
#pragma unroll
          for (int k = 0; k < N; ++k) dst[k] = tot[k];
        }
      } else {
        finish_row<GT, TT, MODE, LPR>(p, u, key, s0, sub, tot, col_live);
      }
    }
    __syncthreads();
  }
}

// Segments longer than kChunk: their chunks' partial rows are added in chunk order (fixed, so the
// result stays run-to-run bit-identical) by one group of LPR lanes each, which then writes the row.
template <typename GT, typename TT, int LPR, int MODE>
__global__ __launch_bounds__(256) void bag_apply_finish_kernel(const ApplyParams p) {
  constexpr int N = Piece<GT>::N;
  constexpr int GPB = 256 / LPR;
  const uint32_t n_multi = p.n_long[2];
  const int sub = threadIdx.x % LPR;
  const int row_pieces = (int)(((int64_t)p.dim * sizeof(GT)) >> 4);
  const bool live = sub < row_pieces;
  if (!live && MODE != kAdagradRow) return;
  for (uint32_t mi = blockIdx.x * GPB + threadIdx.x / LPR; mi < n_multi; mi += gridDim.x * GPB) {
    const MultiSeg ms = p.multi_list[mi];
    const int64_t s0 = p.seg_start[ms.seg];
    const uint32_t key = p.keys[s0];
    // a trailing run of invalid keys longer than kChunk (out-of-range ids, the padded tail of a static-capacity
    // exchange) is listed here too: bag_apply_long_kernel wrote no partial rows for it and it names no table row
    if (key == kInvalidKey) continue;
    float tot[N];
#pragma unroll
    for (int k = 0; k < N; ++k) tot[k] = 0.0f;
    if (live)
      for (uint32_t c = 0; c < ms.n_chunks; ++c) {
        const float* src = p.partials + (int64_t)(ms.partial_base + c) * (kPartialBytes / 4) + sub * N;
#pragma unroll
        for (int k = 0; k < N; ++k) tot[k] += src[k];
      }
    finish_row<GT, TT, MODE, LPR>(p, ms.seg, key, s0, sub, tot, live);
  }
}

// Any dim / dtype: LPR lanes per segment, one column per lane per pass.
template <int MODE>
__global__ __launch_bounds__(256) void bag_apply_generic(const ApplyParams p, int grad_dtype, int table_dtype,
                                                         int lpr) {
  const int64_t u = ((int64_t)blockIdx.x * 256 + threadIdx.x) / lpr;
  const int sub = threadIdx.x % lpr;
  const uint32_t n_seg = *p.n_seg;
  if (u >= n_seg) return;
  const int64_t s0 = p.seg_start[u];
  const int64_t e0 = u + 1 < n_seg ? (int64_t)p.seg_start[u + 1] : p.nnz;
  const uint32_t key = p.keys[s0];
  if (key == kInvalidKey) return;
  // the table of the segment's first lookup, as in finish_row (row bases are disjoint, in no particular order)
  const int t = MODE == kSparse ? 0 : p.feats[(uint32_t)(p.vals[s0] >> 32) / (uint32_t)p.batch].table;
  auto column_grad = [&](int c) {
    float acc = 0.0f;
    for (int64_t j = s0; j < e0; ++j) {
      const uint64_t v = p.vals[j];
      const uint32_t bag = (uint32_t)(v >> 32);
      const int f = (int)(bag / (uint32_t)p.batch);
      const int b = (int)(bag - (uint32_t)f * (uint32_t)p.batch);
      float coef = p.weights ? p.weights[(uint32_t)v] : 1.0f;
      if (p.bag_scale) coef *= p.bag_scale[bag];
      acc = fmaf(coef, ld_elem(p.grad, grad_dtype, (int64_t)b * p.grad_ld + p.feats[f].out_col + c), acc);
    }
    return acc;
  };
  if constexpr (MODE == kAdagradRow) {
    // two passes over the row's columns: sum of squares (group-wide), then the update
    const krs_table tb = p.tables[t];
    const int64_t row = (int64_t)key - tb.row_base;
    float ss = 0.0f;
    for (int c = sub; c < p.dim; c += lpr) {
      const float gc = column_grad(c);
      ss = fmaf(gc, gc, ss);
    }
    for (int o = lpr / 2; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    const float a_new = tb.slot[row] + ss / (float)p.dim;
    const float inv = a_new > 0.0f ? tb.lr / sqrtf(a_new) : 0.0f;  // untouched accumulator + zero gradient: leave the row
    for (int c = sub; c < p.dim; c += lpr) {
      const int64_t off = row * p.dim + c;
      st_elem(tb.weights, table_dtype, off, ld_elem(tb.weights, table_dtype, off) - inv * column_grad(c));
    }
    // every lane of the group has read the old accumulator before lane 0 overwrites it (lanes of a wave run in
    // lock step through the shuffle above)
    if (sub == 0) tb.slot[row] = a_new;
    return;
  }
  for (int c = sub; c < p.dim; c += lpr) {
    const float acc = column_grad(c);
    if (MODE == kSparse) {
      if (c == 0) p.unique_rows[u] = (int64_t)key;
      p.row_grads[(int64_t)u * p.dim + c] = acc;
    } else {
      const krs_table tb = p.tables[t];
      const int64_t off = ((int64_t)key - tb.row_base) * p.dim + c;
      if (MODE == kDense) {
        reinterpret_cast<float*>(tb.weights)[off] = acc;
      } else {
        float w = ld_elem(tb.weights, table_dtype, off);
        const int64_t plane = tb.vocab * p.dim;
        float s0 = mode_slots(MODE) >= 1 ? tb.slot[off] : 0.0f;
        float s1 = mode_slots(MODE) == 2 ? tb.slot[plane + off] : 0.0f;
        row_update<MODE>(w, s0, s1, acc, tb.lr, live_hyper<MODE>(p));
        if (mode_slots(MODE) >= 1) tb.slot[off] = s0;
        if (mode_slots(MODE) == 2) tb.slot[plane + off] = s1;
        st_elem(tb.weights, table_dtype, off, w);
      }
    }
  }
}

__global__ void count_unique_kernel(const uint32_t* keys, const uint32_t* n_seg, const uint32_t* sort_mode, int64_t nnz,
                                    int64_t* n_unique) {
  // segments minus the trailing run of invalid keys, if any.  A table-segmented plan leaves the out-of-range lookups at
  // the end of every TABLE's run: the compact form cannot be built from it (-1, which
  // the caller turns into an error: embedding_ops.backward_sparse)
  if (*sort_mode != 0) { *n_unique = -1; return; }
  *n_unique = (int64_t)*n_seg - (nnz > 0 && keys[nnz - 1] == kInvalidKey ? 1 : 0);
}

template <typename GT, typename TT, int MODE>
int launch_apply_lpr(const ApplyParams& p, int pieces, hipStream_t st) {
  const int lpr = pieces <= 8 ? 8 : (pieces <= 16 ? 16 : (pieces <= 32 ? 32 : 64));
  const int64_t groups = p.nnz;  // upper bound of the segment count (device-side n_seg trims it)
  const int64_t blocks = ceil_div(groups, (256 / lpr) * segs_per_group(MODE));
  if (blocks > 0x7fffffffLL) return fail(KRS_ERR_UNSUPPORTED, "embed_bag_bwd: grid too large");
#define KRS_LAUNCH_FAST_D(L, W, SC, DP) \
  hipLaunchKernelGGL((bag_apply_fast_kernel<GT, TT, L, MODE, W, SC, DP>), dim3((unsigned)blocks), dim3(256), 0, st, p)
#define KRS_LAUNCH_FAST(L, W, SC)                                   \
  do {                                                              \
    switch (g_apply_depth) {                                        \
      case 0: KRS_LAUNCH_FAST_D(L, W, SC, 0); break;                \
      case 8: KRS_LAUNCH_FAST_D(L, W, SC, 8); break;                \
      case 16: KRS_LAUNCH_FAST_D(L, W, SC, 16); break;              \
      default: KRS_LAUNCH_FAST_D(L, W, SC, 4); break;               \
    }                                                               \
  } while (0)
#define KRS_LAUNCH_APPLY(L)                                                                             \
  if (p.weights) { if (p.bag_scale) KRS_LAUNCH_FAST(L, true, true); else KRS_LAUNCH_FAST(L, true, false); }   \
  else { if (p.bag_scale) KRS_LAUNCH_FAST(L, false, true); else KRS_LAUNCH_FAST(L, false, false); }
  if (lpr == 8) { KRS_LAUNCH_APPLY(8) }
  else if (lpr == 16) { KRS_LAUNCH_APPLY(16) }
  else if (lpr == 32) { KRS_LAUNCH_APPLY(32) }
  else { KRS_LAUNCH_APPLY(64) }
#undef KRS_LAUNCH_APPLY
#undef KRS_LAUNCH_FAST
#undef KRS_LAUNCH_FAST_D
  KRS_CHECK_LAUNCH("bag_apply_fast_kernel");
  // hot rows: upper bound of the item count is nnz / kLongSeg + nnz / kChunk; surplus workgroups leave at once
  const int64_t max_long = p.nnz / kLongSeg;
  if (max_long > 0) {
    const unsigned lb = (unsigned)(max_long < 8192 ? max_long : 8192);
    const size_t lds = (size_t)(256 / lpr) * p.dim * sizeof(float);
#define KRS_LAUNCH_LONG(L)                                                                              \
  if (p.weights)                                                                                        \
    hipLaunchKernelGGL((bag_apply_long_kernel<GT, TT, L, MODE, true>), dim3(lb), dim3(256), lds, st, p); \
  else                                                                                                  \
    hipLaunchKernelGGL((bag_apply_long_kernel<GT, TT, L, MODE, false>), dim3(lb), dim3(256), lds, st, p);
    if (lpr == 8) { KRS_LAUNCH_LONG(8) }
    else if (lpr == 16) { KRS_LAUNCH_LONG(16) }
    else if (lpr == 32) { KRS_LAUNCH_LONG(32) }
    else { KRS_LAUNCH_LONG(64) }
#undef KRS_LAUNCH_LONG
    KRS_CHECK_LAUNCH("bag_apply_long_kernel");
    const int64_t max_multi = p.nnz / kChunk;
    if (max_multi > 0) {
      const unsigned fb = (unsigned)std::min<int64_t>(ceil_div(max_multi, 256 / lpr), 1024);
      if (lpr == 8) hipLaunchKernelGGL((bag_apply_finish_kernel<GT, TT, 8, MODE>), dim3(fb), dim3(256), 0, st, p);
      else if (lpr == 16) hipLaunchKernelGGL((bag_apply_finish_kernel<GT, TT, 16, MODE>), dim3(fb), dim3(256), 0, st, p);
      else if (lpr == 32) hipLaunchKernelGGL((bag_apply_finish_kernel<GT, TT, 32, MODE>), dim3(fb), dim3(256), 0, st, p);
      else hipLaunchKernelGGL((bag_apply_finish_kernel<GT, TT, 64, MODE>), dim3(fb), dim3(256), 0, st, p);
      KRS_CHECK_LAUNCH("bag_apply_finish_kernel");
    }
  }
  return KRS_OK;
}

template <int MODE>
int run_apply(ApplyParams p, int grad_dtype, int table_dtype, hipStream_t st) {
  if (p.nnz == 0) return KRS_OK;
  const int64_t gbytes = (int64_t)p.dim * (grad_dtype == KRS_BF16 ? 2 : 4);
  // the per-lane piece must also map to whole table / accumulator elements: N elements each
  // (vector kernels: descriptors cached in LDS -- up to kMaxLdsDesc features / tables -- and the dtype pairs the Keras
  //  policies produce: float32, bfloat16, mixed_bfloat16 = bf16 gradients into fp32 tables; fp32 gradients into bf16
  //  tables and wider descriptor lists take the any-shape kernel below)
  const bool vec_pair = !(grad_dtype == KRS_F32 && table_dtype == KRS_BF16 && mode_is_fused(MODE));
  if (gbytes % 16 == 0 && gbytes <= 1024 && vec_pair && p.n_feats <= kMaxLdsDesc && p.n_tables <= kMaxLdsDesc) {
    const int pieces = (int)(gbytes / 16);
    if (grad_dtype == KRS_F32) return launch_apply_lpr<float, float, MODE>(p, pieces, st);
    return table_dtype == KRS_F32 ? launch_apply_lpr<uint16_t, float, MODE>(p, pieces, st)
                                  : launch_apply_lpr<uint16_t, uint16_t, MODE>(p, pieces, st);
  }
  int lpr = 1;
  while (lpr < p.dim && lpr < 64) lpr <<= 1;
  const int64_t blocks = ceil_div(p.nnz * lpr, 256);
  if (blocks > 0x7fffffffLL) return fail(KRS_ERR_UNSUPPORTED, "embed_bag_bwd: grid too large");
  hipLaunchKernelGGL(bag_apply_generic<MODE>, dim3((unsigned)blocks), dim3(256), 0, st, p, grad_dtype,
                     table_dtype, lpr);
  KRS_CHECK_LAUNCH("bag_apply_generic");
  return KRS_OK;
}

int check_apply_args(const void* tables_or_null, int need_tables, const krs_feature* feats, const void* grad,
                     int grad_dtype, int batch, int dim, int64_t nnz, const void* workspace) {
  KRS_REQUIRE(!need_tables || tables_or_null, "embed_bag_bwd: null tables");
  KRS_REQUIRE(feats && grad && (workspace || nnz == 0), "embed_bag_bwd: null feats/grad/workspace");
  KRS_REQUIRE(grad_dtype == KRS_F32 || grad_dtype == KRS_BF16, "embed_bag_bwd: bad grad dtype");
  KRS_REQUIRE(batch > 0 && dim > 0 && nnz >= 0, "embed_bag_bwd: bad sizes");
  return KRS_OK;
}

ApplyParams make_apply(const krs_table* tables, int n_tables, const krs_feature* feats, int n_feats,
                       const float* weights,
                       const float* bag_scale, const void* grad, int64_t grad_ld, int batch, int dim, int64_t nnz,
                       const void* workspace) {
  ApplyParams p;
  const PlanLayout l = plan_layout(const_cast<void*>(workspace), nnz);
  p.tables = tables; p.n_tables = n_tables; p.feats = feats; p.n_feats = n_feats; p.weights = weights;
  p.bag_scale = bag_scale;
  p.grad = grad; p.grad_ld = grad_ld; p.batch = batch; p.dim = dim; p.nnz = nnz;
  p.keys = l.keys_sorted; p.vals = l.vals_sorted; p.seg_start = l.seg_start; p.n_seg = l.n_seg;
  p.n_long = l.n_long; p.long_list = l.long_list; p.multi_list = l.multi_list; p.partials = l.partials;
  p.unique_rows = nullptr; p.row_grads = nullptr;
  p.hyper = Hyper{0.0f, 0.0f, 0.0f, 0.0f};
  p.hyper_d_dev = nullptr;
  return p;
}

// What the entry points of the table forms do: check the arguments, point an ApplyParams at the plan in the workspace,
// run MODE.  hyper_d_dev: Adam's bias-correction factor in device memory (ApplyParams::hyper_d_dev).
template <int MODE>
int apply_tables(const krs_table* tables, int n_tables, const krs_feature* feats, int n_feats, const float* weights,
                 const float* bag_scale, const void* grad, int grad_dtype, int64_t grad_ld, int batch, int dim,
                 int table_dtype, int64_t nnz, const void* workspace, void* stream,
                 Hyper hyper = Hyper{0.0f, 0.0f, 0.0f, 0.0f}, const float* hyper_d_dev = nullptr) {
  if (int rc = check_apply_args(tables, 1, feats, grad, grad_dtype, batch, dim, nnz, workspace)) return rc;
  ApplyParams p = make_apply(tables, n_tables, feats, n_feats, weights, bag_scale, grad, grad_ld, batch, dim, nnz, workspace);
  p.hyper = hyper;
  p.hyper_d_dev = hyper_d_dev;
  return run_apply<MODE>(p, grad_dtype, table_dtype, reinterpret_cast<hipStream_t>(stream));
}

}  // namespace
}  // namespace krs

using namespace krs;

#if KRS_BWD_HAS(0)
extern "C" int krs_embed_bag_bwd_dense(const krs_table* grad_tables, int n_tables, const krs_feature* feats,
                                       int n_feats, const float* weights, const float* bag_scale,
                                       const void* grad, int grad_dtype, int64_t grad_ld, int batch, int dim,
                                       int64_t nnz, const void* workspace, void* stream) {
  return apply_tables<kDense>(grad_tables, n_tables, feats, n_feats, weights, bag_scale, grad, grad_dtype, grad_ld, batch,
                              dim, KRS_F32, nnz, workspace, stream);
}

extern "C" int krs_embed_bag_bwd_fused_sgd(const krs_table* tables, int n_tables, const krs_feature* feats,
                                           int n_feats, const float* weights, const float* bag_scale,
                                           const void* grad, int grad_dtype, int64_t grad_ld, int batch, int dim,
                                           int table_dtype, int64_t nnz, const void* workspace, void* stream) {
  return apply_tables<kSgd>(tables, n_tables, feats, n_feats, weights, bag_scale, grad, grad_dtype, grad_ld, batch, dim,
                            table_dtype, nnz, workspace, stream);
}
#endif

#if KRS_BWD_HAS(1)
extern "C" int krs_embed_bag_bwd_fused_adagrad(const krs_table* tables, int n_tables, const krs_feature* feats,
                                               int n_feats, const float* weights, const float* bag_scale,
                                               const void* grad, int grad_dtype, int64_t grad_ld, int batch,
                                               int dim, int table_dtype, int64_t nnz, const void* workspace,
                                               void* stream) {
  return apply_tables<kAdagrad>(tables, n_tables, feats, n_feats, weights, bag_scale, grad, grad_dtype, grad_ld, batch,
                                dim, table_dtype, nnz, workspace, stream);
}

extern "C" int krs_embed_bag_bwd_fused_adagrad_rowwise(const krs_table* tables, int n_tables,
                                                       const krs_feature* feats, int n_feats, const float* weights,
                                                       const float* bag_scale, const void* grad, int grad_dtype,
                                                       int64_t grad_ld, int batch, int dim, int table_dtype,
                                                       int64_t nnz, const void* workspace, void* stream) {
  return apply_tables<kAdagradRow>(tables, n_tables, feats, n_feats, weights, bag_scale, grad, grad_dtype, grad_ld, batch,
                                   dim, table_dtype, nnz, workspace, stream);
}
#endif

#if KRS_BWD_HAS(2)
extern "C" int krs_embed_bag_bwd_fused_adam(const krs_table* tables, int n_tables, const krs_feature* feats,
                                            int n_feats, const float* weights, const float* bag_scale,
                                            const void* grad, int grad_dtype, int64_t grad_ld, int batch,
                                            int dim, int table_dtype, int64_t nnz, float beta_1, float beta_2,
                                            float epsilon, float bias_correction, const void* workspace,
                                            void* stream) {
  return apply_tables<kAdam>(tables, n_tables, feats, n_feats, weights, bag_scale, grad, grad_dtype, grad_ld, batch, dim,
                             table_dtype, nnz, workspace, stream, Hyper{beta_1, beta_2, epsilon, bias_correction});
}

extern "C" int krs_embed_bag_bwd_fused_adam_dyn(const krs_table* tables, int n_tables, const krs_feature* feats,
                                                int n_feats, const float* weights, const float* bag_scale,
                                                const void* grad, int grad_dtype, int64_t grad_ld, int batch,
                                                int dim, int table_dtype, int64_t nnz, float beta_1, float beta_2,
                                                float epsilon, const float* bias_correction_dev, const void* workspace,
                                                void* stream) {
  KRS_REQUIRE(bias_correction_dev, "krs_embed_bag_bwd_fused_adam_dyn: null bias_correction_dev");
  return apply_tables<kAdam>(tables, n_tables, feats, n_feats, weights, bag_scale, grad, grad_dtype, grad_ld, batch, dim,
                             table_dtype, nnz, workspace, stream, Hyper{beta_1, beta_2, epsilon, 1.0f},
                             bias_correction_dev);
}
#endif

#if KRS_BWD_HAS(3)
extern "C" int krs_embed_bag_bwd_fused_ftrl(const krs_table* tables, int n_tables, const krs_feature* feats,
                                            int n_feats, const float* weights, const float* bag_scale,
                                            const void* grad, int grad_dtype, int64_t grad_ld, int batch,
                                            int dim, int table_dtype, int64_t nnz, float learning_rate_power,
                                            float l1, float l2, float beta, const void* workspace, void* stream) {
  return apply_tables<kFtrl>(tables, n_tables, feats, n_feats, weights, bag_scale, grad, grad_dtype, grad_ld, batch, dim,
                             table_dtype, nnz, workspace, stream, Hyper{learning_rate_power, l1, l2, beta});
}
#endif

#if KRS_BWD_HAS(0)
extern "C" int krs_embed_bag_bwd_sparse(const krs_feature* feats, int n_feats, const float* weights,
                                        const float* bag_scale, const void* grad, int grad_dtype,
                                        int64_t grad_ld, int batch, int dim, int64_t nnz, const void* workspace,
                                        int64_t* unique_rows, float* row_grads, int64_t* n_unique, void* stream) {
  if (int rc = check_apply_args(nullptr, 0, feats, grad, grad_dtype, batch, dim, nnz, workspace)) return rc;
  KRS_REQUIRE(unique_rows && row_grads && n_unique, "embed_bag_bwd_sparse: null outputs");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (nnz == 0) {
    KRS_HIP(hipMemsetAsync(n_unique, 0, sizeof(int64_t), st));
    return KRS_OK;
  }
  const PlanLayout l = plan_layout(const_cast<void*>(workspace), nnz);
  hipLaunchKernelGGL(count_unique_kernel, dim3(1), dim3(1), 0, st, l.keys_sorted, l.n_seg, l.sort_mode, nnz, n_unique);
  KRS_CHECK_LAUNCH("count_unique_kernel");
  ApplyParams p = make_apply(nullptr, 0, feats, n_feats, weights, bag_scale, grad, grad_ld, batch, dim, nnz, workspace);
  p.unique_rows = unique_rows;
  p.row_grads = row_grads;
  return run_apply<kSparse>(p, grad_dtype, KRS_F32, st);
}
#endif
