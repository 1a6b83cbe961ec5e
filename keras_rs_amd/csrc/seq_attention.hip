// K19 -- fused multi-head self-attention over [B, L] token sequences with a causal and a padding mask; the score
// matrix and the dropout mask are never stored.  The arithmetic is fixed in include/krs.h (K19).
//
// Fast path (bf16, dh <= 128), attn_kernel<DPAD, MODE, VEC>: K13's body ("owner on the lane") batched over (b, h).  The
// tile image, the chunk loads, the accumulator-row rule, the packing and the transposed read are krs_owner_tile.h's,
// shared with K13; the score chain and the gather's addresses are written out here as they are there.
//   * a wave owns 32 rows of one side as B operands of the score product, a workgroup of 4 waves 128 rows of one
//     (b, h); the other side streams through LDS in double-buffered tiles of 32 rows, TWO tiles per step (X and Y):
//       MODE_FWD  owner = queries (q);       X = keys, Y = values
//       MODE_DQ   owner = queries (q, dO);   X = keys, Y = values
//       MODE_DKV  owner = keys (k, v);       X = queries, Y = dO
//   * score tile S[t][o] = X[t] . own1[o] and, in the backward, dP[t][o] = Y[t] . own2[o]: v_mfma_f32_32x32x16_bf16
//     chains whose A operand is the streamed tile.  The owner is on the lane and the streamed row on the 16
//     registers (row acc_row(r, lane >> 5)), so m, Z, lse, delta of the owner are per-lane values;
//   * the tile's probabilities (or dS), rounded pairwise to bf16, ARE the A operand of the second product
//     (O += P~ V;  dQ += dS K;  dV += P~ dO, dK += dS Q); its B operand is gathered from the same LDS tile with
//     ds_read_b64_tr_b16 in the accumulator's row order (K13);
//   * MODE_FWD keeps an online (m, Z) per lane; the two lanes of a query agree on m every tile (one cross-half
//     exchange).  The output accumulator has the query on the REGISTER index, so the per-query factor
//     exp(m_old - m_new), and 1 / Z at the end, cross from lanes to registers through 32 floats of LDS per wave;
//   * under `causal`, tiles wholly beyond the diagonal of the workgroup are not streamed and those beyond the
//     diagonal of a wave are not computed by it.
// Every output element has one owner, there are no float atomics: bit-identical from call to call.
//
// Generic path (fp32 at any dh <= 256, bf16 above 128): one workgroup per (b, h, row), fp32 FMA, one row of scores in
// LDS.  gen_fwd / gen_dq own a query row, gen_dkv a key row.  Same masks, same hash, same ownership rule.
//
// delta_i = sum_d dO_id o_id is written to the workspace by a small kernel before either backward sweep.
#include <atomic>

#include "krs_owner_tile.h"
#include "seq_attn_plan.h"

namespace krs {
namespace {

using seqattn::kOwnRows;
using seqattn::kTile;

static_assert(kTile == kOwnerTile, "the streamed tile is krs_owner_tile.h's");

constexpr int kThreads = 256;
enum { MODE_FWD = 0, MODE_DQ = 1, MODE_DKV = 2 };

struct Params {
  const void *q, *k, *v;
  int64_t ldq, ldk, ldv;
  void* out;            // forward: written; backward: read
  int64_t ldo;
  const void* dout;
  int64_t lddo;
  float* lse;           // [b, h, l]; forward: written; backward: read
  float* delta;         // [b, h, l] (workspace)
  void *dq, *dk, *dv;
  int64_t lddq, lddk, lddv;
  const uint8_t* kv;    // [b, l] or null
  int h, l, dh, causal;
  float scale;
  int dropout;
  uint32_t thr;
  float inv_keep;
  uint32_t seed_lo, seed_hi;
  const int64_t* draw;
  int64_t oblocks;
};

__device__ __forceinline__ uint32_t hash_base_of(const Params& p, int64_t bh) {
  if (!p.dropout) return 0u;
  const uint64_t draw = p.draw ? (uint64_t)*p.draw : 0ull;
  return seqattn::hash_base(p.seed_lo, p.seed_hi, (uint32_t)draw, (uint32_t)(draw >> 32), (uint32_t)bh);
}
// keep / (1 - p) of element (i, j)
__device__ __forceinline__ float keep_factor(const Params& p, uint32_t base, int i, int j) {
  if (!p.dropout) return 1.0f;
  return seqattn::hash_ij(base, (uint32_t)i, (uint32_t)j) >= p.thr ? p.inv_keep : 0.0f;
}

template <int DPAD, int MODE, bool VEC>
__global__ __launch_bounds__(kThreads) void attn_kernel(const Params p) {
  constexpr bool BWD = MODE != MODE_FWD, KOWN = MODE == MODE_DKV;
  constexpr int NKS = DPAD / 16, DT = DPAD / 32, CH = DPAD / 8;
  constexpr int TILE_BYTES = kTile * DPAD * 2;
  constexpr int U = (kTile * CH + kThreads - 1) / kThreads;   // chunks of each tile a thread stages
  __shared__ __attribute__((aligned(16))) char tx[2][TILE_BYTES];
  __shared__ __attribute__((aligned(16))) char ty[2][TILE_BYTES];
  __shared__ __attribute__((aligned(16))) float side_a[2][kTile];
  __shared__ __attribute__((aligned(16))) float side_b[2][kTile];
  __shared__ __attribute__((aligned(16))) float xch[kThreads / 64][32];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int frow = lane & 31, fhalf = lane >> 5;
  const int64_t oblock = blockIdx.x % p.oblocks, bh = blockIdx.x / p.oblocks;
  const int64_t bi = bh / p.h;
  const int hi = (int)(bh % p.h);
  const int l = p.l, dh = p.dh;
  const int64_t tok0 = bi * l;
  const int col0 = hi * dh;

  const uint16_t* own1 = reinterpret_cast<const uint16_t*>(KOWN ? p.k : p.q) + col0;
  const int64_t ld1 = KOWN ? p.ldk : p.ldq;
  const uint16_t* own2 = reinterpret_cast<const uint16_t*>(KOWN ? p.v : p.dout) + col0;   // (backward only)
  const int64_t ld2 = KOWN ? p.ldv : p.lddo;
  const uint16_t* X = reinterpret_cast<const uint16_t*>(KOWN ? p.q : p.k) + col0;
  const int64_t ldx = KOWN ? p.ldq : p.ldk;
  const uint16_t* Y = reinterpret_cast<const uint16_t*>(KOWN ? p.dout : p.v) + col0;
  const int64_t ldy = KOWN ? p.lddo : p.ldv;

  // the owner row of this lane
  const int wfirst = (int)oblock * kOwnRows + wave * 32;
  const int oi = wfirst + frow;
  const bool ovalid = oi < l;
  u32x4 of1[NKS], of2[BWD ? NKS : 1];
  {
    const int64_t row = tok0 + (ovalid ? oi : 0);
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      const int e0 = (2 * ks + fhalf) * 8;
      of1[ks] = load_chunk<VEC>(own1 + row * ld1 + e0, e0, dh, ovalid);
      if constexpr (BWD) of2[ks] = load_chunk<VEC>(own2 + row * ld2 + e0, e0, dh, ovalid);
      if constexpr (!VEC) __builtin_amdgcn_sched_barrier(0);
    }
  }
  float my_lse = 0.0f, my_delta = 0.0f;
  bool my_kv = true;
  if constexpr (MODE == MODE_DQ) {
    if (ovalid) my_lse = p.lse[bh * l + oi], my_delta = p.delta[bh * l + oi];
  }
  if constexpr (KOWN) my_kv = ovalid && (!p.kv || p.kv[tok0 + oi] != 0);
  const uint32_t hbase = hash_base_of(p, bh);

  // streamed range of the workgroup, and whether this wave computes a tile
  const int t_begin = (KOWN && p.causal) ? (int)oblock * kOwnRows : 0;
  const int own_end = ((int)oblock + 1) * kOwnRows;
  const int t_end = (!KOWN && p.causal && own_end < l) ? own_end : l;
  const bool wave_live = wfirst < l;

  // staging of one streamed step: registers first, LDS after the current tiles have been consumed
  u32x4 sregx[U], sregy[U];
  float sa = 0.0f, sb = 0.0f;
  auto stage_load = [&](int t0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = tid + u * kThreads;
      const int srow = i / CH, ch = i % CH;          // (a thread beyond the tile stages nothing)
      const bool ok = srow < kTile && t0 + srow < t_end;
      const int64_t row = tok0 + (ok ? t0 + srow : 0);
      sregx[u] = load_chunk<VEC>(X + row * ldx + ch * 8, ch * 8, dh, ok);
      // (element-wise rows: eight loads and their addresses per chunk; keep one chunk in flight at a time)
      if constexpr (!VEC) __builtin_amdgcn_sched_barrier(0);
      sregy[u] = load_chunk<VEC>(Y + row * ldy + ch * 8, ch * 8, dh, ok);
      if constexpr (!VEC) __builtin_amdgcn_sched_barrier(0);
    }
    if (tid < kTile) {
      const int t = t0 + tid;
      const bool ok = t < t_end;
      if constexpr (KOWN) {
        sa = ok ? p.lse[bh * l + t] : 0.0f;
        sb = ok ? p.delta[bh * l + t] : 0.0f;
      } else {
        sa = ok && (!p.kv || p.kv[tok0 + t] != 0) ? 1.0f : 0.0f;
      }
    }
  };
  auto stage_store = [&](int buf) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = tid + u * kThreads;
      if (i < kTile * CH) {
        const int dst = tile_off<DPAD>(i / CH, i % CH);
        *reinterpret_cast<u32x4*>(&tx[buf][dst]) = sregx[u];
        *reinterpret_cast<u32x4*>(&ty[buf][dst]) = sregy[u];
      }
    }
    if (tid < kTile) {
      side_a[buf][tid] = sa;
      side_b[buf][tid] = sb;
    }
  };

  // accumulators: FWD o, DQ dq: acc_a;  DKV: acc_a = dk, acc_b = dv
  f32x16 acc_a[DT], acc_b[KOWN ? DT : 1];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      acc_a[dt][r] = 0.0f;
      if constexpr (KOWN) acc_b[dt][r] = 0.0f;
    }
  float m_run = kNegInf, z_run = 0.0f;   // MODE_FWD: this lane's 16 rows of every tile (m shared by the two lanes)

  // B operand of the second product from a tile: rows 16 s2 + acc_row(j, fhalf), column 32 dt + frow.  The addresses
  // are krs_owner_tile.h's gather_at (row, chunk, byte), written out -- a second copy, with K13's, of what
  // tests/host/owner_tile_check.cpp checks: through gather_at, or with the header's gather composed of it, hipcc
  // rescheduled all 18 builds and two rows of the benchmark ran slower (docs/measurement_log.md section 28).  So are the
  // score chains and the product loops below.  Change the three together.
  const int li = lane & 15, tq = li >> 2, tp = li & 3, chalf = (lane >> 4) & 1;
  auto gather_b = [&](const char* tile, int dt, int s2) -> u32x4 {
    const int r0 = 16 * s2 + 4 * fhalf;
    const int ch = 4 * dt + 2 * chalf + (tp >> 1);
    const char* a0 = tile + tile_off<DPAD>(r0 + tq, ch) + 8 * (tp & 1);
    const char* a1 = tile + tile_off<DPAD>(r0 + 8 + tq, ch) + 8 * (tp & 1);
    const u32x2 lo = lds_read_tr16(a0), hi2 = lds_read_tr16(a1);
    return (u32x4){lo[0], lo[1], hi2[0], hi2[1]};
  };
  // a per-owner value (the same on both lanes of an owner) by accumulator register: row acc_row(r, fhalf)
  auto lane_to_reg = [&](float v, float* byreg) {
    __builtin_amdgcn_wave_barrier();
    if (fhalf == 0) xch[wave][frow] = v;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      const float4 t = *reinterpret_cast<const float4*>(&xch[wave][8 * gq + 4 * fhalf]);
      byreg[4 * gq] = t.x, byreg[4 * gq + 1] = t.y, byreg[4 * gq + 2] = t.z, byreg[4 * gq + 3] = t.w;
    }
    __builtin_amdgcn_wave_barrier();
  };

  const int ntiles = (t_end - t_begin + kTile - 1) / kTile;
  if (ntiles > 0) {
    stage_load(t_begin);
    stage_store(0);
  }
  __syncthreads();
  for (int it = 0; it < ntiles; ++it) {
    const int buf = it & 1;
    const int t0 = t_begin + it * kTile;
    const bool more = it + 1 < ntiles;
    if (more) stage_load(t0 + kTile);

    // (causal: a wave whose owners all lie on the masked side of this tile has nothing to add)
    const bool active = wave_live && (!p.causal || (KOWN ? t0 + kTile - 1 >= wfirst : t0 <= wfirst + 31));
    if (active) {
      f32x16 acc1, acc2;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc1[r] = 0.0f, acc2[r] = 0.0f;
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        const u32x4 fa = *reinterpret_cast<const u32x4*>(&tx[buf][tile_off<DPAD>(frow, 2 * ks + fhalf)]);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa),
                                                       __builtin_bit_cast(bf16x8, of1[ks]), acc1, 0, 0, 0);
      }
      if constexpr (BWD) {
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
          const u32x4 fa = *reinterpret_cast<const u32x4*>(&ty[buf][tile_off<DPAD>(frow, 2 * ks + fhalf)]);
          acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa),
                                                         __builtin_bit_cast(bf16x8, of2[ks]), acc2, 0, 0, 0);
        }
      }

      // ---- per element: register r is streamed row t0 + acc_row(r, fhalf) ----
      float sv[16], sw[KOWN ? 16 : 1];
      float kf[MODE == MODE_FWD ? 16 : 1];
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const int tb = 8 * gq + 4 * fhalf;
        const float4 va = *reinterpret_cast<const float4*>(&side_a[buf][tb]);
        const float ta[4] = {va.x, va.y, va.z, va.w};
        float tbv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (KOWN) {
          const float4 vb = *reinterpret_cast<const float4*>(&side_b[buf][tb]);
          tbv[0] = vb.x, tbv[1] = vb.y, tbv[2] = vb.z, tbv[3] = vb.w;
        }
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          const int r = 4 * gq + x;
          const int ts = t0 + tb + x;
          const int qi = KOWN ? ts : oi, kj = KOWN ? oi : ts;
          const bool kvalid = KOWN ? my_kv : ta[x] != 0.0f;
          const bool okr = ovalid & (ts < t_end) & kvalid & (!p.causal | (kj <= qi));
          const float kfr = keep_factor(p, hbase, qi, kj);
          const float s = acc1[r] * p.scale;
          if constexpr (MODE == MODE_FWD) {
            sv[r] = okr ? s : kNegInf;
            kf[r] = kfr;
          } else {
            const float lse = KOWN ? ta[x] : my_lse;
            const float delta = KOWN ? tbv[x] : my_delta;
            const float pv = okr ? __expf(s - lse) : 0.0f;
            sv[r] = okr ? pv * (kfr * acc2[r] - delta) : 0.0f;   // dS
            if constexpr (KOWN) sw[r] = pv * kfr;                 // P~
          }
        }
      }

      u32x4 pa[2];
      if constexpr (MODE == MODE_FWD) {
        float top = sv[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) top = fmaxf(top, sv[r]);
        top = fmaxf(top, __shfl_xor(top, 32, 64));
        const float m_new = fmaxf(m_run, top);
        // (an allowed element has a finite s <= m_new; while no key has been allowed m_new is -inf and nothing is added)
        const float alpha = m_new > kNegInf ? __expf(m_run - m_new) : 1.0f;
        float zs = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float pv = sv[r] > kNegInf ? __expf(sv[r] - m_new) : 0.0f;
          zs += pv;
          sv[r] = pv * kf[r];
        }
        z_run = z_run * alpha + zs;
        m_run = m_new;
        float al[16];
        lane_to_reg(alpha, al);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc_a[dt][r] *= al[r];
        pack16(sv, pa);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2)
            acc_a[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, pa[s2]),
                                                                __builtin_bit_cast(bf16x8, gather_b(ty[buf], dt, s2)),
                                                                acc_a[dt], 0, 0, 0);
      } else {
        pack16(sv, pa);   // dS: dQ += dS K, or dK += dS Q (B from the X tile)
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2)
            acc_a[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, pa[s2]),
                                                                __builtin_bit_cast(bf16x8, gather_b(tx[buf], dt, s2)),
                                                                acc_a[dt], 0, 0, 0);
        if constexpr (KOWN) {
          u32x4 pb[2];
          pack16(sw, pb);   // P~: dV += P~ dO (B from the Y tile)
#pragma unroll
          for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
              acc_b[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, pb[s2]),
                                                                  __builtin_bit_cast(bf16x8, gather_b(ty[buf], dt, s2)),
                                                                  acc_b[dt], 0, 0, 0);
        }
      }
    }

    if (more) stage_store(buf ^ 1);
    __syncthreads();
  }

  // ---- results: accumulator tile dt holds column 32 dt + frow of owner rows acc_row(r, fhalf) ----
  float rowf[16];
  if constexpr (MODE == MODE_FWD) {
    const float z = z_run + __shfl_xor(z_run, 32, 64);
    // a row with no allowed key: o = 0 and lse = -inf (include/krs.h)
    lane_to_reg(z > 0.0f ? 1.0f / z : 0.0f, rowf);
    if (fhalf == 0 && ovalid) p.lse[bh * l + oi] = z > 0.0f ? m_run + logf(z) : kNegInf;
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) rowf[r] = p.scale;
  }
  auto store_tile = [&](void* dst, int64_t ldd, const f32x16* acc, bool scaled) {
    uint16_t* out = reinterpret_cast<uint16_t*>(dst) + col0;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const int col = 32 * dt + frow;
      if (col >= dh) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wfirst + acc_row(r, fhalf);
        if (row >= l) continue;
        out[(tok0 + row) * ldd + col] = f32_to_bf16(scaled ? acc[dt][r] * rowf[r] : acc[dt][r]);
      }
    }
  };
  if constexpr (MODE == MODE_FWD) store_tile(p.out, p.ldo, acc_a, true);
  if constexpr (MODE == MODE_DQ) store_tile(p.dq, p.lddq, acc_a, true);
  if constexpr (KOWN) {
    if (p.dk) store_tile(p.dk, p.lddk, acc_a, true);
    if (p.dv) store_tile(p.dv, p.lddv, acc_b, false);
  }
}

// ---- delta_i = sum_d dO_id o_id, one thread per (b, h, i) ----
template <typename T>
__global__ __launch_bounds__(256) void delta_kernel(const Params p, int64_t rows) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows) return;
  const int64_t bh = idx / p.l;
  const int i = (int)(idx - bh * p.l);
  const int64_t tok = (bh / p.h) * p.l + i;
  const int col0 = (int)(bh % p.h) * p.dh;
  const T* o = reinterpret_cast<const T*>(p.out) + tok * p.ldo + col0;
  const T* g = reinterpret_cast<const T*>(p.dout) + tok * p.lddo + col0;
  float acc = 0.0f;
  for (int d = 0; d < p.dh; ++d) acc = fmaf(load1(g + d), load1(o + d), acc);
  p.delta[idx] = acc;
}

// ---- the generic path: one workgroup per (b, h, row) ----
constexpr int kGenThreads = 256;

// sum or max of one value per thread, in a fixed tree; every thread gets the result
template <bool MAX>
__device__ __forceinline__ float block_reduce(float v, float* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = kGenThreads / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = MAX ? fmaxf(red[tid], red[tid + s]) : red[tid] + red[tid + s];
    __syncthreads();
  }
  return red[0];
}

template <typename T>
__device__ __forceinline__ float dot_row(const float* a, const T* b, int d) {
  float acc = 0.0f;
  for (int x = 0; x < d; ++x) acc = fmaf(a[x], load1(b + x), acc);
  return acc;
}

struct GenRow {
  int64_t bh, tok0;
  int row, col0;
};
__device__ __forceinline__ GenRow gen_row(const Params& p) {
  GenRow g;
  g.bh = blockIdx.x / p.l;
  g.row = (int)(blockIdx.x - g.bh * p.l);
  g.tok0 = (g.bh / p.h) * p.l;
  g.col0 = (int)(g.bh % p.h) * p.dh;
  return g;
}

template <typename T>
__global__ __launch_bounds__(kGenThreads) void gen_fwd_kernel(const Params p) {
  __shared__ float qs[seqattn::kMaxDh];
  __shared__ float sc[seqattn::kMaxL];
  __shared__ float red[kGenThreads];
  const int tid = threadIdx.x, l = p.l, dh = p.dh;
  const GenRow g = gen_row(p);
  const int i = g.row;
  const T* Q = reinterpret_cast<const T*>(p.q) + g.col0;
  const T* K = reinterpret_cast<const T*>(p.k) + g.col0;
  const T* V = reinterpret_cast<const T*>(p.v) + g.col0;
  T* O = reinterpret_cast<T*>(p.out) + (g.tok0 + i) * p.ldo + g.col0;
  for (int d = tid; d < dh; d += kGenThreads) qs[d] = load1(Q + (g.tok0 + i) * p.ldq + d);
  __syncthreads();
  const uint32_t hbase = hash_base_of(p, g.bh);
  const int jn = p.causal ? i + 1 : l;
  float top = kNegInf;
  for (int j = tid; j < jn; j += kGenThreads) {
    const bool ok = !p.kv || p.kv[g.tok0 + j] != 0;
    const float s = ok ? p.scale * dot_row(qs, K + (g.tok0 + j) * p.ldk, dh) : kNegInf;
    sc[j] = s;
    top = fmaxf(top, s);
  }
  const float m = block_reduce<true>(top, red);
  if (m == kNegInf) {   // no allowed key: o = 0, lse = -inf
    for (int d = tid; d < dh; d += kGenThreads) store1(O + d, 0.0f);
    if (tid == 0) p.lse[g.bh * l + i] = kNegInf;
    return;
  }
  float zs = 0.0f;
  for (int j = tid; j < jn; j += kGenThreads) {
    const float pv = sc[j] > kNegInf ? expf(sc[j] - m) : 0.0f;
    zs += pv;
    sc[j] = pv * keep_factor(p, hbase, i, j);
  }
  const float z = block_reduce<false>(zs, red);   // (its barriers also publish sc)
  for (int d = tid; d < dh; d += kGenThreads) {
    float acc = 0.0f;
    for (int j = 0; j < jn; ++j) acc = fmaf(sc[j], load1(V + (g.tok0 + j) * p.ldv + d), acc);
    store1(O + d, acc / z);
  }
  if (tid == 0) p.lse[g.bh * l + i] = m + logf(z);
}

template <typename T>
__global__ __launch_bounds__(kGenThreads) void gen_dq_kernel(const Params p) {
  __shared__ float qs[seqattn::kMaxDh];
  __shared__ float gs[seqattn::kMaxDh];
  __shared__ float sc[seqattn::kMaxL];
  const int tid = threadIdx.x, l = p.l, dh = p.dh;
  const GenRow g = gen_row(p);
  const int i = g.row;
  const T* Q = reinterpret_cast<const T*>(p.q) + g.col0;
  const T* K = reinterpret_cast<const T*>(p.k) + g.col0;
  const T* V = reinterpret_cast<const T*>(p.v) + g.col0;
  const T* G = reinterpret_cast<const T*>(p.dout) + g.col0;
  T* DQ = reinterpret_cast<T*>(p.dq) + (g.tok0 + i) * p.lddq + g.col0;
  for (int d = tid; d < dh; d += kGenThreads) {
    qs[d] = load1(Q + (g.tok0 + i) * p.ldq + d);
    gs[d] = load1(G + (g.tok0 + i) * p.lddo + d);
  }
  __syncthreads();
  const uint32_t hbase = hash_base_of(p, g.bh);
  const float lse = p.lse[g.bh * l + i], delta = p.delta[g.bh * l + i];
  const int jn = p.causal ? i + 1 : l;
  for (int j = tid; j < jn; j += kGenThreads) {
    const bool ok = (!p.kv || p.kv[g.tok0 + j] != 0) && lse > kNegInf;
    float ds = 0.0f;
    if (ok) {
      const float pv = expf(p.scale * dot_row(qs, K + (g.tok0 + j) * p.ldk, dh) - lse);
      const float dp = dot_row(gs, V + (g.tok0 + j) * p.ldv, dh);
      ds = pv * (keep_factor(p, hbase, i, j) * dp - delta);
    }
    sc[j] = ds;
  }
  __syncthreads();
  for (int d = tid; d < dh; d += kGenThreads) {
    float acc = 0.0f;
    for (int j = 0; j < jn; ++j) acc = fmaf(sc[j], load1(K + (g.tok0 + j) * p.ldk + d), acc);
    store1(DQ + d, p.scale * acc);
  }
}

template <typename T>
__global__ __launch_bounds__(kGenThreads) void gen_dkv_kernel(const Params p) {
  __shared__ float ks[seqattn::kMaxDh];
  __shared__ float vs[seqattn::kMaxDh];
  __shared__ float sp[seqattn::kMaxL];
  __shared__ float sd[seqattn::kMaxL];
  const int tid = threadIdx.x, l = p.l, dh = p.dh;
  const GenRow g = gen_row(p);
  const int j = g.row;
  const T* Q = reinterpret_cast<const T*>(p.q) + g.col0;
  const T* K = reinterpret_cast<const T*>(p.k) + g.col0;
  const T* V = reinterpret_cast<const T*>(p.v) + g.col0;
  const T* G = reinterpret_cast<const T*>(p.dout) + g.col0;
  for (int d = tid; d < dh; d += kGenThreads) {
    ks[d] = load1(K + (g.tok0 + j) * p.ldk + d);
    vs[d] = load1(V + (g.tok0 + j) * p.ldv + d);
  }
  __syncthreads();
  const uint32_t hbase = hash_base_of(p, g.bh);
  const bool kvalid = !p.kv || p.kv[g.tok0 + j] != 0;
  const int i0 = p.causal ? j : 0;
  for (int i = i0 + tid; i < l; i += kGenThreads) {
    const float lse = p.lse[g.bh * l + i];
    float pt = 0.0f, ds = 0.0f;
    if (kvalid && lse > kNegInf) {
      const float pv = expf(p.scale * dot_row(ks, Q + (g.tok0 + i) * p.ldq, dh) - lse);
      const float dp = dot_row(vs, G + (g.tok0 + i) * p.lddo, dh);
      const float kf = keep_factor(p, hbase, i, j);
      pt = pv * kf;
      ds = pv * (kf * dp - p.delta[g.bh * l + i]);
    }
    sp[i] = pt;
    sd[i] = ds;
  }
  __syncthreads();
  for (int d = tid; d < dh; d += kGenThreads) {
    float av = 0.0f, ak = 0.0f;
    for (int i = i0; i < l; ++i) {
      av = fmaf(sp[i], load1(G + (g.tok0 + i) * p.lddo + d), av);
      ak = fmaf(sd[i], load1(Q + (g.tok0 + i) * p.ldq + d), ak);
    }
    if (p.dv) store1(reinterpret_cast<T*>(p.dv) + (g.tok0 + j) * p.lddv + g.col0 + d, av);
    if (p.dk) store1(reinterpret_cast<T*>(p.dk) + (g.tok0 + j) * p.lddk + g.col0 + d, p.scale * ak);
  }
}

// ---- host ----
// (one record per process, not per thread: torch runs a backward on an autograd thread, and the caller that asks for
//  the route afterwards is another; kernel and dpad travel in one word)
std::atomic<uint32_t> g_route{0};
inline void set_route(int kernel, int dpad) { g_route.store((uint32_t)kernel << 16 | (uint32_t)dpad); }

inline bool vec_ok(const void* p, int64_t ld) { return !p || (aligned16(p) && ld % 8 == 0); }

template <int MODE>
void launch_fast(const Params& p, const seqattn::Plan& pl, hipStream_t st) {
  const dim3 grid((unsigned)pl.groups), block(kThreads);
#define KRS_ATTN(DPAD_)                                                                       \
  {                                                                                           \
    if (pl.vec) hipLaunchKernelGGL((attn_kernel<DPAD_, MODE, true>), grid, block, 0, st, p);  \
    else hipLaunchKernelGGL((attn_kernel<DPAD_, MODE, false>), grid, block, 0, st, p);        \
  }
  if (pl.dpad == 32) KRS_ATTN(32)
  else if (pl.dpad == 64) KRS_ATTN(64)
  else KRS_ATTN(128)
#undef KRS_ATTN
}

int check_common(const char* what, const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                 int dtype, int64_t b, int64_t h, int64_t l, int64_t dh, float dropout_p, const int64_t* draw, bool aligned,
                 seqattn::Plan& pl) {
  pl = seqattn::plan(b, h, l, dh, dtype, aligned);
  if (pl.status == seqattn::kInvalid)
    return fail(KRS_ERR_INVALID, "%s: b=%lld h=%lld l=%lld dh=%lld dtype=%d: needs %s", what, (long long)b, (long long)h,
                (long long)l, (long long)dh, dtype, pl.why);
  KRS_REQUIRE(dropout_p >= 0.0f && dropout_p < 1.0f, "%s: dropout_p %g outside [0, 1)", what, (double)dropout_p);
  KRS_REQUIRE(ldq >= h * dh && ldk >= h * dh && ldv >= h * dh, "%s: token stride below h * dh", what);
  if (pl.status == seqattn::kUnsupported)
    return fail(KRS_ERR_UNSUPPORTED, "%s: b=%lld h=%lld l=%lld dh=%lld: supported is %s", what, (long long)b, (long long)h,
                (long long)l, (long long)dh, pl.why);
  if (pl.kernel == seqattn::kRouteNone) return KRS_OK;
  KRS_REQUIRE(q && k && v, "%s: null operand", what);
  KRS_REQUIRE(dropout_p == 0.0f || draw, "%s: dropout needs the draw counter", what);
  return KRS_OK;
}

void fill_common(Params& p, const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, int64_t h,
                 int64_t l, int64_t dh, const uint8_t* key_valid, int causal, float scale, float dropout_p, uint64_t seed,
                 const int64_t* draw, const seqattn::Plan& pl) {
  p.q = q, p.k = k, p.v = v, p.ldq = ldq, p.ldk = ldk, p.ldv = ldv;
  p.kv = key_valid;
  p.h = (int)h, p.l = (int)l, p.dh = (int)dh, p.causal = causal != 0;
  p.scale = scale;
  p.dropout = dropout_p > 0.0f;
  p.thr = seqattn::drop_threshold(dropout_p);
  p.inv_keep = 1.0f / (1.0f - dropout_p);
  p.seed_lo = (uint32_t)seed, p.seed_hi = (uint32_t)(seed >> 32);
  p.draw = p.dropout ? draw : nullptr;
  p.oblocks = pl.oblocks;
}

}  // namespace
}  // namespace krs

extern "C" size_t krs_seq_attn_workspace_bytes(int64_t b, int64_t h, int64_t l, int64_t dh, int dtype) {
  (void)dh, (void)dtype;
  return krs::seqattn::workspace_bytes(b, h, l);
}

extern "C" int krs_seq_attn_last_route(int* kernel, int* dpad) {
  const uint32_t r = krs::g_route.load();
  if (kernel) *kernel = (int)(r >> 16);
  if (dpad) *dpad = (int)(r & 0xffffu);
  return (int)(r >> 16);
}

extern "C" int krs_seq_attn_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                int dtype, int64_t b, int64_t h, int64_t l, int64_t dh, const uint8_t* key_valid,
                                int causal, float scale, float dropout_p, uint64_t seed, const int64_t* draw, void* out,
                                int64_t ldo, float* lse, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace krs;
  (void)workspace, (void)workspace_bytes;   // (the forward keeps nothing outside out and lse)
  const char* what = "krs_seq_attn_fwd";
  set_route(KRS_SEQ_ATTN_NONE, 0);
  seqattn::Plan pl;
  const bool aligned = vec_ok(q, ldq) && vec_ok(k, ldk) && vec_ok(v, ldv);
  const int rc = check_common(what, q, ldq, k, ldk, v, ldv, dtype, b, h, l, dh, dropout_p, draw, aligned, pl);
  if (rc != KRS_OK || pl.kernel == seqattn::kRouteNone) return rc;
  KRS_REQUIRE(out && lse, "%s: null output", what);
  KRS_REQUIRE(ldo >= h * dh, "%s: output token stride below h * dh", what);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  Params p{};
  fill_common(p, q, ldq, k, ldk, v, ldv, h, l, dh, key_valid, causal, scale, dropout_p, seed, draw, pl);
  p.out = out, p.ldo = ldo, p.lse = lse;
  if (pl.kernel == seqattn::kRouteFast) {
    launch_fast<MODE_FWD>(p, pl, st);
  } else if (dtype == KRS_BF16) {
    hipLaunchKernelGGL(gen_fwd_kernel<uint16_t>, dim3((unsigned)pl.groups), dim3(kGenThreads), 0, st, p);
  } else {
    hipLaunchKernelGGL(gen_fwd_kernel<float>, dim3((unsigned)pl.groups), dim3(kGenThreads), 0, st, p);
  }
  KRS_CHECK_LAUNCH("krs_seq_attn_fwd kernel");
  set_route(pl.kernel, pl.dpad);
  return KRS_OK;
}

extern "C" int krs_seq_attn_bwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                int dtype, int64_t b, int64_t h, int64_t l, int64_t dh, const uint8_t* key_valid,
                                int causal, float scale, float dropout_p, uint64_t seed, const int64_t* draw,
                                const void* out, int64_t ldo, const void* dout, int64_t lddo, const float* lse, void* dq,
                                int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv, void* workspace,
                                size_t workspace_bytes, void* stream) {
  using namespace krs;
  const char* what = "krs_seq_attn_bwd";
  set_route(KRS_SEQ_ATTN_NONE, 0);
  seqattn::Plan pl;
  const bool aligned = vec_ok(q, ldq) && vec_ok(k, ldk) && vec_ok(v, ldv) && vec_ok(dout, lddo);
  const int rc = check_common(what, q, ldq, k, ldk, v, ldv, dtype, b, h, l, dh, dropout_p, draw, aligned, pl);
  if (rc != KRS_OK) return rc;
  KRS_REQUIRE(dq || dk || dv, "%s: no gradient is wanted", what);
  KRS_REQUIRE((!dq || lddq >= h * dh) && (!dk || lddk >= h * dh) && (!dv || lddv >= h * dh) && ldo >= h * dh &&
                  lddo >= h * dh,
              "%s: token stride below h * dh", what);
  if (pl.kernel == seqattn::kRouteNone) return KRS_OK;
  KRS_REQUIRE(out && dout && lse, "%s: null out, dout or lse", what);
  const size_t need = seqattn::workspace_bytes(b, h, l);
  if (!workspace || workspace_bytes < need)
    return fail(KRS_ERR_WORKSPACE, "%s: needs %zu workspace bytes, got %zu", what, need, workspace_bytes);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  Params p{};
  fill_common(p, q, ldq, k, ldk, v, ldv, h, l, dh, key_valid, causal, scale, dropout_p, seed, draw, pl);
  p.out = const_cast<void*>(out), p.ldo = ldo, p.dout = dout, p.lddo = lddo;
  p.lse = const_cast<float*>(lse), p.delta = reinterpret_cast<float*>(workspace);
  p.dq = dq, p.dk = dk, p.dv = dv, p.lddq = lddq, p.lddk = lddk, p.lddv = lddv;
  const int64_t rows = b * h * l;
  const bool bf16 = dtype == KRS_BF16;
  if (bf16) hipLaunchKernelGGL(delta_kernel<uint16_t>, dim3((unsigned)ceil_div(rows, 256)), dim3(256), 0, st, p, rows);
  else hipLaunchKernelGGL(delta_kernel<float>, dim3((unsigned)ceil_div(rows, 256)), dim3(256), 0, st, p, rows);
  KRS_CHECK_LAUNCH("delta_kernel");
  const dim3 ggrid((unsigned)pl.groups), gblock(kGenThreads);
  if (dq) {
    if (pl.kernel == seqattn::kRouteFast) launch_fast<MODE_DQ>(p, pl, st);
    else if (bf16) hipLaunchKernelGGL(gen_dq_kernel<uint16_t>, ggrid, gblock, 0, st, p);
    else hipLaunchKernelGGL(gen_dq_kernel<float>, ggrid, gblock, 0, st, p);
    KRS_CHECK_LAUNCH("krs_seq_attn_bwd dq sweep");
  }
  if (dk || dv) {
    if (pl.kernel == seqattn::kRouteFast) launch_fast<MODE_DKV>(p, pl, st);
    else if (bf16) hipLaunchKernelGGL(gen_dkv_kernel<uint16_t>, ggrid, gblock, 0, st, p);
    else hipLaunchKernelGGL(gen_dkv_kernel<float>, ggrid, gblock, 0, st, p);
    KRS_CHECK_LAUNCH("krs_seq_attn_bwd dk/dv sweep");
  }
  set_route(pl.kernel, pl.dpad);
  return KRS_OK;
}
