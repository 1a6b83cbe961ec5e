// K30 -- the shared-negative sampled softmax of a sequence model: all tokens of a group (a sequence, or the batch)
// share N sampled negatives, so the scores are a [Lg, d] x [d, N] product per group whose streamed side is GATHERED
// from the item table by id.  Keys and values are the same rows: d loss / d emb_t = softmax(e_t R^T) R minus the
// positive's row, so one sweep leaves the loss and the embedding gradient together.  The [T, N] scores are never
// stored.  The arithmetic, the dead-token rule and the order of every sum are include/krs.h's (K30).
//
// Fast route (emb bf16, d <= 128; table bf16 or fp32, rounded to bf16 as it is staged): K19's body, the
// owner-on-the-lane tile of krs_owner_tile.h, with ONE streamed tile array -- the score product's A operand and the
// second product's B operand are the same LDS image.
//   tokens_kernel    owner = 128 tokens of one group (a wave: 32 as the B operand).  The group's negative rows are
//                    gathered into double-buffered tiles of 32: the ids of tile i + 2 are loaded while the rows of tile
//                    i + 1 are requested (registers) and tile i is computed; the rows go to the other buffer after the
//                    compute; one barrier per step.  The tile's ids sit beside it in LDS: hit removal compares them
//                    with the owner's positive id.  Online (m, Z) per lane as K19's forward; P~ (bf16) is the A operand
//                    of acc += P~ R.  THE POSITIVE enters as the diagonal of one extra tile per wave (the 32 positives
//                    of its owners, kept in LDS to the end): it seeds (m, Z) = (x_t0, 1) and takes no part in the
//                    second product; its term gpos_t r_pos(t) is added in fp32 when demb is written.
//   negs_kernel      owner = 128 negatives of one group (rows gathered once into registers); the group's token tiles
//                    stream (emb, lse, c_t, pos id); the score tile is recomputed, c_t p_tj (bf16) is the A operand of
//                    dneg += P^T E.  K19's dk sweep without dv.  With `splits` > 1 a workgroup streams a run of whole
//                    tiles and writes a partial that reduce_kernel adds in split order.
// Generic route (fp32 anywhere, bf16 above d = 128): fp32 FMA, one workgroup per token with its 1 + N scores in LDS,
// then one workgroup per negative.  Same masks, same owners, same order rule; there for coverage and as the second
// implementation the tests hold the fast route against.
// No float atomics; every output element has one owner; no kernel uses scratch.
#include "krs_owner_tile.h"
#include "sampled_softmax_plan.h"

namespace krs {
namespace {

using ssm::kThreads;
constexpr int kTile = ssm::kTile;
constexpr int kOwn = ssm::kOwn;
static_assert(kTile == kOwnerTile && kOwn == 4 * kOwnerTile && kThreads == 256, "four waves of krs_owner_tile.h's tile");

struct Args {
  const void* emb;
  const void* table;
  const void* pos;
  const void* neg;
  const float *w, *pos_q, *neg_q;
  float *loss, *lse, *gpos;
  void* demb;
  float* dneg;
  int* err;
  const float* w_partials;   // the W pass's w_blocks partials (with weights)
  float* cw;                 // [tokens]: c_t, 0 for a dead token
  float* lpart;              // [grid_tokens]: sum w_t l_t of a workgroup
  float* dpart;              // [splits][g * n * d] with splits > 1
  int64_t lde, ldt, ldd, tokens, vocab, lg, gn;
  int d, n, is64, remove, w_blocks, emb_dtype, table_dtype;
  int oblocks, nblocks, splits, split_tiles, grid_tokens;
  float count;               // S without weights: float(tokens)
};

// the W pass's partials in workgroup order
__device__ __forceinline__ float w_sum(const Args& a) {
  float s = 0.0f;
  for (int j = 0; j < a.w_blocks; ++j) s += a.w_partials[j];
  return s;
}
// S, the same value in every thread (one barrier with weights)
__device__ __forceinline__ float total_weight(const Args& a, float* shared) {
  if (!a.w) return a.count;
  if (threadIdx.x == 0) *shared = w_sum(a);
  __syncthreads();
  return *shared;
}

// what a token is to the loss: its weight, its positive id (-1 when dead) and c_t (0 when dead)
struct Token {
  float w, c;
  int64_t pos;
  bool bad;      // a live weight with a positive id outside the table
};
__device__ __forceinline__ Token token_of(const Args& a, int64_t t, bool in, float S) {
  Token k = {0.0f, 0.0f, -1, false};
  if (!in) return k;
  k.w = a.w ? a.w[t] : 1.0f;
  if (k.w == 0.0f || S == 0.0f) return k;
  const int64_t id = ld_index(a.pos, a.is64, t);
  if (id < 0 || id >= a.vocab) {
    k.bad = true;
    return k;
  }
  k.pos = id;
  k.c = k.w / S;
  return k;
}

// 8 columns of a table row from element e0 as bf16 (round to nearest even); zero beyond d and for a row not asked for
template <typename TT, bool VEC>
__device__ __forceinline__ u32x4 load_row_chunk(const TT* at, int e0, int d, bool valid) {
  if constexpr (sizeof(TT) == 2) {
    return load_chunk<VEC>(at, e0, d, valid);
  } else {
    u32x4 v = {0u, 0u, 0u, 0u};
    if (!valid || e0 >= d) return v;
    float f[8];
    if constexpr (VEC) {
      const float4 lo = *reinterpret_cast<const float4*>(at), hi = *reinterpret_cast<const float4*>(at + 4);
      f[0] = lo.x, f[1] = lo.y, f[2] = lo.z, f[3] = lo.w, f[4] = hi.x, f[5] = hi.y, f[6] = hi.z, f[7] = hi.w;
    } else {
#pragma unroll
      for (int x = 0; x < 8; ++x) f[x] = e0 + x < d ? at[x] : 0.0f;
    }
    return (u32x4){pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]), pack_bf16x2(f[4], f[5]), pack_bf16x2(f[6], f[7])};
  }
}

// ---- the fast route -------------------------------------------------------------------------------------------------
// What both sweeps share: the score chain over a tile, the gather of the second product's B operand (gather_at's three
// integers written out, as in attn_kernel) and the lane-to-register exchange of a per-owner value.
template <int DPAD>
struct OwnerTile {
  static constexpr int NKS = DPAD / 16, DT = DPAD / 32, CH = DPAD / 8;
  static constexpr int TILE_BYTES = kTile * DPAD * 2;
  static constexpr int U = (kTile * CH + kThreads - 1) / kThreads;   // chunks of a tile a thread stages

  static __device__ __forceinline__ f32x16 scores(const char* tile, const u32x4 (&own)[NKS], int frow, int fhalf) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      const u32x4 fa = *reinterpret_cast<const u32x4*>(tile + tile_off<DPAD>(frow, 2 * ks + fhalf));
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa), __builtin_bit_cast(bf16x8, own[ks]),
                                                    acc, 0, 0, 0);
    }
    return acc;
  }
  // acc[dt] += A (16 per-lane values by accumulator register, rounded to bf16) x the tile's rows in that order
  static __device__ __forceinline__ void second(const char* tile, const float* sv, f32x16 (&acc)[DT], int lane) {
    const int fhalf = lane >> 5, li = lane & 15, tq = li >> 2, tp = li & 3, chalf = (lane >> 4) & 1;
    u32x4 pa[2];
    pack16(sv, pa);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const int r0 = 16 * s2 + 4 * fhalf, ch = 4 * dt + 2 * chalf + (tp >> 1);
        const u32x2 lo = lds_read_tr16(tile + tile_off<DPAD>(r0 + tq, ch) + 8 * (tp & 1));
        const u32x2 hi = lds_read_tr16(tile + tile_off<DPAD>(r0 + 8 + tq, ch) + 8 * (tp & 1));
        const u32x4 fb = {lo[0], lo[1], hi[0], hi[1]};
        acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, pa[s2]),
                                                          __builtin_bit_cast(bf16x8, fb), acc[dt], 0, 0, 0);
      }
  }
};

// a per-owner value (the same on both lanes of an owner) by accumulator register: owner acc_row(r, fhalf)
__device__ __forceinline__ void lane_to_reg(float v, float* xch, int frow, int fhalf, float* byreg) {
  __builtin_amdgcn_wave_barrier();
  if (fhalf == 0) xch[frow] = v;
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int gq = 0; gq < 4; ++gq) {
    const float4 t = *reinterpret_cast<const float4*>(&xch[8 * gq + 4 * fhalf]);
    byreg[4 * gq] = t.x, byreg[4 * gq + 1] = t.y, byreg[4 * gq + 2] = t.z, byreg[4 * gq + 3] = t.w;
  }
  __builtin_amdgcn_wave_barrier();
}

template <int DPAD, bool VEC, typename TT>
__global__ __launch_bounds__(kThreads) void tokens_kernel(const Args a) {
  using OT = OwnerTile<DPAD>;
  constexpr int NKS = OT::NKS, DT = OT::DT, CH = OT::CH, U = OT::U;
  __shared__ __attribute__((aligned(16))) char tx[2][OT::TILE_BYTES];     // the streamed negatives
  __shared__ __attribute__((aligned(16))) char tp[4][OT::TILE_BYTES];     // a wave's 32 positives
  __shared__ __attribute__((aligned(16))) long long sid[2][kTile];        // the tile's ids, -1: no such item
  __shared__ __attribute__((aligned(16))) float sq[2][kTile];             // the tile's log q
  __shared__ __attribute__((aligned(16))) float xch[4][32];
  __shared__ float part[kOwn];
  __shared__ float s_shared;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int frow = lane & 31, fhalf = lane >> 5;
  const int64_t grp = blockIdx.x / a.oblocks;
  const int oblock = (int)(blockIdx.x % a.oblocks);
  const int d = a.d, n = a.n;
  const int64_t lg = a.lg, tok0 = grp * lg, nbase = grp * n;
  const uint16_t* emb = reinterpret_cast<const uint16_t*>(a.emb);
  const TT* table = reinterpret_cast<const TT*>(a.table);
  const float S = total_weight(a, &s_shared);

  // the owner token of this lane
  const int64_t wfirst = (int64_t)oblock * kOwn + wave * 32;
  const int64_t oi = wfirst + frow;
  const bool in = oi < lg;
  const int64_t t = tok0 + (in ? oi : 0);
  const Token tk = token_of(a, t, in, S);
  const bool live = tk.c != 0.0f;
  const float my_q = live && a.pos_q ? a.pos_q[t] : 0.0f;
  u32x4 own[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const int e0 = (2 * ks + fhalf) * 8;
    own[ks] = load_chunk<VEC>(emb + t * a.lde + e0, e0, d, live);
    if constexpr (!VEC) __builtin_amdgcn_sched_barrier(0);
  }

  // the wave's positives: row r of tp[wave] is table[pos] of owner r (zeros for a dead one)
  for (int i = lane; i < kTile * CH; i += 64) {       // (kTile * CH is a multiple of 64: every lane takes every trip)
    const int srow = i / CH, ch = i % CH;
    const int64_t id = __shfl(tk.pos, srow, 64);
    const u32x4 v = load_row_chunk<TT, VEC>(table + (id < 0 ? 0 : id) * a.ldt + ch * 8, ch * 8, d, id >= 0);
    *reinterpret_cast<u32x4*>(&tp[wave][tile_off<DPAD>(srow, ch)]) = v;
    if constexpr (!VEC) __builtin_amdgcn_sched_barrier(0);
  }

  // staging of a streamed tile: ids a tile ahead of the rows, rows in registers a tile ahead of LDS
  int64_t nid[U], nsid = -1, sidr = -1;
  float nsq = 0.0f, sqr = 0.0f;
  u32x4 sreg[U];
  auto neg_id = [&](int j) -> int64_t {
    if (j >= n) return -1;
    const int64_t id = ld_index(a.neg, a.is64, nbase + j);
    return id >= 0 && id < a.vocab ? id : -1;
  };
  auto ids_load = [&](int j0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int srow = (tid + u * kThreads) / CH;
      nid[u] = srow < kTile ? neg_id(j0 + srow) : -1;
    }
    if (tid < kTile) {
      nsid = neg_id(j0 + tid);
      nsq = nsid >= 0 && a.neg_q ? a.neg_q[nbase + j0 + tid] : 0.0f;
    }
  };
  auto rows_load = [&]() {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int ch = (tid + u * kThreads) % CH;
      sreg[u] = load_row_chunk<TT, VEC>(table + (nid[u] < 0 ? 0 : nid[u]) * a.ldt + ch * 8, ch * 8, d, nid[u] >= 0);
      if constexpr (!VEC) __builtin_amdgcn_sched_barrier(0);
    }
    sidr = nsid, sqr = nsq;
  };
  auto stage_store = [&](int buf) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = tid + u * kThreads;
      if (i < kTile * CH) *reinterpret_cast<u32x4*>(&tx[buf][tile_off<DPAD>(i / CH, i % CH)]) = sreg[u];
    }
    if (tid < kTile) sid[buf][tid] = sidr, sq[buf][tid] = sqr;
  };

  const int ntiles = (n + kTile - 1) / kTile;
  ids_load(0);
  rows_load();
  stage_store(0);
  if (ntiles > 1) ids_load(kTile);
  __syncthreads();

  f32x16 acc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[dt][r] = 0.0f;
  const bool wave_live = wfirst < lg;

  // the positive: the diagonal of the wave's own tile seeds (m, Z) = (x_t0, 1); Z is this lane's share (K19)
  float x0 = 0.0f;
  if (wave_live) {
    const f32x16 s0 = OT::scores(tp[wave], own, frow, fhalf);
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (acc_row(r, fhalf) == frow) x0 = s0[r];
    x0 += __shfl_xor(x0, 32, 64);       // (the other lane of the owner holds 0)
    x0 -= my_q;
  }
  float m_run = live ? x0 : kNegInf, z_run = live && fhalf == 0 ? 1.0f : 0.0f;

  for (int it = 0; it < ntiles; ++it) {
    const int buf = it & 1;
    const bool more = it + 1 < ntiles;
    if (more) {
      rows_load();
      if (it + 2 < ntiles) ids_load((it + 2) * kTile);
    }
    if (wave_live) {
      const f32x16 s1 = OT::scores(tx[buf], own, frow, fhalf);
      float sv[16];
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {       // register r is tile row acc_row(r, fhalf) = 8 gq + 4 fhalf + x
        const int tb = 8 * gq + 4 * fhalf;
        const float4 qv = *reinterpret_cast<const float4*>(&sq[buf][tb]);
        const float q4[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          const int64_t id = sid[buf][tb + x];
          const bool ok = live & (id >= 0) & !(a.remove && id == tk.pos);
          sv[4 * gq + x] = ok ? s1[4 * gq + x] - q4[x] : kNegInf;
        }
      }
      float top = sv[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) top = fmaxf(top, sv[r]);
      top = fmaxf(top, __shfl_xor(top, 32, 64));
      const float m_new = fmaxf(m_run, top);
      const float alpha = m_new > kNegInf ? __expf(m_run - m_new) : 1.0f;
      float zs = 0.0f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        sv[r] = sv[r] > kNegInf ? __expf(sv[r] - m_new) : 0.0f;
        zs += sv[r];
      }
      z_run = z_run * alpha + zs;
      m_run = m_new;
      float al[16];
      lane_to_reg(alpha, xch[wave], frow, fhalf, al);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[dt][r] *= al[r];
      OT::second(tx[buf], sv, acc, lane);
    }
    if (more) stage_store(buf ^ 1);
    __syncthreads();
  }

  // ---- per token: lse, gpos, c_t and the loss term ----
  const float z = z_run + __shfl_xor(z_run, 32, 64);
  const float lse = live ? m_run + logf(z) : 0.0f;
  const float gp = live ? tk.c * (expf(x0 - lse) - 1.0f) : 0.0f;
  if (fhalf == 0) {
    if (in) a.lse[t] = lse, a.gpos[t] = gp, a.cw[t] = tk.c;
    part[wave * 32 + frow] = live ? tk.w * (lse - x0) : 0.0f;
  }
  if (tk.bad && a.err) atomicOr(a.err, KRS_FLAG_ID_OUT_OF_RANGE);

  // ---- demb: accumulator tile dt holds column 32 dt + frow of the owners acc_row(r, fhalf) ----
  if (wave_live) {
    float ra[16], rb[16];
    lane_to_reg(live ? tk.c / z : 0.0f, xch[wave], frow, fhalf, ra);
    lane_to_reg(gp, xch[wave], frow, fhalf, rb);
    uint16_t* out = reinterpret_cast<uint16_t*>(a.demb);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const int col = 32 * dt + frow;
      if (col >= d) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int orow = acc_row(r, fhalf);
        if (wfirst + orow >= lg) continue;
        const float rp = bf16_to_f32(*reinterpret_cast<const uint16_t*>(&tp[wave][tile_off<DPAD>(orow, col >> 3) + 2 * (col & 7)]));
        // (a dead owner: ra = 0, and nothing the products hold may reach its row)
        const float v = ra[r] != 0.0f ? fmaf(acc[dt][r], ra[r], rb[r] * rp) : 0.0f;
        out[(tok0 + wfirst + orow) * a.ldd + col] = f32_to_bf16(v);
      }
    }
  }

  __syncthreads();
  for (int o = kOwn / 2; o > 0; o >>= 1) {
    if (tid < o) part[tid] += part[tid + o];
    __syncthreads();
  }
  if (tid == 0) a.lpart[blockIdx.x] = part[0];
}

template <int DPAD, bool VEC, typename TT>
__global__ __launch_bounds__(kThreads) void negs_kernel(const Args a) {
  using OT = OwnerTile<DPAD>;
  constexpr int NKS = OT::NKS, DT = OT::DT, CH = OT::CH, U = OT::U;
  __shared__ __attribute__((aligned(16))) char tx[2][OT::TILE_BYTES];     // the streamed tokens' emb rows
  __shared__ __attribute__((aligned(16))) long long spos[2][kTile];       // their positive ids (-1: nothing to remove)
  __shared__ __attribute__((aligned(16))) float slse[2][kTile];
  __shared__ __attribute__((aligned(16))) float sc[2][kTile];             // c_t, 0: the row takes no part

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int frow = lane & 31, fhalf = lane >> 5;
  const int split = (int)(blockIdx.x % a.splits);
  const int nb = (int)((blockIdx.x / a.splits) % a.nblocks);
  const int64_t grp = blockIdx.x / ((int64_t)a.splits * a.nblocks);
  const int d = a.d, n = a.n;
  const int64_t lg = a.lg, tok0 = grp * lg, nbase = grp * n;
  const uint16_t* emb = reinterpret_cast<const uint16_t*>(a.emb);
  const TT* table = reinterpret_cast<const TT*>(a.table);

  // the owner negative of this lane
  const int wfirst = nb * kOwn + wave * 32;
  const int oj = wfirst + frow;
  int64_t my_id = -1;
  if (oj < n) {
    const int64_t id = ld_index(a.neg, a.is64, nbase + oj);
    if (id >= 0 && id < a.vocab) my_id = id;
    else if (split == 0 && fhalf == 0 && a.err) atomicOr(a.err, KRS_FLAG_ID_OUT_OF_RANGE);
  }
  const bool live = my_id >= 0;
  const float my_q = live && a.neg_q ? a.neg_q[nbase + oj] : 0.0f;
  u32x4 own[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const int e0 = (2 * ks + fhalf) * 8;
    own[ks] = load_row_chunk<TT, VEC>(table + (live ? my_id : 0) * a.ldt + e0, e0, d, live);
    if constexpr (!VEC) __builtin_amdgcn_sched_barrier(0);
  }

  const int64_t t_begin = (int64_t)split * a.split_tiles * kTile;
  const int64_t t_stop = t_begin + (int64_t)a.split_tiles * kTile;
  const int64_t t_end = t_stop < lg ? t_stop : lg;

  u32x4 sreg[U];
  float slr = 0.0f, scr = 0.0f;
  int64_t spr = -1;
  auto stage_load = [&](int64_t t0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = tid + u * kThreads;
      const int srow = i / CH, ch = i % CH;
      const bool ok = srow < kTile && t0 + srow < t_end;
      const int64_t t = tok0 + (ok ? t0 + srow : 0);
      const bool ask = ok && a.cw[t] != 0.0f;             // (a dead token's row is not requested)
      sreg[u] = load_chunk<VEC>(emb + t * a.lde + ch * 8, ch * 8, d, ask);
      if constexpr (!VEC) __builtin_amdgcn_sched_barrier(0);
    }
    if (tid < kTile) {
      const bool ok = t0 + tid < t_end;
      const int64_t t = tok0 + (ok ? t0 + tid : 0);
      scr = ok ? a.cw[t] : 0.0f;
      slr = ok ? a.lse[t] : 0.0f;
      spr = ok && a.remove && scr != 0.0f ? ld_index(a.pos, a.is64, t) : -1;
    }
  };
  auto stage_store = [&](int buf) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = tid + u * kThreads;
      if (i < kTile * CH) *reinterpret_cast<u32x4*>(&tx[buf][tile_off<DPAD>(i / CH, i % CH)]) = sreg[u];
    }
    if (tid < kTile) spos[buf][tid] = spr, slse[buf][tid] = slr, sc[buf][tid] = scr;
  };

  f32x16 acc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[dt][r] = 0.0f;
  const bool wave_live = wfirst < n;

  const int ntiles = (int)((t_end - t_begin + kTile - 1) / kTile);
  if (ntiles > 0) {
    stage_load(t_begin);
    stage_store(0);
  }
  __syncthreads();
  for (int it = 0; it < ntiles; ++it) {
    const int buf = it & 1;
    const bool more = it + 1 < ntiles;
    if (more) stage_load(t_begin + (int64_t)(it + 1) * kTile);
    if (wave_live) {
      const f32x16 s1 = OT::scores(tx[buf], own, frow, fhalf);
      float sv[16];
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const int tb = 8 * gq + 4 * fhalf;
        const float4 lv = *reinterpret_cast<const float4*>(&slse[buf][tb]);
        const float4 cv = *reinterpret_cast<const float4*>(&sc[buf][tb]);
        const float l4[4] = {lv.x, lv.y, lv.z, lv.w}, c4[4] = {cv.x, cv.y, cv.z, cv.w};
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          const bool ok = live & (c4[x] != 0.0f) & (spos[buf][tb + x] != my_id);
          sv[4 * gq + x] = ok ? c4[x] * __expf(s1[4 * gq + x] - my_q - l4[x]) : 0.0f;
        }
      }
      OT::second(tx[buf], sv, acc, lane);
    }
    if (more) stage_store(buf ^ 1);
    __syncthreads();
  }

  // accumulator tile dt holds column 32 dt + frow of the owners acc_row(r, fhalf)
  if (!wave_live) return;
  float* dst = a.splits > 1 ? a.dpart + (int64_t)split * a.gn * d : a.dneg;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    const int col = 32 * dt + frow;
    if (col >= d) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = wfirst + acc_row(r, fhalf);
      if (row < n) dst[(nbase + row) * d + col] = acc[dt][r];
    }
  }
}

// dneg = the splits' partials added in split order
__global__ __launch_bounds__(256) void reduce_kernel(const Args a, int64_t elems) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < elems; i += (int64_t)gridDim.x * 256) {
    float s = 0.0f;
    for (int k = 0; k < a.splits; ++k) s += a.dpart[(int64_t)k * elems + i];
    a.dneg[i] = s;
  }
}

// ---- the generic route ----------------------------------------------------------------------------------------------
// sum or max of one value per thread, in a fixed tree; every thread gets the result
template <bool MAX>
__device__ __forceinline__ float block_reduce(float v, float* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = MAX ? fmaxf(red[tid], red[tid + s]) : red[tid] + red[tid + s];
    __syncthreads();
  }
  return red[0];
}

__device__ __forceinline__ float dot_lds(const float* e, const void* row, int dtype, int d) {
  float acc = 0.0f;
  for (int x = 0; x < d; ++x) acc = fmaf(e[x], ld_elem(row, dtype, x), acc);
  return acc;
}
__device__ __forceinline__ const void* row_at(const void* base, int dtype, int64_t row, int64_t ld) {
  return reinterpret_cast<const char*>(base) + row * ld * (dtype == KRS_BF16 ? 2 : 4);
}

// one workgroup per token
__global__ __launch_bounds__(kThreads) void gen_tokens_kernel(const Args a) {
  __shared__ float es[KRS_SAMPLED_SOFTMAX_MAX_DIM];
  __shared__ float xs[KRS_SAMPLED_SOFTMAX_MAX_NEGATIVES + 1];
  __shared__ float red[kThreads];
  __shared__ float s_shared;
  const int tid = threadIdx.x, d = a.d, n = a.n;
  const int64_t t = blockIdx.x, nbase = (t / a.lg) * n;
  const float S = total_weight(a, &s_shared);
  const Token tk = token_of(a, t, true, S);
  if (tk.c == 0.0f) {        // dead: no row is requested, zeros go out
    for (int c = tid; c < d; c += kThreads) st_elem(a.demb, a.emb_dtype, t * a.ldd + c, 0.0f);
    if (tid == 0) {
      a.lse[t] = 0.0f, a.gpos[t] = 0.0f, a.cw[t] = 0.0f, a.lpart[t] = 0.0f;
      if (tk.bad && a.err) atomicOr(a.err, KRS_FLAG_ID_OUT_OF_RANGE);
    }
    return;
  }
  const void* erow = row_at(a.emb, a.emb_dtype, t, a.lde);
  for (int c = tid; c < d; c += kThreads) es[c] = ld_elem(erow, a.emb_dtype, c);
  __syncthreads();
  float top = kNegInf;
  for (int j = tid; j <= n; j += kThreads) {      // item 0 is the positive
    const int64_t id = j == 0 ? tk.pos : ld_index(a.neg, a.is64, nbase + j - 1);
    const bool ok = id >= 0 && id < a.vocab && !(j > 0 && a.remove && id == tk.pos);
    float x = kNegInf;
    if (ok) {
      const float q = !a.pos_q ? 0.0f : j == 0 ? a.pos_q[t] : a.neg_q[nbase + j - 1];
      x = dot_lds(es, row_at(a.table, a.table_dtype, id, a.ldt), a.table_dtype, d) - q;
    }
    xs[j] = x;
    top = fmaxf(top, x);
  }
  const float m = block_reduce<true>(top, red);
  float zs = 0.0f;
  for (int j = tid; j <= n; j += kThreads) zs += xs[j] > kNegInf ? expf(xs[j] - m) : 0.0f;
  const float z = block_reduce<false>(zs, red);
  const float lse = m + logf(z), x0 = xs[0];
  __syncthreads();
  for (int j = tid; j <= n; j += kThreads) xs[j] = xs[j] > kNegInf ? expf(xs[j] - lse) : 0.0f;
  __syncthreads();
  const float gp = tk.c * (xs[0] - 1.0f);
  for (int c = tid; c < d; c += kThreads) {
    float acc = 0.0f;
    for (int j = 1; j <= n; ++j) {
      if (xs[j] == 0.0f) continue;        // (left out, or out of range: its row is not requested)
      const int64_t id = ld_index(a.neg, a.is64, nbase + j - 1);
      acc = fmaf(xs[j], ld_elem(row_at(a.table, a.table_dtype, id, a.ldt), a.table_dtype, c), acc);
    }
    const float rp = ld_elem(row_at(a.table, a.table_dtype, tk.pos, a.ldt), a.table_dtype, c);
    st_elem(a.demb, a.emb_dtype, t * a.ldd + c, fmaf(tk.c, acc, gp * rp));
  }
  if (tid == 0) a.lse[t] = lse, a.gpos[t] = gp, a.cw[t] = tk.c, a.lpart[t] = tk.w * (lse - x0);
}

// one workgroup per negative; the group's tokens in runs of kGenRun, added in token order
constexpr int kGenRun = 1024;
__global__ __launch_bounds__(kThreads) void gen_negs_kernel(const Args a) {
  constexpr int kColsPer = KRS_SAMPLED_SOFTMAX_MAX_DIM / kThreads;
  __shared__ float rs[KRS_SAMPLED_SOFTMAX_MAX_DIM];
  __shared__ float cp[kGenRun];
  const int tid = threadIdx.x, d = a.d;
  const int64_t gj = blockIdx.x, tok0 = (gj / a.n) * a.lg;
  const int64_t id = ld_index(a.neg, a.is64, gj);
  float acc[kColsPer];
#pragma unroll
  for (int k = 0; k < kColsPer; ++k) acc[k] = 0.0f;
  const bool live = id >= 0 && id < a.vocab;
  if (!live && tid == 0 && a.err) atomicOr(a.err, KRS_FLAG_ID_OUT_OF_RANGE);
  if (live) {
    const void* rrow = row_at(a.table, a.table_dtype, id, a.ldt);
    for (int c = tid; c < d; c += kThreads) rs[c] = ld_elem(rrow, a.table_dtype, c);
    const float q = a.neg_q ? a.neg_q[gj] : 0.0f;
    for (int64_t t0 = 0; t0 < a.lg; t0 += kGenRun) {
      const int run = (int)(a.lg - t0 < kGenRun ? a.lg - t0 : kGenRun);
      __syncthreads();
      for (int i = tid; i < run; i += kThreads) {
        const int64_t t = tok0 + t0 + i;
        const float c = a.cw[t];
        float v = 0.0f;
        if (c != 0.0f && !(a.remove && ld_index(a.pos, a.is64, t) == id))
          v = c * expf(dot_lds(rs, row_at(a.emb, a.emb_dtype, t, a.lde), a.emb_dtype, d) - q - a.lse[t]);
        cp[i] = v;
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < kColsPer; ++k) {
        const int c = tid + k * kThreads;
        if (c >= d) continue;
        for (int i = 0; i < run; ++i)
          if (cp[i] != 0.0f)
            acc[k] = fmaf(cp[i], ld_elem(row_at(a.emb, a.emb_dtype, tok0 + t0 + i, a.lde), a.emb_dtype, c), acc[k]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kColsPer; ++k) {
    const int c = tid + k * kThreads;
    if (c < d) a.dneg[gj * d + c] = acc[k];
  }
}

// ---- the sums -------------------------------------------------------------------------------------------------------
// W pass (K29's): a grid-strided sum per thread, the halving tree, one partial per workgroup
__global__ __launch_bounds__(KRS_SAMPLED_BCE_W_THREADS) void wsum_kernel(const float* __restrict__ w, int64_t tokens,
                                                                         float* __restrict__ partials) {
  constexpr int kW = KRS_SAMPLED_BCE_W_THREADS;
  __shared__ float part[kW];
  float acc = 0.0f;
  for (int64_t i = (int64_t)blockIdx.x * kW + threadIdx.x; i < tokens; i += (int64_t)gridDim.x * kW) acc += w[i];
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int o = kW / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = part[0];
}

// the tokens sweep's partials: thread k adds k, k + THREADS, ..; the halving tree; the division by S
__global__ __launch_bounds__(KRS_SAMPLED_SOFTMAX_FINISH_THREADS) void finish_kernel(const Args a) {
  constexpr int kF = KRS_SAMPLED_SOFTMAX_FINISH_THREADS;
  __shared__ float part[kF];
  float acc = 0.0f;
  for (int i = threadIdx.x; i < a.grid_tokens; i += kF) acc += a.lpart[i];
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int o = kF / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float S = a.w ? w_sum(a) : a.count;
    a.loss[0] = S != 0.0f ? part[0] / S : 0.0f;
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------
template <int DPAD, bool VEC>
void launch_fast_typed(const Args& a, const krs_sampled_softmax_route& rt, hipStream_t st) {
  const dim3 block(kThreads);
  if (a.table_dtype == KRS_BF16) {
    hipLaunchKernelGGL((tokens_kernel<DPAD, VEC, uint16_t>), dim3(rt.grid_tokens), block, 0, st, a);
    hipLaunchKernelGGL((negs_kernel<DPAD, VEC, uint16_t>), dim3(rt.grid_negs), block, 0, st, a);
  } else {
    hipLaunchKernelGGL((tokens_kernel<DPAD, VEC, float>), dim3(rt.grid_tokens), block, 0, st, a);
    hipLaunchKernelGGL((negs_kernel<DPAD, VEC, float>), dim3(rt.grid_negs), block, 0, st, a);
  }
}
template <int DPAD>
void launch_fast(const Args& a, const krs_sampled_softmax_route& rt, hipStream_t st) {
  if (rt.vec) launch_fast_typed<DPAD, true>(a, rt, st);
  else launch_fast_typed<DPAD, false>(a, rt, st);
}

thread_local krs_sampled_softmax_route g_route = {};

int refuse(const char* what, const ssm::Plan& pl, const ssm::Call& c) {
  return fail(pl.status,
              "%s: needs %s (t %lld, g %lld, n %lld, d %lld, vocab %lld, emb dtype %d, table dtype %d, itype %d, ld_emb "
              "%lld, ld_table %lld, ld_demb %lld)",
              what, pl.why, (long long)c.t, (long long)c.g, (long long)c.n, (long long)c.d, (long long)c.vocab,
              c.emb_dtype, c.table_dtype, c.itype, (long long)c.ld_emb, (long long)c.ld_table, (long long)c.ld_demb);
}

}  // namespace
}  // namespace krs

extern "C" size_t krs_sampled_softmax_workspace_bytes(int64_t t, int64_t g, int64_t n, int64_t d, int emb_dtype) {
  return krs::ssm::workspace_bytes(t, g, n, d, emb_dtype);
}

extern "C" int krs_sampled_softmax_last_route(krs_sampled_softmax_route* route) {
  if (route) *route = krs::g_route;
  return krs::g_route.kernel;
}

#define KRS_SSM_CALL()                                                                                               \
  krs::ssm::Call call;                                                                                               \
  call.emb = emb, call.ld_emb = ld_emb, call.emb_dtype = emb_dtype;                                                  \
  call.table = table, call.ld_table = ld_table, call.table_dtype = table_dtype, call.vocab = vocab;                  \
  call.pos = pos, call.neg = neg, call.itype = itype, call.weight = weight;                                          \
  call.pos_logq = pos_logq, call.neg_logq = neg_logq;                                                                \
  call.t = t, call.g = g, call.n = n, call.d = d;                                                                    \
  call.lse = lse, call.gpos = gpos, call.demb = demb, call.ld_demb = ld_demb, call.dneg = dneg;                      \
  (void)remove_hits;                                                                                                 \
  const krs::ssm::Plan pl = krs::ssm::plan(call)

extern "C" int krs_sampled_softmax_plan_route(const void* emb, int64_t ld_emb, int emb_dtype, const void* table,
                                              int64_t ld_table, int table_dtype, int64_t vocab, const void* pos,
                                              const void* neg, int itype, const float* weight, const float* pos_logq,
                                              const float* neg_logq, int64_t t, int64_t g, int64_t n, int64_t d,
                                              int remove_hits, const float* lse, const float* gpos, const void* demb,
                                              int64_t ld_demb, const float* dneg, krs_sampled_softmax_route* route) {
  KRS_SSM_CALL();
  if (route) *route = pl.route;
  return pl.status == KRS_OK ? KRS_OK : krs::refuse("krs_sampled_softmax_fwd_bwd", pl, call);
}

extern "C" int krs_sampled_softmax_fwd_bwd(const void* emb, int64_t ld_emb, int emb_dtype, const void* table,
                                           int64_t ld_table, int table_dtype, int64_t vocab, const void* pos,
                                           const void* neg, int itype, const float* weight, const float* pos_logq,
                                           const float* neg_logq, int64_t t, int64_t g, int64_t n, int64_t d,
                                           int remove_hits, float* loss, float* lse, float* gpos, void* demb,
                                           int64_t ld_demb, float* dneg, int* err_flag, void* workspace,
                                           size_t workspace_bytes, void* stream) {
  using namespace krs;
  const char* what = "krs_sampled_softmax_fwd_bwd";
  g_route = {};
  KRS_SSM_CALL();
  if (pl.status != KRS_OK) return refuse(what, pl, call);
  if (t == 0) return KRS_OK;
  KRS_REQUIRE(loss != nullptr, "%s: null loss", what);
  const size_t need = pl.floats * sizeof(float);
  if (!workspace || workspace_bytes < need)
    return fail(KRS_ERR_WORKSPACE, "%s: workspace of %zu bytes at %p, %zu needed", what, workspace_bytes, workspace,
                need);
  float* ws = reinterpret_cast<float*>(workspace);
  const krs_sampled_softmax_route& rt = pl.route;
  Args a = {};
  a.emb = emb, a.table = table, a.pos = pos, a.neg = neg, a.w = weight, a.pos_q = pos_logq, a.neg_q = neg_logq;
  a.loss = loss, a.lse = lse, a.gpos = gpos, a.demb = demb, a.dneg = dneg, a.err = err_flag;
  a.w_partials = weight ? ws : nullptr;
  a.cw = ws + pl.off_c, a.lpart = ws + pl.off_loss, a.dpart = ws + pl.off_dneg;
  a.lde = ld_emb, a.ldt = ld_table, a.ldd = ld_demb, a.tokens = t, a.vocab = vocab, a.lg = pl.lg, a.gn = g * n;
  a.d = (int)d, a.n = (int)n, a.is64 = itype == KRS_I64, a.remove = remove_hits != 0, a.w_blocks = pl.w_blocks;
  a.emb_dtype = emb_dtype, a.table_dtype = table_dtype;
  a.oblocks = (int)ssm::cdiv(pl.lg, ssm::kOwn), a.nblocks = (int)ssm::cdiv(n, ssm::kOwn);
  a.splits = rt.splits, a.split_tiles = rt.split_tiles, a.grid_tokens = rt.grid_tokens;
  a.count = (float)t;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (weight)
    hipLaunchKernelGGL(wsum_kernel, dim3(pl.w_blocks), dim3(KRS_SAMPLED_BCE_W_THREADS), 0, st, weight, t, ws);
  if (rt.kernel == KRS_SAMPLED_SOFTMAX_FAST) {
    if (rt.dpad == 32) launch_fast<32>(a, rt, st);
    else if (rt.dpad == 64) launch_fast<64>(a, rt, st);
    else launch_fast<128>(a, rt, st);
    if (rt.splits > 1) {
      const int64_t elems = a.gn * d, blocks = ssm::cdiv(elems, 256);
      hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, st, a, elems);
    }
  } else {
    hipLaunchKernelGGL(gen_tokens_kernel, dim3(rt.grid_tokens), dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL(gen_negs_kernel, dim3(rt.grid_negs), dim3(kThreads), 0, st, a);
  }
  hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(KRS_SAMPLED_SOFTMAX_FINISH_THREADS), 0, st, a);
  KRS_CHECK_LAUNCH(what);
  g_route = pl.route;
  return KRS_OK;
}
