// K13 -- the in-batch softmax retrieval loss computed from the two embedding matrices, the scores never stored.
//
// Replaces, for query [B, D] and candidates [N, D] in bf16 with 1 <= D <= 256, the stored-matrix head of the
// reference's retrieval examples (scores = q c^T, labels = eye(B, N), SamplingProbabilityCorrection,
// RemoveAccidentalHits, CategoricalCrossentropy(from_logits=True)); the arithmetic is fixed in include/krs.h (K13).
//
// One body, xent_kernel<DPAD, MODE, VEC>, "owner on the lane" (krs_owner_tile.h: the tile image, the chunk loads, the
// accumulator-row rule, the packing and the transposed read are that header's, shared with K19; the score chain and the
// gather's addresses are written out here as they are there):
//   * a wave owns 32 rows of one side (its bf16 rows live in registers as the B operand of the score product), a
//     workgroup of 4 waves 128 rows; the other side is streamed through LDS in tiles of 32 rows, double-buffered:
//     the next tile's global loads are issued before the current tile is computed and written to the other buffer
//     after, one barrier per tile;
//   * score tile X[t][o] = sum_k T[t][k] O[o][k], one MFMA chain.  The owner index is on the lane, the streamed index on
//     the 16 registers, so the owner's constants (m, Z, lse, g, pos) are plain per-lane values and the streamed rows'
//     constants are read from LDS by register index;
//   * MODE_FWD (owner = queries): online {m, Z, S, A} of K11's RowStats per lane over its 16 rows of each tile; the two
//     lanes of a query are merged once at the end;
//   * MODE_DQ (owner = queries) and MODE_DC (owner = candidates): P = g (exp(s - lse) - y') in the same registers,
//     rounded pairwise to bf16, IS the A operand of the gradient product Z[o][d] += sum_t P[t][o] T[t][d], its B
//     operand gathered from the same LDS tile by transposed reads.  Z stays in DPAD / 32 accumulator tiles per wave and
//     is stored once.
//
// Slices: when the owner side alone gives too few workgroups, the streamed side is cut into S slices
// (retrieval_xent_plan.h, from (b, n) alone); a workgroup then writes its slice's partial -- (m, Z, S, A) per query,
// or fp32 [S, rows, d] gradients -- to the caller's workspace and a second small launch combines them in slice
// order.  Every output element has one owner and no float atomics are used: results are bit-identical from call to
// call.  No host synchronisation, no allocation, no scratch.
//
// K15 (krs_retrieval_rank) -- the positive's rank in K8's order, on the same body (owner = queries; staging, tile
// image, score chain and id test are MODE_FWD's):
//   * MODE_POS, a short first launch without slices: the streamed rows of a workgroup are its own 128 owners'
//     positives, gathered through pos, four tiles; wave w keeps, from tile w, the diagonal element of each lane's
//     owner.  s_pos therefore leaves the very MFMA chain that produces the streamed scores, so a candidate row
//     byte-identical to the positive's ties with it exactly (and the positive's own streamed score equals it);
//   * MODE_RANK: per-lane state is one int32, the number of the lane's tile rows whose order_key beats s_pos's, or
//     equals it at a lower index; the positive and its accidental hits are left out.  The two lanes of a query are
//     added at the end; the slices' counts go to the workspace and are added by combine_rank_kernel.  Integers only:
//     exact in any order.
#include <algorithm>

#include "krs_owner_tile.h"
#include "retrieval_xent_plan.h"

namespace krs {
namespace {

using xent::kOwnRows;
using xent::kTile;

static_assert(kTile == kOwnerTile, "the streamed tile is krs_owner_tile.h's");

constexpr int kThreads = 256;
enum { MODE_FWD = 0, MODE_DQ = 1, MODE_DC = 2, MODE_POS = 3, MODE_RANK = 4 };

struct Params {
  const uint16_t* q;
  int64_t ldq;
  const uint16_t* c;
  int64_t ldc;
  int64_t b, n;
  int d;
  const int32_t* pos;
  const float* bias;
  const void* ids;
  int id64;
  float hit_value, keep, spread;   // keep = 1 - ls, spread = ls / n
  const float* lse;
  const float* g;
  float g_scale;
  int S;
  int64_t slice, oblocks;
  float* row_loss;
  float* row_lse;
  float4* fwd_part;   // [S][b] of (m, Z, S, A)
  uint16_t* dout;     // dq or dc
  int64_t ldd;
  float* dpart;       // [S][rows][d]
  float* pos_score;   // K15: s_{i,pos_i}, written by MODE_POS and read by MODE_RANK
  int32_t* rank;      // K15
  int32_t* rank_part; // K15: [S][b] counts
};

// the constants of a row: a query's {lse, g, pos, id of its positive} or a candidate's {bias, -, index, id}
struct RowC {
  float a, b;
  int32_t idx;
  uint32_t idlo, idhi;
};

template <bool QUERY>
__device__ __forceinline__ RowC load_rowc(const Params& p, int64_t i, bool valid) {
  RowC rc{0.0f, 0.0f, QUERY ? -1 : -2, 0u, 0u};
  if (!valid) return rc;
  int64_t id = 0;
  if constexpr (QUERY) {
    const int64_t pos = p.pos ? (int64_t)p.pos[i] : i;
    const bool bad = pos < 0 || pos >= p.n;     // never used as an address
    if (p.ids && !bad) id = ld_index(p.ids, p.id64, pos);
    rc.a = p.lse ? p.lse[i] : 0.0f;
    rc.b = bad ? quiet_nan() : (p.g ? p.g_scale * p.g[i] : p.g_scale);
    rc.idx = bad ? -1 : (int32_t)pos;
  } else {
    if (p.ids) id = ld_index(p.ids, p.id64, i);
    rc.a = p.bias ? p.bias[i] : 0.0f;
    rc.idx = (int32_t)i;
  }
  rc.idlo = (uint32_t)(uint64_t)id;
  rc.idhi = (uint32_t)((uint64_t)id >> 32);
  return rc;
}

// K11's online row statistics (softmax_xent.hip): every term stays non-negative
struct RowStats {
  float m = kNegInf, z = 0.0f, s = 0.0f, a = 0.0f;
  __device__ __forceinline__ void lift(float top) {
    const float mn = fmaxf(m, top);
    if (mn > m) {
      z *= __expf(m - mn);
      if (m > kNegInf) a += s * (mn - m);
      m = mn;
    }
  }
  // adds the statistics `o` of further elements of the row
  __device__ __forceinline__ void merge(const RowStats& o) {
    const float mn = fmaxf(m, o.m);
    const float z0 = m > kNegInf ? z * __expf(m - mn) : 0.0f, z1 = o.m > kNegInf ? o.z * __expf(o.m - mn) : 0.0f;
    const float a0 = m > kNegInf ? a + s * (mn - m) : 0.0f, a1 = o.m > kNegInf ? o.a + o.s * (mn - o.m) : 0.0f;
    m = mn;
    z = z0 + z1;
    a = a0 + a1;
    s = s + o.s;
  }
};

template <int DPAD, int MODE, bool VEC>
__global__ __launch_bounds__(kThreads) void xent_kernel(const Params p) {
  constexpr bool SWAP = MODE == MODE_DC;        // owner = candidates
  constexpr bool XENT = MODE == MODE_FWD || MODE == MODE_DQ || MODE == MODE_DC, GRAD = XENT && MODE != MODE_FWD;
  constexpr int NKS = DPAD / 16, DT = DPAD / 32, CH = DPAD / 8;
  constexpr int TILE_BYTES = kTile * DPAD * 2;
  constexpr int U = (kTile * CH + kThreads - 1) / kThreads;   // chunks a thread stages per tile
  __shared__ __attribute__((aligned(16))) char tile[2][TILE_BYTES];
  __shared__ __attribute__((aligned(16))) float side_a[2][kTile];
  __shared__ __attribute__((aligned(16))) float side_b[2][kTile];
  __shared__ __attribute__((aligned(16))) int32_t side_idx[2][kTile];
  __shared__ __attribute__((aligned(16))) uint32_t side_lo[2][kTile];
  __shared__ __attribute__((aligned(16))) uint32_t side_hi[2][kTile];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int frow = lane & 31, fhalf = lane >> 5;
  const int64_t oblock = blockIdx.x % p.oblocks, slice = blockIdx.x / p.oblocks;
  const uint16_t* O = SWAP ? p.c : p.q;
  const uint16_t* T = SWAP ? p.q : p.c;
  const int64_t ldo = SWAP ? p.ldc : p.ldq, ldt = SWAP ? p.ldq : p.ldc;
  const int64_t RO = SWAP ? p.n : p.b, RT = SWAP ? p.b : p.n;
  // (MODE_POS streams the positives of the workgroup's own owners: "row t" is then owner oblock * kOwnRows + t)
  const int64_t t_begin = MODE == MODE_POS ? 0 : std::min<int64_t>(slice * p.slice, RT);
  const int64_t t_end = MODE == MODE_POS ? std::min<int64_t>(kOwnRows, RO - oblock * kOwnRows)
                                         : std::min<int64_t>(t_begin + p.slice, RT);
  const bool has_ids = p.ids != nullptr;

  // the owner rows of this lane: fragments of the score product's B operand, and the row's constants
  const int64_t orow = oblock * kOwnRows + wave * 32 + frow;
  const bool ovalid = orow < RO;
  u32x4 ofrag[NKS];
  {
    const uint16_t* src = O + (ovalid ? orow : 0) * ldo;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks)
      ofrag[ks] = load_chunk<VEC>(src + (2 * ks + fhalf) * 8, (2 * ks + fhalf) * 8, p.d, ovalid);
  }
  const RowC mine = load_rowc<!SWAP>(p, orow, ovalid);
  uint32_t pos_key = 0;        // MODE_RANK: the positive's place in K8's order
  int32_t ahead = 0;           //            candidates of this lane's 16 rows per tile that precede it
  float diag = 0.0f;           // MODE_POS: the owner's score against its own positive
  if constexpr (MODE == MODE_RANK) pos_key = order_key(ovalid ? p.pos_score[orow] : 0.0f);

  // staging of one streamed tile: registers first, LDS after the current tile has been consumed
  u32x4 sreg[U];
  RowC srow;
  const uint16_t* sptr[U];   // this thread's chunks of the slice's first tile
  int srow_of[U], sdst[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int i = tid + u * kThreads;
    const int row = i / CH, ch = i % CH;
    srow_of[u] = i < kTile * CH ? row : (1 << 30);      // (a thread beyond the tile stages nothing)
    sdst[u] = tile_off<DPAD>(row % kTile, ch);
    sptr[u] = T + (t_begin + row) * ldt + ch * 8;
  }
  auto stage_load = [&](int64_t t0) {
    const int64_t step = (t0 - t_begin) * ldt;
    const int left = (int)std::min<int64_t>(t_end - t0, kTile);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int ch = (tid + u * kThreads) % CH;
      if constexpr (MODE == MODE_POS) {
        // gathered through pos; a positive outside [0, n) is never an address: its row is staged as zeros
        int64_t at = -1;
        if (srow_of[u] < left) {
          const int64_t own = oblock * kOwnRows + t0 + srow_of[u];
          at = p.pos ? (int64_t)p.pos[own] : own;
        }
        const bool ok = at >= 0 && at < p.n;
        sreg[u] = load_chunk<VEC>(T + (ok ? at : 0) * ldt + ch * 8, ch * 8, p.d, ok);
      } else {
        sreg[u] = load_chunk<VEC>(sptr[u] + step, ch * 8, p.d, srow_of[u] < left);
      }
    }
    if constexpr (MODE != MODE_POS) {
      if (tid < kTile) srow = load_rowc<SWAP>(p, t0 + tid, t0 + tid < t_end);
    }
  };
  auto stage_store = [&](int buf) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (tid + u * kThreads < kTile * CH) *reinterpret_cast<u32x4*>(&tile[buf][sdst[u]]) = sreg[u];
    }
    if (MODE != MODE_POS && tid < kTile) {
      side_a[buf][tid] = srow.a;
      side_b[buf][tid] = srow.b;
      side_idx[buf][tid] = srow.idx;
      side_lo[buf][tid] = srow.idlo;
      side_hi[buf][tid] = srow.idhi;
    }
  };

  RowStats st;
  f32x16 dacc[GRAD ? DT : 1];
  if constexpr (GRAD) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) dacc[dt][r] = 0.0f;
  }

  const int64_t ntiles = ceil_div(t_end - t_begin, kTile);
  if (ntiles > 0) {
    stage_load(t_begin);
    stage_store(0);
  }
  __syncthreads();
  for (int64_t it = 0; it < ntiles; ++it) {
    const int buf = (int)(it & 1);
    const int64_t t0 = t_begin + it * kTile;
    const bool more = it + 1 < ntiles;
    if (more) stage_load(t0 + kTile);

    // ---- scores of this wave's 32 owners against the tile's 32 rows ----
    // (the same chain as attn_kernel's, a second copy: as a shared function it changed the code hipcc lays out for the
    //  MODE_POS builds at DPAD = 256, docs/measurement_log.md section 28)
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      const u32x4 fa = *reinterpret_cast<const u32x4*>(&tile[buf][tile_off<DPAD>(frow, 2 * ks + fhalf)]);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa), __builtin_bit_cast(bf16x8, ofrag[ks]),
                                                    acc, 0, 0, 0);
    }

    const int live = (int)std::min<int64_t>(t_end - t0, kTile);   // rows of the tile that exist
    if constexpr (MODE == MODE_POS) {
      // the diagonal of tile `wave`: tile row frow of owner frow sits in half (frow >> 2) & 1, register
      // (frow & 3) + 4 (frow >> 3)
      if (it == wave) {
#pragma unroll
        for (int r = 0; r < 16; ++r) diag = r == (frow & 3) + 4 * (frow >> 3) ? acc[r] : diag;
      }
    }
    if constexpr (MODE == MODE_RANK) {
      // ---- K15: count the tile's candidates that precede the positive: key descending, then index ascending; the
      //      positive itself and, with ids, its accidental hits are left out ----
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const int tb = 8 * gq + 4 * fhalf;
        uint32_t tlo[4] = {0, 0, 0, 0}, thi[4] = {0, 0, 0, 0};
        if (has_ids) {
          const uint4 vl = *reinterpret_cast<const uint4*>(&side_lo[buf][tb]);
          const uint4 vh = *reinterpret_cast<const uint4*>(&side_hi[buf][tb]);
          tlo[0] = vl.x, tlo[1] = vl.y, tlo[2] = vl.z, tlo[3] = vl.w;
          thi[0] = vh.x, thi[1] = vh.y, thi[2] = vh.z, thi[3] = vh.w;
        }
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          const int32_t c_idx = (int32_t)(t0 + tb + x);
          const uint32_t key = order_key(acc[4 * gq + x]);
          // (bitwise on purpose: sixteen short-circuit tests per tile would be sixteen branches)
          const bool before = (key > pos_key) | ((key == pos_key) & (c_idx < mine.idx));
          const bool same_id = has_ids & (tlo[x] == mine.idlo) & (thi[x] == mine.idhi);
          ahead += ((tb + x < live) & (c_idx != mine.idx) & before & !same_id) ? 1 : 0;
        }
      }
    }
    // ---- corrected score, smoothed label and what MODE makes of them; register r is tile row acc_row(r, fhalf) ----
    float sv[16], yv[16];
    if constexpr (XENT) {
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const int tb = 8 * gq + 4 * fhalf;
        float ta[4], tbv[4];
        int32_t tidx[4];
        uint32_t tlo[4] = {0, 0, 0, 0}, thi[4] = {0, 0, 0, 0};
        {
          const float4 va = *reinterpret_cast<const float4*>(&side_a[buf][tb]);
          ta[0] = va.x, ta[1] = va.y, ta[2] = va.z, ta[3] = va.w;
          if constexpr (SWAP) {
            const float4 vb = *reinterpret_cast<const float4*>(&side_b[buf][tb]);
            tbv[0] = vb.x, tbv[1] = vb.y, tbv[2] = vb.z, tbv[3] = vb.w;
            const int4 vi = *reinterpret_cast<const int4*>(&side_idx[buf][tb]);
            tidx[0] = vi.x, tidx[1] = vi.y, tidx[2] = vi.z, tidx[3] = vi.w;
          } else {
#pragma unroll
            for (int x = 0; x < 4; ++x) {
              tbv[x] = 0.0f;
              tidx[x] = (int32_t)(t0 + tb + x);
            }
          }
          if (has_ids) {
            const uint4 vl = *reinterpret_cast<const uint4*>(&side_lo[buf][tb]);
            const uint4 vh = *reinterpret_cast<const uint4*>(&side_hi[buf][tb]);
            tlo[0] = vl.x, tlo[1] = vl.y, tlo[2] = vl.z, tlo[3] = vl.w;
            thi[0] = vh.x, thi[1] = vh.y, thi[2] = vh.z, thi[3] = vh.w;
          }
        }
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          const int r = 4 * gq + x;
          const bool valid = tb + x < live;
          // the query's and the candidate's constants, whichever side owns the lane
          const float bias = SWAP ? mine.a : ta[x];
          const float lse = SWAP ? ta[x] : mine.a;
          const float g = SWAP ? tbv[x] : mine.b;
          const int32_t q_pos = SWAP ? tidx[x] : mine.idx;
          const int32_t c_idx = SWAP ? mine.idx : tidx[x];
          float s = acc[r] + bias;
          if (has_ids) {
            const bool hit = tlo[x] == mine.idlo && thi[x] == mine.idhi && c_idx != q_pos;
            s = hit ? s + p.hit_value : s;
          }
          const float yp = c_idx == q_pos ? p.keep + p.spread : p.spread;
          if constexpr (MODE == MODE_FWD) {
            sv[r] = valid ? s : kNegInf;
            yv[r] = valid ? yp : 0.0f;
          } else {
            sv[r] = valid ? g * (__expf(s - lse) - yp) : 0.0f;
          }
        }
      }
    }

    if constexpr (MODE == MODE_FWD) {
      float top = sv[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) top = fmaxf(top, sv[r]);
      st.lift(top);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const bool valid = sv[r] > kNegInf;
        st.z += valid ? __expf(sv[r] - st.m) : 0.0f;
        st.s += yv[r];
        st.a += valid ? yv[r] * (st.m - sv[r]) : 0.0f;
      }
    } else if constexpr (GRAD) {
      // ---- Z[o][d] += sum_t P[t][o] T[t][d]: P is the A operand, the tile it was scored against the B operand.  The
      //      addresses are krs_owner_tile.h's gather_at (row, chunk, byte), written out -- a second copy, with
      //      attn_kernel's, of what tests/host/owner_tile_check.cpp checks: taken from gather_at, or as a shared gather,
      //      they made hipcc reschedule the dq / dc builds, which then ran 0.2 - 0.4 % slower
      //      (docs/measurement_log.md section 28).  Change the three together. ----
      u32x4 pa[2];
      pack16(sv, pa);
      const int li = lane & 15, tq = li >> 2, tp = li & 3, chalf = (lane >> 4) & 1;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          const int r0 = 16 * s2 + 4 * fhalf, ch = 4 * dt + 2 * chalf + (tp >> 1);
          const u32x2 lo = lds_read_tr16(&tile[buf][tile_off<DPAD>(r0 + tq, ch) + 8 * (tp & 1)]);
          const u32x2 hi = lds_read_tr16(&tile[buf][tile_off<DPAD>(r0 + 8 + tq, ch) + 8 * (tp & 1)]);
          const u32x4 fb = {lo[0], lo[1], hi[0], hi[1]};
          dacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, pa[s2]),
                                                             __builtin_bit_cast(bf16x8, fb), dacc[dt], 0, 0, 0);
        }
      }
    }

    if (more) stage_store(buf ^ 1);
    __syncthreads();
  }

  // ---- results ----
  if constexpr (MODE == MODE_FWD) {
    RowStats other;
    other.m = __shfl_xor(st.m, 32, 64);
    other.z = __shfl_xor(st.z, 32, 64);
    other.s = __shfl_xor(st.s, 32, 64);
    other.a = __shfl_xor(st.a, 32, 64);
    if (fhalf == 0 && ovalid) {
      st.merge(other);   // (rows 0-3, 8-11, .. of each tile, then rows 4-7, 12-15, ..)
      if (p.S > 1) {
        p.fwd_part[slice * p.b + orow] = make_float4(st.m, st.z, st.s, st.a);
      } else {
        const float lz = logf(st.z);
        p.row_loss[orow] = mine.idx < 0 ? quiet_nan() : st.a + st.s * lz;
        p.row_lse[orow] = st.m + lz;
      }
    }
  } else if constexpr (MODE == MODE_POS) {
    if (fhalf == ((frow >> 2) & 1) && ovalid) p.pos_score[orow] = mine.idx < 0 ? quiet_nan() : diag;
  } else if constexpr (MODE == MODE_RANK) {
    ahead += __shfl_xor(ahead, 32, 64);   // (rows 0-3, 8-11, .. of each tile, and rows 4-7, 12-15, ..)
    if (fhalf == 0 && ovalid) {
      if (p.S > 1) p.rank_part[slice * p.b + orow] = ahead;
      else p.rank[orow] = mine.idx < 0 ? -1 : ahead;
    }
  } else {
    // Z tile dt: column 32 dt + (lane & 31), owner row acc_row(r, fhalf) of the wave's 32
    const int64_t obase = oblock * kOwnRows + wave * 32;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const int col = 32 * dt + frow;
      if (col >= p.d) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t row = obase + acc_row(r, fhalf);
        if (row >= RO) continue;
        if (p.S > 1) p.dpart[(slice * RO + row) * p.d + col] = dacc[dt][r];
        else p.dout[row * p.ldd + col] = f32_to_bf16(dacc[dt][r]);
      }
    }
  }
}

// ---- second launches: the slices' partials in slice order ----
__global__ __launch_bounds__(256) void combine_fwd_kernel(const float4* __restrict__ part, int S, int64_t b, int64_t n,
                                                          const int32_t* __restrict__ pos, float* __restrict__ row_loss,
                                                          float* __restrict__ row_lse) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= b) return;
  RowStats st;
  for (int s = 0; s < S; ++s) {
    const float4 v = part[(int64_t)s * b + i];
    RowStats o;
    o.m = v.x, o.z = v.y, o.s = v.z, o.a = v.w;
    st.merge(o);
  }
  const int64_t ps = pos ? (int64_t)pos[i] : i;
  const float lz = logf(st.z);
  row_loss[i] = (ps < 0 || ps >= n) ? quiet_nan() : st.a + st.s * lz;
  row_lse[i] = st.m + lz;
}

__global__ __launch_bounds__(256) void combine_grad_kernel(const float* __restrict__ part, int S, int64_t rows, int d,
                                                           uint16_t* __restrict__ out, int64_t ldo) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * d) return;
  const int64_t row = i / d;
  const int col = (int)(i - row * d);
  float v = part[i];
  for (int s = 1; s < S; ++s) v += part[(int64_t)s * rows * d + i];
  out[row * ldo + col] = f32_to_bf16(v);
}

__global__ __launch_bounds__(256) void combine_rank_kernel(const int32_t* __restrict__ part, int S, int64_t b, int64_t n,
                                                           const int32_t* __restrict__ pos, int32_t* __restrict__ rank) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= b) return;
  int32_t v = 0;
  for (int s = 0; s < S; ++s) v += part[(int64_t)s * b + i];
  const int64_t ps = pos ? (int64_t)pos[i] : i;
  rank[i] = (ps < 0 || ps >= n) ? -1 : v;
}

template <int MODE>
void launch_sweep(const Params& p, unsigned groups, hipStream_t st) {
  const bool vec = aligned16(p.q) && aligned16(p.c) && p.ldq % 8 == 0 && p.ldc % 8 == 0 && p.d % 8 == 0;
#define KRS_XENT(DPAD_)                                                                                   \
  {                                                                                                       \
    if (vec) hipLaunchKernelGGL((xent_kernel<DPAD_, MODE, true>), dim3(groups), dim3(kThreads), 0, st, p); \
    else hipLaunchKernelGGL((xent_kernel<DPAD_, MODE, false>), dim3(groups), dim3(kThreads), 0, st, p);    \
  }
  if (p.d <= 32) KRS_XENT(32)
  else if (p.d <= 64) KRS_XENT(64)
  else if (p.d <= 128) KRS_XENT(128)
  else KRS_XENT(256)
#undef KRS_XENT
}

int check_common(const char* what, const void* q, int64_t ldq, const void* c, int64_t ldc, int dtype, int64_t b,
                 int64_t n, int64_t d, const void* cand_ids, int id_dtype, float label_smoothing) {
  KRS_REQUIRE(b >= 0 && n >= 1 && d >= 1, "%s: bad shape b=%lld n=%lld d=%lld", what, (long long)b, (long long)n,
              (long long)d);
  KRS_REQUIRE(dtype == KRS_BF16, "%s: bf16 inputs only (dtype %d): other inputs take the slab path of the wrapper", what,
              dtype);
  KRS_REQUIRE(d <= xent::kMaxD, "%s: d = %lld above %d: wider inputs take the slab path of the wrapper", what,
              (long long)d, xent::kMaxD);
  KRS_REQUIRE(b <= INT32_MAX && n <= INT32_MAX, "%s: more than 2^31 - 1 rows", what);
  KRS_REQUIRE(ldq >= d && ldc >= d, "%s: row stride below d", what);
  KRS_REQUIRE(!cand_ids || id_dtype == KRS_I32 || id_dtype == KRS_I64, "%s: bad id dtype %d", what, id_dtype);
  KRS_REQUIRE(label_smoothing >= 0.0f && label_smoothing < 1.0f, "%s: label_smoothing %g outside [0, 1)", what,
              (double)label_smoothing);
  KRS_REQUIRE(b == 0 || (q && c), "%s: null operand", what);
  return KRS_OK;
}

}  // namespace
}  // namespace krs

extern "C" size_t krs_retrieval_xent_workspace_bytes(int64_t b, int64_t n, int64_t d, int dtype) {
  (void)dtype;
  if (b <= 0 || n <= 0 || d <= 0) return 0;
  return krs::xent::workspace_bytes(b, n, d);
}

extern "C" int krs_retrieval_xent_fwd(const void* q, int64_t ldq, const void* c, int64_t ldc, int dtype, int64_t b,
                                      int64_t n, int64_t d, const int32_t* pos, const float* cand_bias,
                                      const void* cand_ids, int id_dtype, float hit_value, float label_smoothing,
                                      float* row_loss, float* row_lse, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  using namespace krs;
  const char* what = "krs_retrieval_xent_fwd";
  const int rc = check_common(what, q, ldq, c, ldc, dtype, b, n, d, cand_ids, id_dtype, label_smoothing);
  if (rc != KRS_OK) return rc;
  if (b == 0) return KRS_OK;
  KRS_REQUIRE(row_loss && row_lse, "%s: null output", what);
  const xent::Sweep sw = xent::plan_sweep(b, n, b, n);
  const size_t need = xent::fwd_bytes(b, n);
  if (need && (!workspace || workspace_bytes < need))
    return fail(KRS_ERR_WORKSPACE, "%s: needs %zu workspace bytes, got %zu", what, need, workspace_bytes);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  Params p{};
  p.q = reinterpret_cast<const uint16_t*>(q), p.ldq = ldq;
  p.c = reinterpret_cast<const uint16_t*>(c), p.ldc = ldc;
  p.b = b, p.n = n, p.d = (int)d;
  p.pos = pos, p.bias = cand_bias, p.ids = cand_ids, p.id64 = id_dtype == KRS_I64;
  p.hit_value = hit_value, p.keep = 1.0f - label_smoothing, p.spread = label_smoothing / (float)n;
  p.g_scale = 1.0f;
  p.S = sw.S, p.slice = sw.slice, p.oblocks = sw.oblocks;
  p.row_loss = row_loss, p.row_lse = row_lse, p.fwd_part = reinterpret_cast<float4*>(workspace);
  launch_sweep<MODE_FWD>(p, (unsigned)(sw.oblocks * sw.S), st);
  KRS_CHECK_LAUNCH("xent_kernel (forward)");
  if (sw.S > 1) {
    hipLaunchKernelGGL(combine_fwd_kernel, dim3((unsigned)ceil_div(b, 256)), dim3(256), 0, st, p.fwd_part, sw.S, b, n,
                       pos, row_loss, row_lse);
    KRS_CHECK_LAUNCH("combine_fwd_kernel");
  }
  return KRS_OK;
}

extern "C" int krs_retrieval_xent_bwd(const void* q, int64_t ldq, const void* c, int64_t ldc, int dtype, int64_t b,
                                      int64_t n, int64_t d, const int32_t* pos, const float* cand_bias,
                                      const void* cand_ids, int id_dtype, float hit_value, float label_smoothing,
                                      const float* row_lse, const float* g, float g_scale, void* dq, int64_t lddq,
                                      void* dc, int64_t lddc, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace krs;
  const char* what = "krs_retrieval_xent_bwd";
  const int rc = check_common(what, q, ldq, c, ldc, dtype, b, n, d, cand_ids, id_dtype, label_smoothing);
  if (rc != KRS_OK) return rc;
  KRS_REQUIRE(dq || dc, "%s: neither gradient is wanted", what);
  KRS_REQUIRE((!dq || lddq >= d) && (!dc || lddc >= d), "%s: gradient row stride below d", what);
  if (b == 0) return KRS_OK;     // (dc of an empty batch is the caller's to zero)
  KRS_REQUIRE(row_lse, "%s: null row_lse", what);
  const size_t need_q = dq ? xent::dq_bytes(b, n, d) : 0, need_c = dc ? xent::dc_bytes(b, n, d) : 0;
  if ((need_q + need_c) && (!workspace || workspace_bytes < need_q + need_c))
    return fail(KRS_ERR_WORKSPACE, "%s: needs %zu workspace bytes, got %zu", what, need_q + need_c, workspace_bytes);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  Params p{};
  p.q = reinterpret_cast<const uint16_t*>(q), p.ldq = ldq;
  p.c = reinterpret_cast<const uint16_t*>(c), p.ldc = ldc;
  p.b = b, p.n = n, p.d = (int)d;
  p.pos = pos, p.bias = cand_bias, p.ids = cand_ids, p.id64 = id_dtype == KRS_I64;
  p.hit_value = hit_value, p.keep = 1.0f - label_smoothing, p.spread = label_smoothing / (float)n;
  p.lse = row_lse, p.g = g, p.g_scale = g_scale;
  char* ws = reinterpret_cast<char*>(workspace);
  if (dq) {
    const xent::Sweep sw = xent::plan_sweep(b, n, b, n);
    p.S = sw.S, p.slice = sw.slice, p.oblocks = sw.oblocks;
    p.dout = reinterpret_cast<uint16_t*>(dq), p.ldd = lddq, p.dpart = reinterpret_cast<float*>(ws);
    launch_sweep<MODE_DQ>(p, (unsigned)(sw.oblocks * sw.S), st);
    KRS_CHECK_LAUNCH("xent_kernel (dq)");
    if (sw.S > 1) {
      hipLaunchKernelGGL(combine_grad_kernel, dim3((unsigned)ceil_div(b * d, 256)), dim3(256), 0, st, p.dpart, sw.S, b,
                         (int)d, p.dout, lddq);
      KRS_CHECK_LAUNCH("combine_grad_kernel (dq)");
    }
  }
  if (dc) {
    const xent::Sweep sw = xent::plan_sweep(n, b, b, n);
    p.S = sw.S, p.slice = sw.slice, p.oblocks = sw.oblocks;
    p.dout = reinterpret_cast<uint16_t*>(dc), p.ldd = lddc, p.dpart = reinterpret_cast<float*>(ws + need_q);
    launch_sweep<MODE_DC>(p, (unsigned)(sw.oblocks * sw.S), st);
    KRS_CHECK_LAUNCH("xent_kernel (dc)");
    if (sw.S > 1) {
      hipLaunchKernelGGL(combine_grad_kernel, dim3((unsigned)ceil_div(n * d, 256)), dim3(256), 0, st, p.dpart, sw.S, n,
                         (int)d, p.dout, lddc);
      KRS_CHECK_LAUNCH("combine_grad_kernel (dc)");
    }
  }
  return KRS_OK;
}

extern "C" size_t krs_retrieval_rank_workspace_bytes(int64_t b, int64_t n, int64_t d, int dtype) {
  (void)dtype;
  if (b <= 0 || n <= 0 || d <= 0) return 0;
  return krs::xent::rank_bytes(b, n);
}

extern "C" int krs_retrieval_rank(const void* q, int64_t ldq, const void* c, int64_t ldc, int dtype, int64_t b, int64_t n,
                                  int64_t d, const int32_t* pos, const void* cand_ids, int id_dtype, int32_t* out_rank,
                                  float* out_pos_score, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace krs;
  const char* what = "krs_retrieval_rank";
  KRS_REQUIRE(b >= 0 && n >= 1 && d >= 1, "%s: bad shape b=%lld n=%lld d=%lld", what, (long long)b, (long long)n,
              (long long)d);
  if (dtype != KRS_BF16)
    return fail(KRS_ERR_UNSUPPORTED, "%s: bf16 inputs only (dtype %d): other inputs take the slab path of the wrapper",
                what, dtype);
  if (d > xent::kMaxD)
    return fail(KRS_ERR_UNSUPPORTED, "%s: d = %lld above %d: wider inputs take the slab path of the wrapper", what,
                (long long)d, xent::kMaxD);
  KRS_REQUIRE(b <= INT32_MAX && n <= INT32_MAX, "%s: more than 2^31 - 1 rows", what);
  KRS_REQUIRE(ldq >= d && ldc >= d, "%s: row stride below d", what);
  KRS_REQUIRE(!cand_ids || id_dtype == KRS_I32 || id_dtype == KRS_I64, "%s: bad id dtype %d", what, id_dtype);
  if (b == 0) return KRS_OK;
  KRS_REQUIRE(q && c, "%s: null operand", what);
  KRS_REQUIRE(out_rank, "%s: null output", what);
  const xent::Sweep sw = xent::plan_sweep(b, n, b, n);
  const size_t need = xent::rank_bytes(b, n);
  if (!workspace || workspace_bytes < need)
    return fail(KRS_ERR_WORKSPACE, "%s: needs %zu workspace bytes, got %zu", what, need, workspace_bytes);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  Params p{};
  p.q = reinterpret_cast<const uint16_t*>(q), p.ldq = ldq;
  p.c = reinterpret_cast<const uint16_t*>(c), p.ldc = ldc;
  p.b = b, p.n = n, p.d = (int)d;
  p.pos = pos, p.ids = cand_ids, p.id64 = id_dtype == KRS_I64;
  char* ws = reinterpret_cast<char*>(workspace);
  p.pos_score = out_pos_score ? out_pos_score : reinterpret_cast<float*>(ws);
  p.rank = out_rank, p.rank_part = reinterpret_cast<int32_t*>(ws + xent::rank_pos_bytes(b));
  p.S = 1, p.slice = xent::kOwnRows, p.oblocks = sw.oblocks;
  launch_sweep<MODE_POS>(p, (unsigned)sw.oblocks, st);
  KRS_CHECK_LAUNCH("xent_kernel (positive scores)");
  p.S = sw.S, p.slice = sw.slice;
  launch_sweep<MODE_RANK>(p, (unsigned)(sw.oblocks * sw.S), st);
  KRS_CHECK_LAUNCH("xent_kernel (rank)");
  if (sw.S > 1) {
    hipLaunchKernelGGL(combine_rank_kernel, dim3((unsigned)ceil_div(b, 256)), dim3(256), 0, st, p.rank_part, sw.S, b, n,
                       pos, out_rank);
    KRS_CHECK_LAUNCH("combine_rank_kernel");
  }
  return KRS_OK;
}
