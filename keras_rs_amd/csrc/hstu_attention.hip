// K31 -- HSTU's pointwise attention over [B, L] token sequences: a weight is silu(alpha q.k + bias[i - j]) / n, with no
// softmax, a learned relative-position bias inside the non-linearity and a mask on padded queries as well as padded keys.
// Neither the scores, the weights nor an [H, L, L] expansion of the bias are ever stored, and the forward keeps nothing
// for the backward.  The arithmetic is fixed in include/krs.h (K31).
//
// Fast route (bf16, dh <= 128), hstu_kernel<DPAD, MODE, VEC>: the "owner on the lane" body of krs_owner_tile.h.
//   * a wave owns 32 rows of one side as B operands of the score product, a workgroup of 4 waves 128 rows of one
//     (b, h); the other side streams through LDS in double-buffered tiles of 32 rows, two tiles per step (X and Y):
//       MODE_FWD  owner = queries (q);       X = keys, Y = values      o  += a V
//       MODE_DQ   owner = queries (q, dO);   X = keys, Y = values      dq += dS K
//       MODE_DKV  owner = keys (k, v);       X = queries, Y = dO       dk += dS Q,  dv += a dO,  dpos
//   * S[t][o] = X[t] . own1[o] and, in the backward, dA[t][o] = Y[t] . own2[o] are v_mfma_f32_32x32x16_bf16 chains; the
//     owner is on the lane and the streamed row on the 16 registers (row acc_row(r, lane >> 5));
//   * the bias a step needs is a window of 159 consecutive entries of one head's row (128 owners against 32 streamed
//     rows), staged into LDS with the tiles; a lane reads its 16 entries at window index (owner - row) + constant;
//   * SiLU, its derivative and the mask run on the 16 accumulator values; a (or dS), rounded pairwise to bf16, IS the
//     A operand of the second product, whose B operand is gathered from the same LDS tile (ds_read_b64_tr_b16);
//   * there is no running maximum, no normaliser and no rescaling: the output accumulator is stored as it is;
//   * under `causal`, tiles wholly beyond the diagonal of the workgroup are not streamed and those beyond the diagonal
//     of a wave are not computed by it.
// dpos (MODE_DKV): a wave's 32 x 32 dS tile goes through 4 KB of LDS and lanes 0 .. 62 each sum one diagonal r - c =
// lane - 31 in row order.  At step `it` lane d of wave w holds offset bin 32 (it - w) + d + 96 of the workgroup's table;
// bins 32 .. 62 of a step are bins 0 .. 30 of the next, so they travel to those lanes as a carry and lanes 0 .. 31 add
// their finished sums to the table: the four waves touch four disjoint runs of 32 bins in a step, and steps are
// ordered by the loop's barrier -- no atomics.  The workgroup writes its table to the workspace; reduce_kernel adds the
// tables of a head in index order.
// Every output element has one owner, there are no float atomics: bit-identical from call to call.
//
// Generic route (fp32 at any dh <= 256, bf16 above 128): one workgroup per (b, h, row), fp32 FMA, one row of weights in
// LDS; gen_fwd / gen_dq own a query row, gen_dkv a key row, gen_dpos 64 offsets of one (b, h).
#include <atomic>

#include "hstu_attn_plan.h"
#include "krs_owner_tile.h"

namespace krs {
namespace {

using hstu::kOwnRows;
using hstu::kTile;
using hstu::kWindow;

static_assert(kTile == kOwnerTile, "the streamed tile is krs_owner_tile.h's");

constexpr int kThreads = 256;
enum { MODE_FWD = 0, MODE_DQ = 1, MODE_DKV = 2 };

struct Params {
  const void *q, *k, *v;
  int64_t ldq, ldk, ldv;
  void* out;
  int64_t ldo;
  const void* dout;
  int64_t lddo;
  void *dq, *dk, *dv;
  int64_t lddq, lddk, lddv;
  const float* pos;     // [hb, 2l - 1] or null
  float* part;          // [parts, bins] partial dpos tables (workspace) or null
  float* dpos;
  const uint8_t* valid; // [b, l] or null
  int h, l, dh, causal, hb, bins, fast;
  float alpha, inv_n;
  int64_t oblocks;
};

__device__ __forceinline__ float sigmoid_of(float s) { return __fdividef(1.0f, 1.0f + __expf(-s)); }

template <int DPAD, int MODE, bool VEC>
__global__ __launch_bounds__(kThreads) void hstu_kernel(const Params p) {
  constexpr bool BWD = MODE != MODE_FWD, KOWN = MODE == MODE_DKV;
  constexpr int NKS = DPAD / 16, DT = DPAD / 32, CH = DPAD / 8;
  constexpr int TILE_BYTES = kTile * DPAD * 2;
  constexpr int U = (kTile * CH + kThreads - 1) / kThreads;   // chunks of each tile a thread stages
  __shared__ __attribute__((aligned(16))) char tx[2][TILE_BYTES];
  __shared__ __attribute__((aligned(16))) char ty[2][TILE_BYTES];
  __shared__ __attribute__((aligned(16))) float side_v[2][kTile];
  __shared__ __attribute__((aligned(16))) float wpos[2][kWindow];
  extern __shared__ __attribute__((aligned(16))) float dyn[];   // MODE_DKV with dpos: exchange [4][32 x 32], bins
  static_assert(sizeof(tx) + sizeof(ty) + sizeof(side_v) + sizeof(wpos) == (size_t)(4 * kTile * DPAD * 2 + 2 * kTile * 4 +
                                                                                  2 * kWindow * 4),
                "hstu::fast_lds_static");

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int frow = lane & 31, fhalf = lane >> 5;
  const int64_t oblock = blockIdx.x % p.oblocks, bh = blockIdx.x / p.oblocks;
  const int64_t bi = bh / p.h;
  const int hi = (int)(bh % p.h);
  const int l = p.l, dh = p.dh;
  const int64_t tok0 = bi * l;
  const int col0 = hi * dh;
  const float* posrow = p.pos ? p.pos + (int64_t)(p.hb == 1 ? 0 : hi) * (2 * l - 1) : nullptr;

  const uint16_t* own1 = reinterpret_cast<const uint16_t*>(KOWN ? p.k : p.q) + col0;
  const int64_t ld1 = KOWN ? p.ldk : p.ldq;
  const uint16_t* own2 = reinterpret_cast<const uint16_t*>(KOWN ? p.v : p.dout) + col0;   // (backward only)
  const int64_t ld2 = KOWN ? p.ldv : p.lddo;
  const uint16_t* X = reinterpret_cast<const uint16_t*>(KOWN ? p.q : p.k) + col0;
  const int64_t ldx = KOWN ? p.ldq : p.ldk;
  const uint16_t* Y = reinterpret_cast<const uint16_t*>(KOWN ? p.dout : p.v) + col0;
  const int64_t ldy = KOWN ? p.lddo : p.ldv;

  // the owner row of this lane
  const int o0 = (int)oblock * kOwnRows;
  const int wfirst = o0 + wave * 32;
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
  const bool my_valid = ovalid && (!p.valid || p.valid[tok0 + oi] != 0);

  // streamed range of the workgroup, and whether this wave computes a tile
  const int t_begin = (KOWN && p.causal) ? o0 : 0;
  const int own_end = o0 + kOwnRows;
  const int t_end = (!KOWN && p.causal && own_end < l) ? own_end : l;
  const bool wave_live = wfirst < l;
  // bias entry of (owner, streamed row t0 + row): window index wl -+ row of the window whose entry 0 is wbase(t0)
  const int wl = KOWN ? kOwnRows - 1 - (wave * 32 + frow) : wave * 32 + frow + kTile - 1;
  const bool want_dpos = KOWN && p.part != nullptr;
  float* bins = dyn + 4 * kTile * kTile;
  if (want_dpos)
    for (int x = tid; x < p.bins; x += kThreads) bins[x] = 0.0f;

  // staging of one streamed step: registers first, LDS after the current tiles have been consumed
  u32x4 sregx[U], sregy[U];
  float sa = 0.0f, sp = 0.0f;
  auto stage_load = [&](int t0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = tid + u * kThreads;
      const int srow = i / CH, ch = i % CH;          // (a thread beyond the tile stages nothing)
      const bool ok = srow < kTile && t0 + srow < t_end;
      const int64_t row = tok0 + (ok ? t0 + srow : 0);
      sregx[u] = load_chunk<VEC>(X + row * ldx + ch * 8, ch * 8, dh, ok);
      if constexpr (!VEC) __builtin_amdgcn_sched_barrier(0);
      sregy[u] = load_chunk<VEC>(Y + row * ldy + ch * 8, ch * 8, dh, ok);
      if constexpr (!VEC) __builtin_amdgcn_sched_barrier(0);
    }
    if (tid < kTile) {
      const int t = t0 + tid;
      sa = t < t_end && (!p.valid || p.valid[tok0 + t] != 0) ? 1.0f : 0.0f;
    }
    if (tid < kWindow) {
      // index i - j + l - 1 of the window's entry `tid` (entries outside the table belong to rows beyond l)
      const int g = (KOWN ? t0 - o0 - kOwnRows : o0 - t0 - kTile) + l + tid;
      sp = posrow && g >= 0 && g < 2 * l - 1 ? posrow[g] : 0.0f;
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
    if (tid < kTile) side_v[buf][tid] = sa;
    if (tid < kWindow) wpos[buf][tid] = sp;
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
  float carry = 0.0f;   // MODE_DKV, lanes 0 .. 30: the sums of the last step's bins 32 .. 62

  // B operand of the second product from a tile: rows 16 s2 + acc_row(j, fhalf), column 32 dt + frow -- the addresses
  // are krs_owner_tile.h's gather_at (row, chunk, byte), written out as K13 and K19 write them
  const int li = lane & 15, tq = li >> 2, tp = li & 3, chalf = (lane >> 4) & 1;
  auto gather_b = [&](const char* tile, int dt, int s2) -> u32x4 {
    const int r0 = 16 * s2 + 4 * fhalf;
    const int ch = 4 * dt + 2 * chalf + (tp >> 1);
    const char* a0 = tile + tile_off<DPAD>(r0 + tq, ch) + 8 * (tp & 1);
    const char* a1 = tile + tile_off<DPAD>(r0 + 8 + tq, ch) + 8 * (tp & 1);
    const u32x2 lo = lds_read_tr16(a0), hi2 = lds_read_tr16(a1);
    return (u32x4){lo[0], lo[1], hi2[0], hi2[1]};
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
    float cur = 0.0f;
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
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const int tb = 8 * gq + 4 * fhalf;
        const float4 va = *reinterpret_cast<const float4*>(&side_v[buf][tb]);
        const float ta[4] = {va.x, va.y, va.z, va.w};
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          const int r = 4 * gq + x;
          const int ts = t0 + tb + x;
          const int qi = KOWN ? ts : oi, kj = KOWN ? oi : ts;
          const bool okr = my_valid & (ta[x] != 0.0f) & (!p.causal | (kj <= qi));
          const float s = fmaf(acc1[r], p.alpha, wpos[buf][KOWN ? wl + tb + x : wl - tb - x]);
          const float sg = sigmoid_of(s);
          if constexpr (MODE == MODE_FWD) {
            sv[r] = okr ? s * sg * p.inv_n : 0.0f;                                        // a
          } else {
            sv[r] = okr ? p.inv_n * acc2[r] * sg * fmaf(s, 1.0f - sg, 1.0f) : 0.0f;       // dS
            if constexpr (KOWN) sw[r] = okr ? s * sg * p.inv_n : 0.0f;                    // a
          }
        }
      }

      u32x4 pa[2];
      pack16(sv, pa);   // a: o += a V (B from the Y tile);  dS: dQ += dS K, or dK += dS Q (B from the X tile)
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
          acc_a[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              __builtin_bit_cast(bf16x8, pa[s2]),
              __builtin_bit_cast(bf16x8, gather_b(MODE == MODE_FWD ? ty[buf] : tx[buf], dt, s2)), acc_a[dt], 0, 0, 0);
      if constexpr (KOWN) {
        u32x4 pb[2];
        pack16(sw, pb);   // a: dV += a dO (B from the Y tile)
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2)
            acc_b[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, pb[s2]),
                                                                __builtin_bit_cast(bf16x8, gather_b(ty[buf], dt, s2)),
                                                                acc_b[dt], 0, 0, 0);
        if (want_dpos) {
          // the fp32 dS tile [streamed query r][owner key c] through LDS; lane d sums the diagonal r - c = d - 31
          float* ex = dyn + wave * (kTile * kTile);
          __builtin_amdgcn_wave_barrier();
#pragma unroll
          for (int r = 0; r < 16; ++r) ex[acc_row(r, fhalf) * kTile + frow] = sv[r];
          __builtin_amdgcn_wave_barrier();
          const int kd = lane - (kTile - 1);
          if (lane < 2 * kTile - 1) {
#pragma unroll 8
            for (int r = 0; r < kTile; ++r) {
              const int c = r - kd;
              if (c >= 0 && c < kTile) cur += ex[r * kTile + c];
            }
          }
          __builtin_amdgcn_wave_barrier();
        }
      }
    }
    if constexpr (KOWN) {
      if (want_dpos) {
        // lanes 0 .. 31 finish bins 32 (it - wave) + 96 + lane (no later step reaches them); 32 .. 62 are carried
        const float tot = cur + carry;
        const float up = __shfl(tot, (lane + 32) & 63, 64);
        if (lane < kTile) bins[kTile * (it - wave) + 96 + lane] += tot;
        carry = lane < kTile ? up : 0.0f;
      }
    }

    if (more) stage_store(buf ^ 1);
    __syncthreads();
  }
  if constexpr (KOWN) {
    if (want_dpos) {
      if (lane < kTile) bins[kTile * (ntiles - wave) + 96 + lane] += carry;
      __syncthreads();
      for (int x = tid; x < p.bins; x += kThreads) p.part[(int64_t)blockIdx.x * p.bins + x] = bins[x];
    }
  }

  // ---- results: accumulator tile dt holds column 32 dt + frow of owner rows acc_row(r, fhalf) ----
  auto store_tile = [&](void* dst, int64_t ldd, const f32x16* acc, float factor) {
    uint16_t* out = reinterpret_cast<uint16_t*>(dst) + col0;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const int col = 32 * dt + frow;
      if (col >= dh) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wfirst + acc_row(r, fhalf);
        if (row >= l) continue;
        out[(tok0 + row) * ldd + col] = f32_to_bf16(acc[dt][r] * factor);
      }
    }
  };
  if constexpr (MODE == MODE_FWD) store_tile(p.out, p.ldo, acc_a, 1.0f);
  if constexpr (MODE == MODE_DQ) store_tile(p.dq, p.lddq, acc_a, p.alpha);
  if constexpr (KOWN) {
    if (p.dk) store_tile(p.dk, p.lddk, acc_a, p.alpha);
    if (p.dv) store_tile(p.dv, p.lddv, acc_b, 1.0f);
  }
}

// ---- dpos[hb_i][idx] = the partial tables of that head added in (b, h, owner block) order ----
// one workgroup per (hb_i, 64 offsets): 4 runs of tables per offset, each added in order, then the 4 in order.
// Table index of offset idx: fast route, owner block ob: idx - l + 128 (+ 128 ob without the causal skip); generic: idx.
__global__ __launch_bounds__(kThreads) void reduce_kernel(const Params p, int64_t b, int64_t chunks) {
  __shared__ float red[4][hstu::kBinChunk];
  const int tid = threadIdx.x, x = tid & 63, s = tid >> 6;
  const int hbi = (int)(blockIdx.x / chunks);
  const int idx = (int)(blockIdx.x % chunks) * hstu::kBinChunk + x;
  const int nb = 2 * p.l - 1;
  float acc = 0.0f;
  if (idx < nb) {
    const int64_t count = b * (p.hb == 1 ? p.h : 1) * p.oblocks;   // tables of this head
    const int64_t run = (count + 3) / 4, g0 = s * run, g1 = g0 + run < count ? g0 + run : count;
    for (int64_t g = g0; g < g1; ++g) {
      const int64_t ob = g % p.oblocks, rest = g / p.oblocks;
      const int64_t bh = p.hb == 1 ? rest : rest * p.h + hbi;
      const int64_t tb = p.fast ? idx - p.l + kOwnRows + (p.causal ? 0 : ob * kOwnRows) : idx;
      if (tb >= 0 && tb < p.bins) acc += p.part[(bh * p.oblocks + ob) * p.bins + tb];
    }
  }
  red[s][x] = acc;
  __syncthreads();
  if (s == 0 && idx < nb) p.dpos[(int64_t)hbi * nb + idx] = ((red[0][x] + red[1][x]) + red[2][x]) + red[3][x];
}

// ---- the generic path: one workgroup per (b, h, row) ----
constexpr int kGenThreads = 256;

template <typename T>
__device__ __forceinline__ float dot_row(const float* a, const T* b, int d) {
  float acc = 0.0f;
  for (int x = 0; x < d; ++x) acc = fmaf(a[x], load1(b + x), acc);
  return acc;
}
template <typename T>
__device__ __forceinline__ float dot_rows(const T* a, const T* b, int d) {
  float acc = 0.0f;
  for (int x = 0; x < d; ++x) acc = fmaf(load1(a + x), load1(b + x), acc);
  return acc;
}

struct GenRow {
  int64_t bh, tok0;
  int row, col0, hi;
};
__device__ __forceinline__ GenRow gen_row(const Params& p, int64_t per) {
  GenRow g;
  g.bh = blockIdx.x / per;
  g.row = (int)(blockIdx.x - g.bh * per);
  g.tok0 = (g.bh / p.h) * p.l;
  g.hi = (int)(g.bh % p.h);
  g.col0 = g.hi * p.dh;
  return g;
}
__device__ __forceinline__ bool gen_allowed(const Params& p, int64_t tok0, int i, int j) {
  return (!p.causal || j <= i) && (!p.valid || (p.valid[tok0 + i] != 0 && p.valid[tok0 + j] != 0));
}
__device__ __forceinline__ float gen_bias(const Params& p, int hi, int i, int j) {
  return p.pos ? p.pos[(int64_t)(p.hb == 1 ? 0 : hi) * (2 * p.l - 1) + (i - j + p.l - 1)] : 0.0f;
}

template <typename T>
__global__ __launch_bounds__(kGenThreads) void gen_fwd_kernel(const Params p) {
  __shared__ float qs[hstu::kMaxDh];
  __shared__ float sc[hstu::kMaxL];
  const int tid = threadIdx.x, dh = p.dh;
  const GenRow g = gen_row(p, p.l);
  const int i = g.row;
  const T* Q = reinterpret_cast<const T*>(p.q) + g.col0;
  const T* K = reinterpret_cast<const T*>(p.k) + g.col0;
  const T* V = reinterpret_cast<const T*>(p.v) + g.col0;
  T* O = reinterpret_cast<T*>(p.out) + (g.tok0 + i) * p.ldo + g.col0;
  for (int d = tid; d < dh; d += kGenThreads) qs[d] = load1(Q + (g.tok0 + i) * p.ldq + d);
  __syncthreads();
  const int jn = p.causal ? i + 1 : p.l;
  for (int j = tid; j < jn; j += kGenThreads) {
    float a = 0.0f;
    if (gen_allowed(p, g.tok0, i, j)) {
      const float s = fmaf(p.alpha, dot_row(qs, K + (g.tok0 + j) * p.ldk, dh), gen_bias(p, g.hi, i, j));
      a = s * (1.0f / (1.0f + expf(-s))) * p.inv_n;
    }
    sc[j] = a;
  }
  __syncthreads();
  for (int d = tid; d < dh; d += kGenThreads) {
    float acc = 0.0f;
    for (int j = 0; j < jn; ++j) acc = fmaf(sc[j], load1(V + (g.tok0 + j) * p.ldv + d), acc);
    store1(O + d, acc);
  }
}

// a and dS of element (i, j) from its score and dA
__device__ __forceinline__ void gen_weights(const Params& p, float s, float da, float& a, float& ds) {
  const float sg = 1.0f / (1.0f + expf(-s));
  a = s * sg * p.inv_n;
  ds = p.inv_n * da * sg * fmaf(s, 1.0f - sg, 1.0f);
}

template <typename T>
__global__ __launch_bounds__(kGenThreads) void gen_dq_kernel(const Params p) {
  __shared__ float qs[hstu::kMaxDh];
  __shared__ float gs[hstu::kMaxDh];
  __shared__ float sc[hstu::kMaxL];
  const int tid = threadIdx.x, dh = p.dh;
  const GenRow g = gen_row(p, p.l);
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
  const int jn = p.causal ? i + 1 : p.l;
  for (int j = tid; j < jn; j += kGenThreads) {
    float a, ds = 0.0f;
    if (gen_allowed(p, g.tok0, i, j)) {
      const float s = fmaf(p.alpha, dot_row(qs, K + (g.tok0 + j) * p.ldk, dh), gen_bias(p, g.hi, i, j));
      gen_weights(p, s, dot_row(gs, V + (g.tok0 + j) * p.ldv, dh), a, ds);
    }
    sc[j] = ds;
  }
  __syncthreads();
  for (int d = tid; d < dh; d += kGenThreads) {
    float acc = 0.0f;
    for (int j = 0; j < jn; ++j) acc = fmaf(sc[j], load1(K + (g.tok0 + j) * p.ldk + d), acc);
    store1(DQ + d, p.alpha * acc);
  }
}

template <typename T>
__global__ __launch_bounds__(kGenThreads) void gen_dkv_kernel(const Params p) {
  __shared__ float ks[hstu::kMaxDh];
  __shared__ float vs[hstu::kMaxDh];
  __shared__ float sp[hstu::kMaxL];
  __shared__ float sd[hstu::kMaxL];
  static_assert(sizeof(ks) + sizeof(vs) + sizeof(sp) + sizeof(sd) == (size_t)hstu::kGenericLds, "hstu::kGenericLds");
  const int tid = threadIdx.x, l = p.l, dh = p.dh;
  const GenRow g = gen_row(p, p.l);
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
  const int i0 = p.causal ? j : 0;
  for (int i = i0 + tid; i < l; i += kGenThreads) {
    float a = 0.0f, ds = 0.0f;
    if (gen_allowed(p, g.tok0, i, j)) {
      const float s = fmaf(p.alpha, dot_row(ks, Q + (g.tok0 + i) * p.ldq, dh), gen_bias(p, g.hi, i, j));
      gen_weights(p, s, dot_row(vs, G + (g.tok0 + i) * p.lddo, dh), a, ds);
    }
    sp[i] = a;
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
    if (p.dk) store1(reinterpret_cast<T*>(p.dk) + (g.tok0 + j) * p.lddk + g.col0 + d, p.alpha * ak);
  }
}

// one workgroup per (b, h, 64 offsets): thread (x, s) adds dS along offset idx over the s-th quarter of the queries, in
// query order; the four quarters are added in order.  part[bh][idx].
template <typename T>
__global__ __launch_bounds__(kGenThreads) void gen_dpos_kernel(const Params p, int64_t chunks) {
  __shared__ float red[4][hstu::kBinChunk];
  const int tid = threadIdx.x, x = tid & 63, s = tid >> 6, l = p.l, dh = p.dh;
  const GenRow g = gen_row(p, chunks);
  const int idx = g.row * hstu::kBinChunk + x;
  const T* Q = reinterpret_cast<const T*>(p.q) + g.col0;
  const T* K = reinterpret_cast<const T*>(p.k) + g.col0;
  const T* V = reinterpret_cast<const T*>(p.v) + g.col0;
  const T* G = reinterpret_cast<const T*>(p.dout) + g.col0;
  float acc = 0.0f;
  if (idx < 2 * l - 1) {
    const int delta = idx - (l - 1), run = (l + 3) / 4;
    const int i1 = (s + 1) * run < l ? (s + 1) * run : l;
    for (int i = s * run; i < i1; ++i) {
      const int j = i - delta;
      if (j < 0 || j >= l || !gen_allowed(p, g.tok0, i, j)) continue;
      const float sc = fmaf(p.alpha, dot_rows(Q + (g.tok0 + i) * p.ldq, K + (g.tok0 + j) * p.ldk, dh),
                            gen_bias(p, g.hi, i, j));
      float a, ds;
      gen_weights(p, sc, dot_rows(G + (g.tok0 + i) * p.lddo, V + (g.tok0 + j) * p.ldv, dh), a, ds);
      acc += ds;
    }
  }
  red[s][x] = acc;
  __syncthreads();
  if (s == 0 && idx < 2 * l - 1) p.part[g.bh * p.bins + idx] = ((red[0][x] + red[1][x]) + red[2][x]) + red[3][x];
}

// ---- host ----
// (one record per process, not per thread: torch runs a backward on an autograd thread, and the caller that asks for
//  the route afterwards is another; the four fields travel in one word: kernel 2 bits, vec 1, dpad 9, lds_bytes 20)
std::atomic<uint64_t> g_route{0};
inline uint64_t route_word(const krs_hstu_attn_route& r) {
  return (uint64_t)r.kernel | (uint64_t)r.vec << 2 | (uint64_t)r.dpad << 3 | (uint64_t)r.lds_bytes << 12;
}
inline krs_hstu_attn_route route_of(uint64_t w) {
  krs_hstu_attn_route r;
  r.kernel = (int32_t)(w & 3), r.vec = (int32_t)(w >> 2 & 1), r.dpad = (int32_t)(w >> 3 & 511), r.lds_bytes = (int32_t)(w >> 12);
  return r;
}
inline krs_hstu_attn_route record_of(const hstu::Plan& pl, bool dpos) {
  krs_hstu_attn_route r;
  r.kernel = pl.kernel, r.dpad = pl.dpad, r.vec = pl.vec;
  r.lds_bytes = pl.kernel == hstu::kRouteNone ? 0 : pl.lds_static + (dpos ? pl.lds_dpos : 0);
  return r;
}

inline bool vec_ok(const void* p, int64_t ld) { return !p || (aligned16(p) && ld % 8 == 0); }

template <int MODE>
int launch_fast(const char* what, const Params& p, const hstu::Plan& pl, size_t dyn_lds, hipStream_t st) {
  const dim3 grid((unsigned)pl.groups), block(kThreads);
#define KRS_HSTU_GO(DPAD_, VEC_)                                                                                    \
  {                                                                                                                 \
    auto kern = hstu_kernel<DPAD_, MODE, VEC_>;                                                                     \
    if (dyn_lds)                                                                                                    \
      KRS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,  \
                                  (int)dyn_lds));                                                                   \
    hipLaunchKernelGGL(kern, grid, block, dyn_lds, st, p);                                                          \
  }
#define KRS_HSTU(DPAD_)                          \
  {                                              \
    if (pl.vec) KRS_HSTU_GO(DPAD_, true)         \
    else KRS_HSTU_GO(DPAD_, false)               \
  }
  if (pl.dpad == 32) KRS_HSTU(32)
  else if (pl.dpad == 64) KRS_HSTU(64)
  else KRS_HSTU(128)
#undef KRS_HSTU
#undef KRS_HSTU_GO
  KRS_CHECK_LAUNCH(what);
  return KRS_OK;
}

// the checks every entry and the route query share; `aligned` from the pointer values
int check_common(const char* what, const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                 int dtype, int64_t b, int64_t h, int64_t l, int64_t dh, const float* pos, int64_t hb, bool aligned,
                 hstu::Plan& pl) {
  pl = hstu::plan(b, h, l, dh, dtype, aligned, pos ? hb : 0);
  if (pl.status == hstu::kInvalid)
    return fail(KRS_ERR_INVALID, "%s: b=%lld h=%lld l=%lld dh=%lld dtype=%d hb=%lld: needs %s", what, (long long)b,
                (long long)h, (long long)l, (long long)dh, dtype, (long long)hb, pl.why);
  KRS_REQUIRE(!pos || hb == 1 || hb == h, "%s: hb=%lld: a position table has 1 or h=%lld rows", what, (long long)hb,
              (long long)h);
  KRS_REQUIRE(ldq >= h * dh && ldk >= h * dh && ldv >= h * dh, "%s: token stride below h * dh", what);
  if (pl.status == hstu::kUnsupported)
    return fail(KRS_ERR_UNSUPPORTED, "%s: b=%lld h=%lld l=%lld dh=%lld: supported is %s", what, (long long)b, (long long)h,
                (long long)l, (long long)dh, pl.why);
  if (pl.kernel == hstu::kRouteNone) return KRS_OK;
  KRS_REQUIRE(q && k && v, "%s: null operand", what);
  return KRS_OK;
}

void fill_common(Params& p, const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, int64_t h,
                 int64_t l, int64_t dh, const float* pos, int64_t hb, const uint8_t* valid, int causal, float alpha,
                 float inv_n, const hstu::Plan& pl) {
  p.q = q, p.k = k, p.v = v, p.ldq = ldq, p.ldk = ldk, p.ldv = ldv;
  p.pos = pos, p.hb = pos ? (int)hb : 0, p.valid = valid;
  p.h = (int)h, p.l = (int)l, p.dh = (int)dh, p.causal = causal != 0;
  p.alpha = alpha, p.inv_n = inv_n;
  p.oblocks = pl.oblocks, p.bins = (int)pl.bins, p.fast = pl.kernel == hstu::kRouteFast;
}

}  // namespace
}  // namespace krs

extern "C" size_t krs_hstu_attn_workspace_bytes(int64_t b, int64_t h, int64_t l, int64_t dh, int dtype, int64_t hb) {
  return krs::hstu::workspace_bytes(krs::hstu::plan(b, h, l, dh, dtype, false, hb));
}

extern "C" int krs_hstu_attn_last_route(krs_hstu_attn_route* route) {
  const krs_hstu_attn_route r = krs::route_of(krs::g_route.load());
  if (route) *route = r;
  return r.kernel;
}

extern "C" int krs_hstu_attn_plan_route(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                        int dtype, int64_t b, int64_t h, int64_t l, int64_t dh, const float* pos,
                                        int64_t hb, const void* dout, int64_t lddo, const float* dpos,
                                        krs_hstu_attn_route* route) {
  using namespace krs;
  hstu::Plan pl;
  const bool aligned = vec_ok(q, ldq) && vec_ok(k, ldk) && vec_ok(v, ldv) && vec_ok(dout, lddo);
  const int rc = check_common("krs_hstu_attn_plan_route", q, ldq, k, ldk, v, ldv, dtype, b, h, l, dh, pos, hb, aligned, pl);
  if (route) *route = rc == KRS_OK ? record_of(pl, dout && dpos) : krs_hstu_attn_route{0, 0, 0, 0};
  return rc;
}

extern "C" int krs_hstu_attn_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                 int dtype, int64_t b, int64_t h, int64_t l, int64_t dh, const float* pos, int64_t hb,
                                 const uint8_t* valid, int causal, float alpha, float inv_n, void* out, int64_t ldo,
                                 void* stream) {
  using namespace krs;
  const char* what = "krs_hstu_attn_fwd";
  g_route.store(0);
  hstu::Plan pl;
  const bool aligned = vec_ok(q, ldq) && vec_ok(k, ldk) && vec_ok(v, ldv);
  const int rc = check_common(what, q, ldq, k, ldk, v, ldv, dtype, b, h, l, dh, pos, hb, aligned, pl);
  if (rc != KRS_OK || pl.kernel == hstu::kRouteNone) return rc;
  KRS_REQUIRE(out, "%s: null output", what);
  KRS_REQUIRE(ldo >= h * dh, "%s: output token stride below h * dh", what);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  Params p{};
  fill_common(p, q, ldq, k, ldk, v, ldv, h, l, dh, pos, hb, valid, causal, alpha, inv_n, pl);
  p.out = out, p.ldo = ldo;
  if (pl.kernel == hstu::kRouteFast) {
    const int lrc = launch_fast<MODE_FWD>(what, p, pl, 0, st);
    if (lrc != KRS_OK) return lrc;
  } else {
    if (dtype == KRS_BF16) hipLaunchKernelGGL(gen_fwd_kernel<uint16_t>, dim3((unsigned)pl.groups), dim3(kGenThreads), 0, st, p);
    else hipLaunchKernelGGL(gen_fwd_kernel<float>, dim3((unsigned)pl.groups), dim3(kGenThreads), 0, st, p);
    KRS_CHECK_LAUNCH("krs_hstu_attn_fwd kernel");
  }
  g_route.store(route_word(record_of(pl, false)));
  return KRS_OK;
}

extern "C" int krs_hstu_attn_bwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                 int dtype, int64_t b, int64_t h, int64_t l, int64_t dh, const float* pos, int64_t hb,
                                 const uint8_t* valid, int causal, float alpha, float inv_n, const void* dout,
                                 int64_t lddo, void* dq, int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv,
                                 float* dpos, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace krs;
  const char* what = "krs_hstu_attn_bwd";
  g_route.store(0);
  hstu::Plan pl;
  const bool aligned = vec_ok(q, ldq) && vec_ok(k, ldk) && vec_ok(v, ldv) && vec_ok(dout, lddo);
  const int rc = check_common(what, q, ldq, k, ldk, v, ldv, dtype, b, h, l, dh, pos, hb, aligned, pl);
  if (rc != KRS_OK) return rc;
  KRS_REQUIRE(dq || dk || dv || dpos, "%s: no gradient is wanted", what);
  KRS_REQUIRE(!dpos || pos, "%s: dpos without pos", what);
  KRS_REQUIRE((!dq || lddq >= h * dh) && (!dk || lddk >= h * dh) && (!dv || lddv >= h * dh) && lddo >= h * dh,
              "%s: token stride below h * dh", what);
  if (pl.kernel == hstu::kRouteNone) return KRS_OK;
  KRS_REQUIRE(dout, "%s: null dout", what);
  const size_t need = dpos ? hstu::workspace_bytes(pl) : 0;
  if (need && (!workspace || workspace_bytes < need))
    return fail(KRS_ERR_WORKSPACE, "%s: needs %zu workspace bytes, got %zu", what, need, workspace_bytes);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  Params p{};
  fill_common(p, q, ldq, k, ldk, v, ldv, h, l, dh, pos, hb, valid, causal, alpha, inv_n, pl);
  p.dout = dout, p.lddo = lddo;
  p.dq = dq, p.dk = dk, p.dv = dv, p.lddq = lddq, p.lddk = lddk, p.lddv = lddv;
  p.part = dpos ? reinterpret_cast<float*>(workspace) : nullptr, p.dpos = dpos;
  const bool bf16 = dtype == KRS_BF16, fast = pl.kernel == hstu::kRouteFast;
  const dim3 ggrid((unsigned)pl.groups), gblock(kGenThreads);
  if (dq) {
    if (fast) {
      const int lrc = launch_fast<MODE_DQ>("krs_hstu_attn_bwd dq sweep", p, pl, 0, st);
      if (lrc != KRS_OK) return lrc;
    } else {
      if (bf16) hipLaunchKernelGGL(gen_dq_kernel<uint16_t>, ggrid, gblock, 0, st, p);
      else hipLaunchKernelGGL(gen_dq_kernel<float>, ggrid, gblock, 0, st, p);
      KRS_CHECK_LAUNCH("krs_hstu_attn_bwd dq sweep");
    }
  }
  if (fast && (dk || dv || dpos)) {
    const int lrc = launch_fast<MODE_DKV>("krs_hstu_attn_bwd dk/dv sweep", p, pl, dpos ? (size_t)pl.lds_dpos : 0, st);
    if (lrc != KRS_OK) return lrc;
  }
  if (!fast && (dk || dv)) {
    if (bf16) hipLaunchKernelGGL(gen_dkv_kernel<uint16_t>, ggrid, gblock, 0, st, p);
    else hipLaunchKernelGGL(gen_dkv_kernel<float>, ggrid, gblock, 0, st, p);
    KRS_CHECK_LAUNCH("krs_hstu_attn_bwd dk/dv sweep");
  }
  if (dpos) {
    const int64_t chunks = hstu::cdiv(2 * l - 1, hstu::kBinChunk);
    if (!fast) {
      const dim3 pgrid((unsigned)pl.dpos_groups);
      if (bf16) hipLaunchKernelGGL(gen_dpos_kernel<uint16_t>, pgrid, gblock, 0, st, p, chunks);
      else hipLaunchKernelGGL(gen_dpos_kernel<float>, pgrid, gblock, 0, st, p, chunks);
      KRS_CHECK_LAUNCH("krs_hstu_attn_bwd dpos sweep");
    }
    hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)pl.reduce_groups), dim3(kThreads), 0, st, p, b, chunks);
    KRS_CHECK_LAUNCH("krs_hstu_attn_bwd dpos reduce");
  }
  g_route.store(route_word(record_of(pl, dpos != nullptr)));
  return KRS_OK;
}
