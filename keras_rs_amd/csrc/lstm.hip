// K25 -- an LSTM layer's recurrence (keras.layers.LSTM: tanh, sigmoid, gate order i, f, c, o) in ONE launch per sweep.
// The arithmetic is fixed in include/krs.h (K25); the input projection xz = x . kernel + bias runs outside, as a Dense
// product, and carries the layer's only bias.
//
// Fast path (bf16, u <= 128), lstm_fwd_fast<UPAD> / lstm_bwd_fast<UPAD>, UPAD = 32 / 64 / 128:
//   * a workgroup owns 32 batch rows and walks all l steps alone: nothing it waits on comes from another workgroup;
//   * wave w owns units 32 w .. 32 w + 31 of ALL FOUR gates.  The unit is on the lane and the batch row on the 16
//     accumulator registers (row acc_row(r, lane >> 5) of krs_owner_tile.h), so i, f, g, o, c and h of one (row, unit)
//     sit in the same register index of one lane and the whole cell update needs no exchange;
//   * forward: a = h . U is four chains of v_mfma_f32_32x32x16_bf16 that start at xz.  A operand: the h tile (32 rows x
//     UPAD, bf16, LDS, double-buffered: one barrier per step).  B operand: the recurrent kernel, staged once into LDS
//     with the contraction axis contiguous ([gate column][k]).  h and c are fp32 in registers for all l steps; h is
//     rounded to bf16 only into the next step's A tile and when stored.  The next step's xz and mask are requested
//     before the current step's MFMAs;
//   * backward: walks t = l - 1 .. 0 with the carried dh and dc in registers.  da (= dxz) of the four gates goes as bf16
//     into a double-buffered LDS tile, the A operand of dh = da . U^T (K = 4 UPAD).  The B operand of that product is
//     rows 32 w .. 32 w + 31 of U -- and a lane needs the SAME 16-byte pieces of its unit's row at every step, so they
//     are loaded once from HBM into UPAD registers a lane and never touch LDS.  That is what makes UPAD = 128 fit: K20's
//     layout (U and da both in LDS) would need 199 680 B; here LDS holds 2 x da = 66 688 B and a lane 128 VGPRs of U.
// Every LDS row carries 16 bytes of padding: the 16-byte operand reads of 16 rows then cover all 64 banks.
//
// Generic path (fp32 at any u <= 1024, bf16 above 128): 4 batch rows per workgroup, fp32 FMA, the carried states in
// LDS, the recurrent kernel read through L2 each step.
// The reserve (lstm_plan.h): i, g in the storage type, f, o and the carried c in fp32, one block per token.
// Every output element has one owner and there are no atomics: bit-identical from call to call.
// (Built without packed fp32 instructions, build.py: the gate arithmetic is scalar per register on purpose.)
#include <atomic>

#include "krs_owner_tile.h"   // the vector types, load_chunk and acc_row, the batch row of an accumulator register
#include "lstm_plan.h"

namespace krs {
namespace {

using lstm::kFastRows;
using lstm::kGenRows;
using lstm::kGenThreads;
using lstm::kPadBytes;

struct Params {
  const void* xz;         // [b, l, 4u], token stride ldxz
  int64_t ldxz;
  const void* rk;         // [u, 4u]
  const uint8_t* valid;   // [b, l] or null
  const void* h0;         // [b, u] or null
  const void* c0;         // [b, u] or null
  void* hs;               // [b, l, u]; forward: written (may be null), backward: read
  void* ht;               // [b, u] or null
  void* ct;               // [b, u] or null
  void* reserve;          // forward: written (may be null), backward: read
  const void* dhs;        // [b, l, u] or null
  const void* dht;        // [b, u] or null
  const void* dct;        // [b, u] or null
  void* dxz;              // [b, l, 4u]
  void* hprev;            // [b, l, u] or null
  void* dh0;              // [b, u] or null
  void* dc0;              // [b, u] or null
  int64_t b;
  int l, u;
};

__device__ __forceinline__ float sigmoid_fast(float x) { return 1.0f / (1.0f + __expf(-x)); }
// (1 - 2 / (1 + e^2x) cancels near 0 -- an absolute error of an ulp of 1 on a value that g and tanh(c') multiply into
//  small products -- so |x| < 0.1 takes the odd series instead, whose first dropped term is 17 x^6 / 315 < 6e-8)
__device__ __forceinline__ float tanh_fast(float x) {
  const float x2 = x * x;
  const float series = x * fmaf(x2, fmaf(x2, 0.13333334f, -0.33333334f), 1.0f);
  return x2 < 0.01f ? series : 1.0f - 2.0f / (1.0f + __expf(2.0f * x));
}
__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

// the first valid step of a row (l when it has none; 0 without a mask)
__device__ __forceinline__ int first_valid(const uint8_t* valid, int64_t row, int l) {
  if (!valid) return 0;
  int t = 0;
  while (t < l && valid[row * l + t] == 0) ++t;
  return t;
}

// The reserve block of one token: i at ig[j] and g at ig[u + j] in the storage type T; f at foc[j], o at foc[u + j], the
// carried c at foc[2u + j] in fp32.  16 u bytes a token for bf16, 20 u for fp32 (lstm::reserve_token_bytes).
template <typename T>
struct Rsv {
  T* ig;
  float* foc;
  __device__ __forceinline__ Rsv(char* block, int u)
      : ig(reinterpret_cast<T*>(block)), foc(reinterpret_cast<float*>(block + 2 * sizeof(T) * u)) {}
  __device__ __forceinline__ Rsv(void* base, int64_t tok, int u)
      : Rsv(reinterpret_cast<char*>(base) + tok * (int64_t)((2 * sizeof(T) + 12) * u), u) {}
};

// the batch row of accumulator register r without the lane's part: acc_row(r, fhalf) = urow(r) + 4 fhalf
__device__ __forceinline__ constexpr int urow(int r) { return (r & 3) + 8 * (r >> 2); }
// a step index as a scalar the optimizer takes for opaque: addresses built on it are recomputed per step, in SALU
__device__ __forceinline__ int step_index(int t) { return __builtin_amdgcn_readfirstlane(t); }

// ------------------------------------------------------------------------------------------------------------------
// the fast path
// ------------------------------------------------------------------------------------------------------------------
template <int UPAD>
__global__ __launch_bounds__(2 * UPAD) void lstm_fwd_fast(const Params p) {
  constexpr int THREADS = 2 * UPAD, NKS = UPAD / 16;
  constexpr int WROW = UPAD * 2 + kPadBytes;   // bytes of one LDS row
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* wl = smem;                         // [4 UPAD][WROW]: row g UPAD + j holds U[k][g u + j] over k
  char* hl = smem + 4 * UPAD * WROW;       // [2][32][WROW]: the A operand, h as bf16

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int frow = lane & 31, fhalf = lane >> 5;
  const int u = p.u, l = p.l;
  const int64_t row0 = (int64_t)blockIdx.x * kFastRows;
  const int j = wave * 32 + frow;          // this lane's unit
  const bool jok = j < u;
  const uint16_t* rk = reinterpret_cast<const uint16_t*>(p.rk);
  const uint16_t* xz = reinterpret_cast<const uint16_t*>(p.xz);

  // ---- the recurrent kernel, once: global reads run along a row of U, the image is its transpose ----
  for (int idx = tid; idx < 4 * UPAD * UPAD; idx += THREADS) {
    const int k = idx / (4 * UPAD), c = idx % (4 * UPAD), g = c / UPAD, jj = c % UPAD;
    const uint16_t v = (k < u && jj < u) ? rk[(int64_t)k * 4 * u + g * u + jj] : (uint16_t)0;
    *reinterpret_cast<uint16_t*>(wl + (g * UPAD + jj) * WROW + 2 * k) = v;
  }

  // ---- the carried states: 16 (row, unit j) values of h and of c per lane ----
  float h[16], c[16];
  uint32_t rowok = 0, seen = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int64_t row = row0 + acc_row(i, fhalf);
    const bool ok = row < p.b;
    rowok |= (uint32_t)ok << i;
    h[i] = (ok && jok && p.h0) ? bf16_to_f32(reinterpret_cast<const uint16_t*>(p.h0)[row * u + j]) : 0.0f;
    c[i] = (ok && jok && p.c0) ? bf16_to_f32(reinterpret_cast<const uint16_t*>(p.c0)[row * u + j]) : 0.0f;
    *reinterpret_cast<uint16_t*>(hl + acc_row(i, fhalf) * WROW + 2 * j) = f32_to_bf16(h[i]);
  }

  // Addresses: register i of a lane is batch row row0 + urow(i) + 4 fhalf, so token (row, t) is a UNIFORM token
  // (row0 + urow(i)) * l + t plus the lane's own 4 fhalf * l.  The uniform part is scalar arithmetic on a step index the
  // optimizer cannot see through (step_index), or it would keep 16 running 64-bit addresses per array in VGPRs.
  const int64_t lane_tok = (int64_t)(4 * fhalf) * l;
  const uint16_t* xz_lane = xz + lane_tok * p.ldxz + j;
  const uint8_t* valid_lane = p.valid ? p.valid + lane_tok : nullptr;
  uint16_t* hs_lane = p.hs ? reinterpret_cast<uint16_t*>(p.hs) + lane_tok * u + j : nullptr;
  char* rs_lane = p.reserve ? reinterpret_cast<char*>(p.reserve) + lane_tok * (16 * (int64_t)u) : nullptr;

  // the next step's inputs, requested one step ahead (i | f and g | o, two bf16 a register)
  uint32_t nif[16], ngo[16];
  uint32_t nvalid = 0;
  auto request = [&](int t) {
    nvalid = 0;
    const int ts = step_index(t);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const bool ok = (rowok >> i) & 1;
      const int64_t utok = (row0 + urow(i)) * l + ts;
      const uint16_t* at = xz_lane + utok * p.ldxz;
      nif[i] = (ok && jok) ? ((uint32_t)at[0] | (uint32_t)at[u] << 16) : 0u;
      ngo[i] = (ok && jok) ? ((uint32_t)at[2 * u] | (uint32_t)at[3 * u] << 16) : 0u;
      const bool v = ok && (!valid_lane || valid_lane[utok] != 0);
      nvalid |= (uint32_t)v << i;
    }
  };
  request(0);
  __syncthreads();

  for (int t = 0; t < l; ++t) {
    const int buf = t & 1;
    f32x16 ai, af, ag, ao;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      ai[i] = __uint_as_float(nif[i] << 16);
      af[i] = __uint_as_float(nif[i] & 0xffff0000u);
      ag[i] = __uint_as_float(ngo[i] << 16);
      ao[i] = __uint_as_float(ngo[i] & 0xffff0000u);
    }
    const uint32_t valid = nvalid;
    if (t + 1 < l) request(t + 1);

    const char* ha = hl + buf * (kFastRows * WROW) + frow * WROW;
    const char* wi = wl + j * WROW;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      const int off = 16 * (2 * ks + fhalf);
      const bf16x8 fa = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(ha + off));
      const bf16x8 bi = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(wi + off));
      const bf16x8 bf = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(wi + UPAD * WROW + off));
      const bf16x8 bg = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(wi + 2 * UPAD * WROW + off));
      const bf16x8 bo = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(wi + 3 * UPAD * WROW + off));
      ai = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, bi, ai, 0, 0, 0);
      af = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, bf, af, 0, 0, 0);
      ag = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, bg, ag, 0, 0, 0);
      ao = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, bo, ao, 0, 0, 0);
    }

    char* hnext = hl + (buf ^ 1) * (kFastRows * WROW);
    const int ts = step_index(t);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float gi = sigmoid_fast(ai[i]), gf = sigmoid_fast(af[i]), gg = tanh_fast(ag[i]), go = sigmoid_fast(ao[i]);
      const float cn = gf * c[i] + gi * gg;
      const float hn = go * tanh_fast(cn);
      const bool v = (valid >> i) & 1;
      // a masked step: both states are carried, the output is the previous output -- zeros before the first valid step
      const float out = v ? hn : ((seen >> i) & 1 ? h[i] : 0.0f);
      if (v) h[i] = hn, c[i] = cn;
      *reinterpret_cast<uint16_t*>(hnext + acc_row(i, fhalf) * WROW + 2 * j) = f32_to_bf16(h[i]);
      if (((rowok >> i) & 1) && jok) {
        const int64_t utok = (row0 + urow(i)) * l + ts;
        if (hs_lane) hs_lane[utok * u] = f32_to_bf16(out);
        if (rs_lane) {
          const Rsv<uint16_t> rs(rs_lane + utok * (16 * (int64_t)u), u);
          rs.ig[j] = f32_to_bf16(gi), rs.ig[u + j] = f32_to_bf16(gg);
          rs.foc[j] = gf, rs.foc[u + j] = go, rs.foc[2 * u + j] = c[i];
        }
      }
    }
    seen |= valid;
    __syncthreads();
  }

  if (jok) {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if ((rowok >> i) & 1) {
        const int64_t at = (row0 + acc_row(i, fhalf)) * u + j;
        if (p.ht) reinterpret_cast<uint16_t*>(p.ht)[at] = f32_to_bf16(h[i]);
        if (p.ct) reinterpret_cast<uint16_t*>(p.ct)[at] = f32_to_bf16(c[i]);
      }
  }
}

template <int UPAD>
__global__ __launch_bounds__(2 * UPAD) void lstm_bwd_fast(const Params p) {
  constexpr int NKS = 4 * UPAD / 16;
  constexpr int WROW = 4 * UPAD * 2 + kPadBytes;   // bytes of one LDS row
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* dal = smem;                                // [2][32][WROW]: the A operand, da as bf16, gate g at column g UPAD + j
  int* first = reinterpret_cast<int*>(dal + 2 * kFastRows * WROW);   // [32]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int frow = lane & 31, fhalf = lane >> 5;
  const int u = p.u, l = p.l;
  const int64_t row0 = (int64_t)blockIdx.x * kFastRows;
  const int j = wave * 32 + frow;
  const bool jok = j < u;
  const uint16_t* rk = reinterpret_cast<const uint16_t*>(p.rk);
  const uint16_t* hs = reinterpret_cast<const uint16_t*>(p.hs);
  const uint16_t* h0 = reinterpret_cast<const uint16_t*>(p.h0);
  const uint16_t* c0 = reinterpret_cast<const uint16_t*>(p.c0);
  const uint16_t* dhs = reinterpret_cast<const uint16_t*>(p.dhs);

  // ---- this lane's share of the recurrent kernel, once: of row j of U, the 16 bytes it feeds to every K step ----
  u32x4 wb[NKS];
  {
    const bool vec = (u & 7) == 0 && (reinterpret_cast<uintptr_t>(rk) & 15) == 0;
    const uint16_t* wrow = rk + (int64_t)(jok ? j : 0) * 4 * u;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      const int col = 16 * ks + 8 * fhalf, g = col / UPAD, jj = col % UPAD;   // (a chunk never straddles two gates)
      const uint16_t* at = wrow + g * u + jj;
      wb[ks] = vec ? load_chunk<true>(at, jj, u, jok) : load_chunk<false>(at, jj, u, jok);
    }
  }
  if (tid < kFastRows) first[tid] = row0 + tid < p.b ? first_valid(p.valid, row0 + tid, l) : l;
  __syncthreads();

  float dh[16], dc[16];
  int fv[16];
  uint32_t rowok = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int64_t row = row0 + acc_row(i, fhalf);
    const bool ok = row < p.b;
    rowok |= (uint32_t)ok << i;
    fv[i] = first[acc_row(i, fhalf)];
    dh[i] = (ok && jok && p.dht) ? bf16_to_f32(reinterpret_cast<const uint16_t*>(p.dht)[row * u + j]) : 0.0f;
    dc[i] = (ok && jok && p.dct) ? bf16_to_f32(reinterpret_cast<const uint16_t*>(p.dct)[row * u + j]) : 0.0f;
  }

  for (int t = l - 1; t >= 0; --t) {
    const int buf = (l - 1 - t) & 1;
    char* dt = dal + buf * (kFastRows * WROW);
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int lr = acc_row(i, fhalf);
      const bool live = ((rowok >> i) & 1) && jok;
      const int64_t row = row0 + lr;
      const int64_t tok = live ? row * l + t : 0;
      const bool v = live && (!p.valid || p.valid[tok] != 0);
      // (an output before the first valid step is a constant zero: its gradient goes nowhere)
      const float gh = dh[i] + ((live && dhs && t >= fv[i]) ? bf16_to_f32(dhs[tok * u + j]) : 0.0f);
      float di = 0.0f, df = 0.0f, dg = 0.0f, dgo = 0.0f, seed = gh;
      if (v) {
        const Rsv<const uint16_t> rs(p.reserve, tok, u);
        const float gi = bf16_to_f32(rs.ig[j]), gg = bf16_to_f32(rs.ig[u + j]);
        const float gf = rs.foc[j], go = rs.foc[u + j], cn = rs.foc[2 * u + j];
        // c_{t-1}: the carried cell state the previous token's block holds, the initial one at t = 0
        float cp = 0.0f;
        if (t > 0) cp = Rsv<const uint16_t>(p.reserve, tok - 1, u).foc[2 * u + j];
        else if (c0) cp = bf16_to_f32(c0[row * u + j]);
        const float tc = tanh_fast(cn);
        const float dcn = dc[i] + gh * go * (1.0f - tc * tc);
        dgo = gh * tc * go * (1.0f - go);
        di = dcn * gg * gi * (1.0f - gi);
        df = dcn * cp * gf * (1.0f - gf);
        dg = dcn * gi * (1.0f - gg * gg);
        dc[i] = dcn * gf;
        seed = 0.0f;        // h' does not read h but through a: dh carried = da . U^T alone
      }
      const uint16_t bi = f32_to_bf16(di), bf = f32_to_bf16(df), bg = f32_to_bf16(dg), bo = f32_to_bf16(dgo);
      *reinterpret_cast<uint16_t*>(dt + lr * WROW + 2 * j) = bi;
      *reinterpret_cast<uint16_t*>(dt + lr * WROW + 2 * (UPAD + j)) = bf;
      *reinterpret_cast<uint16_t*>(dt + lr * WROW + 2 * (2 * UPAD + j)) = bg;
      *reinterpret_cast<uint16_t*>(dt + lr * WROW + 2 * (3 * UPAD + j)) = bo;
      if (live) {
        uint16_t* ox = reinterpret_cast<uint16_t*>(p.dxz) + tok * 4 * u + j;
        ox[0] = bi, ox[u] = bf, ox[2 * u] = bg, ox[3 * u] = bo;
        if (p.hprev) {
          // h_{t-1}: the stored output from the first valid step on, the initial state before it
          float hp = 0.0f;
          if (t - 1 >= fv[i]) hp = bf16_to_f32(hs[(tok - 1) * u + j]);
          else if (h0) hp = bf16_to_f32(h0[row * u + j]);
          reinterpret_cast<uint16_t*>(p.hprev)[tok * u + j] = f32_to_bf16(hp);
        }
      }
      acc[i] = seed;
    }
    __syncthreads();
    const char* aa = dt + frow * WROW + 16 * fhalf;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      const bf16x8 fa = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(aa + 32 * ks));
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, __builtin_bit_cast(bf16x8, wb[ks]), acc, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) dh[i] = acc[i];
  }

  if (jok) {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if ((rowok >> i) & 1) {
        const int64_t at = (row0 + acc_row(i, fhalf)) * u + j;
        if (p.dh0) reinterpret_cast<uint16_t*>(p.dh0)[at] = f32_to_bf16(dh[i]);
        if (p.dc0) reinterpret_cast<uint16_t*>(p.dc0)[at] = f32_to_bf16(dc[i]);
      }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// the generic path
// ------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kGenThreads) void lstm_fwd_gen(const Params p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* hb = reinterpret_cast<float*>(smem);   // [2][kGenRows][u]
  const int tid = threadIdx.x, u = p.u, l = p.l;
  float* cb = hb + 2 * kGenRows * u;            // [kGenRows][u]: element (rr, j) is read and written by j's thread alone
  const int64_t row0 = (int64_t)blockIdx.x * kGenRows;
  const T* rk = reinterpret_cast<const T*>(p.rk);
  const T* xz = reinterpret_cast<const T*>(p.xz);
  const T* h0 = reinterpret_cast<const T*>(p.h0);
  const T* c0 = reinterpret_cast<const T*>(p.c0);
  T* hs = reinterpret_cast<T*>(p.hs);

  for (int j = tid; j < u; j += kGenThreads)
#pragma unroll
    for (int rr = 0; rr < kGenRows; ++rr) {
      const int64_t row = row0 + rr;
      hb[rr * u + j] = (row < p.b && h0) ? load1(h0 + row * u + j) : 0.0f;
      cb[rr * u + j] = (row < p.b && c0) ? load1(c0 + row * u + j) : 0.0f;
    }
  uint32_t seen = 0;
  __syncthreads();

  for (int t = 0; t < l; ++t) {
    const float* hc = hb + (t & 1) * kGenRows * u;
    float* hn = hb + ((t & 1) ^ 1) * kGenRows * u;
    uint32_t valid = 0;
#pragma unroll
    for (int rr = 0; rr < kGenRows; ++rr) {
      const int64_t row = row0 + rr;
      const bool v = row < p.b && (!p.valid || p.valid[row * l + t] != 0);
      valid |= (uint32_t)v << rr;
    }
    for (int j = tid; j < u; j += kGenThreads) {
      float ai[kGenRows], af[kGenRows], ag[kGenRows], ao[kGenRows];
#pragma unroll
      for (int rr = 0; rr < kGenRows; ++rr) ai[rr] = af[rr] = ag[rr] = ao[rr] = 0.0f;
      for (int k = 0; k < u; ++k) {
        const T* w = rk + (int64_t)k * 4 * u + j;
        const float wi = load1(w), wf = load1(w + u), wg = load1(w + 2 * u), wo = load1(w + 3 * u);
#pragma unroll
        for (int rr = 0; rr < kGenRows; ++rr) {
          const float hv = hc[rr * u + k];
          ai[rr] = fmaf(hv, wi, ai[rr]);
          af[rr] = fmaf(hv, wf, af[rr]);
          ag[rr] = fmaf(hv, wg, ag[rr]);
          ao[rr] = fmaf(hv, wo, ao[rr]);
        }
      }
#pragma unroll
      for (int rr = 0; rr < kGenRows; ++rr) {
        const int64_t row = row0 + rr;
        const float hold = hc[rr * u + j], cold = cb[rr * u + j];
        if (row >= p.b) {
          hn[rr * u + j] = hold;
          continue;
        }
        const int64_t tok = row * l + t;
        const T* x = xz + tok * p.ldxz + j;
        const float gi = sigmoid_f(load1(x) + ai[rr]), gf = sigmoid_f(load1(x + u) + af[rr]);
        const float gg = tanhf(load1(x + 2 * u) + ag[rr]), go = sigmoid_f(load1(x + 3 * u) + ao[rr]);
        const float cv = gf * cold + gi * gg;
        const float hv = go * tanhf(cv);
        const bool v = (valid >> rr) & 1;
        const float ckeep = v ? cv : cold;
        hn[rr * u + j] = v ? hv : hold;
        cb[rr * u + j] = ckeep;
        if (hs) store1(hs + tok * u + j, v ? hv : ((seen >> rr) & 1 ? hold : 0.0f));
        if (p.reserve) {
          const Rsv<T> rs(p.reserve, tok, u);
          store1(rs.ig + j, gi), store1(rs.ig + u + j, gg);
          rs.foc[j] = gf, rs.foc[u + j] = go, rs.foc[2 * u + j] = ckeep;
        }
      }
    }
    seen |= valid;
    __syncthreads();
  }

  const float* hf = hb + (l & 1) * kGenRows * u;
  for (int j = tid; j < u; j += kGenThreads)
#pragma unroll
    for (int rr = 0; rr < kGenRows; ++rr) {
      const int64_t row = row0 + rr;
      if (row >= p.b) continue;
      if (p.ht) store1(reinterpret_cast<T*>(p.ht) + row * u + j, hf[rr * u + j]);
      if (p.ct) store1(reinterpret_cast<T*>(p.ct) + row * u + j, cb[rr * u + j]);
    }
}

// a value as the storage type holds it
template <typename T>
__device__ __forceinline__ float as_stored(float v) {
  if constexpr (sizeof(T) == 2) return bf16_to_f32(f32_to_bf16(v));
  else return v;
}

template <typename T>
__global__ __launch_bounds__(kGenThreads) void lstm_bwd_gen(const Params p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, u = p.u, l = p.l;
  float* dh = reinterpret_cast<float*>(smem);          // [kGenRows][u]
  float* dc = dh + kGenRows * u;                       // [kGenRows][u]: element idx belongs to idx's thread alone
  float* das = dc + kGenRows * u;                      // [kGenRows][4u]
  int* first = reinterpret_cast<int*>(das + kGenRows * 4 * u);   // [kGenRows]
  const int64_t row0 = (int64_t)blockIdx.x * kGenRows;
  const T* rk = reinterpret_cast<const T*>(p.rk);
  const T* hs = reinterpret_cast<const T*>(p.hs);
  const T* h0 = reinterpret_cast<const T*>(p.h0);
  const T* c0 = reinterpret_cast<const T*>(p.c0);
  const T* dhs = reinterpret_cast<const T*>(p.dhs);
  const T* dht = reinterpret_cast<const T*>(p.dht);
  const T* dct = reinterpret_cast<const T*>(p.dct);

  for (int idx = tid; idx < kGenRows * u; idx += kGenThreads) {
    const int64_t row = row0 + idx / u;
    dh[idx] = (row < p.b && dht) ? load1(dht + row * u + idx % u) : 0.0f;
    dc[idx] = (row < p.b && dct) ? load1(dct + row * u + idx % u) : 0.0f;
  }
  if (tid < kGenRows) first[tid] = row0 + tid < p.b ? first_valid(p.valid, row0 + tid, l) : l;
  __syncthreads();

  for (int t = l - 1; t >= 0; --t) {
    for (int idx = tid; idx < kGenRows * u; idx += kGenThreads) {
      const int rr = idx / u, j = idx % u;
      const int64_t row = row0 + rr;
      float di = 0.0f, df = 0.0f, dg = 0.0f, dgo = 0.0f;
      if (row < p.b) {
        const int64_t tok = row * l + t;
        const bool v = !p.valid || p.valid[tok] != 0;
        const int fv = first[rr];
        const float gh = dh[idx] + ((dhs && t >= fv) ? load1(dhs + tok * u + j) : 0.0f);
        float seed = gh;
        if (v) {
          const Rsv<const T> rs(p.reserve, tok, u);
          const float gi = load1(rs.ig + j), gg = load1(rs.ig + u + j);
          const float gf = rs.foc[j], go = rs.foc[u + j], cn = rs.foc[2 * u + j];
          float cp = 0.0f;
          if (t > 0) cp = Rsv<const T>(p.reserve, tok - 1, u).foc[2 * u + j];
          else if (c0) cp = load1(c0 + row * u + j);
          const float tc = tanhf(cn);
          const float dcn = dc[idx] + gh * go * (1.0f - tc * tc);
          dgo = gh * tc * go * (1.0f - go);
          di = dcn * gg * gi * (1.0f - gi);
          df = dcn * cp * gf * (1.0f - gf);
          dg = dcn * gi * (1.0f - gg * gg);
          dc[idx] = dcn * gf;
          seed = 0.0f;
        }
        dh[idx] = seed;
        T* ox = reinterpret_cast<T*>(p.dxz) + tok * 4 * u + j;
        store1(ox, di), store1(ox + u, df), store1(ox + 2 * u, dg), store1(ox + 3 * u, dgo);
        if (p.hprev) {
          float hp = 0.0f;
          if (t - 1 >= fv) hp = load1(hs + (tok - 1) * u + j);
          else if (h0) hp = load1(h0 + row * u + j);
          store1(reinterpret_cast<T*>(p.hprev) + tok * u + j, hp);
        }
      }
      das[rr * 4 * u + j] = as_stored<T>(di);
      das[rr * 4 * u + u + j] = as_stored<T>(df);
      das[rr * 4 * u + 2 * u + j] = as_stored<T>(dg);
      das[rr * 4 * u + 3 * u + j] = as_stored<T>(dgo);
    }
    __syncthreads();
    // dh[., k] += da . U[k, :]: a wave per k, lanes along the row of U, a fixed shuffle tree
    for (int k = wave; k < u; k += kGenThreads / 64) {
      float s[kGenRows];
#pragma unroll
      for (int rr = 0; rr < kGenRows; ++rr) s[rr] = 0.0f;
      const T* w = rk + (int64_t)k * 4 * u;
      for (int jj = lane; jj < 4 * u; jj += 64) {
        const float wv = load1(w + jj);
#pragma unroll
        for (int rr = 0; rr < kGenRows; ++rr) s[rr] = fmaf(das[rr * 4 * u + jj], wv, s[rr]);
      }
#pragma unroll
      for (int rr = 0; rr < kGenRows; ++rr) {
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) s[rr] += __shfl_xor(s[rr], m, 64);
        if (lane == 0) dh[rr * u + k] += s[rr];
      }
    }
    __syncthreads();
  }

  for (int idx = tid; idx < kGenRows * u; idx += kGenThreads) {
    const int64_t row = row0 + idx / u;
    if (row >= p.b) continue;
    if (p.dh0) store1(reinterpret_cast<T*>(p.dh0) + row * u + idx % u, dh[idx]);
    if (p.dc0) store1(reinterpret_cast<T*>(p.dc0) + row * u + idx % u, dc[idx]);
  }
}

// ---- host ----
// (one record per process, not per thread: torch runs a backward on an autograd thread; kernel and upad in one word)
std::atomic<uint32_t> g_route{0};
inline void set_route(int kernel, int upad) { g_route.store((uint32_t)kernel << 16 | (uint32_t)upad); }

template <typename K>
int launch(const char* what, K kern, const lstm::Plan& pl, int64_t lds, const Params& p, hipStream_t st) {
  KRS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)pl.groups), dim3((unsigned)pl.threads), (size_t)lds, st, p);
  KRS_CHECK_LAUNCH(what);
  return KRS_OK;
}

int plan_call(const char* what, int dtype, int64_t b, int64_t l, int64_t u, lstm::Plan& pl) {
  pl = lstm::plan(b, l, u, dtype);
  if (pl.status == lstm::kInvalid)
    return fail(KRS_ERR_INVALID, "%s: b=%lld l=%lld u=%lld dtype=%d: needs %s", what, (long long)b, (long long)l,
                (long long)u, dtype, pl.why);
  if (pl.status == lstm::kUnsupported)
    return fail(KRS_ERR_UNSUPPORTED, "%s: b=%lld l=%lld u=%lld: supported is %s", what, (long long)b, (long long)l,
                (long long)u, pl.why);
  return KRS_OK;
}

}  // namespace
}  // namespace krs

extern "C" size_t krs_lstm_reserve_bytes(int64_t b, int64_t l, int64_t u, int dtype) {
  return krs::lstm::reserve_bytes(b, l, u, dtype);
}

extern "C" int krs_lstm_last_route(int* kernel, int* upad) {
  const uint32_t r = krs::g_route.load();
  if (kernel) *kernel = (int)(r >> 16);
  if (upad) *upad = (int)(r & 0xffffu);
  return (int)(r >> 16);
}

extern "C" int krs_lstm_fwd(const void* xz, int64_t ldxz, const void* recurrent_kernel, const uint8_t* valid,
                            const void* h0, const void* c0, int dtype, int64_t b, int64_t l, int64_t u, void* hs,
                            void* h_last, void* c_last, void* reserve, void* stream) {
  using namespace krs;
  const char* what = "krs_lstm_fwd";
  set_route(KRS_LSTM_NONE, 0);
  lstm::Plan pl;
  const int rc = plan_call(what, dtype, b, l, u, pl);
  if (rc != KRS_OK || pl.kernel == lstm::kRouteNone) return rc;
  KRS_REQUIRE(xz && recurrent_kernel, "%s: null xz or recurrent_kernel", what);
  KRS_REQUIRE(ldxz >= 4 * u, "%s: token stride of xz below 4 u", what);
  KRS_REQUIRE(hs || h_last || c_last, "%s: no output is wanted", what);
  KRS_REQUIRE(!reserve || hs, "%s: a training forward (reserve) writes hs too", what);
  Params p{};
  p.xz = xz, p.ldxz = ldxz, p.rk = recurrent_kernel, p.valid = valid, p.h0 = h0, p.c0 = c0;
  p.hs = hs, p.ht = h_last, p.ct = c_last, p.reserve = reserve;
  p.b = b, p.l = (int)l, p.u = (int)u;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int lrc;
  if (pl.kernel == lstm::kRouteFast) {
    if (pl.upad == 32) lrc = launch(what, lstm_fwd_fast<32>, pl, pl.lds_fwd, p, st);
    else if (pl.upad == 64) lrc = launch(what, lstm_fwd_fast<64>, pl, pl.lds_fwd, p, st);
    else lrc = launch(what, lstm_fwd_fast<128>, pl, pl.lds_fwd, p, st);
  } else if (dtype == KRS_BF16) {
    lrc = launch(what, lstm_fwd_gen<uint16_t>, pl, pl.lds_fwd, p, st);
  } else {
    lrc = launch(what, lstm_fwd_gen<float>, pl, pl.lds_fwd, p, st);
  }
  if (lrc != KRS_OK) return lrc;
  set_route(pl.kernel, pl.upad);
  return KRS_OK;
}

extern "C" int krs_lstm_bwd(const void* recurrent_kernel, const uint8_t* valid, const void* h0, const void* c0,
                            const void* hs, const void* reserve, const void* dhs, const void* dh_last,
                            const void* dc_last, int dtype, int64_t b, int64_t l, int64_t u, void* dxz, void* hprev,
                            void* dh0, void* dc0, void* stream) {
  using namespace krs;
  const char* what = "krs_lstm_bwd";
  set_route(KRS_LSTM_NONE, 0);
  lstm::Plan pl;
  const int rc = plan_call(what, dtype, b, l, u, pl);
  if (rc != KRS_OK || pl.kernel == lstm::kRouteNone) return rc;
  KRS_REQUIRE(recurrent_kernel && hs && reserve, "%s: null recurrent_kernel, hs or reserve", what);
  KRS_REQUIRE(dxz, "%s: null dxz", what);
  Params p{};
  p.rk = recurrent_kernel, p.valid = valid, p.h0 = h0, p.c0 = c0, p.hs = const_cast<void*>(hs);
  p.reserve = const_cast<void*>(reserve), p.dhs = dhs, p.dht = dh_last, p.dct = dc_last;
  p.dxz = dxz, p.hprev = hprev, p.dh0 = dh0, p.dc0 = dc0;
  p.b = b, p.l = (int)l, p.u = (int)u;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int lrc;
  if (pl.kernel == lstm::kRouteFast) {
    if (pl.upad == 32) lrc = launch(what, lstm_bwd_fast<32>, pl, pl.lds_bwd, p, st);
    else if (pl.upad == 64) lrc = launch(what, lstm_bwd_fast<64>, pl, pl.lds_bwd, p, st);
    else lrc = launch(what, lstm_bwd_fast<128>, pl, pl.lds_bwd, p, st);
  } else if (dtype == KRS_BF16) {
    lrc = launch(what, lstm_bwd_gen<uint16_t>, pl, pl.lds_bwd, p, st);
  } else {
    lrc = launch(what, lstm_bwd_gen<float>, pl, pl.lds_bwd, p, st);
  }
  if (lrc != KRS_OK) return lrc;
  set_route(pl.kernel, pl.upad);
  return KRS_OK;
}
