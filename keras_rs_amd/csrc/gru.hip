// K20 -- a GRU layer's recurrence (keras.layers.GRU, reset_after=True) in ONE launch per sweep.  The arithmetic is fixed in
// include/krs.h (K20); the input projection xz = x . kernel + bias[0] runs outside, as a Dense product.
//
// Fast path (bf16, u <= 128), gru_fwd_fast<UPAD> / gru_bwd_fast<UPAD>, UPAD = 32 / 64 / 128:
//   * a workgroup owns 32 batch rows and walks all l steps alone: nothing it waits on comes from another workgroup;
//   * wave w owns units 32 w .. 32 w + 31 of ALL THREE gates.  The step's product a = h . U is three chains of
//     v_mfma_f32_32x32x16_bf16 whose A operand is the h tile (32 rows x UPAD, bf16, LDS) and whose B operand is the
//     recurrent kernel, staged once into LDS with the contraction axis contiguous (forward: [gate column][k];
//     backward: [unit][gate column]).  The unit is on the lane and the batch row on the 16 accumulator registers
//     (row acc_row(r, lane >> 5) of krs_owner_tile.h), so z, r, q of one (row, unit) sit in the same register of three
//     accumulators and the gate arithmetic needs no exchange;
//   * the z / r accumulators start at xz + rb, the h accumulator at rb_h;
//   * the carried state is fp32 in those 16 registers for all l steps; it is rounded to bf16 only into the next step's A
//     tile (double-buffered: one barrier per step) and when stored;
//   * the next step's xz and mask are requested before the current step's MFMAs.
//   The backward walks t = l - 1 .. 0 with the carried dh in the same registers: gate gradients from the reserve and
//   h_{t-1}, da as bf16 into a double-buffered LDS tile (the A operand of da . U^T), dxz / da / h_{t-1} to HBM.
// Every LDS row carries 16 bytes of padding: the 16-byte operand reads of 16 rows then cover all 64 banks.
//
// Generic path (fp32 at any u <= 1024, bf16 above 128): 4 batch rows per workgroup, fp32 FMA, the carried state in LDS,
// the recurrent kernel read through L2 each step.
// Every output element has one owner and there are no atomics: bit-identical from call to call.
#include <atomic>

#include "gru_plan.h"
#include "krs_owner_tile.h"   // the vector types and acc_row, the batch row of an accumulator register

namespace krs {
namespace {

using gru::kFastRows;
using gru::kGenRows;
using gru::kGenThreads;
using gru::kPadBytes;

struct Params {
  const void* xz;         // [b, l, 3u], token stride ldxz
  int64_t ldxz;
  const void* rk;         // [u, 3u]
  const float* rb;        // [3u] or null
  const uint8_t* valid;   // [b, l] or null
  const void* h0;         // [b, u] or null
  void* hs;               // [b, l, u]; forward: written (may be null), backward: read
  void* ht;               // [b, u] or null
  void* reserve;          // [b, l, 4u]; forward: written (may be null), backward: read
  const void* dhs;        // [b, l, u] or null
  const void* dht;        // [b, u] or null
  void *dxz, *da;         // [b, l, 3u]
  void* hprev;            // [b, l, u] or null
  void* dh0;              // [b, u] or null
  int64_t b;
  int l, u;
};

__device__ __forceinline__ float sigmoid_fast(float x) { return 1.0f / (1.0f + __expf(-x)); }
__device__ __forceinline__ float tanh_fast(float x) { return 1.0f - 2.0f / (1.0f + __expf(2.0f * x)); }
__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

// the first valid step of a row (l when it has none; 0 without a mask)
__device__ __forceinline__ int first_valid(const uint8_t* valid, int64_t row, int l) {
  if (!valid) return 0;
  int t = 0;
  while (t < l && valid[row * l + t] == 0) ++t;
  return t;
}

// ------------------------------------------------------------------------------------------------------------------
// the fast path
// ------------------------------------------------------------------------------------------------------------------
template <int UPAD>
__global__ __launch_bounds__(2 * UPAD) void gru_fwd_fast(const Params p) {
  constexpr int THREADS = 2 * UPAD, NKS = UPAD / 16;
  constexpr int WROW = UPAD * 2 + kPadBytes;   // bytes of one LDS row
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* wl = smem;                         // [3 UPAD][WROW]: row g UPAD + j holds U[k][g u + j] over k
  char* hl = smem + 3 * UPAD * WROW;       // [2][32][WROW]: the A operand, h as bf16

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int frow = lane & 31, fhalf = lane >> 5;
  const int u = p.u, l = p.l;
  const int64_t row0 = (int64_t)blockIdx.x * kFastRows;
  const int j = wave * 32 + frow;          // this lane's unit
  const bool jok = j < u;
  const uint16_t* rk = reinterpret_cast<const uint16_t*>(p.rk);
  const uint16_t* xz = reinterpret_cast<const uint16_t*>(p.xz);

  // ---- the recurrent kernel, once: global reads run along a row of U, the image is its transpose ----
  for (int idx = tid; idx < 3 * UPAD * UPAD; idx += THREADS) {
    const int k = idx / (3 * UPAD), c = idx % (3 * UPAD), g = c / UPAD, jj = c % UPAD;
    const uint16_t v = (k < u && jj < u) ? rk[(int64_t)k * 3 * u + g * u + jj] : (uint16_t)0;
    *reinterpret_cast<uint16_t*>(wl + (g * UPAD + jj) * WROW + 2 * k) = v;
  }

  float rbz = 0.0f, rbr = 0.0f, rbh = 0.0f;
  if (p.rb && jok) rbz = p.rb[j], rbr = p.rb[u + j], rbh = p.rb[2 * u + j];

  // ---- the carried state: 16 (row, unit j) values per lane ----
  float h[16];
  uint32_t rowok = 0, seen = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int64_t row = row0 + acc_row(i, fhalf);
    const bool ok = row < p.b;
    rowok |= (uint32_t)ok << i;
    h[i] = (ok && jok && p.h0) ? bf16_to_f32(reinterpret_cast<const uint16_t*>(p.h0)[row * u + j]) : 0.0f;
    *reinterpret_cast<uint16_t*>(hl + acc_row(i, fhalf) * WROW + 2 * j) = f32_to_bf16(h[i]);
  }

  // the next step's inputs, requested one step ahead
  uint16_t nz[16], nr[16], nh[16];
  uint32_t nvalid = 0;
  auto request = [&](int t) {
    nvalid = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int64_t row = row0 + acc_row(i, fhalf);
      const bool ok = (rowok >> i) & 1;
      const int64_t tok = ok ? row * l + t : 0;
      const uint16_t* at = xz + tok * p.ldxz + j;
      nz[i] = (ok && jok) ? at[0] : (uint16_t)0;
      nr[i] = (ok && jok) ? at[u] : (uint16_t)0;
      nh[i] = (ok && jok) ? at[2 * u] : (uint16_t)0;
      const bool v = ok && (!p.valid || p.valid[tok] != 0);
      nvalid |= (uint32_t)v << i;
    }
  };
  request(0);
  __syncthreads();

  for (int t = 0; t < l; ++t) {
    const int buf = t & 1;
    f32x16 az, ar, ah;
    float xh[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      az[i] = bf16_to_f32(nz[i]) + rbz;
      ar[i] = bf16_to_f32(nr[i]) + rbr;
      ah[i] = rbh;
      xh[i] = bf16_to_f32(nh[i]);
    }
    const uint32_t valid = nvalid;
    if (t + 1 < l) request(t + 1);

    const char* ha = hl + buf * (kFastRows * WROW) + frow * WROW;
    const char* wz = wl + j * WROW;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      const int off = 16 * (2 * ks + fhalf);
      const bf16x8 fa = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(ha + off));
      const bf16x8 bz = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(wz + off));
      const bf16x8 br = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(wz + UPAD * WROW + off));
      const bf16x8 bh = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(wz + 2 * UPAD * WROW + off));
      az = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, bz, az, 0, 0, 0);
      ar = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, br, ar, 0, 0, 0);
      ah = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, bh, ah, 0, 0, 0);
    }

    char* hnext = hl + (buf ^ 1) * (kFastRows * WROW);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float z = sigmoid_fast(az[i]), r = sigmoid_fast(ar[i]), q = ah[i];
      const float c = tanh_fast(xh[i] + r * q);
      const float hn = z * h[i] + (1.0f - z) * c;
      const bool v = (valid >> i) & 1;
      // a masked step: the state is carried, the output is the previous output -- zeros before the first valid step
      const float out = v ? hn : ((seen >> i) & 1 ? h[i] : 0.0f);
      if (v) h[i] = hn;
      *reinterpret_cast<uint16_t*>(hnext + acc_row(i, fhalf) * WROW + 2 * j) = f32_to_bf16(h[i]);
      if (((rowok >> i) & 1) && jok) {
        const int64_t tok = (row0 + acc_row(i, fhalf)) * l + t;
        if (p.hs) reinterpret_cast<uint16_t*>(p.hs)[tok * u + j] = f32_to_bf16(out);
        if (p.reserve) {
          uint16_t* rs = reinterpret_cast<uint16_t*>(p.reserve) + tok * 4 * u + j;
          rs[0] = f32_to_bf16(z), rs[u] = f32_to_bf16(r), rs[2 * u] = f32_to_bf16(c), rs[3 * u] = f32_to_bf16(q);
        }
      }
    }
    seen |= valid;
    __syncthreads();
  }

  if (p.ht && jok) {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if ((rowok >> i) & 1)
        reinterpret_cast<uint16_t*>(p.ht)[(row0 + acc_row(i, fhalf)) * u + j] = f32_to_bf16(h[i]);
  }
}

template <int UPAD>
__global__ __launch_bounds__(2 * UPAD) void gru_bwd_fast(const Params p) {
  constexpr int THREADS = 2 * UPAD, NKS = 3 * UPAD / 16;
  constexpr int WROW = 3 * UPAD * 2 + kPadBytes;   // bytes of one LDS row
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* wl = smem;                                 // [UPAD][WROW]: row k holds U[k][g u + j] at column g UPAD + j
  char* dal = smem + UPAD * WROW;                  // [2][32][WROW]: the A operand, da as bf16
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
  const uint16_t* rsv = reinterpret_cast<const uint16_t*>(p.reserve);
  const uint16_t* dhs = reinterpret_cast<const uint16_t*>(p.dhs);

  for (int idx = tid; idx < 3 * UPAD * UPAD; idx += THREADS) {
    const int k = idx / (3 * UPAD), c = idx % (3 * UPAD), g = c / UPAD, jj = c % UPAD;
    const uint16_t v = (k < u && jj < u) ? rk[(int64_t)k * 3 * u + g * u + jj] : (uint16_t)0;
    *reinterpret_cast<uint16_t*>(wl + k * WROW + 2 * c) = v;
  }
  if (tid < kFastRows) first[tid] = row0 + tid < p.b ? first_valid(p.valid, row0 + tid, l) : l;
  __syncthreads();

  float dh[16];
  int fv[16];
  uint32_t rowok = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int64_t row = row0 + acc_row(i, fhalf);
    const bool ok = row < p.b;
    rowok |= (uint32_t)ok << i;
    fv[i] = first[acc_row(i, fhalf)];
    dh[i] = (ok && jok && p.dht) ? bf16_to_f32(reinterpret_cast<const uint16_t*>(p.dht)[row * u + j]) : 0.0f;
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
      // h_{t-1}: the stored output from the first valid step on, the initial state before it
      float hp = 0.0f;
      if (live) {
        if (t - 1 >= fv[i]) hp = bf16_to_f32(hs[(tok - 1) * u + j]);
        else if (h0) hp = bf16_to_f32(h0[row * u + j]);
      }
      // (an output before the first valid step is a constant zero: its gradient goes nowhere)
      const float g = dh[i] + ((live && dhs && t >= fv[i]) ? bf16_to_f32(dhs[tok * u + j]) : 0.0f);
      float dz = 0.0f, dr = 0.0f, dc = 0.0f, dq = 0.0f, seed = g;
      if (v) {
        const uint16_t* rs = rsv + tok * 4 * u + j;
        const float z = bf16_to_f32(rs[0]), r = bf16_to_f32(rs[u]), c = bf16_to_f32(rs[2 * u]),
                    q = bf16_to_f32(rs[3 * u]);
        dc = g * (1.0f - z) * (1.0f - c * c);
        dz = g * (hp - c) * z * (1.0f - z);
        dq = dc * r;
        dr = dc * q * r * (1.0f - r);
        seed = g * z;
      }
      const uint16_t bz = f32_to_bf16(dz), br = f32_to_bf16(dr), bc = f32_to_bf16(dc), bq = f32_to_bf16(dq);
      *reinterpret_cast<uint16_t*>(dt + lr * WROW + 2 * j) = bz;
      *reinterpret_cast<uint16_t*>(dt + lr * WROW + 2 * (UPAD + j)) = br;
      *reinterpret_cast<uint16_t*>(dt + lr * WROW + 2 * (2 * UPAD + j)) = bq;
      if (live) {
        uint16_t* ox = reinterpret_cast<uint16_t*>(p.dxz) + tok * 3 * u + j;
        ox[0] = bz, ox[u] = br, ox[2 * u] = bc;
        uint16_t* oa = reinterpret_cast<uint16_t*>(p.da) + tok * 3 * u + j;
        oa[0] = bz, oa[u] = br, oa[2 * u] = bq;
        if (p.hprev) reinterpret_cast<uint16_t*>(p.hprev)[tok * u + j] = f32_to_bf16(hp);
      }
      acc[i] = seed;
    }
    __syncthreads();
    const char* aa = dt + frow * WROW;
    const char* wb = wl + j * WROW;
#pragma unroll 4
    for (int ks = 0; ks < NKS; ++ks) {
      const int off = 16 * (2 * ks + fhalf);
      const bf16x8 fa = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(aa + off));
      const bf16x8 fb = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(wb + off));
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) dh[i] = acc[i];
  }

  if (p.dh0 && jok) {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if ((rowok >> i) & 1)
        reinterpret_cast<uint16_t*>(p.dh0)[(row0 + acc_row(i, fhalf)) * u + j] = f32_to_bf16(dh[i]);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// the generic path
// ------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kGenThreads) void gru_fwd_gen(const Params p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* hb = reinterpret_cast<float*>(smem);   // [2][kGenRows][u]
  const int tid = threadIdx.x, u = p.u, l = p.l;
  const int64_t row0 = (int64_t)blockIdx.x * kGenRows;
  const T* rk = reinterpret_cast<const T*>(p.rk);
  const T* xz = reinterpret_cast<const T*>(p.xz);
  const T* h0 = reinterpret_cast<const T*>(p.h0);
  T* hs = reinterpret_cast<T*>(p.hs);
  T* rsv = reinterpret_cast<T*>(p.reserve);

  for (int idx = tid; idx < kGenRows * u; idx += kGenThreads) {
    const int64_t row = row0 + idx / u;
    hb[idx] = (row < p.b && h0) ? load1(h0 + row * u + idx % u) : 0.0f;
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
      float az[kGenRows], ar[kGenRows], ah[kGenRows];
#pragma unroll
      for (int rr = 0; rr < kGenRows; ++rr) az[rr] = ar[rr] = ah[rr] = 0.0f;
      for (int k = 0; k < u; ++k) {
        const T* w = rk + (int64_t)k * 3 * u + j;
        const float wz = load1(w), wr = load1(w + u), wh = load1(w + 2 * u);
#pragma unroll
        for (int rr = 0; rr < kGenRows; ++rr) {
          const float hv = hc[rr * u + k];
          az[rr] = fmaf(hv, wz, az[rr]);
          ar[rr] = fmaf(hv, wr, ar[rr]);
          ah[rr] = fmaf(hv, wh, ah[rr]);
        }
      }
      const float rbz = p.rb ? p.rb[j] : 0.0f, rbr = p.rb ? p.rb[u + j] : 0.0f, rbh = p.rb ? p.rb[2 * u + j] : 0.0f;
#pragma unroll
      for (int rr = 0; rr < kGenRows; ++rr) {
        const int64_t row = row0 + rr;
        const float hold = hc[rr * u + j];
        if (row >= p.b) {
          hn[rr * u + j] = hold;
          continue;
        }
        const int64_t tok = row * l + t;
        const T* x = xz + tok * p.ldxz + j;
        const float z = sigmoid_f(load1(x) + az[rr] + rbz), r = sigmoid_f(load1(x + u) + ar[rr] + rbr);
        const float q = ah[rr] + rbh;
        const float c = tanhf(load1(x + 2 * u) + r * q);
        const float hv = z * hold + (1.0f - z) * c;
        const bool v = (valid >> rr) & 1;
        hn[rr * u + j] = v ? hv : hold;
        if (hs) store1(hs + tok * u + j, v ? hv : ((seen >> rr) & 1 ? hold : 0.0f));
        if (rsv) {
          T* rs = rsv + tok * 4 * u + j;
          store1(rs, z), store1(rs + u, r), store1(rs + 2 * u, c), store1(rs + 3 * u, q);
        }
      }
    }
    seen |= valid;
    __syncthreads();
  }

  if (p.ht) {
    const float* hf = hb + (l & 1) * kGenRows * u;
    for (int idx = tid; idx < kGenRows * u; idx += kGenThreads) {
      const int64_t row = row0 + idx / u;
      if (row < p.b) store1(reinterpret_cast<T*>(p.ht) + row * u + idx % u, hf[idx]);
    }
  }
}

// a value as the storage type holds it
template <typename T>
__device__ __forceinline__ float as_stored(float v) {
  if constexpr (sizeof(T) == 2) return bf16_to_f32(f32_to_bf16(v));
  else return v;
}

template <typename T>
__global__ __launch_bounds__(kGenThreads) void gru_bwd_gen(const Params p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, u = p.u, l = p.l;
  float* dh = reinterpret_cast<float*>(smem);          // [kGenRows][u]
  float* das = dh + kGenRows * u;                      // [kGenRows][3u]
  int* first = reinterpret_cast<int*>(das + kGenRows * 3 * u);   // [kGenRows]
  const int64_t row0 = (int64_t)blockIdx.x * kGenRows;
  const T* rk = reinterpret_cast<const T*>(p.rk);
  const T* hs = reinterpret_cast<const T*>(p.hs);
  const T* h0 = reinterpret_cast<const T*>(p.h0);
  const T* rsv = reinterpret_cast<const T*>(p.reserve);
  const T* dhs = reinterpret_cast<const T*>(p.dhs);
  const T* dht = reinterpret_cast<const T*>(p.dht);

  for (int idx = tid; idx < kGenRows * u; idx += kGenThreads) {
    const int64_t row = row0 + idx / u;
    dh[idx] = (row < p.b && dht) ? load1(dht + row * u + idx % u) : 0.0f;
  }
  if (tid < kGenRows) first[tid] = row0 + tid < p.b ? first_valid(p.valid, row0 + tid, l) : l;
  __syncthreads();

  for (int t = l - 1; t >= 0; --t) {
    for (int idx = tid; idx < kGenRows * u; idx += kGenThreads) {
      const int rr = idx / u, j = idx % u;
      const int64_t row = row0 + rr;
      float dz = 0.0f, dr = 0.0f, dc = 0.0f, dq = 0.0f;
      if (row < p.b) {
        const int64_t tok = row * l + t;
        const bool v = !p.valid || p.valid[tok] != 0;
        const int fv = first[rr];
        float hp = 0.0f;
        if (t - 1 >= fv) hp = load1(hs + (tok - 1) * u + j);
        else if (h0) hp = load1(h0 + row * u + j);
        const float g = dh[idx] + ((dhs && t >= fv) ? load1(dhs + tok * u + j) : 0.0f);
        float seed = g;
        if (v) {
          const T* rs = rsv + tok * 4 * u + j;
          const float z = load1(rs), r = load1(rs + u), c = load1(rs + 2 * u), q = load1(rs + 3 * u);
          dc = g * (1.0f - z) * (1.0f - c * c);
          dz = g * (hp - c) * z * (1.0f - z);
          dq = dc * r;
          dr = dc * q * r * (1.0f - r);
          seed = g * z;
        }
        dh[idx] = seed;
        T* ox = reinterpret_cast<T*>(p.dxz) + tok * 3 * u + j;
        store1(ox, dz), store1(ox + u, dr), store1(ox + 2 * u, dc);
        T* oa = reinterpret_cast<T*>(p.da) + tok * 3 * u + j;
        store1(oa, dz), store1(oa + u, dr), store1(oa + 2 * u, dq);
        if (p.hprev) store1(reinterpret_cast<T*>(p.hprev) + tok * u + j, hp);
      }
      das[rr * 3 * u + j] = as_stored<T>(dz);
      das[rr * 3 * u + u + j] = as_stored<T>(dr);
      das[rr * 3 * u + 2 * u + j] = as_stored<T>(dq);
    }
    __syncthreads();
    // dh[., k] += da . U[k, :]: a wave per k, lanes along the row of U, a fixed shuffle tree
    for (int k = wave; k < u; k += kGenThreads / 64) {
      float s[kGenRows];
#pragma unroll
      for (int rr = 0; rr < kGenRows; ++rr) s[rr] = 0.0f;
      const T* w = rk + (int64_t)k * 3 * u;
      for (int jj = lane; jj < 3 * u; jj += 64) {
        const float wv = load1(w + jj);
#pragma unroll
        for (int rr = 0; rr < kGenRows; ++rr) s[rr] = fmaf(das[rr * 3 * u + jj], wv, s[rr]);
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

  if (p.dh0) {
    for (int idx = tid; idx < kGenRows * u; idx += kGenThreads) {
      const int64_t row = row0 + idx / u;
      if (row < p.b) store1(reinterpret_cast<T*>(p.dh0) + row * u + idx % u, dh[idx]);
    }
  }
}

// ---- host ----
// (one record per process, not per thread: torch runs a backward on an autograd thread; kernel and upad in one word)
std::atomic<uint32_t> g_route{0};
inline void set_route(int kernel, int upad) { g_route.store((uint32_t)kernel << 16 | (uint32_t)upad); }

template <typename K>
int launch(const char* what, K kern, const gru::Plan& pl, int64_t lds, const Params& p, hipStream_t st) {
  KRS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)pl.groups), dim3((unsigned)pl.threads), (size_t)lds, st, p);
  KRS_CHECK_LAUNCH(what);
  return KRS_OK;
}

int plan_call(const char* what, int dtype, int64_t b, int64_t l, int64_t u, gru::Plan& pl) {
  pl = gru::plan(b, l, u, dtype);
  if (pl.status == gru::kInvalid)
    return fail(KRS_ERR_INVALID, "%s: b=%lld l=%lld u=%lld dtype=%d: needs %s", what, (long long)b, (long long)l,
                (long long)u, dtype, pl.why);
  if (pl.status == gru::kUnsupported)
    return fail(KRS_ERR_UNSUPPORTED, "%s: b=%lld l=%lld u=%lld: supported is %s", what, (long long)b, (long long)l,
                (long long)u, pl.why);
  return KRS_OK;
}

}  // namespace
}  // namespace krs

extern "C" size_t krs_gru_reserve_bytes(int64_t b, int64_t l, int64_t u, int dtype) {
  return krs::gru::reserve_bytes(b, l, u, dtype);
}

extern "C" int krs_gru_last_route(int* kernel, int* upad) {
  const uint32_t r = krs::g_route.load();
  if (kernel) *kernel = (int)(r >> 16);
  if (upad) *upad = (int)(r & 0xffffu);
  return (int)(r >> 16);
}

extern "C" int krs_gru_fwd(const void* xz, int64_t ldxz, const void* recurrent_kernel, const float* recurrent_bias,
                           const uint8_t* valid, const void* h0, int dtype, int64_t b, int64_t l, int64_t u, void* hs,
                           void* h_last, void* reserve, void* stream) {
  using namespace krs;
  const char* what = "krs_gru_fwd";
  set_route(KRS_GRU_NONE, 0);
  gru::Plan pl;
  const int rc = plan_call(what, dtype, b, l, u, pl);
  if (rc != KRS_OK || pl.kernel == gru::kRouteNone) return rc;
  KRS_REQUIRE(xz && recurrent_kernel, "%s: null xz or recurrent_kernel", what);
  KRS_REQUIRE(ldxz >= 3 * u, "%s: token stride of xz below 3 u", what);
  KRS_REQUIRE(hs || h_last, "%s: no output is wanted", what);
  KRS_REQUIRE(!reserve || hs, "%s: a training forward (reserve) writes hs too", what);
  Params p{};
  p.xz = xz, p.ldxz = ldxz, p.rk = recurrent_kernel, p.rb = recurrent_bias, p.valid = valid, p.h0 = h0;
  p.hs = hs, p.ht = h_last, p.reserve = reserve;
  p.b = b, p.l = (int)l, p.u = (int)u;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int lrc;
  if (pl.kernel == gru::kRouteFast) {
    if (pl.upad == 32) lrc = launch(what, gru_fwd_fast<32>, pl, pl.lds_fwd, p, st);
    else if (pl.upad == 64) lrc = launch(what, gru_fwd_fast<64>, pl, pl.lds_fwd, p, st);
    else lrc = launch(what, gru_fwd_fast<128>, pl, pl.lds_fwd, p, st);
  } else if (dtype == KRS_BF16) {
    lrc = launch(what, gru_fwd_gen<uint16_t>, pl, pl.lds_fwd, p, st);
  } else {
    lrc = launch(what, gru_fwd_gen<float>, pl, pl.lds_fwd, p, st);
  }
  if (lrc != KRS_OK) return lrc;
  set_route(pl.kernel, pl.upad);
  return KRS_OK;
}

extern "C" int krs_gru_bwd(const void* recurrent_kernel, const uint8_t* valid, const void* h0, const void* hs,
                           const void* reserve, const void* dhs, const void* dh_last, int dtype, int64_t b, int64_t l,
                           int64_t u, void* dxz, void* da, void* h_prev, void* dh0, void* stream) {
  using namespace krs;
  const char* what = "krs_gru_bwd";
  set_route(KRS_GRU_NONE, 0);
  gru::Plan pl;
  const int rc = plan_call(what, dtype, b, l, u, pl);
  if (rc != KRS_OK || pl.kernel == gru::kRouteNone) return rc;
  KRS_REQUIRE(recurrent_kernel && hs && reserve, "%s: null recurrent_kernel, hs or reserve", what);
  KRS_REQUIRE(dxz && da, "%s: null dxz or da", what);
  Params p{};
  p.rk = recurrent_kernel, p.valid = valid, p.h0 = h0, p.hs = const_cast<void*>(hs);
  p.reserve = const_cast<void*>(reserve), p.dhs = dhs, p.dht = dh_last;
  p.dxz = dxz, p.da = da, p.hprev = h_prev, p.dh0 = dh0;
  p.b = b, p.l = (int)l, p.u = (int)u;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int lrc;
  if (pl.kernel == gru::kRouteFast) {
    if (pl.upad == 32) lrc = launch(what, gru_bwd_fast<32>, pl, pl.lds_bwd, p, st);
    else if (pl.upad == 64) lrc = launch(what, gru_bwd_fast<64>, pl, pl.lds_bwd, p, st);
    else lrc = launch(what, gru_bwd_fast<128>, pl, pl.lds_bwd, p, st);
  } else if (dtype == KRS_BF16) {
    lrc = launch(what, gru_bwd_gen<uint16_t>, pl, pl.lds_bwd, p, st);
  } else {
    lrc = launch(what, gru_bwd_gen<float>, pl, pl.lds_bwd, p, st);
  }
  if (lrc != KRS_OK) return lrc;
  set_route(pl.kernel, pl.upad);
  return KRS_OK;
}
