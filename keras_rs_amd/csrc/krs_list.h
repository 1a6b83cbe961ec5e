// What the list kernels (K8 - K12) share: how lists are packed into a workgroup, the LDS bitonic sort of 64-bit keys,
// the (key, index) pair, reductions and scans over the threads of one list, and the host check of a [batch, list]
// operand.  Everything here assumes workgroups of kListThreads threads.  A new list kernel starts from this header.
#ifndef KRS_LIST_H_
#define KRS_LIST_H_

#include "krs_common.h"

namespace krs {

constexpr int kListThreads = 1024;
constexpr int kListWaves = kListThreads / 64;

// Geometry of a launch whose lists (or rows) all have `len` items, the same on host and device.  Lists of up to
// kListThreads items are packed several per workgroup, so every workgroup runs one uniform schedule; longer lists
// take a workgroup each and a thread holds ept items.
struct ListPack {
  int P;     // pow2 >= len: sort slots of a list
  int tpl;   // threads per list
  int ept;   // slots per thread
  int lpb;   // lists per workgroup
  __host__ __device__ __forceinline__ explicit ListPack(int len) {
    P = pow2_at_least(len);
    tpl = P >= kListThreads ? kListThreads : P;
    ept = P / tpl;
    lpb = kListThreads / tpl;
  }
  __host__ __device__ __forceinline__ int n_slots() const { return lpb * P; }
  __host__ __forceinline__ dim3 grid(int64_t batch) const { return dim3((unsigned)ceil_div(batch, lpb)); }
  __device__ __forceinline__ int64_t row0() const { return (int64_t)blockIdx.x * lpb; }   // the workgroup's first list
  __device__ __forceinline__ int q() const { return threadIdx.x / tpl; }                  // this thread's list
  __device__ __forceinline__ int u() const { return threadIdx.x - q() * tpl; }            // and its place in it
};

// ---- (key, index) pair ---------------------------------------------------------------------------------------------
// (key << 32) | ~index: "descending uint64" is key descending, then index ascending, and no two pairs are equal.
// With key = order_key(x) the value 0 is below every real pair and pads partial lists.
__device__ __forceinline__ uint64_t pair_key(uint32_t key, uint32_t index) {
  return ((uint64_t)key << 32) | (uint32_t)~index;
}
__device__ __forceinline__ uint32_t pair_index(uint64_t e) { return ~(uint32_t)e; }

// ---- bitonic sort of LDS keys, descending --------------------------------------------------------------------------
// One compare-exchange step (kk, j) over s[0 .. n).  s holds whole lists of P slots each (P a power of two), and
// slot 0 of each sits at the position `base` of the sorted sequence it belongs to: 0 for a list that is sorted whole,
// the block's offset for a block of a longer list (then P = n).  Ends with a barrier.
__device__ __forceinline__ void bitonic_step(uint64_t* s, int n, int P, int64_t base, int64_t kk, int j) {
  for (int p = threadIdx.x; p < n / 2; p += kListThreads) {
    const int e = ((p & ~(j - 1)) << 1) | (p & (j - 1));
    const uint64_t a = s[e], b = s[e + j];
    const bool desc = ((base + (e & (P - 1))) & kk) == 0;
    if (desc ? a < b : a > b) {
      s[e] = b;
      s[e + j] = a;
    }
  }
  __syncthreads();
}
// full sort of every P-long list of s[0 .. n) (descending when base & P == 0)
__device__ __forceinline__ void bitonic_sort(uint64_t* s, int n, int P, int64_t base) {
  for (int kk = 2; kk <= P; kk <<= 1)
    for (int j = kk >> 1; j > 0; j >>= 1) bitonic_step(s, n, P, base, kk, j);
}

// ---- reductions and scans over the tpl threads of each list --------------------------------------------------------
// tpl is a power of two and uniform over the workgroup; every thread of the workgroup makes the call.

// All-reduce of NV values; slot j is a maximum when bit j of max_mask is set, a sum otherwise.  A butterfly over the
// lanes of a wave, then a butterfly over the wave partials of the list: every thread ends with its list's totals.
template <int NV>
__device__ __forceinline__ void seg_all_reduce(float (*red)[kListWaves], float (&v)[NV], unsigned max_mask, int tpl) {
  const int w = tpl < 64 ? tpl : 64;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const bool mx = (max_mask >> j) & 1u;
    for (int o = 1; o < w; o <<= 1) {
      const float t = __shfl_xor(v[j], o);
      v[j] = mx ? fmaxf(v[j], t) : v[j] + t;
    }
  }
  if (tpl > 64) {
    const int wave = threadIdx.x >> 6, nw = tpl >> 6, w0 = (wave / nw) * nw;
    __syncthreads();   // (the previous call's partials have been read)
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int j = 0; j < NV; ++j) red[j][wave] = v[j];
    }
    __syncthreads();
    const int mine = w0 + (threadIdx.x & (nw - 1));   // (nw is a power of two: a butterfly over the list's waves)
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const bool mx = (max_mask >> j) & 1u;
      float a = red[j][mine];
      for (int o = 1; o < nw; o <<= 1) {
        const float t = __shfl_xor(a, o);
        a = mx ? fmaxf(a, t) : a + t;
      }
      v[j] = a;
    }
  }
}

// exclusive prefix sum of cnt; ibuf holds kListWaves ints
__device__ __forceinline__ int seg_exclusive_scan(int* ibuf, int cnt, int tpl) {
  const int w = tpl < 64 ? tpl : 64;
  const int lane = threadIdx.x & (w - 1);
  int inc = cnt;
  for (int o = 1; o < w; o <<= 1) {
    const int t = __shfl_up(inc, o, w);
    if (lane >= o) inc += t;
  }
  int pre = inc - cnt;
  if (tpl > 64) {
    const int wave = threadIdx.x >> 6, nw = tpl >> 6, w0 = (wave / nw) * nw;
    __syncthreads();
    if ((threadIdx.x & 63) == 63) ibuf[wave] = inc;
    __syncthreads();
    for (int i = w0; i < wave; ++i) pre += ibuf[i];
  }
  return pre;
}

// inclusive scan (REVERSE: suffix) of v, a sum or a maximum; buf holds kListThreads floats and keeps every thread's
// result until the next call; u is the thread's place in its list
template <bool REVERSE, bool MAX>
__device__ __forceinline__ float seg_scan(float* buf, float v, int u, int tpl) {
  __syncthreads();   // (the previous scan's results have been read)
  buf[threadIdx.x] = v;
  __syncthreads();
  for (int o = 1; o < tpl; o <<= 1) {
    const bool has = REVERSE ? u + o < tpl : u >= o;
    if (has) {
      const float w = buf[REVERSE ? threadIdx.x + o : threadIdx.x - o];
      v = MAX ? fmaxf(v, w) : v + w;
    }
    __syncthreads();
    buf[threadIdx.x] = v;
    __syncthreads();
  }
  return v;
}

// ---- host ----------------------------------------------------------------------------------------------------------
// the shape and dtype of a [batch, list] operand with the leading dimension ld
inline int check_lists(const char* what, int64_t ld, int dtype, int64_t batch, int64_t list) {
  KRS_REQUIRE(list >= 1 && list <= KRS_RANK_MAX_LIST,
              "%s: list length %lld outside the supported 1..%d (KRS_RANK_MAX_LIST)", what, (long long)list,
              KRS_RANK_MAX_LIST);
  KRS_REQUIRE(batch >= 0, "%s: negative batch", what);
  KRS_REQUIRE(ld >= list, "%s: ld %lld below the list length %lld", what, (long long)ld, (long long)list);
  KRS_REQUIRE(dtype == KRS_F32 || dtype == KRS_BF16, "%s: bad dtype", what);
  return KRS_OK;
}

}  // namespace krs
#endif
