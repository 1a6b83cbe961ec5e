// Device pieces shared by the GEMM translation units (gemm.hip, gemm_q8.hip): the kernel parameter block and its host-side
// fill, the register staging of a K-contiguous 128-row tile, the epilogue of
// one element and of eight consecutive columns (bias, activation, cross form, residual, one rounding to the output dtype),
// the wave epilogue that stages accumulators through LDS (general, cross and residual builds), and the wait / barrier forms
// of the LDS-DMA rings.  One copy of the epilogue arithmetic: every product kernel calls these.
#ifndef KRS_GEMM_DEVICE_H_
#define KRS_GEMM_DEVICE_H_

#include "gemm_plan.h"
#include "krs_dense_common.h"

namespace krs {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct GemmParams {
  const char* a; int64_t lda; int a_km;
  const char* b; int64_t ldb; int b_nk;
  char* c; int64_t ldc;
  int64_t m, n, k;
  int out_dtype;
  krs_gemm_epilogue ep;
  int has_ep;
  // split-K
  int splits; int64_t k_per_split; float* slabs;
  int ep_vec;  // every epilogue operand allows 8-wide vector access
  // fused cross-backward epilogue (EPI 3 .. 8 of gemm_pp256_kernel, krs_gemm_cross_bwd): operands of the layer below
  const void* f_x0; const void* f_u; const void* f_uup; void* f_dz; void* f_dx0; float* f_partial; int64_t f_ld; int f_act; int f_fold;
};

// operands, shape and epilogue of a product (host); the caller then sets what is its own: splits, slabs, ep_vec, the f_* fields
inline GemmParams gemm_params(const void* a, int64_t lda, bool a_km, const void* b, int64_t ldb, bool b_nk, void* c, int64_t ldc,
                              int64_t m, int64_t n, int64_t k, int out_dtype, const krs_gemm_epilogue* ep) {
  GemmParams p{};
  p.a = reinterpret_cast<const char*>(a); p.lda = lda; p.a_km = a_km;
  p.b = reinterpret_cast<const char*>(b); p.ldb = ldb; p.b_nk = b_nk;
  p.c = reinterpret_cast<char*>(c); p.ldc = ldc; p.m = m; p.n = n; p.k = k; p.out_dtype = out_dtype;
  p.has_ep = ep != nullptr;
  if (ep) p.ep = *ep;
  p.splits = 1; p.k_per_split = k;
  return p;
}

// ---- staging of a 128-row tile: HBM -> registers -> LDS ([row][k] with 144-byte rows) ---------
// operand stored K-contiguous, ES bytes per element: elem(row, k) at base + (row*ld + k)*ES.  `row0` tile origin along the
// operand's row axis (m for A, n for B), `k0` along K; rows/kk are the operand extents.  A thread takes 16-byte chunk (t & 7)
// of rows (t >> 3) + 32 i; a chunk at or beyond kk and a row beyond the operand are zero.
template <int ES>
__device__ __forceinline__ void load_kcontig(const char* base, int64_t ld, int64_t row0, int64_t k0,
                                             int64_t rows, int64_t kk, u32x4 (&r)[4]) {
  const int t = threadIdx.x;
  const int c = t & 7;
  const int64_t kel = k0 + c * (16 / ES);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t row = row0 + (t >> 3) + 32 * i;
    u32x4 v = {0, 0, 0, 0};
    if (row < rows && kel < kk) v = *reinterpret_cast<const u32x4*>(base + (row * ld + kel) * ES);
    r[i] = v;
  }
}
// LDS address of 16-byte chunk `c` (0..7) of tile row `row`.
//   K-contiguous staged operands: 144-byte rows, no swizzle: fragment reads (ds_read_b128) and
//     the row-wise ds_write_b128 stores are both conflict-free;
//   transposed-staged operands: 128-byte rows, chunk XOR (row >> 3): the column-wise
//     ds_write_b64 / b128 stores drop from 16-way to the 2-way minimum of that access shape
//     and fragment reads cost 2 cycles per lane group (scripts/lds_conflicts.py).
template <bool KS>
__device__ __forceinline__ int lds_chunk_off(int row, int c) {
  if constexpr (KS) return row * gplan::kRowBytes + ((c ^ ((row >> 3) & 7)) << 4);
  else return row * gplan::kLdsStride + (c << 4);
}

__device__ __forceinline__ void store_kcontig(char* tile, const u32x4 (&r)[4]) {
  const int t = threadIdx.x;
  const int c = t & 7;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    *reinterpret_cast<u32x4*>(tile + lds_chunk_off<false>((t >> 3) + 32 * i, c)) = r[i];
}

// epilogue of one element; `odt` = dtype of C, x0, x, u_out, r
__device__ __forceinline__ void epilogue_store(const GemmParams& p, int64_t i, int64_t j, float v) {
  const int odt = p.out_dtype;
  if (p.has_ep) {
    const krs_gemm_epilogue& e = p.ep;
    if (e.bias) v += e.bias[j];
    v = apply_act(e.act, v);
    if (e.x0) {
      const float xv = ld_elem(e.x, odt, i * e.ldx + j);
      if (e.u_out) st_elem(e.u_out, odt, i * e.ldu + j, v);
      const float u = v + e.diag_scale * xv;
      v = ld_elem(e.x0, odt, i * e.ldx + j) * u + xv;
    }
    if (e.r) v += e.beta * ld_elem(e.r, odt, i * e.ldr + j);
  }
  st_elem(p.c, odt, i * p.ldc + j, v);
}

// 8 consecutive columns of one row; every pointer 16-byte aligned, every ld a multiple of 8
__device__ __forceinline__ void load8(const void* base, int dt, int64_t off, float (&f)[8]) {
  if (dt == KRS_BF16) {
    const uint4 r = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(base) + off);
    f[0] = __uint_as_float(r.x << 16); f[1] = __uint_as_float(r.x & 0xffff0000u);
    f[2] = __uint_as_float(r.y << 16); f[3] = __uint_as_float(r.y & 0xffff0000u);
    f[4] = __uint_as_float(r.z << 16); f[5] = __uint_as_float(r.z & 0xffff0000u);
    f[6] = __uint_as_float(r.w << 16); f[7] = __uint_as_float(r.w & 0xffff0000u);
  } else {
    const float4 a = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(base) + off);
    const float4 b = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(base) + off + 4);
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
  }
}
__device__ __forceinline__ void store8(void* base, int dt, int64_t off, const float (&f)[8]) {
  if (dt == KRS_BF16) {
    *reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(base) + off) =
        make_uint4(pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]), pack_bf16x2(f[4], f[5]),
                   pack_bf16x2(f[6], f[7]));
  } else {
    float* d = reinterpret_cast<float*>(base) + off;
    *reinterpret_cast<float4*>(d) = make_float4(f[0], f[1], f[2], f[3]);
    *reinterpret_cast<float4*>(d + 4) = make_float4(f[4], f[5], f[6], f[7]);
  }
}

// The streams of the specialised epilogues (x0, x, R in; u, y out) are touched once per launch and
// are two orders of magnitude larger than L2: non-temporal accesses keep them from evicting the
// operand panels the other N tiles of the same M panel are about to re-read.
__device__ __forceinline__ void store8_bf16_nt(void* base, int64_t off, const float (&f)[8]) {
  const u32x4 v = {pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]), pack_bf16x2(f[4], f[5]), pack_bf16x2(f[6], f[7])};
  __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(reinterpret_cast<uint16_t*>(base) + off));
}
__device__ __forceinline__ uint4 load8_bf16_nt(const void* base, int64_t off) {
  const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(reinterpret_cast<const uint16_t*>(base) + off));
  return make_uint4(v[0], v[1], v[2], v[3]);
}

__device__ __forceinline__ void unpack_bf16x8(const uint4& r, float (&f)[8]) {
  f[0] = __uint_as_float(r.x << 16); f[1] = __uint_as_float(r.x & 0xffff0000u);
  f[2] = __uint_as_float(r.y << 16); f[3] = __uint_as_float(r.y & 0xffff0000u);
  f[4] = __uint_as_float(r.z << 16); f[5] = __uint_as_float(r.z & 0xffff0000u);
  f[6] = __uint_as_float(r.w << 16); f[7] = __uint_as_float(r.w & 0xffff0000u);
}

__device__ __forceinline__ void epilogue_store_vec8(const GemmParams& p, int64_t i, int64_t j, float (&v)[8]) {
  const int odt = p.out_dtype;
  if (p.has_ep) {
    const krs_gemm_epilogue& e = p.ep;
    if (e.bias) {
      const float4 b0 = *reinterpret_cast<const float4*>(e.bias + j);
      const float4 b1 = *reinterpret_cast<const float4*>(e.bias + j + 4);
      v[0] += b0.x; v[1] += b0.y; v[2] += b0.z; v[3] += b0.w;
      v[4] += b1.x; v[5] += b1.y; v[6] += b1.z; v[7] += b1.w;
    }
    if (e.act != KRS_ACT_NONE) {
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = apply_act(e.act, v[q]);
    }
    if (e.x0) {
      float xv[8], x0v[8];
      load8(e.x, odt, i * e.ldx + j, xv);
      load8(e.x0, odt, i * e.ldx + j, x0v);
      if (e.u_out) store8(e.u_out, odt, i * e.ldu + j, v);
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = x0v[q] * (v[q] + e.diag_scale * xv[q]) + xv[q];
    }
    if (e.r) {
      float rv[8];
      load8(e.r, odt, i * e.ldr + j, rv);
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] += e.beta * rv[q];
    }
  }
  store8(p.c, odt, i * p.ldc + j, v);
}

// Epilogue shared by the GEMM kernels.  The accumulators go through LDS (the operand tiles are
// dead by now) so that each lane ends up with 8 consecutive columns of one row: x0 / x / R are
// read and y / u written as 16-byte (bf16) or 2x16-byte (fp32) vectors.
// ---- epilogue, in chunks of 32 rows x 64 columns per wave --------------------------------------
// The accumulators go through LDS (the operand tiles are dead: every wave passed the loop's last
// barrier) so that each lane ends up with 8 consecutive columns of one row: x0 / x / R are read
// and y / u written as 16-byte (bf16) or 2x16-byte (fp32) vectors.
// MFMA C/D layout: col = lane & 31, row = (r & 3) + 8*(r >> 2) + 4*(lane >> 5).
// epi_prefetch issues a chunk's x0 / x / R loads (specialised forms EPI 1 / 2), epi_process stages
// the chunk's accumulators and writes it; callers order them so that a chunk's loads are in
// flight while the previous chunk is processed.

struct EpiOperands {
  uint4 ex[4], ex0[4];
};
// The cross form of a call whose x IS its x0 (the planner's KRS_GEMM_SCHED_X_IS_X0, gemm_pp64_kernel only): build 1's
// arithmetic on ONE loaded operand -- ex0 is never touched, so a chunk costs half the registers.
constexpr int kEpiCrossXIsX0 = 11;

template <int EPI>
__device__ __forceinline__ void epi_prefetch(const GemmParams& p, EpiOperands& o, int64_t row0, int64_t wn0) {
  if constexpr (EPI == 1 || EPI == 2 || EPI == kEpiCrossXIsX0) {
    const int lane = threadIdx.x & 63;
    const int64_t gnc = min(wn0 + (lane & 7) * 8, p.n - 8);
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int64_t gmc = min(row0 + it * 8 + (lane >> 3), p.m - 1);
      if constexpr (EPI == kEpiCrossXIsX0) {
        o.ex[it] = load8_bf16_nt(p.ep.x, gmc * p.ep.ldx + gnc);
      } else if constexpr (EPI == 1) {
        o.ex[it] = load8_bf16_nt(p.ep.x, gmc * p.ep.ldx + gnc);
        // (unconditional even when x is x0: a predicated load makes hipcc drain the whole load queue)
        o.ex0[it] = load8_bf16_nt(p.ep.x0, gmc * p.ep.ldx + gnc);
      } else {
        o.ex[it] = load8_bf16_nt(p.ep.r, gmc * p.ep.ldr + gnc);
      }
    }
  }
}

// The lane's eight bias values (columns wn0 + (lane & 7) * 8 .. + 7, the same for every row of the wave's block; the column
// clamped as epi_prefetch clamps it: a lane beyond n stores nothing), loaded once for epi_process<EPI, true>.  Needs n >= 8
// and the bias on 16 bytes, which the specialised builds have (ep_vec).  Always TWO load instructions, so that a ring's
// counted waits can count them: without a bias they read the first 32 bytes of B (any readable address would do) and
// epi_process never looks at the values.
__device__ __forceinline__ void epi_load_bias(const GemmParams& p, int64_t wn0, float (&b)[8]) {
  const float* src = p.ep.bias ? p.ep.bias + min(wn0 + (threadIdx.x & 7) * 8, p.n - 8) : reinterpret_cast<const float*>(p.b);
  const float4 b0 = *reinterpret_cast<const float4*>(src);
  const float4 b1 = *reinterpret_cast<const float4*>(src + 4);
  b[0] = b0.x; b[1] = b0.y; b[2] = b0.z; b[3] = b0.w; b[4] = b1.x; b[5] = b1.y; b[6] = b1.z; b[7] = b1.w;
}

// acc2: the chunk's two 32x32 accumulator fragments (columns 0..31 / 32..63); `stage`: the wave's
// private 32 x SST floats of LDS; (row0, wn0): origin of the chunk in C.
// PREBIAS (cross builds): the lane's eight bias values are in `pre_bias` (epi_load_bias) instead of being loaded here, per
// eight-row step.  Such a load is the youngest memory operation when it is used, so hipcc waits vmcnt(0) for it: every
// step then also waits for the operands requested ahead and for the acknowledgement of every earlier store.
template <int EPI, bool PREBIAS = false>
__device__ __forceinline__ void epi_process(const GemmParams& p, f32x16 (&acc2)[2], const EpiOperands& o, float* stage,
                                            int64_t row0, int64_t wn0, int split, const float* pre_bias = nullptr) {
  const int lane = threadIdx.x & 63;
  const int frow = lane & 31;
  const int fhalf = lane >> 5;
  constexpr int SST = 68;  // staging row stride in floats (64 + pad)
  const int ec = (lane & 7) * 8;
  const int64_t gn = wn0 + ec;
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      stage[((r & 3) + 8 * (r >> 2) + 4 * fhalf) * SST + j * 32 + frow] = acc2[j][r];
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // wave-private staging: no workgroup barrier
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int er = it * 8 + (lane >> 3);
    const int64_t gm = row0 + er;
    if (gm >= p.m || gn >= p.n) continue;
    float v[8];
    const float4 v0 = *reinterpret_cast<const float4*>(stage + er * SST + ec);
    const float4 v1 = *reinterpret_cast<const float4*>(stage + er * SST + ec + 4);
    v[0] = v0.x; v[1] = v0.y; v[2] = v0.z; v[3] = v0.w; v[4] = v1.x; v[5] = v1.y; v[6] = v1.z; v[7] = v1.w;
    if constexpr (EPI == 1 || EPI == kEpiCrossXIsX0) {
      if (p.ep.bias) {
        if constexpr (PREBIAS) {
#pragma unroll
          for (int q = 0; q < 8; ++q) v[q] += pre_bias[q];
        } else {
          const float4 b0 = *reinterpret_cast<const float4*>(p.ep.bias + gn);
          const float4 b1 = *reinterpret_cast<const float4*>(p.ep.bias + gn + 4);
          v[0] += b0.x; v[1] += b0.y; v[2] += b0.z; v[3] += b0.w;
          v[4] += b1.x; v[5] += b1.y; v[6] += b1.z; v[7] += b1.w;
        }
      }
      if (p.ep.act != KRS_ACT_NONE) {
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = apply_act(p.ep.act, v[q]);
      }
      if (p.ep.u_out) store8_bf16_nt(p.ep.u_out, gm * p.ep.ldu + gn, v);
      float xv[8], x0v[8];
      unpack_bf16x8(o.ex[it], xv);
      unpack_bf16x8(EPI == 1 ? o.ex0[it] : o.ex[it], x0v);
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = x0v[q] * (v[q] + p.ep.diag_scale * xv[q]) + xv[q];
      store8_bf16_nt(p.c, gm * p.ldc + gn, v);
    } else if constexpr (EPI == 2) {
      float rv[8];
      unpack_bf16x8(o.ex[it], rv);
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] += p.ep.beta * rv[q];
      store8_bf16_nt(p.c, gm * p.ldc + gn, v);
    } else if (p.splits > 1) {
      float* dst = p.slabs + ((int64_t)split * p.m + gm) * p.n + gn;
      if (p.ep_vec) {
        *reinterpret_cast<float4*>(dst) = v0;
        *reinterpret_cast<float4*>(dst + 4) = v1;
      } else {
        for (int q = 0; q < 8 && gn + q < p.n; ++q) dst[q] = v[q];
      }
    } else if (p.ep_vec) {
      epilogue_store_vec8(p, gm, gn, v);
    } else {
      for (int q = 0; q < 8 && gn + q < p.n; ++q) epilogue_store(p, gm, gn + q, v[q]);
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// a wave's 64x64 block of C (two chunks)
template <int EPI>
__device__ __forceinline__ void gemm_epilogue_wave(const GemmParams& p, f32x16 (&acc)[2][2], float* stage, int64_t wm0,
                                                   int64_t wn0, int split) {
  EpiOperands o0, o1;
  epi_prefetch<EPI>(p, o0, wm0, wn0);
  epi_prefetch<EPI>(p, o1, wm0 + 32, wn0);
  epi_process<EPI>(p, acc[0], o0, stage, wm0, wn0, split);
  epi_process<EPI>(p, acc[1], o1, stage, wm0 + 32, wn0, split);
}

// a wave's 128x64 block of C (four chunks), two chunks of operands in flight
template <int EPI>
__device__ __forceinline__ void gemm_epilogue_wave128(const GemmParams& p, f32x16 (&acc)[2][2][2], float* stage,
                                                      int64_t wm0, int64_t wn0, int split) {
  EpiOperands o0, o1;
  epi_prefetch<EPI>(p, o0, wm0, wn0);
  epi_prefetch<EPI>(p, o1, wm0 + 32, wn0);
  epi_process<EPI>(p, acc[0][0], o0, stage, wm0, wn0, split);
  epi_prefetch<EPI>(p, o0, wm0 + 64, wn0);
  epi_process<EPI>(p, acc[0][1], o1, stage, wm0 + 32, wn0, split);
  epi_prefetch<EPI>(p, o1, wm0 + 96, wn0);
  epi_process<EPI>(p, acc[1][0], o0, stage, wm0 + 64, wn0, split);
  epi_process<EPI>(p, acc[1][1], o1, stage, wm0 + 96, wn0, split);
}

// After a loop that waited for its LDS-DMA with opaque assembly, hipcc still believes the DMA may be in flight
// and fences EVERY later LDS read with `s_waitcnt vmcnt(0)` -- in the epilogue that made each 16-byte store wait
// for the acknowledgement of all earlier stores of the wave.  A counted wait it can see (free at run time: the
// loop has retired everything but the ALLOW youngest loads) tells it that the DMA has landed.
template <int ALLOW>
__device__ __forceinline__ void lds_dma_retired() {
  static_assert(ALLOW >= 0 && ALLOW < 64, "vmcnt is a 6-bit counter");
  __builtin_amdgcn_s_waitcnt((ALLOW & 15) | ((ALLOW >> 4) << 14) | (7 << 4) | (15 << 8));  // vmcnt only
}

__device__ __forceinline__ void pp_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_barrier" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}
template <int N>
__device__ __forceinline__ void pp_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// Launches Kern with `lds` bytes of dynamic LDS.  The kernel's dynamic-LDS limit is raised on its first launch: a
// function-local static, initialised once per kernel (and thread-safe).  `what` names the launch in error messages.
template <auto Kern, class... Args>
int launch_lds(const char* what, dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
  static const hipError_t attr =
      hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (attr != hipSuccess) return fail(KRS_ERR_LAUNCH, "%s: hipFuncSetAttribute: %s", what, hipGetErrorString(attr));
  hipLaunchKernelGGL(Kern, grid, block, lds, st, args...);
  KRS_CHECK_LAUNCH(what);
  return KRS_OK;
}

}  // namespace
}  // namespace krs
#endif
