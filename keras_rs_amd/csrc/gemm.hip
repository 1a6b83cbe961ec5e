// K3 -- FeatureCross (DCN-v2): the dense projection on MFMA with the cross
// epilogue fused, plus the elementwise backward pieces.
//
// Replaces FeatureCross.call (keras_rs/src/layers/feature_interaction/feature_cross.py:182-194):
//   keras Dense (matmul + bias + activation, :134-151) -> cast -> + diag_scale*x
//   -> x0 * u + x, which the reference runs as one GEMM and three separate
//   elementwise passes over [B, d].
//
// krs_gemm: C[M,N] = epilogue(A[M,K] . B[K,N]) for the three operand layouts
// the layer needs (forward, data gradient, weight gradient).  MFMA throughout:
// v_mfma_f32_32x32x16_bf16 (bf16) / v_mfma_f32_32x32x2_f32 (fp32, exact fmaf chain), fp32
// accumulators in registers, a lane's operand = 16 bytes of LDS.  Kernels, by shape:
//   * gemm_pp64_kernel      the big K-contiguous bf16 products -- h = x U, dh = dz K^T, the cross / residual / fused-backward
//                           forms -- whenever K is whole 64-k blocks: gemm_pp256_kernel's tile and ping-pong on 64-k pieces
//                           whose rows are whole 128-byte lines, five 32 KB slots, LDS-DMA issued among the MFMAs;
//   * gemm_pp256_kernel     the weight gradients (K-strided operands) and the K-contiguous shapes gemm_pp64_kernel does not
//                           take: the 256x256 tile (8 waves as 2(M) x 4(N), 128x64 per wave) on a four-stage LDS-DMA ring
//                           (global_load_lds, XOR swizzle on the source side), ping-pong wave groups, counted vmcnt, epilogue
//                           operands fetched under the tail of the main loop; bit-identical to the 128x128 two-stage kernels
//                           below, which every shape takes under pipeline 0 of krs_gemm_set_option;
//   * gemm_glds_kernel      two 32 KB stages filled by LDS-DMA on a 128x128 tile for smaller M / N (K >= 1024);
//   * gemm_tn_glds_kernel   bf16 weight gradients (both operands K-strided): tiles DMA'd as they lie in memory, fragments by
//                           the transposing ds_read_b64_tr_b16, split along K into fp32 slabs (one split per XCD at a time)
//                           that are reduced in a fixed order (deterministic, no atomics);
//   * gemm_mfma_kernel      every other aligned shape: global -> register -> LDS staging (K-strided operands transposed in
//                           registers), one 36 KB buffer, three workgroups per CU;
//   * gemm_thin_kernel      weight gradients with min(M, N) <= 16 (13 dense inputs, 1 unit);
//   * gemm_rowdot_kernel / gemm_smallk_kernel   N <= 8 / K <= 16 with a row-major A (the 1-unit and 13-input Dense layers);
//   * gemm_generic_kernel   anything else (the reference's toy shapes, d = 3).
// Epilogue on the accumulator, staged through LDS so that a lane owns 8 consecutive columns: + bias, activation, cross
// (x0*(v+diag*x)+x), + beta*R, one rounding to the output dtype; the cross / residual forms stream x0 / x / R / u / y with
// non-temporal accesses.  What bounds these products on MI355X is the L2 -> LDS operand path, not MFMA issue (DESIGN.md
// section 3, scripts/exp/gemm_probe.hip): hence the large tiles.
// (The epilogue's device functions live in gemm_device.h, shared with the int8 products of gemm_q8.hip.)
// Which kernel a call gets is decided in gemm_plan.h, a pure host function of the call (every threshold is named there,
// once); the host code at the end of this file validates, plans and launches what the plan names.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "gemm_device.h"
#include "gemm_plan.h"
#include "gemm_ring64.h"

namespace krs {
namespace {

constexpr int BM = gplan::kTile, BN = gplan::kTile;
constexpr int ROW_BYTES = gplan::kRowBytes;  // K extent of a tile row in bytes (64 bf16 / 32 fp32)
constexpr int TILE_BYTES = gplan::kTileBytes;  // one operand tile (BM == BN)

// ---- staging: HBM -> registers -> LDS (load_kcontig / store_kcontig / lds_chunk_off: gemm_device.h) ---------
// operand stored K-strided: elem(row, k) at base + (k*ld + row)*ES.  A thread
// takes a 4(k) x (16/ES)(row) block: four 16-byte loads along `row`.
template <int ES>
__device__ __forceinline__ void load_kstrided(const char* base, int64_t ld, int64_t row0, int64_t k0,
                                              int64_t rows, int64_t kk, u32x4 (&r)[4]) {
  constexpr int RPB = 16 / ES;          // rows per block: 8 (bf16) | 4 (fp32)
  constexpr int NRB = BM / RPB;         // row blocks per tile: 16 | 32
  const int t = threadIdx.x;
  const int rb = t % NRB;
  const int kb = t / NRB;
  const int64_t row = row0 + rb * RPB;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t kel = k0 + kb * 4 + i;
    u32x4 v = {0, 0, 0, 0};
    if (row < rows && kel < kk) v = *reinterpret_cast<const u32x4*>(base + (kel * ld + row) * ES);
    r[i] = v;
  }
}
template <int ES>
__device__ __forceinline__ void store_kstrided(char* tile, const u32x4 (&r)[4]) {
  constexpr int RPB = 16 / ES;
  constexpr int NRB = BM / RPB;
  const int t = threadIdx.x;
  const int rb = t % NRB;
  const int kb = t / NRB;
  if constexpr (ES == 4) {
    // 4x4 fp32 transpose is pure register renaming
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int j = jj;
      u32x4 o = {r[0][j], r[1][j], r[2][j], r[3][j]};
      *reinterpret_cast<u32x4*>(tile + lds_chunk_off<true>(rb * 4 + j, kb)) = o;
    }
  } else {
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
      const int j = jj;
      const int w = j >> 1;
      uint32_t lo, hi;
      if (j & 1) {
        lo = (r[0][w] >> 16) | (r[1][w] & 0xffff0000u);
        hi = (r[2][w] >> 16) | (r[3][w] & 0xffff0000u);
      } else {
        lo = (r[0][w] & 0xffffu) | (r[1][w] << 16);
        hi = (r[2][w] & 0xffffu) | (r[3][w] << 16);
      }
      *reinterpret_cast<uint2*>(tile + lds_chunk_off<true>(rb * 8 + j, kb >> 1) + (kb & 1) * 8) = make_uint2(lo, hi);
    }
  }
}

// Takes a chunk's operands as arrived at THIS point (empty statements that name the registers: hipcc waits here, once).
// hipcc cannot count an epilogue's stores -- each sits behind a branch over its lanes -- so a wait of its own for operands
// still in flight allows only the LOADS behind them to stay outstanding: consumed step by step that is vmcnt(6), (4), (2),
// (0), and every step waits for the acknowledgement of the stores before it.  One wait where the operands are due anyway
// leaves the steps behind it without any.  X0: the chunk holds x0 as well as x.
template <bool X0>
__device__ __forceinline__ void epi_settle(EpiOperands& o) {
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    asm volatile("" : "+v"(o.ex[it].x), "+v"(o.ex[it].y), "+v"(o.ex[it].z), "+v"(o.ex[it].w));
    if constexpr (X0) asm volatile("" : "+v"(o.ex0[it].x), "+v"(o.ex0[it].y), "+v"(o.ex0[it].z), "+v"(o.ex0[it].w));
  }
}

// gemm_epilogue_wave128 (gemm_device.h) with the operands of the first NPFC chunks already requested by the caller (under the tail of its
// main loop): 4 = all of them (residual form, cross form with x == x0: one operand), 2 = the first two (cross form: x0 and x)
// (PREBIAS: the bias values are in `pre_bias`, see epi_process; the builds that have them also settle their four chunks,
//  requested under the tail, before the first store)
template <int EPI, int NPFC, bool PREBIAS = false>
__device__ __forceinline__ void gemm_epilogue_wave128_pre(const GemmParams& p, f32x16 (&acc)[2][2][2], float* stage,
                                                          int64_t wm0, int64_t wn0, int split, EpiOperands (&o)[4],
                                                          const float* pre_bias = nullptr) {
  static_assert(NPFC == 2 || NPFC == 4, "two or four chunks of operands are fetched ahead");
  if constexpr (PREBIAS && NPFC == 4) {
#pragma unroll
    for (int c = 0; c < 4; ++c) epi_settle<EPI == 1>(o[c]);
  }
  epi_process<EPI, PREBIAS>(p, acc[0][0], o[0], stage, wm0, wn0, split, pre_bias);
  if constexpr (NPFC == 2) epi_prefetch<EPI>(p, o[2], wm0 + 64, wn0);
  epi_process<EPI, PREBIAS>(p, acc[0][1], o[1], stage, wm0 + 32, wn0, split, pre_bias);
  if constexpr (NPFC == 2) epi_prefetch<EPI>(p, o[3], wm0 + 96, wn0);
  epi_process<EPI, PREBIAS>(p, acc[1][0], o[2], stage, wm0 + 64, wn0, split, pre_bias);
  epi_process<EPI, PREBIAS>(p, acc[1][1], o[3], stage, wm0 + 96, wn0, split, pre_bias);
}

// ---- the cross epilogue of the 64-k ring with chunk 2 of x0 / x landed in the dead ring LDS (KRS_GEMM_SCHED_LDS_LANDING) --------
// gemm_epilogue_wave128_pre<1, 2> keeps two chunks of x0 / x in registers and asks for chunks 2 and 3 one epi_process before
// each is needed; the registers for a third chunk do not exist (232 VGPRs).  The LDS does: in the epilogue the ring is dead
// and only its first kEpiStageBytes stage accumulators.  So chunk 2 is requested at epilogue ENTRY by LDS-DMA into the
// wave's own kEpiLandWaveBytes behind the staging area (x: 4 instructions of 1 KB, then x0: 4), and chunk 3 goes into the
// registers chunk 0 frees, one chunk earlier than before.  Lanes land linearly, at the clamped addresses of epi_prefetch, so
// a lane reads back ITS 16 bytes (one ds_read_b128, no swizzle, no other wave involved): the values, and with them every
// bit of the result, are those of the register path.
// The DMA and its wait are assembly statements hipcc does not count: a DMA it CAN see makes it fence the next LDS access --
// the staging stores of chunk 0 -- with vmcnt(0) (the comment at lds_dma_retired), which would put the whole HBM latency in
// front of the epilogue.  The counted wait is ours: memory operations retire in order, and what is issued between the DMA and
// the wait cannot leave that span (both statements clobber memory): the eight loads of chunk 3 always, the stores of chunks
// 0 and 1 where the tile is whole (gemm_epilogue_wave128_land counts them).  A wait that allows no more than those has
// retired the DMA.  What hipcc waits for on its own account can only be stricter than it thinks (eight more operations are
// in flight than it counts) -- which is why no wait of its own may fall between the DMA and ours: chunks 0 and 1 are
// settled in front of the DMA, and the bias, which epi_process would load step by step, comes in registers.
// M0 (the DMA's LDS base) belongs to the compiler: saved and restored inside the statement that sets it.
__device__ __forceinline__ void epi_land_issue(const GemmParams& p, uint32_t land, int64_t row0, int64_t wn0) {
  const int lane = threadIdx.x & 63;
  const int64_t gnc = min(wn0 + (lane & 7) * 8, p.n - 8);
  const uint16_t* src[8];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int64_t gmc = min(row0 + it * 8 + (lane >> 3), p.m - 1);
    src[it] = reinterpret_cast<const uint16_t*>(p.ep.x) + gmc * p.ep.ldx + gnc;
    src[4 + it] = reinterpret_cast<const uint16_t*>(p.ep.x0) + gmc * p.ep.ldx + gnc;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(src[i]), "s"(land + i * 1024)
                 : "memory");
  }
}
// the landed chunk into a chunk's registers; behind epi_land_issue at least BEHIND memory operations have been issued
template <int BEHIND>
__device__ __forceinline__ void epi_land_read(const char* land, EpiOperands& o) {
  static_assert(BEHIND >= 8 && BEHIND < 64, "vmcnt is a 6-bit counter");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(BEHIND) : "memory");
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    o.ex[it] = *reinterpret_cast<const uint4*>(land + it * 1024 + lane * 16);
    o.ex0[it] = *reinterpret_cast<const uint4*>(land + 4096 + it * 1024 + lane * 16);
  }
}
// `o`: chunks 0 and 1 requested by the caller under the tail of its main loop; `land`: the wave's kEpiLandWaveBytes;
// `pre_bias`: epi_load_bias's values (a bias load inside epi_process, younger than the DMA, would wait for it at once)
__device__ __forceinline__ void gemm_epilogue_wave128_land(const GemmParams& p, f32x16 (&acc)[2][2][2], float* stage, char* land,
                                                           int64_t wm0, int64_t wn0, int split, EpiOperands (&o)[4],
                                                           const float* pre_bias) {
  const uint32_t land_lds = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)land);
  // Chunks 0 and 1 are taken as arrived HERE (they were requested most of two 64-k blocks ago): hipcc's wait for chunk 1 in
  // front of its epi_process would allow the operations hipcc counts behind it -- the stores of chunk 0, the loads of
  // chunk 3 -- and, not knowing of the DMA between, retire the DMA with chunk 1.
  epi_settle<true>(o[0]);
  epi_settle<true>(o[1]);
  epi_land_issue(p, land_lds, wm0 + 64, wn0);
  epi_process<1, true>(p, acc[0][0], o[0], stage, wm0, wn0, split, pre_bias);
  epi_prefetch<1>(p, o[0], wm0 + 96, wn0);      // chunk 3: eight loads, whatever the tile
  epi_process<1, true>(p, acc[0][1], o[1], stage, wm0 + 32, wn0, split, pre_bias);
  // Behind the DMA: the stores of chunks 0 and 1 and the loads of chunk 3.  Where the wave's first 64 rows and its 64 columns
  // lie inside C every lane stores -- four steps per chunk, y and (with u_out) u -- so that many operations are certain
  // and chunk 3 may stay in flight with them; on an edge of C only the eight loads are.  (Wave-uniform: scalar branches.)
  if (wm0 + 64 <= p.m && wn0 + 64 <= p.n) {
    if (p.ep.u_out) epi_land_read<8 + 16>(land, o[1]);
    else epi_land_read<8 + 8>(land, o[1]);
  } else {
    epi_land_read<8>(land, o[1]);
  }
  epi_process<1, true>(p, acc[1][0], o[1], stage, wm0 + 64, wn0, split, pre_bias);
  epi_settle<true>(o[0]);
  epi_process<1, true>(p, acc[1][1], o[0], stage, wm0 + 96, wn0, split, pre_bias);
}

// 128x128 workgroup tile, 4 waves as 2x2
template <int EPI>
__device__ __forceinline__ void gemm_epilogue(const GemmParams& p, f32x16 (&acc)[2][2], char* smem, int64_t m0,
                                              int64_t n0, int split) {
  const int wave = threadIdx.x >> 6;
  gemm_epilogue_wave<EPI>(p, acc, reinterpret_cast<float*>(smem) + wave * (32 * 68), m0 + (wave >> 1) * 64,
                          n0 + (wave & 1) * 64, split);
}

// EPI: 0 = general epilogue, 1 = cross (bf16, vector access), 2 = residual add (bf16, vector access).
// The specialised forms issue all their x0 / x / R loads for a 32-row half before the accumulators
// are staged, so the epilogue is one memory latency deep instead of one per row group.
template <int ES, bool A_KM, bool B_NK, int EPI>
__global__ __launch_bounds__(256, 3) void gemm_mfma_kernel(const GemmParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int BK = ROW_BYTES / ES;  // K elements per tile
  // ONE operand buffer (A tile, then B tile): 36 KB of LDS per workgroup, so three workgroups
  // share a CU and one's staging / epilogue phases hide under the others' MFMA phases.
  auto tile_a = [&](int) -> char* { return smem; };
  auto tile_b = [&](int) -> char* { return smem + TILE_BYTES; };

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  // XCD-aware tile order.  Workgroup ids are dealt round-robin to the 8 XCDs (observed: id % 8),
  // each with a private L2.  The N tiles of one M panel re-read the same A rows, so they are
  // mapped to ONE XCD, back to back: (xcd, slot) -> panel (slot / Nt) * 8 + xcd, tile slot % Nt.
  // A wrong placement guess only costs speed.  grid.x = ceil(Mt / 8) * 8 * Nt; surplus panels exit.
  const int64_t nt = (p.n + BN - 1) / BN;
  int64_t m_tile, n_tile;
  if constexpr (A_KM) {  // weight-gradient shapes: few tiles, split along K instead
    m_tile = blockIdx.x / nt;
    n_tile = blockIdx.x % nt;
  } else {
    const int64_t xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    m_tile = (slot / nt) * 8 + xcd;
    n_tile = slot % nt;
  }
  if (m_tile * BM >= p.m) return;
  const int64_t m0 = m_tile * BM;
  const int64_t n0 = n_tile * BN;
  const int split = blockIdx.z;
  const int64_t kbeg = (int64_t)split * p.k_per_split;
  const int64_t kend = min(p.k, kbeg + p.k_per_split);
  const int64_t ntiles = (kend - kbeg + BK - 1) / BK;

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

  u32x4 ra[4], rb[4];
  auto load_tiles = [&](int64_t t) {
    const int64_t k0 = kbeg + t * BK;
    if constexpr (A_KM) load_kstrided<ES>(p.a, p.lda, m0, k0, p.m, kend, ra);
    else load_kcontig<ES>(p.a, p.lda, m0, k0, p.m, kend, ra);
    if constexpr (B_NK) load_kcontig<ES>(p.b, p.ldb, n0, k0, p.n, kend, rb);
    else load_kstrided<ES>(p.b, p.ldb, n0, k0, p.n, kend, rb);
  };
  auto store_tiles = [&](int buf) {
    if constexpr (A_KM) store_kstrided<ES>(tile_a(buf), ra); else store_kcontig(tile_a(buf), ra);
    if constexpr (B_NK) store_kcontig(tile_b(buf), rb); else store_kstrided<ES>(tile_b(buf), rb);
  };

  if (ntiles > 0) load_tiles(0);

  const int frow = lane & 31;          // fragment row (m for A, n for B)
  const int fhalf = lane >> 5;         // which 16-byte half of a 32-byte K step this lane feeds
  for (int64_t t = 0; t < ntiles; ++t) {
    const int cur = 0;
    __syncthreads();          // every wave is done reading the previous tile
    store_tiles(0);
    __syncthreads();
    if (t + 1 < ntiles) load_tiles(t + 1);  // in flight under the MFMAs below
    const char* ta = tile_a(cur);
    const char* tb = tile_b(cur);
#pragma unroll
    for (int ks = 0; ks < ROW_BYTES / 32; ++ks) {  // 32 bytes of K per step (2 lane halves x 16 B)
      u32x4 fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        fa[i] = *reinterpret_cast<const u32x4*>(ta + lds_chunk_off<A_KM>(wm * 64 + i * 32 + frow, ks * 2 + fhalf));
        fb[i] = *reinterpret_cast<const u32x4*>(tb + lds_chunk_off<!B_NK>(wn * 64 + i * 32 + frow, ks * 2 + fhalf));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if constexpr (ES == 2) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                __builtin_bit_cast(bf16x8, fa[i]), __builtin_bit_cast(bf16x8, fb[j]), acc[i][j], 0, 0, 0);
          } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(fa[i][q]),
                                                               __uint_as_float(fb[j][q]), acc[i][j], 0, 0, 0);
          }
        }
    }
  }
  __syncthreads();  // operand tiles are dead from here on

  gemm_epilogue<EPI>(p, acc, smem, m0, n0, split);
}

// Forward / data-gradient shapes (both operands K-contiguous, K a multiple of the 64-element tile):
// the operand tiles are written straight into LDS by the memory pipeline
// (global_load_lds_dwordx4: no staging registers, no ds_write traffic), two stages deep:
//   issue tile t+1 -> MFMA on tile t -> vmcnt(0) + one barrier.
// An LDS-DMA instruction writes 64 lanes x 16 B = 1 KB contiguous (8 tile rows of 128 B), so the
// tile cannot be padded; the conflict-free read layout is produced on the SOURCE side instead:
// lane (row r, physical chunk pc) fetches the logical chunk pc ^ ((r >> 1) & 7), and fragment
// reads apply the same XOR (scripts/lds_conflicts.py: 4 cycles per ds_read_b128, the minimum).
// Rows beyond M / N are clamped (their results are never stored).
template <int ES, int EPI>
__global__ __launch_bounds__(256, 2) void gemm_glds_kernel(const GemmParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int BK = ROW_BYTES / ES;
  constexpr int OP_BYTES = BM * ROW_BYTES;   // 16 KB per operand tile
  constexpr int STAGE_BYTES = 2 * OP_BYTES;  // A then B
  typedef const __attribute__((address_space(1))) void* gptr;
  typedef __attribute__((address_space(3))) void* lptr;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int64_t nt = (p.n + BN - 1) / BN;
  const int64_t xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int64_t m_tile = (slot / nt) * 8 + xcd;
  if (m_tile * BM >= p.m) return;
  const int64_t m0 = m_tile * BM;
  const int64_t n0 = (slot % nt) * BN;
  const int64_t ntiles = p.k / BK;

  // per-lane source rows / chunks of the 4 DMA pieces this wave issues per operand and tile
  const char* asrc[4];
  const char* bsrc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = (wave * 4 + i) * 8 + (lane >> 3);            // tile row this lane fills
    const int c = (lane & 7) ^ ((r >> 1) & 7);                  // logical 16-byte chunk it must fetch
    const int64_t ar = min(m0 + r, p.m - 1);
    const int64_t br = min(n0 + r, p.n - 1);
    asrc[i] = p.a + (ar * p.lda) * ES + c * 16;
    bsrc[i] = p.b + (br * p.ldb) * ES + c * 16;
  }
  auto issue = [&](int64_t t, int stage) {
    char* sa = smem + stage * STAGE_BYTES + (wave * 4) * 1024;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      __builtin_amdgcn_global_load_lds((gptr)(asrc[i] + t * ROW_BYTES), (lptr)(sa + i * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((gptr)(bsrc[i] + t * ROW_BYTES), (lptr)(sa + OP_BYTES + i * 1024), 16, 0, 0);
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

  if (ntiles > 0) issue(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const int frow = lane & 31;
  const int fhalf = lane >> 5;
  // fragment row offsets (bytes) and swizzle keys are loop invariant
  int aoff[2], boff[2], akey[2], bkey[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int ra = wm * 64 + i * 32 + frow, rb = wn * 64 + i * 32 + frow;
    aoff[i] = ra * ROW_BYTES; akey[i] = (ra >> 1) & 7;
    boff[i] = OP_BYTES + rb * ROW_BYTES; bkey[i] = (rb >> 1) & 7;
  }
  for (int64_t t = 0; t < ntiles; ++t) {
    const int cur = (int)(t & 1);
    if (t + 1 < ntiles) issue(t + 1, cur ^ 1);
    const char* st = smem + cur * STAGE_BYTES;
#pragma unroll
    for (int ks = 0; ks < ROW_BYTES / 32; ++ks) {
      const int c = ks * 2 + fhalf;
      u32x4 fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        fa[i] = *reinterpret_cast<const u32x4*>(st + aoff[i] + ((c ^ akey[i]) << 4));
        fb[i] = *reinterpret_cast<const u32x4*>(st + boff[i] + ((c ^ bkey[i]) << 4));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if constexpr (ES == 2) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                __builtin_bit_cast(bf16x8, fa[i]), __builtin_bit_cast(bf16x8, fb[j]), acc[i][j], 0, 0, 0);
          } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(fa[i][q]),
                                                               __uint_as_float(fb[j][q]), acc[i][j], 0, 0, 0);
          }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // tile t+1 has landed
    __syncthreads();                                   // and every wave is done with tile t
  }
  lds_dma_retired<0>();
  gemm_epilogue<EPI>(p, acc, smem, m0, n0, 0);
}

// Weight-gradient shapes in bf16 (C = A^T B with BOTH operands K-strided in HBM: activations
// contracted over the batch).  The operand tiles go to LDS by DMA exactly as they lie in memory --
// rows of K, 16-byte chunks of 8 columns -- and the MFMA fragments (8 consecutive K per lane) are
// read with gfx950's transposing ds_read_b64_tr_b16: no staging registers, no in-register
// transposes, no ds_write traffic (the register-staged path spends half its LDS cycles on the
// bank conflicts of its transposed writes).
// LDS image of one operand tile (64 k x 128 columns): 16 blocks of 1 KB, block kb = 4 k-rows;
// inside a block the 64-byte unit (cq, kr) (32-column quarter cq, k-row kr) sits at (cq*4 + kr)*64,
// which is the lane-linear order of one DMA instruction whose lanes 4u..4u+3 fetch the 64
// contiguous bytes of unit u (so the memory side still sees whole 64-byte quads).
// A transposing read hands lane i of a 16-lane group column i of the 4 x 16 matrix whose row r is
// the 4 x 8 bytes addressed by lanes 4r..4r+3: a 32-lane half addresses the four k-rows of one
// 32-column quarter, i.e. 256 contiguous bytes -- every bank once.  Two reads (blocks kb, kb+1)
// give a lane its 8 k-values.
template <int EPI>
__global__ __launch_bounds__(256, 2) void gemm_tn_glds_kernel(const GemmParams p, int mt, int nt) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int BK = 64;
  constexpr int OP_BYTES = BK * 128 * 2;     // 16 KB
  constexpr int STAGE_BYTES = 2 * OP_BYTES;
  typedef const __attribute__((address_space(1))) void* gptr;
  typedef __attribute__((address_space(3))) void* lptr;
  typedef short s16x4 __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(3))) s16x4* trptr;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  // One K split = one XCD at a time (workgroup id % 8 picks the XCD): all mt*nt tiles of a split walk
  // the same K rows together, so a row of A / B is consumed whole (by the tiles side by side) while
  // its DRAM page and TLB entry are hot, and the operand tiles are shared through that XCD's L2.
  const int64_t tiles = (int64_t)mt * nt;
  const int64_t xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int split = (int)((slot / tiles) * 8 + xcd);
  if (split >= p.splits) return;
  const int64_t tile = slot % tiles;
  const int64_t m0 = (tile % mt) * BM;
  const int64_t n0 = (tile / mt) * BN;
  const int64_t kbeg = (int64_t)split * p.k_per_split;
  const int64_t kend = min(p.k, kbeg + p.k_per_split);
  const int64_t ntiles = (kend - kbeg) / BK;   // K extents are multiples of 64 (checked on the host)

  // DMA: this wave fills blocks kb = wave*4 + j of each operand; lane = (quarter*4 + k-row)*4 + chunk
  const int dkr = (lane >> 2) & 3, dcol = (lane >> 4) * 32 + (lane & 3) * 8;
  const int64_t acol = min(m0 + dcol, p.m - 8);   // clamped: surplus columns are never stored
  const int64_t bcol = min(n0 + dcol, p.n - 8);
  const char* asrc = p.a + ((kbeg + wave * 16 + dkr) * p.lda + acol) * 2;
  const char* bsrc = p.b + ((kbeg + wave * 16 + dkr) * p.ldb + bcol) * 2;
  const int64_t astep = p.lda * 8, bstep = p.ldb * 8;   // 4 k-rows, in bytes
  auto issue = [&](int64_t t, int stage) {
    char* sa = smem + stage * STAGE_BYTES + (wave * 4) * 1024;
    const char* at = asrc + t * BK * p.lda * 2;
    const char* bt = bsrc + t * BK * p.ldb * 2;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      __builtin_amdgcn_global_load_lds((gptr)(at + j * astep), (lptr)(sa + j * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((gptr)(bt + j * bstep), (lptr)(sa + OP_BYTES + j * 1024), 16, 0, 0);
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

  if (ntiles > 0) issue(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // transposing-read addresses: group g = lane >> 4 (columns (g & 1) * 16 .., k half g >> 1),
  // lane-in-group ii: k-row ii >> 2, 4-column quad ii & 3
  const int g = lane >> 4, ii = lane & 15;
  const int lane_off = (ii >> 2) * 64 + (g & 1) * 32 + (ii & 3) * 8 + (g >> 1) * 2048;
  int aoff[2], boff[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {  // a fragment's 32 columns are one quarter of the tile
    aoff[i] = (wm * 2 + i) * 256 + lane_off;
    boff[i] = OP_BYTES + (wn * 2 + i) * 256 + lane_off;
  }
  for (int64_t t = 0; t < ntiles; ++t) {
    const int cur = (int)(t & 1);
    if (t + 1 < ntiles) issue(t + 1, cur ^ 1);
    char* st = smem + cur * STAGE_BYTES;
#pragma unroll
    for (int ks = 0; ks < BK / 16; ++ks) {
      u32x4 fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const s16x4 a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((trptr)(st + aoff[i] + ks * 4096));
        const s16x4 a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((trptr)(st + aoff[i] + ks * 4096 + 1024));
        const s16x4 b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((trptr)(st + boff[i] + ks * 4096));
        const s16x4 b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((trptr)(st + boff[i] + ks * 4096 + 1024));
        const uint2 ua0 = __builtin_bit_cast(uint2, a0), ua1 = __builtin_bit_cast(uint2, a1);
        const uint2 ub0 = __builtin_bit_cast(uint2, b0), ub1 = __builtin_bit_cast(uint2, b1);
        fa[i] = u32x4{ua0.x, ua0.y, ua1.x, ua1.y};
        fb[i] = u32x4{ub0.x, ub0.y, ub1.x, ub1.y};
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[i]),
                                                              __builtin_bit_cast(bf16x8, fb[j]), acc[i][j], 0, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // tile t+1 has landed
    __syncthreads();                                   // and every wave is done with tile t
  }
  lds_dma_retired<0>();
  gemm_epilogue<EPI>(p, acc, smem, m0, n0, split);
}

// ---- fused epilogue of krs_gemm_cross_bwd (round 4) ----------------------------------------------------------------
// The data-gradient product of a cross layer, G = A B^T + beta R, is dL/dy of the layer BELOW it in a stack on one x0,
// whose elementwise backward (cross_bwd_vec_kernel) starts by re-reading G.  This epilogue does that pass on the tile
// while it is in registers: G is rounded and stored (the layer below needs it again as the residual of ITS data-gradient
// product), then from the ROUNDED value -- what the separate pass would have read --
//   dz = G x0 act'(u),   dx0 = [dx0 +] G u,   column sums of dz -> partial[group][n]  (bias gradient, fixed order)
// with the arithmetic of cross_bwd_vec_kernel for diag_scale = 0: G, dz and dx0 are bit-identical to the two calls.
// A wave's 128 x 64 block in four chunks of 32 rows; a chunk's R / x0 / u / dx0 vectors are requested before its
// accumulators are staged.  ACC: dx0 already holds the terms of the layers above (a template parameter: a load behind
// a run-time branch makes hipcc drain the load queue).
// DX0: where the running dL/dx0 comes from -- 0: nothing yet, 1: the dx0 buffer (terms of the layers above), 2: R * u_upper,
// the term of the layer ABOVE computed here from its dL/dy (= R, already loaded) and its saved u, so that the top layer of a
// stack neither writes nor this launch reads a [M, N] matrix for it (that one sum is rounded once instead of twice);
// 3: no dL/dx0 at all from this launch (the caller hands u to the NEXT launch as its u_upper: a Dense layer above a stack).
// X0 = false: the DENSE form (krs_gemm_dense_bwd, round 6) -- the layer below is a Dense layer, dz = G act'(y)
// with y in the place of u, no x0 stream, no dL/dx0.  STORE_G: G is stored as well (the caller passed g_out: autograd hands
// G, the true dL/dy, to whoever observes that output); without it two streams (y in, dz out) instead of krs_dense_act_bwd's
// three behind a stored and re-read G.
template <int DX0, bool HAS_R, bool X0 = true, bool STORE_G = true>
__device__ __forceinline__ void gemm_epilogue_wave128_crossbwd(const GemmParams& p, f32x16 (&acc)[2][2][2], float* stage,
                                                               int64_t wm0, int64_t wn0, int64_t group) {
  static_assert(X0 || (DX0 == 3 && !HAS_R), "the dense form has no R and no dL/dx0");
  static_assert(!X0 || STORE_G, "the cross forms always store G");
  const int lane = threadIdx.x & 63;
  const int frow = lane & 31, fhalf = lane >> 5;
  constexpr int SST = 68;
  const int ec = (lane & 7) * 8;
  const int64_t gn = wn0 + ec;
  const int64_t gnc = min(gn, p.n - 8);
  float db[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) db[q] = 0.0f;
  // operand vectors of a chunk, two sets: chunk c + 1's are requested while chunk c is processed -- x0 and u as soon as
  // chunk c's accumulators are staged (their registers are free from then on), R and the dL/dx0 source too from the second
  // chunk on.  (Requesting them earlier -- right behind the staging of chunk c's accumulators -- measured equal,
  // profiles/r4y_cross_bwd_fused_prefetch.txt: every stream of chunk c + 1 is requested behind chunk c's stores.)
  uint4 vr2[2][4], vx02[2][4], vu2[2][4], vd2[2][4];
  auto ld_x0u = [&](int c, int b) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int64_t gmc = min(wm0 + c * 32 + it * 8 + (lane >> 3), p.m - 1);
      if constexpr (X0) vx02[b][it] = load8_bf16_nt(p.f_x0, gmc * p.f_ld + gnc);
      vu2[b][it] = load8_bf16_nt(p.f_u, gmc * p.f_ld + gnc);
    }
  };
  auto ld_rd = [&](int c, int b) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int64_t gmc = min(wm0 + c * 32 + it * 8 + (lane >> 3), p.m - 1);
      if constexpr (HAS_R) vr2[b][it] = load8_bf16_nt(p.ep.r, gmc * p.ep.ldr + gnc);
      if constexpr (DX0 == 1) vd2[b][it] = load8_bf16_nt(p.f_dx0, gmc * p.f_ld + gnc);
      else if constexpr (DX0 == 2) vd2[b][it] = load8_bf16_nt(p.f_uup, gmc * p.f_ld + gnc);
    }
  };
  ld_x0u(0, 0);
  ld_rd(0, 0);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int64_t row0 = wm0 + c * 32;
    uint4(&er)[4] = vr2[c & 1];
    uint4(&ex0)[4] = vx02[c & 1];
    uint4(&eu)[4] = vu2[c & 1];
    uint4(&ed)[4] = vd2[c & 1];
    f32x16(&acc2)[2] = acc[c >> 1][c & 1];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        stage[((r & 3) + 8 * (r >> 2) + 4 * fhalf) * SST + j * 32 + frow] = acc2[j][r];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int er_ = it * 8 + (lane >> 3);
      const int64_t gm = row0 + er_;
      if (gm >= p.m || gn >= p.n) continue;
      float v[8], rv[8], x0v[8], uv[8], tv[8], g[8], dz[8];
      const float4 v0 = *reinterpret_cast<const float4*>(stage + er_ * SST + ec);
      const float4 v1 = *reinterpret_cast<const float4*>(stage + er_ * SST + ec + 4);
      v[0] = v0.x; v[1] = v0.y; v[2] = v0.z; v[3] = v0.w; v[4] = v1.x; v[5] = v1.y; v[6] = v1.z; v[7] = v1.w;
      if constexpr (HAS_R) {
        unpack_bf16x8(er[it], rv);
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] += p.ep.beta * rv[q];
      }
      // G as it is stored (one rounding) is what everything below sees
      const uint4 gq = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]),
                                  pack_bf16x2(v[6], v[7]));
      if constexpr (STORE_G) {
        const u32x4 gs = {gq.x, gq.y, gq.z, gq.w};
        __builtin_nontemporal_store(gs, reinterpret_cast<u32x4*>(reinterpret_cast<uint16_t*>(p.c) + gm * p.ldc + gn));
      }
      unpack_bf16x8(gq, g);
      if constexpr (X0) unpack_bf16x8(ex0[it], x0v);
      unpack_bf16x8(eu[it], uv);
      if constexpr (DX0 == 1 || DX0 == 2) unpack_bf16x8(ed[it], tv);
      else {
#pragma unroll
        for (int q = 0; q < 8; ++q) tv[q] = 0.0f;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const float gx0 = X0 ? g[q] * x0v[q] : g[q];
        dz[q] = gx0 * act_grad_from_output(p.f_act, uv[q]);
        db[q] += dz[q];
        const float told = DX0 == 1 ? tv[q] : (DX0 == 2 ? rv[q] * tv[q] : 0.0f);
        tv[q] = __builtin_fmaf(g[q], uv[q], told);
        if (p.f_fold) tv[q] += g[q];     // the layer below is the bottom of its stack (x is x0): the direct term too
      }
      store8_bf16_nt(p.f_dz, gm * p.f_ld + gn, dz);   // (nt like the other streams: 657-660 us against 664-667 with a plain store;
                                                       //  the dh / dK products that read dz next measure the same either way)
      if constexpr (DX0 != 3) store8_bf16_nt(p.f_dx0, gm * p.f_ld + gn, tv);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (c < 3) {
      ld_x0u(c + 1, (c + 1) & 1);
      ld_rd(c + 1, (c + 1) & 1);
    }
  }
  if (p.f_partial) {
    // column sums over the wave's 128 rows: the eight lanes with one (lane & 7) hold the same 8 columns
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      float t = db[q];
      t += __shfl_xor(t, 8);
      t += __shfl_xor(t, 16);
      t += __shfl_xor(t, 32);
      db[q] = t;
    }
    if ((lane >> 3) == 0 && gn < p.n) {
      float* dst = p.f_partial + group * p.n + gn;
      *reinterpret_cast<float4*>(dst) = make_float4(db[0], db[1], db[2], db[3]);
      *reinterpret_cast<float4*>(dst + 4) = make_float4(db[4], db[5], db[6], db[7]);
    }
  }
}

// ---- ping-pong ring pipeline: the 256x256 bf16 tile of both operand layouts -------------------------
// The two kernels above run "issue tile t+1 -> 32 MFMA on tile t -> vmcnt(0) -> barrier": the DMA queue is
// filled in one burst and drained to empty once per tile, all eight waves read LDS at the same time and
// feed the matrix pipes at the same time (profiles/r1j_gemm_pmc.md: waves parked 44-53 % of their cycles).
// This kernel keeps the tile, the LDS images and the epilogue and replaces the loop:
//   * K advances in blocks of 32; a block is two 16 KB PIECES (A: 256 rows x 64 B, B likewise; for the
//     K-strided layout 32 k-rows x 256 columns), 2 LDS-DMA instructions per thread each; the pieces live in
//     a ring of NSTG stages (4 = 128 KB, 5 = all 160 KB of the CU);
//   * a block is consumed in two PHASES of 16 k (6 ds_read_b128 / 12 transposing reads + 8 MFMA per wave),
//     each phase = a LOAD segment (fragment reads of this phase) and a COMPUTE segment (the 8 MFMA with the
//     phase's ONE piece of DMA issue -- two instructions per wave -- behind its 2nd and 5th MFMA, round 6),
//     every segment closed by s_barrier;
//   * waves 0-3 (rows 0..127 of the tile: one wave per SIMD) and waves 4-7 (rows 128..255: the other wave
//     of every SIMD) run one segment apart -- waves 4-7 pass one extra barrier first -- so on every SIMD
//     one wave computes while its partner reads LDS and issues DMA;
//   * nothing is ever drained: pieces A(j), B(j) are issued in phases 2(j-NSTG)+3 / +4 (a slot is refilled
//     two phases after the last read of its previous content: that read was retired by the reader's
//     lgkmcnt(0) one barrier earlier), and the only wait is a COUNTED vmcnt at the end of every odd phase
//     2kb+1, which retires the two pieces of block kb+1 and leaves the younger pieces in flight (that phase's
//     own piece is issued behind the wait, in its compute segment: 2*NSTG-6 pieces = STEADY - 2 instructions).
//     A wave's vmcnt covers its own DMA writes; the barrier that follows publishes them.
// Results are bit-identical to the two-stage kernels (same MFMA chain per accumulator: k ascending).
// Measured and not kept (profiles/archive/r2_gemm_ab.txt): 128-byte rows with a row-wise walk of the wave's block (the
// "half-tile" ring of the 8-phase template: 205 us against 207 for h = x U, 342 against 338 for dx -- round 6's
// gemm_pp64_kernel is that idea on 64-k pieces with the DMA among the MFMAs: 189 us); in ROUND 2 issuing the
// phase's DMA between the MFMAs of the compute segment instead of beside the fragment reads measured worse (212 / 319 us
// against 205 / 274 for the K-contiguous / K-strided forms of that day's kernel) -- re-measured in round 6 on today's
// kernels it is the better place (215 -> 212 us here, 195 -> 189 in gemm_pp64_kernel:
// profiles/r6_gemm_k64_dma_in_compute_ab.txt); five stages instead of four (equal); for the short-K
// products with heavy epilogues, 256 x 128 tiles on a three-stage ring at TWO workgroups per CU, so that one's
// epilogue runs under the other's main loop (467 / 344 us against 450 / 323: 1.5x the operand bytes per flop cost
// more than the overlap returns).
// (Rounds 2-4 carried timing-only build switches in this kernel -- KRS_PP_PROBE: DMA stream alone / LDS reads + MFMA alone /
//  epilogue alone; KRS_PP_LAYOUT_EXP: operands read as if pre-tiled; KRS_PP_{A,B}_AUX: cache policy of the LDS-DMA loads -- and
//  two more schedules behind krs_gemm_set_option: a five-stage ring and a prefetch schedule.  What they measured is in
//  profiles/archive/r2_pp_probe_dma_lds_mfma.txt, r4_gemm_layout_waves_clock_probe.txt, r2_gemm_ab.txt; round 5 removed them from
//  the product source: the default cache policy, four stages and the ping-pong schedule are what ships.)
namespace pp {
constexpr int PIECE = 16384;
constexpr int STAGE = 2 * PIECE;
}  // namespace pp

// Transposing LDS read as opaque assembly: hipcc treats the intrinsic as a read of memory an LDS-DMA may have
// written and puts `s_waitcnt vmcnt(0)` in front of every group of them -- which drained the ring's DMA queue
// once per phase in the K-strided form.  The caller orders these reads against the DMA itself (counted vmcnt +
// barrier) and waits for them with pp_lgkm_wait().
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
template <int OFF>
__device__ __forceinline__ u32x2 pp_read_tr16(uint32_t addr) {
  u32x2 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
  return v;
}
// s_waitcnt lgkmcnt(N) that the fragments' consumers depend on (the registers pass through the statement)
template <int N>
__device__ __forceinline__ void pp_lgkm_wait(u32x4 (&fa)[4], u32x4 (&fb)[2]) {
  asm volatile("s_waitcnt lgkmcnt(%6)"
               : "+v"(fa[0]), "+v"(fa[1]), "+v"(fa[2]), "+v"(fa[3]), "+v"(fb[0]), "+v"(fb[1])
               : "n"(N));
}

// ---- what the two ring kernels (gemm_pp256_kernel, gemm_pp64_kernel) share besides the tile ---------------------------------
// A wave's 128 x 64 block of C is acc[upper / lower 64 rows][m fragment][n fragment].  One MFMA of a main loop: 32-row chunk
// i (0..3) of the wave's rows, 32-column half j, a lane's 16 bytes = 8 k of each operand.
struct RingMmaBf16 {
  f32x16 (&acc)[2][2][2];
  __device__ __forceinline__ void operator()(int i, int j, const u32x4& fa, const u32x4& fb) const {
    f32x16& d = acc[i >> 1][i & 1][j];
    d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa), __builtin_bit_cast(bf16x8, fb), d, 0, 0, 0);
  }
};
// epilogue operands fetched under the tail of the main loop: 32-row chunks (residual form: all four of R; cross form: x0 and x
// of the first two), and how many load instructions that is
// (the cross form with x == x0 loads one operand: all four chunks fit the registers the cross form spends on two)
template <int EPI> constexpr int kRingEpiChunks = EPI == 2 || EPI == kEpiCrossXIsX0 ? 4 : EPI == 1 ? 2 : 0;
template <int EPI> constexpr int kRingEpiLoads = kRingEpiChunks<EPI> * (EPI == 1 ? 8 : 4);
// (The accumulator zeroing and the epilogue dispatch stay written out in both kernels: as shared functions, forced inline or
//  not, they made hipcc reschedule every build of gemm_pp256_kernel -- docs/measurement_log.md, "One ring main loop".)

// (Round 4 also built the 128x128 tile on a deep ring -- gemm_ring128_kernel, KRS_GEMM_OPT_PIPELINE = 7 -- for the per-rank
//  shapes of a strongly-scaled job; it measured equal or slower than gemm_glds_kernel (47.2 against 44.9 us at M = 8192,
//  profiles/archive/r4_gemm_ring128_b8192.txt: one 128x128 tile per CU already draws the ~40 GB/s per CU of the L2 -> LDS path) and
//  was deleted in round 5.)
// The steady state's LDS-DMA instructions are issued INSIDE the compute segment, behind its 2nd and 5th MFMA, not in the load
// segment (round 6: the load segment -- six fragment reads + two DMA instructions at 60-185 cycles each -- was the longer
// of the two and set the phase length; weight gradients 215 -> 212 us, profiles/r6_gemm_k64_dma_in_compute_ab.txt)
template <bool TN, int NSTG, int EPI>
__global__ __launch_bounds__(512) void gemm_pp256_kernel(const GemmParams p, int mt, int nt) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TM = 256, TN_ = 256;
  typedef const __attribute__((address_space(1))) void* gptr;
  typedef __attribute__((address_space(3))) void* lptr;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int grp = wave >> 2;
  const int wm = grp, wn = wave & 3;
  const int64_t xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  int64_t m0, n0, kbeg = 0, nkb;
  int split = 0;
  if constexpr (TN) {
    // work items (split, tile), split-major, are dealt to the XCDs in contiguous runs of q = ceil(W / 8): the
    // tiles of one K split run side by side on one XCD (at most two splits meet on an XCD), so a k-row of
    // A / B is consumed whole while its DRAM page is open and the operand tiles are shared through that L2
    const int64_t tiles = (int64_t)mt * nt, items = tiles * p.splits, q = (items + 7) / 8;
    const int64_t w = xcd * q + slot;
    if (slot >= q || w >= items) return;
    split = (int)(w / tiles);
    const int64_t tile = w % tiles;
    m0 = (tile % mt) * TM;
    n0 = (tile / mt) * TN_;
    kbeg = (int64_t)split * p.k_per_split;
    nkb = (min(p.k, kbeg + p.k_per_split) - kbeg) / 32;
  } else {
    // the N tiles of one M panel run back to back on one XCD (workgroup id % 8) and share A in its L2.  With split-K
    // (outputs too small to fill the chip with 256x256 tiles: the per-rank products of a strongly-scaled job) the
    // splits of a tile are neighbours on that XCD too: slot = ((m group * nt) + n tile) * splits + split
    const int64_t tslot = slot / p.splits;
    split = (int)(slot - tslot * p.splits);
    const int64_t m_tile = (tslot / nt) * 8 + xcd;
    if (m_tile * TM >= p.m) return;
    m0 = m_tile * TM;
    n0 = (tslot % nt) * TN_;
    kbeg = (int64_t)split * p.k_per_split;
    nkb = (min(p.k, kbeg + p.k_per_split) - kbeg) / 32;
  }

  // DMA sources of this thread's two instructions per piece; `astep` / `bstep` = bytes per K block
  const char* ap[2];
  const char* bp[2];
  int64_t astep, bstep;
  if constexpr (!TN) {
    // instruction q = wave*2 + i fills rows q*16 .. q*16+15 (64 B each): lane = row*4 + physical chunk,
    // which holds the logical 16-byte chunk pc ^ ((row >> 2) & 3) (conflict-free ds_read_b128, see below)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = (wave * 2 + i) * 16 + (lane >> 2);
      const int c = (lane & 3) ^ ((r >> 2) & 3);
      ap[i] = p.a + (min(m0 + r, p.m - 1) * p.lda + kbeg) * 2 + c * 16;
      bp[i] = p.b + (min(n0 + r, p.n - 1) * p.ldb + kbeg) * 2 + c * 16;
    }
    astep = bstep = 64;
  } else {
    // instruction q fills the 1 KB block (128-column half q >> 3, k-rows (q & 7)*4 .. +3) with the image of
    // gemm_tn_glds_kernel: lane = (quarter*4 + k-row)*4 + chunk
    const int kr = (lane >> 2) & 3, col = (wave >> 2) * 128 + (lane >> 4) * 32 + (lane & 3) * 8;
    const int64_t acol = min(m0 + col, p.m - 8), bcol = min(n0 + col, p.n - 8);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int64_t krow = kbeg + ((wave & 3) * 2 + i) * 4 + kr;
      ap[i] = p.a + (krow * p.lda + acol) * 2;
      bp[i] = p.b + (krow * p.ldb + bcol) * 2;
    }
    astep = p.lda * 64;
    bstep = p.ldb * 64;
  }
  const int dma_off = wave * 2048;  // + i*1024: where instruction q = wave*2 + i lands inside a piece
  auto issue_a = [&](int stage) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      __builtin_amdgcn_global_load_lds((gptr)ap[i], (lptr)(smem + stage * pp::STAGE + dma_off + i * 1024), 16, 0, 0);
      ap[i] += astep;
    }
  };
  auto issue_b = [&](int stage) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      __builtin_amdgcn_global_load_lds((gptr)bp[i], (lptr)(smem + stage * pp::STAGE + pp::PIECE + dma_off + i * 1024), 16,
                                       0, 0);
      bp[i] += bstep;
    }
  };
  auto issue_one = [&](bool is_a, int stage, int i) {
    if (is_a) {
      __builtin_amdgcn_global_load_lds((gptr)ap[i], (lptr)(smem + stage * pp::STAGE + dma_off + i * 1024), 16, 0, 0);
      ap[i] += astep;
    } else {
      __builtin_amdgcn_global_load_lds((gptr)bp[i], (lptr)(smem + stage * pp::STAGE + pp::PIECE + dma_off + i * 1024), 16, 0, 0);
      bp[i] += bstep;
    }
  };

  // fragment addresses inside a stage (phase hk = 1: ^ 32 for the K-contiguous image, + 4096 for the other)
  int a_lane, b_lane;
  if constexpr (!TN) {
    // 64-byte rows: lane (frow, fhalf) wants chunk hk*2 + fhalf of row frow; a ds_read_b128 is served in
    // groups of 16 lanes whose rows are {0-3, 12-15, 20-27} / {4-11, 16-19, 28-31} (+32): with the chunk
    // XOR (row >> 2) & 3 every group covers the sixteen 16-byte slots of the 256-byte bank row once
    const int frow = lane & 31, fhalf = lane >> 5, key = (frow >> 2) & 3;
    a_lane = (wm * 128 + frow) * 64 + ((fhalf ^ key) << 4);
    b_lane = pp::PIECE + (wn * 64 + frow) * 64 + ((fhalf ^ key) << 4);
  } else {
    const int g = lane >> 4, ii = lane & 15;
    const int lane_off = (ii >> 2) * 64 + (g & 1) * 32 + (ii & 3) * 8 + (g >> 1) * 2048;
    a_lane = wm * 8192 + lane_off;
    b_lane = pp::PIECE + (wn >> 1) * 8192 + (wn & 1) * 512 + lane_off;
  }
  const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  auto load_frags = [&](int stage, int hk, u32x4(&fa)[4], u32x4(&fb)[2]) {
    const char* st = smem + stage * pp::STAGE;
    if constexpr (!TN) {
      const int x = hk * 32;
#pragma unroll
      for (int j = 0; j < 2; ++j) fb[j] = *reinterpret_cast<const u32x4*>(st + (b_lane ^ x) + j * 2048);
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[i] = *reinterpret_cast<const u32x4*>(st + (a_lane ^ x) + i * 2048);
    } else {
      const uint32_t sa = lds_base + stage * pp::STAGE + hk * 4096 + a_lane, sb = lds_base + stage * pp::STAGE + hk * 4096 + b_lane;
#define KRS_TR2(dst, base, off)                                                            \
  {                                                                                        \
    const u32x2 lo_ = pp_read_tr16<(off)>(base), hi_ = pp_read_tr16<(off) + 1024>(base);   \
    dst = u32x4{lo_.x, lo_.y, hi_.x, hi_.y};                                               \
  }
      KRS_TR2(fb[0], sb, 0)
      KRS_TR2(fb[1], sb, 256)
      KRS_TR2(fa[0], sa, 0)
      KRS_TR2(fa[1], sa, 256)
      KRS_TR2(fa[2], sa, 512)
      KRS_TR2(fa[3], sa, 768)
#undef KRS_TR2
    }
  };

  f32x16 acc[2][2][2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[h][i][j][r] = 0.0f;
  const RingMmaBf16 mma{acc};
  constexpr int NPFC = kRingEpiChunks<EPI>, NPF = kRingEpiLoads<EPI>;
  EpiOperands opf[4];
  auto mfma8 = [&](const u32x4(&fa)[4], const u32x4(&fb)[2]) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) mma(i, j, fa[i], fb[j]);
    __builtin_amdgcn_s_setprio(0);
  };
  auto mfma8_dma = [&](const u32x4(&fa)[4], const u32x4(&fb)[2], bool is_a, int stage) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        mma(i, j, fa[i], fb[j]);
        if (i * 2 + j == 1) { __builtin_amdgcn_sched_barrier(0); issue_one(is_a, stage, 0); __builtin_amdgcn_sched_barrier(0); }
        if (i * 2 + j == 4) { __builtin_amdgcn_sched_barrier(0); issue_one(is_a, stage, 1); __builtin_amdgcn_sched_barrier(0); }
      }
    __builtin_amdgcn_s_setprio(0);
  };

  {
    // prologue (the host guarantees nkb >= NSTG): A(0), B(0), ..., A(NSTG-3), B(NSTG-3), A(NSTG-2)
  #pragma unroll
    for (int j = 0; j < NSTG - 2; ++j) {
      issue_a(j);
      issue_b(j);
    }
    issue_a(NSTG - 2);
    constexpr int STEADY = 4 * NSTG - 10;  // DMA instructions of the 2*NSTG-5 pieces that may stay in flight
    pp_vmcnt<STEADY>();
    pp_barrier();
    if (grp == 1) pp_barrier();  // rows 128..255 run one segment behind rows 0..127

    int rd = 0, wa = NSTG - 1, wb = NSTG - 2;  // stages of block kb, of the A piece issued in its odd / the B piece in its even phase
    const int64_t last = nkb - 1;
    auto advance = [&]() {
      rd = rd + 1 == NSTG ? 0 : rd + 1;
      wa = wa + 1 == NSTG ? 0 : wa + 1;
      wb = wb + 1 == NSTG ? 0 : wb + 1;
    };
    int64_t kb = 0;
    for (; kb + NSTG - 1 <= last; ++kb) {  // steady state: one piece issued per phase
      u32x4 fa[4], fb[2];
      // ---- phase 2kb ----
      load_frags(rd, 0, fa, fb);
      pp_barrier();
      if constexpr (TN) pp_lgkm_wait<0>(fa, fb);
      mfma8_dma(fa, fb, false, wb);
      pp_barrier();
      // ---- phase 2kb+1 ----
      load_frags(rd, 1, fa, fb);
      pp_vmcnt<STEADY - 2>();    // (this phase's piece is issued behind the wait, among the MFMAs)
      pp_barrier();
      if constexpr (TN) pp_lgkm_wait<0>(fa, fb);
      mfma8_dma(fa, fb, true, wa);
      pp_barrier();
      advance();
    }
    // tail: the last NSTG-1 blocks; only B(last) is still to be issued.  The epilogue's operands (residual form:
    // all four 32-row chunks of R; cross form: x0 and x of the first two) are requested here, behind the last
    // piece, so that their HBM latency runs under the remaining 2*(NSTG-1) phases instead of in front of the
    // epilogue; they are younger than every piece, so the counted waits simply allow NPF more loads in flight.
#pragma unroll
    for (int t = 0; t < NSTG - 1; ++t) {
      u32x4 fa[4], fb[2];
      load_frags(rd, 0, fa, fb);
      if (t == 0) issue_b(wb);
      pp_barrier();
      if constexpr (TN) pp_lgkm_wait<0>(fa, fb);
      mfma8(fa, fb);
      pp_barrier();
      load_frags(rd, 1, fa, fb);
      if constexpr (NPFC > 0) {
        if (t == 0) {
#pragma unroll
          for (int c = 0; c < NPFC; ++c) epi_prefetch<EPI>(p, opf[c], m0 + wm * 128 + c * 32, n0 + wn * 64);
        }
      }
      // block kb+1 must have landed; behind it only the pieces of blocks kb+2 .. last (rem = NSTG-3-t of them)
      // and the epilogue operands are still in flight
      if (NSTG - 3 - t >= 2) pp_vmcnt<8 + NPF>();
      else if (NSTG - 3 - t == 1) pp_vmcnt<4 + NPF>();
      else if (NSTG - 3 - t == 0) pp_vmcnt<NPF>();
      pp_barrier();
      if constexpr (TN) pp_lgkm_wait<0>(fa, fb);
      mfma8(fa, fb);
      pp_barrier();
      advance();
    }
    if (grp == 0) pp_barrier();
  }
  lds_dma_retired<NPF>();
  float* stage_f = reinterpret_cast<float*>(smem) + wave * (32 * 68);
  if constexpr (EPI >= 3) {   // 3: + R, 4: + R, dx0 accumulates, 5: no R, 6: no R, dx0 accumulates, 7: + R, dx0 = R u_upper + ...,
                              // 8: no R, no dx0, 9: the dense form (no x0, no R, no dx0, G not stored), 10: the dense form, G stored
    gemm_epilogue_wave128_crossbwd<(EPI == 4 || EPI == 6) ? 1 : (EPI == 7 ? 2 : (EPI >= 8 ? 3 : 0)),
                                   EPI == 3 || EPI == 4 || EPI == 7, EPI < 9, EPI != 9>(
        p, acc, stage_f, m0 + wm * 128, n0 + wn * 64, (m0 >> 8) * 2 + wm);
    return;
  }
  if constexpr (NPFC > 0)
    gemm_epilogue_wave128_pre<EPI, NPFC>(p, acc, stage_f, m0 + wm * 128, n0 + wn * 64, split, opf);
  else
    gemm_epilogue_wave128<EPI>(p, acc, stage_f, m0 + wm * 128, n0 + wn * 64, split);
}

// ---- gemm_pp64_kernel: the ring on 64-k blocks with WHOLE 128-byte lines per LDS-DMA row (round 6) --------------------------
// gemm_pp256_kernel's tile, accumulators and epilogues on the main loop of gemm_ring64.h (the schedule and its derivation are
// there; gemm_q8.hip's gemm_q8_ring_kernel runs the same loop): a piece is 256 rows x 64 k, the epilogue's operands are
// requested at the loop's tail point.
// SCHED (KRS_GEMM_SCHED_* bits, the streaming epilogue builds only; 0 = the reference schedule):
//   LDS_LANDING  build 1: gemm_epilogue_wave128_land instead of gemm_epilogue_wave128_pre;
//   STAGGER      The reading it was built on: the 3584 equal tiles of a C3 product start together on 256 CUs and stay in step
//                for all 14 rounds, every CU streaming its epilogue while no CU needs HBM for a main loop.  Here odd M panels
//                start half way round their N tiles (gplan::ring_tile_of_slot) and, of the first round (one workgroup per
//                CU), every other workgroup of an XCD starts half a tile period late, so that the epilogues of half the
//                CUs fall on the main loops of the other half.  The period is an estimate (a 64-k block of the main loop
//                at 1.56 us, a 128 KB epilogue stream at 5.2 us: the C3 shapes' own timings); a wrong one costs phase, not
//                bits, and the wait is bounded by iterations as well as by the clock.
//                MEASURED NEGATIVE (profiles/gemm_epi_schedule_ab.txt): dx unchanged, the cross form 9 us slower alone and
//                8 - 17 us slower on top of LDS_LANDING / X_IS_X0 -- the half period is spent and not returned.  Not the
//                default; kept behind the switch so the reading can be repeated.
template <int EPI> constexpr int kRingEpiStreams = EPI == 1 ? 4 : EPI == kEpiCrossXIsX0 ? 3 : EPI == 2 ? 2 : 6;
template <int EPI, int SCHED>
__global__ __launch_bounds__(512) void gemm_pp64_kernel(const GemmParams p, int nt) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TM = 256, TN_ = 256;
  constexpr bool LAND = (SCHED & KRS_GEMM_SCHED_LDS_LANDING) != 0, STAGGER = (SCHED & KRS_GEMM_SCHED_STAGGER) != 0;
  static_assert(!LAND || EPI == 1, "only the cross build lands operands in LDS");
  static_assert(!STAGGER || EPI != 0, "the general build keeps the panel order");
  static_assert(gplan::kEpiStageBytes + gplan::kEpiLandBytes <= gplan::kRing64Lds, "the landing region lies inside the ring");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int64_t xcd = blockIdx.x & 7, slot_id = blockIdx.x >> 3;
  // (work-item order of gemm_pp256_kernel's K-contiguous form: the N tiles of an M panel, and the K splits of a tile, are
  //  neighbours on one XCD)
  const int64_t tslot = slot_id / p.splits;
  const int split = (int)(slot_id - tslot * p.splits);
  const int64_t m_tile = (tslot / nt) * 8 + xcd;
  if (m_tile * TM >= p.m) return;
  // (panel order written out as it always was -- the same numbers as ring_tile_of_slot(tslot, nt, false), which as a call
  //  made hipcc reallocate the registers of the general build)
  const int64_t m0 = m_tile * TM, n0 = (STAGGER ? gplan::ring_tile_of_slot(tslot, nt, true).n_tile : tslot % nt) * TN_;
  const int64_t kbeg = (int64_t)split * p.k_per_split;
  const int64_t nb = (min(p.k, kbeg + p.k_per_split) - kbeg) / 64;     // 64-k blocks (the host guarantees >= 3, whole)
  if constexpr (STAGGER) {
    if (blockIdx.x < gplan::kCUs && (slot_id & 1)) {
      const uint64_t half_period = (uint64_t)nb * 78 + kRingEpiStreams<EPI> * 260, t0 = wall_clock64();   // 10 ns ticks
      for (int i = 0; i < 256 && wall_clock64() - t0 < half_period; ++i) __builtin_amdgcn_s_sleep(16);
    }
  }

  f32x16 acc[2][2][2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[h][i][j][r] = 0.0f;
  constexpr int NPFC = kRingEpiChunks<EPI>;
  EpiOperands opf[4];
  // the builds of KRS_GEMM_OPT_EPI_SCHEDULE 1 request the lane's bias values with the epilogue operands, two more loads
  // under the tail, instead of loading them in every step of the epilogue (epi_process, PREBIAS)
  constexpr bool PREBIAS = LAND || EPI == kEpiCrossXIsX0;
  float pre_bias[8];
  ring64_main_loop<2, kRingEpiLoads<EPI> + (PREBIAS ? 2 : 0)>(smem, p, m0, n0, kbeg, nb, lane, wave, RingMmaBf16{acc}, [&]() {
    if constexpr (PREBIAS) epi_load_bias(p, n0 + wn * 64, pre_bias);
#pragma unroll
    for (int c = 0; c < NPFC; ++c) epi_prefetch<EPI>(p, opf[c], m0 + wm * 128 + c * 32, n0 + wn * 64);
  });
  float* stage_f = reinterpret_cast<float*>(smem) + wave * (32 * 68);
  if constexpr (EPI >= 3 && EPI <= 10) {
    gemm_epilogue_wave128_crossbwd<(EPI == 4 || EPI == 6) ? 1 : (EPI == 7 ? 2 : (EPI >= 8 ? 3 : 0)),
                                   EPI == 3 || EPI == 4 || EPI == 7, EPI < 9, EPI != 9>(
        p, acc, stage_f, m0 + wm * 128, n0 + wn * 64, (m0 >> 8) * 2 + wm);
    return;
  }
  if constexpr (LAND)
    gemm_epilogue_wave128_land(p, acc, stage_f, smem + gplan::kEpiStageBytes + wave * gplan::kEpiLandWaveBytes, m0 + wm * 128,
                               n0 + wn * 64, split, opf, pre_bias);
  else if constexpr (NPFC > 0)
    gemm_epilogue_wave128_pre<EPI, NPFC, PREBIAS>(p, acc, stage_f, m0 + wm * 128, n0 + wn * 64, split, opf, pre_bias);
  else
    gemm_epilogue_wave128<EPI>(p, acc, stage_f, m0 + wm * 128, n0 + wn * 64, split);
}

// Weight gradients with one tiny dimension (C = A^T B, both operands K-strided, min(M, N) <= 16, long K):
// the first Dense of the bottom MLP (13 dense features) and the last of the top MLP (1 unit).  The
// MFMA tiles do not apply and one thread per output would walk K = batch alone; here a thread owns
// one column of the WIDE operand (coalesced across the workgroup), the THIN operand's rows are
// staged in LDS and broadcast, K is split over blockIdx.y into fp32 slabs (fixed-order reduce).
// ES: operand element size (2 = bf16, 4 = fp32); NT: thin extent rounded up to 1 / 4 / 8 / 16 (the LDS rows are
// read as float4).  Eight rows of the wide operand are requested before they are consumed (the first version
// walked its 1024 rows one dependent load at a time behind a run-time dtype switch: 394 us for the 13 x 512 gradient).
template <int ES, int NT>
__global__ __launch_bounds__(256) void gemm_thin_kernel(const GemmParams p, int thin_is_a) {
  typedef typename std::conditional<ES == 2, uint16_t, float>::type elem_t;
  __shared__ __attribute__((aligned(16))) float thin[128][NT];
  const elem_t* wide_p = reinterpret_cast<const elem_t*>(thin_is_a ? p.b : p.a);
  const elem_t* thin_p = reinterpret_cast<const elem_t*>(thin_is_a ? p.a : p.b);
  const int64_t ldw = thin_is_a ? p.ldb : p.lda, ldt = thin_is_a ? p.lda : p.ldb;
  const int64_t n_wide = thin_is_a ? p.n : p.m;
  const int n_thin = (int)(thin_is_a ? p.m : p.n);
  const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t ccol = col < n_wide ? col : n_wide - 1;   // idle threads load a valid column and store nothing
  const int split = blockIdx.y;
  const int64_t kbeg = (int64_t)split * p.k_per_split;
  const int64_t kend = min(p.k, kbeg + p.k_per_split);
  auto cvt = [](elem_t v) -> float {
    if constexpr (ES == 2) return bf16_to_f32(v);
    else return v;
  };
  float acc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) acc[i] = 0.0f;
  for (int64_t k0 = kbeg; k0 < kend; k0 += 128) {
    const int rows = (int)min<int64_t>(128, kend - k0);
    __syncthreads();
    for (int e = threadIdx.x; e < 128 * NT; e += 256) {
      const int r = e / NT, i = e % NT;
      thin[r][i] = (r < rows && i < n_thin) ? cvt(thin_p[(k0 + r) * ldt + i]) : 0.0f;
    }
    __syncthreads();
    for (int r = 0; r < rows; r += 8) {
      elem_t wv[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) wv[q] = wide_p[min(k0 + r + q, kend - 1) * ldw + ccol];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const float w = r + q < rows ? cvt(wv[q]) : 0.0f;
        if constexpr (NT == 1) {
          acc[0] = fmaf(thin[r + q][0], w, acc[0]);
        } else {
#pragma unroll
          for (int i4 = 0; i4 < NT / 4; ++i4) {
            const float4 t = *reinterpret_cast<const float4*>(&thin[(r + q) & 127][i4 * 4]);
            acc[i4 * 4 + 0] = fmaf(t.x, w, acc[i4 * 4 + 0]);
            acc[i4 * 4 + 1] = fmaf(t.y, w, acc[i4 * 4 + 1]);
            acc[i4 * 4 + 2] = fmaf(t.z, w, acc[i4 * 4 + 2]);
            acc[i4 * 4 + 3] = fmaf(t.w, w, acc[i4 * 4 + 3]);
          }
        }
      }
    }
  }
  if (col >= n_wide) return;
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    if (i < n_thin) {
      const int64_t m = thin_is_a ? i : col, n = thin_is_a ? col : i;
      if (p.splits > 1) p.slabs[((int64_t)split * p.m + m) * p.n + n] = acc[i];
      else epilogue_store(p, m, n, acc[i]);
    }
  }
}

// Products with ONE tiny dimension on the output side or in the contraction, row-major A (the last Dense of the
// DLRM top MLP: 256 -> 1 unit, forward and data gradient; one thread per output element with 64-bit divisions
// took 235 us for either):
//   gemm_rowdot_kernel  N <= 8, any K: 16 lanes per row of A, each lane walks its 16-byte chunks of the row and
//                       keeps N partial dots; butterfly reduction; lane 0 stores through the epilogue
//   gemm_smallk_kernel  K <= 16, N a multiple of 8: a thread owns 8 consecutive outputs of one row
template <int ES>
__global__ __launch_bounds__(256) void gemm_rowdot_kernel(const GemmParams p) {
  typedef typename std::conditional<ES == 2, uint16_t, float>::type elem_t;
  constexpr int VE = 16 / ES;
  const int sub = threadIdx.x & 15;
  const int64_t row = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int64_t r = row < p.m ? row : p.m - 1;
  const elem_t* a = reinterpret_cast<const elem_t*>(p.a) + r * p.lda;
  const elem_t* b = reinterpret_cast<const elem_t*>(p.b);
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.0f;
  for (int64_t k0 = (int64_t)sub * VE; k0 < p.k; k0 += 16 * VE) {
    float av[VE];
    if (k0 + VE <= p.k && (reinterpret_cast<uintptr_t>(a + k0) & 15) == 0) {
      const uint4 raw = *reinterpret_cast<const uint4*>(a + k0);
      if constexpr (ES == 2) {
        const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) { av[2 * q] = __uint_as_float(w[q] << 16); av[2 * q + 1] = __uint_as_float(w[q] & 0xffff0000u); }
      } else {
        av[0] = __uint_as_float(raw.x); av[1] = __uint_as_float(raw.y); av[2] = __uint_as_float(raw.z); av[3] = __uint_as_float(raw.w);
      }
    } else {
#pragma unroll
      for (int q = 0; q < VE; ++q) {
        if constexpr (ES == 2) av[q] = k0 + q < p.k ? bf16_to_f32(a[k0 + q]) : 0.0f;
        else av[q] = k0 + q < p.k ? a[k0 + q] : 0.0f;
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j < p.n) {
#pragma unroll
        for (int q = 0; q < VE; ++q) {
          if (k0 + q < p.k) {
            const elem_t bv = p.b_nk ? b[(int64_t)j * p.ldb + k0 + q] : b[(k0 + q) * p.ldb + j];
            float bf;
            if constexpr (ES == 2) bf = bf16_to_f32(bv); else bf = bv;
            acc[j] = fmaf(av[q], bf, acc[j]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int o = 8; o; o >>= 1) acc[j] += __shfl_xor(acc[j], o, 64);
  if (sub == 0 && row < p.m)
    for (int j = 0; j < p.n; ++j) epilogue_store(p, row, j, acc[j]);
}

template <int ES>
__global__ __launch_bounds__(256) void gemm_smallk_kernel(const GemmParams p, int rows_per_wg) {
  typedef typename std::conditional<ES == 2, uint16_t, float>::type elem_t;
  extern __shared__ __attribute__((aligned(16))) float bs[];   // B as fp32 [K][N]: a thread reads its 8 columns as 2 x float4
  auto f = [](elem_t v) -> float {
    if constexpr (ES == 2) return bf16_to_f32(v);
    else return v;
  };
  const elem_t* b = reinterpret_cast<const elem_t*>(p.b);
  const int K = (int)p.k, N = (int)p.n;
  for (int e = threadIdx.x; e < K * N; e += 256) {
    const int kk = e / N, j = e - kk * N;
    bs[e] = f(p.b_nk ? b[(int64_t)j * p.ldb + kk] : b[(int64_t)kk * p.ldb + j]);
  }
  __syncthreads();
  const int n8 = N / 8;
  const int64_t row0 = (int64_t)blockIdx.x * rows_per_wg;
  const int64_t items = (int64_t)min<int64_t>(rows_per_wg, p.m - row0) * n8;
  for (int64_t it = threadIdx.x; it < items; it += 256) {
    const int64_t i = row0 + it / n8;
    const int j0 = (int)(it % n8) * 8;
    const elem_t* a = reinterpret_cast<const elem_t*>(p.a) + i * p.lda;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.0f;
    for (int kk = 0; kk < K; ++kk) {
      const float av = f(a[kk]);
      const float4 b0 = *reinterpret_cast<const float4*>(bs + kk * N + j0);
      const float4 b1 = *reinterpret_cast<const float4*>(bs + kk * N + j0 + 4);
      v[0] = fmaf(av, b0.x, v[0]); v[1] = fmaf(av, b0.y, v[1]); v[2] = fmaf(av, b0.z, v[2]); v[3] = fmaf(av, b0.w, v[3]);
      v[4] = fmaf(av, b1.x, v[4]); v[5] = fmaf(av, b1.y, v[5]); v[6] = fmaf(av, b1.z, v[6]); v[7] = fmaf(av, b1.w, v[7]);
    }
    if (p.ep_vec) {
      epilogue_store_vec8(p, i, j0, v);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) epilogue_store(p, i, j0 + j, v[j]);
    }
  }
}

// fixed-order reduction of the split-K slabs + epilogue
__global__ __launch_bounds__(256) void gemm_slab_reduce_kernel(const GemmParams p) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.m * p.n) return;
  float v = 0.0f;
  for (int s = 0; s < p.splits; ++s) v += p.slabs[(int64_t)s * p.m * p.n + idx];
  epilogue_store(p, idx / p.n, idx % p.n, v);
}
// the common weight-gradient case (fp32 C, no epilogue, N % 4 == 0): four columns per thread, same order
__global__ __launch_bounds__(256) void gemm_slab_reduce_vec4_kernel(const GemmParams p) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;   // group of 4 consecutive columns
  const int64_t nq = p.n / 4;
  if (q >= p.m * nq) return;
  const int64_t i = q / nq, j = (q - i * nq) * 4;
  float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  for (int s = 0; s < p.splits; ++s) {
    const float4 t = *reinterpret_cast<const float4*>(p.slabs + ((int64_t)s * p.m + i) * p.n + j);
    v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
  }
  *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.c) + i * p.ldc + j) = v;
}

// eight columns per thread + the vector epilogue (bf16 or fp32 output, bias / activation / cross / residual forms): the
// reduce of the K-contiguous split products (round 5), same slab order
__global__ __launch_bounds__(256) void gemm_slab_reduce_vec8_kernel(const GemmParams p) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;   // group of 8 consecutive columns
  const int64_t nq = p.n / 8;
  if (q >= p.m * nq) return;
  const int64_t i = q / nq, j = (q - i * nq) * 8;
  float v[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) v[c] = 0.0f;
  for (int s = 0; s < p.splits; ++s) {
    const float* src = p.slabs + ((int64_t)s * p.m + i) * p.n + j;
    const float4 t0 = *reinterpret_cast<const float4*>(src), t1 = *reinterpret_cast<const float4*>(src + 4);
    v[0] += t0.x; v[1] += t0.y; v[2] += t0.z; v[3] += t0.w; v[4] += t1.x; v[5] += t1.y; v[6] += t1.z; v[7] += t1.w;
  }
  epilogue_store_vec8(p, i, j, v);
}

// any shape / alignment: one thread per output element
__global__ __launch_bounds__(256) void gemm_generic_kernel(const GemmParams p, int in_dtype) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.m * p.n) return;
  const int64_t i = idx / p.n, j = idx % p.n;
  float acc = 0.0f;
  for (int64_t kk = 0; kk < p.k; ++kk) {
    const float av = p.a_km ? ld_elem(p.a, in_dtype, kk * p.lda + i) : ld_elem(p.a, in_dtype, i * p.lda + kk);
    const float bv = p.b_nk ? ld_elem(p.b, in_dtype, j * p.ldb + kk) : ld_elem(p.b, in_dtype, kk * p.ldb + j);
    acc = fmaf(av, bv, acc);
  }
  epilogue_store(p, i, j, acc);
}

// Main loop of the big bf16 shapes: 4 = the ping-pong rings on 256x256 tiles (default: gemm_pp64_kernel where K is whole 64-k
// blocks, gemm_pp256_kernel otherwise and for the weight gradients); 5 = gemm_pp256_kernel for all of them (A/B of the two);
// 0 = the two-stage 128x128 kernels for every shape (gemm_glds_kernel / gemm_tn_glds_kernel / gemm_mfma_kernel) and the
// two-call form of krs_gemm_cross_bwd -- the reference schedule for A/B and bit-for-bit tests.
// krs_gemm_set_option(KRS_GEMM_OPT_PIPELINE, v) / environment KRS_GEMM_PIPE (read once).
int g_pipe = -1;
int gemm_pipe() {
  if (g_pipe < 0) {
    const char* e = getenv("KRS_GEMM_PIPE");
    g_pipe = e ? atoi(e) : 4;
    if (g_pipe != 0 && g_pipe != 5) g_pipe = 4;
  }
  return g_pipe;
}
// Epilogue schedule of gemm_pp64_kernel's streaming builds (krs.h, KRS_GEMM_OPT_EPI_SCHEDULE): 0 = the reference schedule,
// 1 = LDS landing + the x == x0 build, 2 = stagger, 3 = both.  krs_gemm_set_option / environment KRS_GEMM_EPI_SCHEDULE
// (read once).  What each measured: docs/measurement_log.md, "Cross GEMM epilogue schedules".
constexpr int kEpiSchedDefault = 1;      // (the stagger measured no gain alone and a loss with 1: it stays behind the switch)
int g_epi_sched = -1;
int gemm_epi_sched() {
  if (g_epi_sched < 0) {
    const char* e = getenv("KRS_GEMM_EPI_SCHEDULE");
    g_epi_sched = e ? atoi(e) : kEpiSchedDefault;
    if (g_epi_sched < 0 || g_epi_sched > 3) g_epi_sched = kEpiSchedDefault;
  }
  return g_epi_sched;
}

// f(std::integral_constant<int, E>()) for the epilogue number e, First <= e <= Last: a kernel's EPI template argument
// picked at run time
template <int First, int Last, class F>
int with_epilogue(int e, F&& f) {
  if constexpr (First < Last) {
    if (e != First) return with_epilogue<First + 1, Last>(e, f);
  }
  return f(std::integral_constant<int, First>());
}

}  // namespace
}  // namespace krs

using namespace krs;

extern "C" int krs_gemm_set_option(int key, int value) {
  if (key == KRS_GEMM_OPT_PIPELINE) {
    KRS_REQUIRE(value == 0 || value == 4 || value == 5, "krs_gemm_set_option: pipeline must be 0, 4 or 5");
    g_pipe = value;
    return KRS_OK;
  }
  if (key == KRS_GEMM_OPT_EPI_SCHEDULE) {
    KRS_REQUIRE(value >= -1 && value <= 3, "krs_gemm_set_option: epilogue schedule must be 0, 1, 2, 3 or -1 (the default)");
    g_epi_sched = value;      // (-1: gemm_epi_sched() reads the environment / the built-in default again)
    return KRS_OK;
  }
  return fail(KRS_ERR_INVALID, "krs_gemm_set_option: unknown key %d", key);
}

extern "C" size_t krs_gemm_workspace_bytes(int64_t m, int64_t n, int64_t k, int a_is_km) {
  return gplan::plan_workspace_bytes(m, n, k, a_is_km != 0);
}

namespace krs {
namespace {
static_assert(gplan::kRingLds == 4 * pp::STAGE && gplan::kRing64Lds == ring64::NSLOT * ring64::SLOT, "the planner's LDS bytes");

// where the calling thread's last krs_gemm ran (krs_gemm_last_route): cleared when gemm_run starts, written when it has
// queued its last kernel, so a refused call and an empty product leave "none"
thread_local krs_gemm_route g_route = {};

// krs_gemm's argument checks, then the call's plan (gemm_plan.h); a refused plan leaves its message.  Host memory only:
// pointer VALUES are read for their alignment, the epilogue struct is read, no operand is dereferenced.
int gemm_plan(const void* a, int64_t lda, int a_is_km, const void* b, int64_t ldb, int b_is_nk, const void* c, int64_t ldc,
              int64_t m, int64_t n, int64_t k, int in_dtype, int out_dtype, const krs_gemm_epilogue* ep,
              size_t workspace_bytes, bool allow_split, gplan::GemmCall& call, gplan::GemmPlan& pl) {
  KRS_REQUIRE(a && b && c, "krs_gemm: null operand");
  KRS_REQUIRE(m >= 0 && n >= 0 && k >= 0, "krs_gemm: negative size");
  KRS_REQUIRE((in_dtype == KRS_F32 || in_dtype == KRS_BF16) && (out_dtype == KRS_F32 || out_dtype == KRS_BF16),
              "krs_gemm: bad dtype");
  if (ep && ep->x0) KRS_REQUIRE(ep->x, "krs_gemm: cross epilogue needs x with x0");
  static const bool tn128 = getenv("KRS_GEMM_TN128") != nullptr;
  call = gplan::GemmCall();
  call.m = m; call.n = n; call.k = k; call.a_km = a_is_km != 0; call.b_nk = b_is_nk != 0;
  call.es = in_dtype == KRS_BF16 ? 2 : 4; call.out_dtype = out_dtype;
  call.lda = lda; call.ldb = ldb; call.ldc = ldc; call.al_a = al16(a); call.al_b = al16(b); call.al_c = al16(c);
  gplan::set_epilogue(call, ep);
  call.workspace_bytes = workspace_bytes; call.allow_split = allow_split; call.pipe = gemm_pipe(); call.tn128 = tn128;
  call.epi_sched = gemm_epi_sched();
  pl = gplan::plan_gemm(call);
  if (pl.status == KRS_ERR_WORKSPACE)
    return fail(pl.status, "krs_gemm: split-K needs %zu workspace bytes, got %zu", pl.need, workspace_bytes);
  if (pl.status != KRS_OK) return fail(pl.status, "krs_gemm: the shape needs a grid beyond the launch limits");
  return KRS_OK;
}

// launches the kernel the plan names; ES = bytes per input element
template <int ES>
int gemm_launch(const GemmParams& p, const gplan::GemmPlan& pl, int in_dtype, hipStream_t st) {
  const krs_gemm_route& rt = pl.route;
  const dim3 grid((unsigned)pl.grid[0], (unsigned)pl.grid[1], (unsigned)pl.grid[2]), block((unsigned)pl.block);
  switch (rt.kernel) {
    case KRS_GEMM_KERNEL_PP64: {
      // the build the plan's schedule bits name (LDS_LANDING and X_IS_X0 exclude each other and come with build 1 only)
      constexpr int LAND = KRS_GEMM_SCHED_LDS_LANDING, STAG = KRS_GEMM_SCHED_STAGGER, X0 = kEpiCrossXIsX0;
      const bool stag = (rt.schedule & STAG) != 0;
      auto run = [&](auto E, auto S) {
        return launch_lds<gemm_pp64_kernel<E, S>>("gemm_pp64_kernel", grid, block, pl.lds, st, p, pl.nt);
      };
      using std::integral_constant;
      if (rt.epilogue == 0) return run(integral_constant<int, 0>(), integral_constant<int, 0>());
      if (rt.epilogue == 2)
        return stag ? run(integral_constant<int, 2>(), integral_constant<int, STAG>())
                    : run(integral_constant<int, 2>(), integral_constant<int, 0>());
      if (rt.schedule & KRS_GEMM_SCHED_X_IS_X0)
        return stag ? run(integral_constant<int, X0>(), integral_constant<int, STAG>())
                    : run(integral_constant<int, X0>(), integral_constant<int, 0>());
      if (rt.schedule & LAND)
        return stag ? run(integral_constant<int, 1>(), integral_constant<int, LAND | STAG>())
                    : run(integral_constant<int, 1>(), integral_constant<int, LAND>());
      return stag ? run(integral_constant<int, 1>(), integral_constant<int, STAG>())
                  : run(integral_constant<int, 1>(), integral_constant<int, 0>());
    }
    case KRS_GEMM_KERNEL_PP256:
      return with_epilogue<0, 2>(rt.epilogue, [&](auto E) {
        return launch_lds<gemm_pp256_kernel<false, 4, E>>("gemm_pp256_kernel", grid, block, pl.lds, st, p, 0, pl.nt);
      });
    case KRS_GEMM_KERNEL_PP256_KSTRIDED:
      return launch_lds<gemm_pp256_kernel<true, 4, 0>>("gemm_pp256_kernel (K-strided operands)", grid, block, pl.lds, st, p,
                                                       pl.mt, pl.nt);
    case KRS_GEMM_KERNEL_TN_GLDS:
      return launch_lds<gemm_tn_glds_kernel<0>>("gemm_tn_glds_kernel", grid, block, pl.lds, st, p, pl.mt, pl.nt);
    case KRS_GEMM_KERNEL_GLDS:
      return with_epilogue<0, 2>(rt.epilogue, [&](auto E) {
        return launch_lds<gemm_glds_kernel<ES, E>>("gemm_glds_kernel", grid, block, pl.lds, st, p);
      });
    case KRS_GEMM_KERNEL_MFMA:
      return with_epilogue<0, 2>(rt.epilogue, [&](auto E) {
        if (p.a_km) return launch_lds<gemm_mfma_kernel<ES, true, false, E>>("gemm_mfma_kernel", grid, block, pl.lds, st, p);
        if (p.b_nk) return launch_lds<gemm_mfma_kernel<ES, false, true, E>>("gemm_mfma_kernel", grid, block, pl.lds, st, p);
        return launch_lds<gemm_mfma_kernel<ES, false, false, E>>("gemm_mfma_kernel", grid, block, pl.lds, st, p);
      });
    case KRS_GEMM_KERNEL_THIN:
      if (rt.thin_width == 1) hipLaunchKernelGGL((gemm_thin_kernel<ES, 1>), grid, block, 0, st, p, rt.thin_is_a);
      else if (rt.thin_width == 4) hipLaunchKernelGGL((gemm_thin_kernel<ES, 4>), grid, block, 0, st, p, rt.thin_is_a);
      else if (rt.thin_width == 8) hipLaunchKernelGGL((gemm_thin_kernel<ES, 8>), grid, block, 0, st, p, rt.thin_is_a);
      else hipLaunchKernelGGL((gemm_thin_kernel<ES, 16>), grid, block, 0, st, p, rt.thin_is_a);
      KRS_CHECK_LAUNCH("gemm_thin_kernel");
      return KRS_OK;
    case KRS_GEMM_KERNEL_ROWDOT:
      hipLaunchKernelGGL(gemm_rowdot_kernel<ES>, grid, block, 0, st, p);
      KRS_CHECK_LAUNCH("gemm_rowdot_kernel");
      return KRS_OK;
    case KRS_GEMM_KERNEL_SMALLK:
      hipLaunchKernelGGL(gemm_smallk_kernel<ES>, grid, block, pl.lds, st, p, gplan::kSmallkRows);
      KRS_CHECK_LAUNCH("gemm_smallk_kernel");
      return KRS_OK;
    default:
      hipLaunchKernelGGL(gemm_generic_kernel, grid, block, 0, st, p, in_dtype);
      KRS_CHECK_LAUNCH("gemm_generic_kernel");
      return KRS_OK;
  }
}

// krs_gemm's body: validate and plan -> launch what the plan names.  `allow_split` false = one pass over K (the two-call
// form of krs_gemm_cross_bwd, whose workspace is sized for the column sums only).
int gemm_run(const void* a, int64_t lda, int a_is_km, const void* b, int64_t ldb, int b_is_nk,
             void* c, int64_t ldc, int64_t m, int64_t n, int64_t k, int in_dtype, int out_dtype,
             const krs_gemm_epilogue* epilogue, void* workspace, size_t workspace_bytes,
             void* stream, bool allow_split) {
  g_route = krs_gemm_route{};
  gplan::GemmCall call;
  gplan::GemmPlan pl;
  if (int rc = gemm_plan(a, lda, a_is_km, b, ldb, b_is_nk, c, ldc, m, n, k, in_dtype, out_dtype, epilogue,
                         workspace ? workspace_bytes : 0, allow_split, call, pl))
    return rc;
  const krs_gemm_route& rt = pl.route;
  if (rt.kernel == KRS_GEMM_KERNEL_NONE) return KRS_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  GemmParams p = gemm_params(a, lda, call.a_km, b, ldb, call.b_nk, c, ldc, m, n, k, out_dtype, epilogue);
  p.splits = rt.splits; p.k_per_split = pl.k_per_split; p.ep_vec = rt.ep_vec;
  p.slabs = rt.splits > 1 ? reinterpret_cast<float*>(workspace) : nullptr;
  if (int rc = call.es == 2 ? gemm_launch<2>(p, pl, in_dtype, st) : gemm_launch<4>(p, pl, in_dtype, st)) return rc;
  if (rt.reduce) {
    const dim3 rgrid((unsigned)pl.reduce_grid);
    if (rt.reduce == KRS_GEMM_REDUCE_VEC4) hipLaunchKernelGGL(gemm_slab_reduce_vec4_kernel, rgrid, dim3(256), 0, st, p);
    else if (rt.reduce == KRS_GEMM_REDUCE_VEC8) hipLaunchKernelGGL(gemm_slab_reduce_vec8_kernel, rgrid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(gemm_slab_reduce_kernel, rgrid, dim3(256), 0, st, p);
    KRS_CHECK_LAUNCH("gemm_slab_reduce_kernel");
  }
  g_route = rt;
  return KRS_OK;
}
}  // namespace
}  // namespace krs

extern "C" int krs_gemm(const void* a, int64_t lda, int a_is_km, const void* b, int64_t ldb, int b_is_nk,
                        void* c, int64_t ldc, int64_t m, int64_t n, int64_t k, int in_dtype, int out_dtype,
                        const krs_gemm_epilogue* epilogue, void* workspace, size_t workspace_bytes,
                        void* stream) {
  return gemm_run(a, lda, a_is_km, b, ldb, b_is_nk, c, ldc, m, n, k, in_dtype, out_dtype, epilogue, workspace,
                  workspace_bytes, stream, true);
}

extern "C" int krs_gemm_plan_route(const void* a, int64_t lda, int a_is_km, const void* b, int64_t ldb, int b_is_nk,
                                   const void* c, int64_t ldc, int64_t m, int64_t n, int64_t k, int in_dtype,
                                   int out_dtype, const krs_gemm_epilogue* epilogue, size_t workspace_bytes,
                                   krs_gemm_route* route) {
  gplan::GemmCall call;
  gplan::GemmPlan pl;
  const int rc = gemm_plan(a, lda, a_is_km, b, ldb, b_is_nk, c, ldc, m, n, k, in_dtype, out_dtype, epilogue,
                           workspace_bytes, true, call, pl);
  if (route) *route = pl.route;
  return rc;
}

extern "C" int krs_gemm_last_route(krs_gemm_route* route) {
  if (route) *route = g_route;
  return g_route.kernel;
}

// ---- krs_gemm_cross_bwd: data-gradient product + the elementwise backward of the layer below, one launch ---------------
extern "C" size_t krs_gemm_cross_bwd_workspace_bytes(int64_t m, int64_t n) {
  if (m <= 0 || n <= 0) return 0;
  return std::max(krs_colsum_workspace_bytes(m, n), (size_t)(2 * ceil_div(m, 256)) * (size_t)n * sizeof(float));
}

// which route the calling thread's last krs_gemm_cross_bwd / krs_gemm_dense_bwd took (krs_gemm_cross_bwd_last_route)
static thread_local int cb_route = KRS_CROSS_BWD_NONE, cb_epilogue = 0;

extern "C" int krs_gemm_cross_bwd_last_route(int* epilogue) {
  if (epilogue) *epilogue = cb_epilogue;
  return cb_route;
}

// The body of krs_gemm_cross_bwd and of krs_gemm_dense_bwd (`dense`: the layer below is a Dense layer, u its saved output:
// dz = G act'(u), dbias; x0, R, dx0, u_upper and fold_direct are absent).  The entries have checked their operands; `who`
// names the entry in error messages.  `plan_only` (krs_gemm_cross_bwd_plan_route): the plan is handed back, nothing runs.
static int cross_bwd(const char* who, bool dense, const void* a, int64_t lda, const void* bt, int64_t ldb, const void* r,
                     int64_t ldr, float beta, void* g_out, int64_t ldg, const void* x0, const void* u, void* dz, void* dx0,
                     int64_t ld, int dx0_accumulate, const void* u_upper, int fold_direct, float* dbias, int64_t m,
                     int64_t n, int64_t k, int act, int dtype, void* workspace, size_t workspace_bytes, void* stream,
                     gplan::CrossBwdPlan* plan_only = nullptr) {
  // dense form: G is stored only where the caller asked for it (g_out != NULL), by either route; without g_out the fused
  // route writes dz alone and the two-call route lands G in dz's buffer and applies the derivative in place
  const bool store_g = g_out != nullptr;
  if (dense && !g_out) { g_out = dz; ldg = ld; }
  if (!r) { ldr = n; beta = 0.0f; }
  KRS_REQUIRE(dtype == KRS_BF16 || dtype == KRS_F32, "%s: bad dtype", who);
  KRS_REQUIRE(m >= 0 && n >= 0 && k > 0 && ld >= n && ldg >= n && ldr >= n, "%s: bad sizes", who);
  // the product as the two-call form hands it to krs_gemm (one pass over K: this entry's workspace holds the column sums,
  // not split-K slabs), and the plan of the whole call
  krs_gemm_epilogue ep;
  memset(&ep, 0, sizeof(ep));
  ep.r = r; ep.ldr = ldr; ep.beta = beta;
  gplan::CrossBwdPlan cb;
  if (m > 0 && n > 0) {
    gplan::GemmCall call;
    if (int rc = gemm_plan(a, lda, 0, bt, ldb, 1, g_out, ldg, m, n, k, dtype, dtype, r ? &ep : nullptr, 0, false, call, cb.product))
      return rc;
    gplan::plan_cross_bwd(cb, r != nullptr, ld, al16(x0) && al16(u) && al16(dz) && al16(dx0) && al16(u_upper), dense, store_g,
                          dx0 != nullptr, dx0_accumulate != 0, u_upper != nullptr, gemm_epi_sched());
  }
  if (plan_only) { *plan_only = cb; return KRS_OK; }
  if (dbias) KRS_REQUIRE(workspace_bytes >= krs_gemm_cross_bwd_workspace_bytes(m, n) && (workspace || m == 0 || n == 0),
                         "%s: workspace too small (krs_gemm_cross_bwd_workspace_bytes)", who);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (m == 0 || n == 0) {   // (the column sums over no rows are zeros)
    if (dbias && n > 0) KRS_HIP(hipMemsetAsync(dbias, 0, (size_t)n * sizeof(float), st));
    return KRS_OK;
  }
  if (cb.route == KRS_CROSS_BWD_TWO_CALL) {
    // any other shape / dtype: the two calls this entry stands for
    cb_route = cb.route;
    if (int rc = gemm_run(a, lda, 0, bt, ldb, 1, g_out, ldg, m, n, k, dtype, dtype, r ? &ep : nullptr, nullptr, 0, stream,
                          false))
      return rc;
    KRS_REQUIRE(ldg == ld, "%s: the two-call form needs one row stride for G, x0, u, dz and dx0", who);
    if (dense)    // G lands in (or is) dz's buffer, the activation derivative is applied in place
      return krs_dense_act_bwd(g_out, ldg, u, ld, dz, ld, dbias, m, n, act, dtype, workspace, workspace_bytes, stream);
    if (u_upper) {   // the upper layer's term first: dx0 = R * u_upper (its own rounding here), then accumulate
      KRS_REQUIRE(ldr == ld, "%s: the two-call form needs R on the common row stride", who);
      if (int rc = krs_cross_epilogue_bwd(r, u_upper, x0, x0, nullptr, dx0, 0, nullptr, nullptr, m, n, ld, 0.0f, KRS_ACT_NONE,
                                          dtype, nullptr, 0, stream)) return rc;
      dx0_accumulate = 1;
    }
    return krs_cross_epilogue_bwd(g_out, u, x0, x0, dz, dx0, dx0_accumulate, fold_direct ? dx0 : nullptr, dbias, m, n,
                                  ld, 0.0f, act, dtype, workspace, workspace_bytes, stream);
  }
  GemmParams p = gemm_params(a, lda, false, bt, ldb, true, g_out, ldg, m, n, k, KRS_BF16, &ep);   // (one pass over K)
  p.ep_vec = 1;
  p.f_x0 = x0; p.f_u = u; p.f_uup = u_upper; p.f_dz = dz; p.f_dx0 = dx0; p.f_ld = ld; p.f_act = act; p.f_fold = fold_direct != 0;
  p.f_partial = dbias ? reinterpret_cast<float*>(workspace) : nullptr;
  // the fused epilogue of this form (EPI 3 .. 10 of both ring kernels) on the ring the planner gives the product (the 64-k
  // ring is level with the 32-k one on this epilogue-bound form: 640-650 us either way)
  const gplan::GemmPlan& pl = cb.product;
  const dim3 grid256((unsigned)pl.grid[0]), block((unsigned)pl.block);
  cb_route = cb.route; cb_epilogue = cb.epilogue;
  const int rc = with_epilogue<3, 10>(cb.epilogue, [&](auto E) {
    if (cb.route == KRS_CROSS_BWD_PP64)
      return cb.stagger ? launch_lds<gemm_pp64_kernel<E, KRS_GEMM_SCHED_STAGGER>>("gemm_pp64_kernel (fused cross backward)",
                                                                                  grid256, block, pl.lds, st, p, pl.nt)
                        : launch_lds<gemm_pp64_kernel<E, 0>>("gemm_pp64_kernel (fused cross backward)", grid256, block, pl.lds,
                                                             st, p, pl.nt);
    return launch_lds<gemm_pp256_kernel<false, 4, E>>("gemm_pp256_kernel (fused cross backward)", grid256, block, pl.lds, st,
                                                      p, 0, pl.nt);
  });
  if (rc != KRS_OK) return rc;
  return dbias ? finish_colsum(p.f_partial, 2 * ceil_div(m, 256), n, dbias, st) : KRS_OK;
}

extern "C" int krs_gemm_cross_bwd_plan_route(const void* a, int64_t lda, const void* bt, int64_t ldb, const void* r,
                                             int64_t ldr, float beta, void* g_out, int64_t ldg, const void* x0, const void* u,
                                             void* dz, void* dx0, int64_t ld, int dx0_accumulate, const void* u_upper,
                                             int64_t m, int64_t n, int64_t k, int dtype, int* epilogue) {
  gplan::CrossBwdPlan cb;
  const int rc = cross_bwd("krs_gemm_cross_bwd_plan_route", x0 == nullptr, a, lda, bt, ldb, r, ldr, beta, g_out, ldg, x0, u, dz,
                           dx0, ld, dx0_accumulate, u_upper, 0, nullptr, m, n, k, KRS_ACT_NONE, dtype, nullptr, 0, nullptr, &cb);
  if (epilogue) *epilogue = cb.epilogue;
  return rc ? rc : cb.route;
}

extern "C" int krs_gemm_cross_bwd(const void* a, int64_t lda, const void* bt, int64_t ldb, const void* r, int64_t ldr,
                                  float beta, void* g_out, int64_t ldg, const void* x0, const void* u, void* dz,
                                  void* dx0, int64_t ld, int dx0_accumulate, const void* u_upper, int fold_direct,
                                  float* dbias, int64_t m, int64_t n, int64_t k, int act, int dtype, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  cb_route = KRS_CROSS_BWD_NONE; cb_epilogue = 0;
  // (an empty product may come with NULL operands: a framework's empty tensors have no storage)
  // (x0 = NULL selected the dense form before it had an entry of its own: the message says where it went)
  KRS_REQUIRE((a && bt && x0 && u && dz && g_out) || m == 0 || n == 0, "krs_gemm_cross_bwd: null operand%s",
              x0 ? "" : " (x0 = NULL: the dense form is krs_gemm_dense_bwd)");
  KRS_REQUIRE(dx0 || (!r && !dx0_accumulate && !u_upper && !fold_direct),
              "krs_gemm_cross_bwd: dx0 = NULL (the term is left to the next launch's u_upper) is the form without R");
  KRS_REQUIRE(!u_upper || (r && !dx0_accumulate && beta == 1.0f),
              "krs_gemm_cross_bwd: u_upper (dx0 = R * u_upper + ...) needs R with beta = 1 and no dx0 to accumulate into");
  return cross_bwd("krs_gemm_cross_bwd", false, a, lda, bt, ldb, r, ldr, beta, g_out, ldg, x0, u, dz, dx0, ld,
                   dx0_accumulate, u_upper, fold_direct, dbias, m, n, k, act, dtype, workspace, workspace_bytes, stream);
}

extern "C" int krs_gemm_dense_bwd(const void* a, int64_t lda, const void* bt, int64_t ldb, void* g_out, int64_t ldg,
                                  const void* y, void* dz, int64_t ld, float* dbias, int64_t m, int64_t n, int64_t k,
                                  int act, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
  cb_route = KRS_CROSS_BWD_NONE; cb_epilogue = 0;
  KRS_REQUIRE((a && bt && y && dz) || m == 0 || n == 0, "krs_gemm_dense_bwd: null operand");
  return cross_bwd("krs_gemm_dense_bwd", true, a, lda, bt, ldb, nullptr, n, 0.0f, g_out, ldg, nullptr, y, dz, nullptr, ld,
                   0, nullptr, 0, dbias, m, n, k, act, dtype, workspace, workspace_bytes, stream);
}
