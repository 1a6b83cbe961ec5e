// K18 -- Dense and FeatureCross in int8: C = epilogue(scale(Aq . Wq^T)) on v_mfma_i32_32x32x32_i8 (include/krs.h, K18).
//
// The serving form of keras.layers.Dense.quantize("int8"): aq [M, K] int8 with one fp32 step per row (the activation
// quantizer, krs_quantize_rows_q8), wq [N, K] int8 with one step per output channel, an exact int32 product,
// z = fmul_rn(fmul_rn((float) idot, wstep_j), astep_i), then krs_gemm's epilogue (gemm_device.h: one copy of it).
// Kernels, by shape (gemm_q8_plan.h decides, a pure host function):
//   * gemm_q8_ring_kernel     gemm_pp64_kernel's main loop (gemm_ring64.h, one copy) with int32 accumulators: 256 x 256 tiles,
//                             eight waves as 2 x 4, 128-byte = 128-k pieces by LDS-DMA into five 32 KB slots -- the loop is
//                             written in bytes, and a lane's 16-byte fragment is one v_mfma_i32_32x32x32_i8 here where it is
//                             one v_mfma_f32_32x32x16_bf16 there (both operands take the same 16-byte chunk, so how the
//                             instruction deals k to lanes cannot matter to an integer sum);
//   * gemm_q8_tile_kernel     128 x 128 tiles staged through registers (gemm_mfma_kernel's form), a K tail zero-filled in
//                             LDS: zero bytes add exactly nothing;
//   * gemm_q8_generic_kernel  any shape and alignment, byte loads, one output per thread.
// The wave epilogue stages the int32 accumulators through LDS so that a lane owns 8 consecutive columns of one row, loads
// astep once per row and wstep as the row's 8 neighbours, converts and scales, and hands v = z to epilogue_store /
// epilogue_store_vec8.  A row whose astep is 0 (a non-finite activation row) is written as quiet NaNs instead.  The ring's
// cross build (bf16 output: the FeatureCross product of a served model) scales in the accumulator layout and runs the wave
// epilogue krs_gemm's rings run, x0 / x requested ahead of the staging.
#include "gemm_device.h"
#include "gemm_q8_plan.h"
#include "gemm_ring64.h"

namespace krs {
namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

struct Q8Params {
  GemmParams g;         // a = aq, b = wq (both K-contiguous, one byte per element), splits = 1
  const float* astep;   // [M]
  const float* wstep;   // [N]
  int ws_vec;           // ep_vec and wstep on 16 bytes: a lane's 8 steps are two 16-byte loads
};

// z of K18: the conversion rounds to nearest even, the two multiplies are rounded separately (never contracted)
__device__ __forceinline__ float q8_scale(int idot, float ws, float as) { return __fmul_rn(__fmul_rn((float)idot, ws), as); }

// one element: a non-finite activation row (astep == 0) is NaN in C and u_out whatever the epilogue, else the epilogue on z
__device__ __forceinline__ void q8_store(const Q8Params& q, int64_t i, int64_t j, int idot, float as) {
  const GemmParams& p = q.g;
  if (as == 0.0f) {
    st_elem(p.c, p.out_dtype, i * p.ldc + j, quiet_nan());
    if (p.has_ep && p.ep.x0 && p.ep.u_out) st_elem(p.ep.u_out, p.out_dtype, i * p.ep.ldu + j, quiet_nan());
    return;
  }
  epilogue_store(p, i, j, q8_scale(idot, q.wstep[j], as));
}

// 8 consecutive columns of one row (ep_vec: n % 8 == 0 and every operand allows 8-wide access)
__device__ __forceinline__ void q8_store_vec8(const Q8Params& q, int64_t i, int64_t j, const int (&d)[8], float as) {
  const GemmParams& p = q.g;
  float v[8];
  if (as == 0.0f) {
#pragma unroll
    for (int t = 0; t < 8; ++t) v[t] = quiet_nan();
    store8(p.c, p.out_dtype, i * p.ldc + j, v);
    if (p.has_ep && p.ep.x0 && p.ep.u_out) store8(p.ep.u_out, p.out_dtype, i * p.ep.ldu + j, v);
    return;
  }
  float ws[8];
  if (q.ws_vec) {
    const float4 w0 = *reinterpret_cast<const float4*>(q.wstep + j);
    const float4 w1 = *reinterpret_cast<const float4*>(q.wstep + j + 4);
    ws[0] = w0.x; ws[1] = w0.y; ws[2] = w0.z; ws[3] = w0.w; ws[4] = w1.x; ws[5] = w1.y; ws[6] = w1.z; ws[7] = w1.w;
  } else {
#pragma unroll
    for (int t = 0; t < 8; ++t) ws[t] = q.wstep[j + t];
  }
#pragma unroll
  for (int t = 0; t < 8; ++t) v[t] = q8_scale(d[t], ws[t], as);
  epilogue_store_vec8(p, i, j, v);
}

// One chunk of a wave's block of C: 32 rows x 64 columns, two 32 x 32 accumulator fragments (columns 0..31 / 32..63), through
// the wave's private 32 x SST words of LDS.  MFMA C/D layout: col = lane & 31, row = (r & 3) + 8*(r >> 2) + 4*(lane >> 5).
__device__ __forceinline__ void q8_epi_chunk(const Q8Params& q, const i32x16 (&acc2)[2], int* stage, int64_t row0, int64_t wn0) {
  const GemmParams& p = q.g;
  const int lane = threadIdx.x & 63;
  const int frow = lane & 31;
  const int fhalf = lane >> 5;
  constexpr int SST = 68;  // staging row stride in words (64 + pad)
  const int ec = (lane & 7) * 8;
  const int64_t gn = wn0 + ec;
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) stage[((r & 3) + 8 * (r >> 2) + 4 * fhalf) * SST + j * 32 + frow] = acc2[j][r];
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // wave-private staging: no workgroup barrier
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int er = it * 8 + (lane >> 3);
    const int64_t gm = row0 + er;
    if (gm >= p.m || gn >= p.n) continue;
    const i32x4 d0 = *reinterpret_cast<const i32x4*>(stage + er * SST + ec);
    const i32x4 d1 = *reinterpret_cast<const i32x4*>(stage + er * SST + ec + 4);
    const int d[8] = {d0[0], d0[1], d0[2], d0[3], d1[0], d1[1], d1[2], d1[3]};
    const float as = q.astep[gm];
    if (p.ep_vec) {
      q8_store_vec8(q, gm, gn, d, as);
    } else {
      for (int t = 0; t < 8 && gn + t < p.n; ++t) q8_store(q, gm, gn + t, d[t], as);
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// The cross build of the ring (bf16 output, vector access everywhere; gemm_device.h's epi_prefetch / epi_process<1>, the
// build krs_gemm's rings use): z is formed in the accumulator's own layout -- a lane's column step once per fragment, a
// row's step once per row -- and the shared wave epilogue takes it from there with its x0 / x loads issued ahead.
__device__ __forceinline__ void q8_scale_chunk(const Q8Params& q, const i32x16 (&acc2)[2], f32x16 (&z)[2], int64_t row0,
                                               int64_t wn0) {
  const int lane = threadIdx.x & 63;
  const float ws0 = q.wstep[min(wn0 + (lane & 31), q.g.n - 1)], ws1 = q.wstep[min(wn0 + 32 + (lane & 31), q.g.n - 1)];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float as = q.astep[min(row0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), q.g.m - 1)];
    z[0][r] = q8_scale(acc2[0][r], ws0, as);
    z[1][r] = q8_scale(acc2[1][r], ws1, as);
  }
}
// ... and the rows whose astep is 0 are overwritten with NaNs afterwards, by the lane that wrote them (epi_process's own
// lane -> (row, 8 columns) map and its store form: one thread's stores to one address keep their order)
__device__ __forceinline__ void q8_nan_rows_wave128(const Q8Params& q, int64_t wm0, int64_t wn0) {
  const GemmParams& p = q.g;
  const int lane = threadIdx.x & 63;
  const int64_t gn = wn0 + (lane & 7) * 8;
  if (gn >= p.n) return;
  const float v[8] = {quiet_nan(), quiet_nan(), quiet_nan(), quiet_nan(), quiet_nan(), quiet_nan(), quiet_nan(), quiet_nan()};
#pragma unroll
  for (int it = 0; it < 16; ++it) {
    const int64_t gm = wm0 + it * 8 + (lane >> 3);
    if (gm >= p.m || q.astep[gm] != 0.0f) continue;
    store8_bf16_nt(p.c, gm * p.ldc + gn, v);
    if (p.ep.u_out) store8_bf16_nt(p.ep.u_out, gm * p.ep.ldu + gn, v);
  }
}

// ---- 128 x 128 tiles, 4 waves as 2 x 2, operands staged HBM -> registers -> LDS ([row][k], 144-byte rows) ----------------
constexpr int BM = gplan::kTile, BN = gplan::kTile;
constexpr int ROW_BYTES = gplan::kRowBytes;   // 128 k per tile row
constexpr int TILE_BYTES = gplan::kTileBytes;

__global__ __launch_bounds__(256, 3) void gemm_q8_tile_kernel(const Q8Params q) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const GemmParams& p = q.g;
  char* ta = smem;
  char* tb = smem + TILE_BYTES;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  // XCD-aware tile order of gemm_mfma_kernel: the N tiles of one M panel run back to back on one XCD
  const int64_t nt = (p.n + BN - 1) / BN;
  const int64_t xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int64_t m_tile = (slot / nt) * 8 + xcd;
  if (m_tile * BM >= p.m) return;
  const int64_t m0 = m_tile * BM;
  const int64_t n0 = (slot % nt) * BN;
  const int64_t ntiles = (p.k + ROW_BYTES - 1) / ROW_BYTES;

  i32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;

  u32x4 ra[4], rb[4];
  auto load_tiles = [&](int64_t t) {
    // (K is a multiple of 16, so a 16-byte chunk lies inside the row or is zero)
    load_kcontig<1>(p.a, p.lda, m0, t * ROW_BYTES, p.m, p.k, ra);
    load_kcontig<1>(p.b, p.ldb, n0, t * ROW_BYTES, p.n, p.k, rb);
  };
  if (ntiles > 0) load_tiles(0);
  const int frow = lane & 31;   // fragment row (m for A, n for B)
  const int fhalf = lane >> 5;  // which 16-byte half of a 32-byte K step this lane feeds
  for (int64_t t = 0; t < ntiles; ++t) {
    __syncthreads();  // every wave is done reading the previous tile
    store_kcontig(ta, ra);
    store_kcontig(tb, rb);
    __syncthreads();
    if (t + 1 < ntiles) load_tiles(t + 1);  // in flight under the MFMAs below
#pragma unroll
    for (int ks = 0; ks < ROW_BYTES / 32; ++ks) {  // 32 k per step (2 lane halves x 16 bytes)
      u32x4 fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        fa[i] = *reinterpret_cast<const u32x4*>(ta + lds_chunk_off<false>(wm * 64 + i * 32 + frow, ks * 2 + fhalf));
        fb[i] = *reinterpret_cast<const u32x4*>(tb + lds_chunk_off<false>(wn * 64 + i * 32 + frow, ks * 2 + fhalf));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(__builtin_bit_cast(i32x4, fa[i]), __builtin_bit_cast(i32x4, fb[j]),
                                                            acc[i][j], 0, 0, 0);
    }
  }
  __syncthreads();  // operand tiles are dead from here on

  int* stage = reinterpret_cast<int*>(smem) + wave * (32 * 68);
  q8_epi_chunk(q, acc[0], stage, m0 + wm * 64, n0 + wn * 64);
  q8_epi_chunk(q, acc[1], stage, m0 + wm * 64 + 32, n0 + wn * 64);
}

// ---- the ring: the main loop of gemm_ring64.h (gemm_pp64_kernel's) on int8 operands ----------------------------------------
// A 128-byte piece row is 128 k here, a phase's 32 bytes one v_mfma_i32_32x32x32_i8 per fragment pair.  The host guarantees
// K = nb whole pieces, nb >= 3, bases on 16 bytes and lda, ldw multiples of 16.
static_assert(q8plan::kRingLds == ring64::NSLOT * ring64::SLOT && q8plan::kTileLds == 2 * TILE_BYTES, "the planner's LDS bytes");
static_assert(q8plan::kTileLds >= 4 * 32 * 68 * 4 && q8plan::kRingLds >= 8 * 32 * 68 * 4, "the epilogue's staging fits");

// EPI: 0 = the general epilogue, 1 = cross (bf16 output, vector access everywhere), as gemm_pp64_kernel's builds 0 and 1.
template <int EPI>
__global__ __launch_bounds__(512) void gemm_q8_ring_kernel(const Q8Params q, int nt) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TM = 256, TN_ = 256;
  const GemmParams& p = q.g;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int64_t xcd = blockIdx.x & 7, tslot = blockIdx.x >> 3;
  const int64_t m_tile = (tslot / nt) * 8 + xcd;
  if (m_tile * TM >= p.m) return;
  const int64_t m0 = m_tile * TM, n0 = (tslot % nt) * TN_;
  const int64_t nb = p.k / 128;   // whole pieces, at least three

  i32x16 acc[4][2];   // [32-row chunk of the wave's 128 rows][32-column half of its 64 columns]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;
  ring64_main_loop<1, 0>(
      smem, p, m0, n0, 0, nb, lane, wave,
      [&](int i, int j, const u32x4& fa, const u32x4& fb) {
        acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(__builtin_bit_cast(i32x4, fa), __builtin_bit_cast(i32x4, fb), acc[i][j],
                                                          0, 0, 0);
      },
      []() {});
  // every wave has passed the loop's last barrier: the slots are dead, a wave's staging words are its own
  int* stage = reinterpret_cast<int*>(smem) + wave * (32 * 68);
  const int64_t wm0 = m0 + wm * 128, wn0 = n0 + wn * 64;
  if constexpr (EPI == 1) {
    // gemm_epilogue_wave128's order -- two chunks of x0 / x in flight -- with a chunk scaled just before it is staged
    float* stage_f = reinterpret_cast<float*>(stage);
    EpiOperands o0, o1;
    f32x16 z[2];
    epi_prefetch<1>(p, o0, wm0, wn0);
    epi_prefetch<1>(p, o1, wm0 + 32, wn0);
    q8_scale_chunk(q, acc[0], z, wm0, wn0);
    epi_process<1>(p, z, o0, stage_f, wm0, wn0, 0);
    epi_prefetch<1>(p, o0, wm0 + 64, wn0);
    q8_scale_chunk(q, acc[1], z, wm0 + 32, wn0);
    epi_process<1>(p, z, o1, stage_f, wm0 + 32, wn0, 0);
    epi_prefetch<1>(p, o1, wm0 + 96, wn0);
    q8_scale_chunk(q, acc[2], z, wm0 + 64, wn0);
    epi_process<1>(p, z, o0, stage_f, wm0 + 64, wn0, 0);
    q8_scale_chunk(q, acc[3], z, wm0 + 96, wn0);
    epi_process<1>(p, z, o1, stage_f, wm0 + 96, wn0, 0);
    q8_nan_rows_wave128(q, wm0, wn0);
    return;
  }
  q8_epi_chunk(q, acc[0], stage, wm0, wn0);
  q8_epi_chunk(q, acc[1], stage, wm0 + 32, wn0);
  q8_epi_chunk(q, acc[2], stage, wm0 + 64, wn0);
  q8_epi_chunk(q, acc[3], stage, wm0 + 96, wn0);
}

// any shape / alignment: one thread per output element
__global__ __launch_bounds__(256) void gemm_q8_generic_kernel(const Q8Params q) {
  const GemmParams& p = q.g;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.m * p.n) return;
  const int64_t i = idx / p.n, j = idx % p.n;
  const int8_t* a = reinterpret_cast<const int8_t*>(p.a) + i * p.lda;
  const int8_t* w = reinterpret_cast<const int8_t*>(p.b) + j * p.ldb;
  int acc = 0;
  for (int64_t e = 0; e < p.k; ++e) acc += (int)a[e] * (int)w[e];
  q8_store(q, i, j, acc, q.astep[i]);
}

// where the calling thread's last krs_gemm_q8 ran: cleared when a call starts, written when its kernel is queued
thread_local krs_gemm_q8_route g_route = {};

// krs_gemm_q8's argument checks (the shape checks first), then the call's plan.  Host memory only: pointer VALUES are read
// for their alignment, the epilogue struct is read, no operand is dereferenced.
int q8_plan(const int8_t* aq, int64_t lda, const float* astep, const int8_t* wq, int64_t ldw, const float* wstep, const void* c,
            int64_t ldc, int64_t m, int64_t n, int64_t k, int out_dtype, const krs_gemm_epilogue* ep, q8plan::Q8Plan& pl) {
  pl = q8plan::Q8Plan();
  KRS_REQUIRE(m >= 0 && n >= 0 && k >= 0, "krs_gemm_q8: negative size");
  KRS_REQUIRE(lda >= k && ldw >= k && ldc >= n, "krs_gemm_q8: a row stride shorter than its row (lda, ldw >= k; ldc >= n)");
  KRS_REQUIRE(out_dtype == KRS_F32 || out_dtype == KRS_BF16, "krs_gemm_q8: bad out_dtype");
  gplan::GemmCall call;
  call.m = m; call.n = n; call.k = k; call.a_km = false; call.b_nk = true; call.es = 1; call.out_dtype = out_dtype;
  call.lda = lda; call.ldb = ldw; call.ldc = ldc; call.al_a = al16(aq); call.al_b = al16(wq); call.al_c = al16(c);
  gplan::set_epilogue(call, ep);
  const q8plan::Q8Plan plan = q8plan::plan_gemm_q8(call);
  if (plan.status != KRS_OK) return fail(plan.status, "krs_gemm_q8: %s", plan.why);
  if (m == 0 || n == 0) return KRS_OK;
  KRS_REQUIRE(aq && astep && wq && wstep && c, "krs_gemm_q8: null operand");
  if (ep && ep->x0) KRS_REQUIRE(ep->x, "krs_gemm_q8: cross epilogue needs x with x0");
  pl = plan;
  return KRS_OK;
}

}  // namespace
}  // namespace krs

using namespace krs;

extern "C" int krs_gemm_q8(const int8_t* aq, int64_t lda, const float* astep, const int8_t* wq, int64_t ldw, const float* wstep,
                           void* c, int64_t ldc, int64_t m, int64_t n, int64_t k, int out_dtype,
                           const krs_gemm_epilogue* epilogue, void* stream) {
  g_route = krs_gemm_q8_route{};
  q8plan::Q8Plan pl;
  if (int rc = q8_plan(aq, lda, astep, wq, ldw, wstep, c, ldc, m, n, k, out_dtype, epilogue, pl)) return rc;
  const krs_gemm_q8_route& rt = pl.route;
  if (rt.kernel == KRS_GEMM_Q8_KERNEL_NONE) return KRS_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  Q8Params q{};
  q.g = gemm_params(aq, lda, false, wq, ldw, true, c, ldc, m, n, k, out_dtype, epilogue);   // (one pass over K)
  q.g.ep_vec = rt.ep_vec;
  q.astep = astep; q.wstep = wstep; q.ws_vec = rt.ep_vec && al16(wstep);
  const dim3 grid((unsigned)pl.grid), block((unsigned)pl.block);
  int rc = KRS_OK;
  if (rt.kernel == KRS_GEMM_Q8_KERNEL_RING) {
    rc = rt.epilogue == 1 ? launch_lds<gemm_q8_ring_kernel<1>>("gemm_q8_ring_kernel (cross)", grid, block, pl.lds, st, q, pl.nt)
                          : launch_lds<gemm_q8_ring_kernel<0>>("gemm_q8_ring_kernel", grid, block, pl.lds, st, q, pl.nt);
  } else if (rt.kernel == KRS_GEMM_Q8_KERNEL_TILE128) {
    rc = launch_lds<gemm_q8_tile_kernel>("gemm_q8_tile_kernel", grid, block, pl.lds, st, q);
  } else {
    hipLaunchKernelGGL(gemm_q8_generic_kernel, grid, block, 0, st, q);
    KRS_CHECK_LAUNCH("gemm_q8_generic_kernel");
  }
  if (rc != KRS_OK) return rc;
  g_route = rt;
  return KRS_OK;
}

extern "C" int krs_gemm_q8_last_route(krs_gemm_q8_route* route) {
  if (route) *route = g_route;
  return g_route.kernel;
}

extern "C" int krs_gemm_q8_plan_route(const int8_t* aq, int64_t lda, const float* astep, const int8_t* wq, int64_t ldw,
                                      const float* wstep, const void* c, int64_t ldc, int64_t m, int64_t n, int64_t k,
                                      int out_dtype, const krs_gemm_epilogue* epilogue, krs_gemm_q8_route* route) {
  q8plan::Q8Plan pl;
  const int rc = q8_plan(aq, lda, astep, wq, ldw, wstep, c, ldc, m, n, k, out_dtype, epilogue, pl);
  if (route) *route = pl.route;
  return rc;
}
