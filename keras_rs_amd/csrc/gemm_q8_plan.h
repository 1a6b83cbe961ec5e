// krs_gemm_q8's routing decision (K18) as a pure function of the call: kernel, grid, LDS bytes, refusals.  Plain C++17 on
// krs.h and gemm_plan.h, no HIP header: tests/host/gemm_q8_plan_check.cpp walks it under the sanitizers and
// krs_gemm_q8_plan_route answers from it without a GPU.  gemm_q8.hip validates, plans here and launches what the plan names.
// The call is described by gemm_plan.h's GemmCall with es = 1 (one byte per element), A [M, K] and W [N, K] both
// K-contiguous (b_nk), ldb = ldw; the epilogue facts and ep_vec are krs_gemm's.
// A plan guarantees (the lattice walk asserts it): on the ring K is whole 128-byte pieces and at least three of them, both
// dimensions hold a 256-tile and the tiles meet the chip-fill bar; on the ring and the 128-tile kernel the bases are on 16
// bytes and lda, ldw, K are multiples of 16; every grid is within the launch limits; a refusal carries no kernel.
#ifndef KRS_GEMM_Q8_PLAN_H_
#define KRS_GEMM_Q8_PLAN_H_

#include "gemm_plan.h"

namespace krs {
namespace q8plan {

constexpr int64_t kMaxK = 131072;                 // 131072 * 128 * 128 = 2^31: the int32 sum of a longer row could overflow
constexpr int kPiece = 128;                       // the ring's unit along K: one 128-byte line per row = 128 k
constexpr int kRingPieces = 3;                    // pieces the ring's prologue and its two tail blocks need
constexpr size_t kRingLds = gplan::kRing64Lds;    // five 32 KB slots, as gemm_pp64_kernel
constexpr size_t kTileLds = 2 * gplan::kTileBytes;   // one A and one B tile of 128 rows x 144 bytes
// The ring against the 128-tile kernel where 256 x 256 tiles do not fill the chip: the ring runs one workgroup per CU, so
// with fewer tiles than kFillTiles most of a round's CUs idle, and there is no split-K here to deal K instead.  The bar is
// krs_gemm's (gemm_plan.h kFillTiles, measured for the bf16 ring); for int8 it is a GUESS carried over, not a measurement.
constexpr int kFillTiles = gplan::kFillTiles;

struct Q8Plan {
  krs_gemm_q8_route route = {};   // all zero ("none") when nothing is launched: m == 0, n == 0 or a refused call
  int status = KRS_OK;            // KRS_OK or KRS_ERR_UNSUPPORTED, decided before any launch
  const char* why = "";           // the limit a refusal names
  int64_t grid = 0;
  int block = 256, nt = 0;        // threads per workgroup; N tiles of the ring
  size_t lds = 0;
};

// c.es == 1, !c.a_km, c.b_nk; sizes are non-negative (the entry checked)
inline Q8Plan plan_gemm_q8(const gplan::GemmCall& c) {
  Q8Plan p;
  auto refuse = [&](const char* why) { p = Q8Plan(); p.status = KRS_ERR_UNSUPPORTED; p.why = why; return p; };
  if (c.k > kMaxK) return refuse("k is limited to 131072 (the int32 dot product of a longer row could overflow)");
  if (c.m > INT32_MAX || c.n > INT32_MAX) return refuse("m and n are limited to 2^31 - 1");
  if (c.m == 0 || c.n == 0) return p;
  krs_gemm_q8_route& rt = p.route;
  rt.ep_vec = gplan::ep_vec(c);
  const int64_t t256 = gplan::cdiv(c.m, gplan::kBigTile) * gplan::cdiv(c.n, gplan::kBigTile);
  if (gplan::tile_eligible(c)) {
    if (c.m >= gplan::kBigTile && c.n >= gplan::kBigTile && c.k % kPiece == 0 && c.k >= kRingPieces * kPiece &&
        t256 >= kFillTiles) {
      rt.kernel = KRS_GEMM_Q8_KERNEL_RING;
      p.nt = (int)gplan::cdiv(c.n, gplan::kBigTile);
      p.grid = gplan::round_up(gplan::cdiv(c.m, gplan::kBigTile), 8) * p.nt;
      p.block = 512;
      p.lds = kRingLds;
      // the cross build of the ring: krs_gemm's condition for its epilogue build 1 (bf16 output, vector access everywhere)
      if (c.has_ep && rt.ep_vec && c.out_dtype == KRS_BF16 && c.x0 && !c.r) rt.epilogue = 1;
    } else {
      rt.kernel = KRS_GEMM_Q8_KERNEL_TILE128;
      rt.k_tail = c.k % gplan::kRowBytes != 0;
      p.grid = gplan::round_up(gplan::cdiv(c.m, gplan::kTile), 8) * gplan::cdiv(c.n, gplan::kTile);
      p.lds = kTileLds;
    }
  } else {
    rt.kernel = KRS_GEMM_Q8_KERNEL_GENERIC;
    p.grid = gplan::cdiv(c.m * c.n, 256);
  }
  if (p.grid * p.block > gplan::kMaxGridThreads) return refuse("the shape needs a grid beyond the launch limits (2^32 - 1 threads)");
  return p;
}

}  // namespace q8plan
}  // namespace krs
#endif
