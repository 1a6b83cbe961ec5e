// The row walk of the dense elementwise kernels (cross_epilogue.hip: cross_fwd_*, cross_bwd_*, colsum_kernel;
// dense_aux.hip: dense_act_bwd_*) as a pure function of the call: vector or scalar kernel, the columns a thread owns,
// the row chunks, the grid and whether the column sums go through the workspace.  Plain C++17 on krs.h, no HIP header:
// tests/host/dense_walk_plan_check.cpp walks it under the sanitizers and krs_dense_walk_plan_route answers from it
// without a GPU.  krs_cross_epilogue_fwd / _bwd, krs_dense_act_bwd and krs_colsum plan here and launch what the plan
// names; krs_colsum_workspace_bytes is the largest grid_y * n of the routes a shape can take.  Device pointers are read
// as VALUES (nullness, alignment).  A plan guarantees (the walk asserts it):
//   * rows_per_block * chunks >= m > rows_per_block * (chunks - 1): every row is in exactly one chunk, none is empty;
//   * grid_y * 4 >= chunks on the vector kernels (a wave per chunk), grid_y == chunks on the scalar ones;
//   * strips * 64 * v >= n > (strips - 1) * 64 * v;
//   * chunks <= ceil(4096 / strips): enough workgroups to fill the chip, few enough to keep the second stage cheap.
#ifndef KRS_DENSE_WALK_PLAN_H_
#define KRS_DENSE_WALK_PLAN_H_

#include <cstddef>
#include <cstdint>

#include "../../include/krs.h"

namespace krs {
namespace dwalk {

constexpr int64_t kTargetBlocks = 4096;         // strips * chunks aims at this many chunks of work
constexpr int64_t kMaxM = 2147483647;           // rows_per_block is an int of the kernels
constexpr int kWavesPerGroup = 4;               // vector kernels: 256 threads, one chunk per wave

struct Call {
  int entry = KRS_DENSE_WALK_CROSS_BWD;
  int64_t m = 0, n = 0;
  int dtype = KRS_F32;
  const int64_t* ld = nullptr;        // leading dimensions of the non-null matrices (all of them must be >= n)
  int n_ld = 0;
  const void* const* ptrs = nullptr;  // the matrix operands; NULL entries take no part
  int n_ptrs = 0;
  bool want_dbias = false;            // column sums are asked for (krs_colsum: always)
  bool has_workspace = false;
  bool dx0_accumulate = false;        // cross backward: dx0 != NULL and the flag set
};

struct Plan {
  int status = KRS_OK;                // KRS_OK, KRS_ERR_INVALID or KRS_ERR_UNSUPPORTED
  const char* why = "";
  krs_dense_walk_route route = {};    // all zero ("none") after a refusal or when m == 0 or n == 0
};

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int vec_width(int dtype) { return dtype == KRS_BF16 ? 8 : 4; }   // elements of 16 bytes

// the chunks and the grid of an [m, n] walk at v columns a thread (m, n > 0; v > 1 needs n % v == 0)
inline krs_dense_walk_route walk(int64_t m, int64_t n, int v) {
  krs_dense_walk_route r = {};
  r.kernel = v > 1 ? KRS_DENSE_WALK_VEC : KRS_DENSE_WALK_SCALAR;
  r.v = v;
  r.strips = cdiv(n / v, 64);
  int64_t chunks = cdiv(kTargetBlocks, r.strips);
  if (chunks > m) chunks = m;
  r.rows_per_block = (int32_t)cdiv(m, chunks);
  r.chunks = cdiv(m, r.rows_per_block);
  r.grid_y = v > 1 ? cdiv(r.chunks, kWavesPerGroup) : r.chunks;
  return r;
}

inline bool vec_ok(const Call& c, int v) {
  if (c.n % v) return false;
  for (int i = 0; i < c.n_ld; ++i)
    if (c.ld[i] % v) return false;
  for (int i = 0; i < c.n_ptrs; ++i)
    if (c.ptrs[i] && (reinterpret_cast<uintptr_t>(c.ptrs[i]) & 15u)) return false;
  return true;
}

inline Plan plan(const Call& c) {
  Plan pl;
  if (c.entry < KRS_DENSE_WALK_CROSS_FWD || c.entry > KRS_DENSE_WALK_COLSUM) {
    pl.status = KRS_ERR_INVALID, pl.why = "unknown entry";
    return pl;
  }
  bool sizes = c.m >= 0 && c.n >= 0 && c.n_ld >= 0 && c.n_ptrs >= 0 && (c.n_ld == 0 || c.ld) && (c.n_ptrs == 0 || c.ptrs);
  for (int i = 0; sizes && i < c.n_ld; ++i) sizes = c.ld[i] >= c.n;
  if (!sizes) {
    pl.status = KRS_ERR_INVALID, pl.why = "bad sizes";
    return pl;
  }
  if (c.dtype != KRS_F32 && c.dtype != KRS_BF16) {
    pl.status = KRS_ERR_INVALID, pl.why = "dtype must be f32 or bf16";
    return pl;
  }
  if (c.m > kMaxM) {
    pl.status = KRS_ERR_UNSUPPORTED, pl.why = "m <= 2^31 - 1";
    return pl;
  }
  if (c.m == 0 || c.n == 0) return pl;
  const int v = vec_width(c.dtype);
  const bool vec = c.entry != KRS_DENSE_WALK_COLSUM && vec_ok(c, v);
  if (c.entry == KRS_DENSE_WALK_CROSS_FWD) {    // a grid-stride pass: no chunks
    pl.route.kernel = vec ? KRS_DENSE_WALK_VEC : KRS_DENSE_WALK_SCALAR;
    pl.route.v = vec ? v : 1;
    return pl;
  }
  pl.route = walk(c.m, c.n, vec ? v : 1);
  pl.route.two_stage = (c.want_dbias || c.entry == KRS_DENSE_WALK_COLSUM) && c.has_workspace;
  pl.route.acc = c.entry == KRS_DENSE_WALK_CROSS_BWD && vec && c.dx0_accumulate;
  return pl;
}

// partial sums of the two-stage column sums: grid_y rows of n floats, for the widest of the routes [m, n] can take
// (the alignment of the operands, which the caller of this function has not got, decides between them)
inline size_t workspace_bytes(int64_t m, int64_t n) {
  if (m <= 0 || n <= 0 || m > kMaxM) return 0;
  int64_t g = walk(m, n, 1).grid_y;
  for (int v : {4, 8})
    if (n % v == 0) {
      const int64_t gv = walk(m, n, v).grid_y;
      if (gv > g) g = gv;
    }
  return (size_t)g * (size_t)n * sizeof(float);
}

}  // namespace dwalk
}  // namespace krs
#endif
