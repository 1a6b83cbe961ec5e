// The route of krs_regression_fwd_bwd (regression.hip) as a pure function of the call: vector or element kernel, the
// rows of an item, the workgroups and the launches.  Plain C++17 on krs.h, no HIP header:
// tests/host/regression_plan_check.cpp walks it under the sanitizers and krs_regression_plan_route answers from it
// without a GPU.  Device pointers are read as VALUES (nullness, alignment).  A plan guarantees (the walk asserts it):
//   * 1 <= blocks <= KRS_REGRESSION_MAX_BLOCKS, and blocks * THREADS < items + THREADS unless items == 0 (no workgroup
//     without an item, but for the one workgroup of a vector call of fewer than v rows);
//   * the vector route only when one row is one element and every operand can move in 16 bytes;
//   * launches = [W pass] + main + [finish when blocks > 1].
#ifndef KRS_REGRESSION_PLAN_H_
#define KRS_REGRESSION_PLAN_H_

#include <cstddef>
#include <cstdint>

#include "../../include/krs.h"

namespace krs {
namespace regr {

constexpr int64_t kMaxSize = 2147483647;   // rows and columns are ints of the kernels
constexpr int kSums = 4;                   // T, sum q, sum a, sum w: the partials of the main pass

struct Call {
  int reduction = KRS_REGRESSION_SUM_OVER_BATCH_SIZE;
  int dtype = KRS_F32;
  int64_t b = 0, c = 1;
  int64_t ld_pred = 1, ld_target = 1, ld_dpred = 1;
  const void* pred = nullptr;
  const void* target = nullptr;
  const void* weight = nullptr;
  const void* g = nullptr;
  const void* loss = nullptr;
  const void* dpred = nullptr;
};

struct Plan {
  int status = KRS_OK;                // KRS_OK or KRS_ERR_INVALID
  const char* why = "";
  krs_regression_route route = {};    // all zero after a refusal or when b == 0
  bool w_pass = false;                // W = sum of the weights is taken before the main pass
  int w_blocks = 0;                   // its workgroups
  int64_t items = 0, tail = 0;        // items of the main pass; rows after the last full vector item
};

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int vec_rows(int dtype) { return dtype == KRS_BF16 ? 8 : 4; }
inline bool on16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline int blocks_for(int64_t items) {
  const int64_t g = cdiv(items, KRS_REGRESSION_THREADS);
  return (int)(g < 1 ? 1 : (g > KRS_REGRESSION_MAX_BLOCKS ? KRS_REGRESSION_MAX_BLOCKS : g));
}

inline Plan plan(const Call& c) {
  Plan pl;
  auto refuse = [&](const char* why) {
    pl.status = KRS_ERR_INVALID, pl.why = why;
    return pl;
  };
  if (c.reduction < KRS_REGRESSION_NONE || c.reduction > KRS_REGRESSION_MEAN_WITH_SAMPLE_WEIGHT) return refuse("reduction");
  if (c.dtype != KRS_F32 && c.dtype != KRS_BF16) return refuse("dtype");
  if (c.b < 0 || c.b > kMaxSize) return refuse("b");
  if (c.c < 1 || c.c > kMaxSize) return refuse("c");
  if (c.ld_pred < c.c) return refuse("ld_pred");
  if (c.ld_target < c.c) return refuse("ld_target");
  if (c.dpred && c.ld_dpred < c.c) return refuse("ld_dpred");
  if (c.b == 0) return pl;
  if (!c.pred || !c.target) return refuse("null operand");
  const bool vec = c.c == 1 && c.ld_pred == 1 && c.ld_target == 1 && (!c.dpred || c.ld_dpred == 1) && on16(c.pred) &&
                   on16(c.target) && on16(c.weight) && on16(c.g) && on16(c.dpred) &&
                   (c.reduction != KRS_REGRESSION_NONE || on16(c.loss));
  const int v = vec ? vec_rows(c.dtype) : 1;
  pl.items = c.b / v;
  pl.tail = c.b % v;
  pl.route.kernel = vec ? KRS_REGRESSION_VEC : KRS_REGRESSION_ELEM;
  pl.route.v = v;
  pl.route.blocks = blocks_for(pl.items);
  pl.w_pass = c.reduction == KRS_REGRESSION_MEAN_WITH_SAMPLE_WEIGHT && c.weight;
  pl.w_blocks = pl.w_pass ? blocks_for(c.b) : 0;
  pl.route.launches = (pl.w_pass ? 1 : 0) + 1 + (pl.route.blocks > 1 ? 1 : 0);
  return pl;
}

// W partials, then kSums rows of partials of the main pass
inline size_t workspace_bytes(int64_t b, int64_t c) {
  if (b <= 0 || c <= 0) return 0;
  return (size_t)(1 + kSums) * KRS_REGRESSION_MAX_BLOCKS * sizeof(float);
}

}  // namespace regr
}  // namespace krs
#endif
