// Host-side planner of K28 (ranking_lambda.hip): the dynamic LDS of a launch and where each buffer lies in it.  Plain
// C++ (constexpr, no device code): the launch sizes the allocation by it and the kernel takes its offsets from it.
#ifndef KRS_RANKING_LAMBDA_PLAN_H_
#define KRS_RANKING_LAMBDA_PLAN_H_

#include <stdint.h>

namespace krs {
namespace lambda_rank {

constexpr int kThreads = 1024;             // krs_list.h's kListThreads
constexpr int kMaxList = 4096;             // KRS_RANK_MAX_LIST
constexpr int64_t kLdsLimit = 160 * 1024;  // LDS of a gfx950 compute unit

struct Layout {
  int64_t keys;    // uint64 [slots]: the sort keys; afterwards the gain keys, then the float2 tails of the cut rows
  int64_t recs;    // float4 [slots]: {s, y, g, G} in rank order
  int64_t dcut;    // float [list]: D_cut(p + 1)
  int64_t rtab;    // float [list]: smooth_fraction * R(d), only when smooth
  int64_t total;   // bytes
};

// sort slots of a workgroup: kThreads / P lists of P = pow2 >= list slots each, or one longer list
inline constexpr int64_t slots(int list) {
  int64_t p = 1;
  while (p < list) p <<= 1;
  return p < kThreads ? kThreads : p;
}

inline constexpr Layout layout(int list, bool smooth) {
  const int64_t n = slots(list), table = ((int64_t)list * 4 + 15) / 16 * 16;
  Layout l{};
  l.keys = 0;
  l.recs = n * 8;
  l.dcut = l.recs + n * 16;
  l.rtab = l.dcut + table;
  l.total = l.rtab + (smooth ? table : 0);
  return l;
}

static_assert(layout(1, false).total == 24 * 1024 + 16, "short lists: 1024 slots and one table row");
static_assert(layout(1024, true).total == 32 * 1024, "1024 items: 24 KB of slots, two 4 KB tables");
static_assert(layout(kMaxList, true).total == 128 * 1024 && layout(kMaxList, true).total <= kLdsLimit,
              "4096 items: keys 32 KB, records 64 KB, two 16 KB tables");

}  // namespace lambda_rank
}  // namespace krs
#endif
