// Host-side planner of K22 (layer_norm.hip): how a row is laid over the lanes of a wave, whether it moves in 16-byte
// chunks, the launch grid, the rows a workgroup owns and the workspace of the weight-gradient partials.  Plain C++ with
// no device code, so it can be compiled and checked on a CPU (tests/host/ln_plan_check.cpp).  The dropout hash is K19's,
// through its header.
#ifndef KRS_LN_PLAN_H_
#define KRS_LN_PLAN_H_

#include <stddef.h>
#include <stdint.h>

#include "seq_attn_plan.h"

namespace krs {
namespace ln {

using seqattn::drop_threshold;
using seqattn::hash_base;
using seqattn::mix32;

constexpr int kThreads = 256;                // 4 waves of 64
constexpr int kWaves = kThreads / 64;
constexpr int kMaxD = 4096;                  // 64 lanes x 64 fp32 registers hold the row
constexpr int kMinLanes = 8;
constexpr int64_t kMaxN = 2147483647;
constexpr int64_t kMaxGroups = 2048;         // workgroups of a launch = rows of the weight-gradient partials

// (the values of KRS_LN_* and krs_dtype in include/krs.h)
enum { kRouteNone = 0, kRouteVec = 1, kRouteElem = 2 };
enum { kF32 = 0, kBF16 = 1 };
enum { kOk = 0, kInvalid = -1, kUnsupported = -2 };

struct Plan {
  int status = kOk;          // kOk, kInvalid or kUnsupported
  const char* why = "";      // the limit a refusal names
  int kernel = kRouteNone;   // kRouteNone after a refusal or a no-op (n == 0)
  int lanes_per_row = 0;     // 8, 16, 32 or 64 lanes of one wave own a row
  int per_lane = 0;          // fp32 registers a lane keeps of its row: 8 below 64 lanes, else 8, 16, 32 or 64
  int vec = 0;               // 1: 16 bytes per lane per access
  int rows_per_pass = 0;     // rows a workgroup has in flight: 256 / lanes_per_row
  int64_t rows_per_group = 0;  // the contiguous rows a workgroup owns: a multiple of rows_per_pass
  int64_t groups = 0;        // workgroups of the row kernels, and rows of the partials
};

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// The smallest of 8, 16, 32, 64 lanes that holds the row at 8 elements a lane; past 512 columns the lanes hold more.
inline int lanes_of(int64_t d) { return d <= 64 ? 8 : d <= 128 ? 16 : d <= 256 ? 32 : 64; }
inline int per_lane_of(int64_t d) { return d <= 512 ? 8 : d <= 1024 ? 16 : d <= 2048 ? 32 : 64; }

// `aligned`: every matrix base is on 16 bytes and every row stride is a whole number of 16-byte chunks (the caller
// reads the pointer VALUES; the planner never sees memory).
inline Plan plan(int64_t n, int64_t d, int dtype, bool aligned) {
  Plan pl;
  if (n < 0 || d < 1) {
    pl.status = kInvalid, pl.why = "n >= 0, d >= 1";
    return pl;
  }
  if (dtype != kF32 && dtype != kBF16) {
    pl.status = kInvalid, pl.why = "dtype is KRS_F32 or KRS_BF16";
    return pl;
  }
  if (d > kMaxD) {
    pl.status = kUnsupported, pl.why = "d <= 4096 (the row lives in a wave's registers)";
    return pl;
  }
  if (n > kMaxN) {
    pl.status = kUnsupported, pl.why = "n <= 2^31 - 1";
    return pl;
  }
  if (n == 0) return pl;
  const int chunk = dtype == kBF16 ? 8 : 4;   // elements of 16 bytes
  pl.vec = aligned && d % chunk == 0;
  pl.kernel = pl.vec ? kRouteVec : kRouteElem;
  pl.lanes_per_row = lanes_of(d);
  pl.per_lane = per_lane_of(d);
  pl.rows_per_pass = kThreads / pl.lanes_per_row;
  const int64_t passes = cdiv(n, (int64_t)pl.rows_per_pass * kMaxGroups);
  pl.rows_per_group = passes * pl.rows_per_pass;
  pl.groups = cdiv(n, pl.rows_per_group);
  return pl;
}

inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }
// backward with dgamma or dbeta: one fp32 row of d for each, per workgroup.  The forward needs none.
inline size_t workspace_bytes(int64_t n, int64_t d) {
  const Plan pl = plan(n, d, kF32, false);
  if (pl.status != kOk || pl.groups == 0) return 0;
  return align256((size_t)pl.groups * 2u * (size_t)d * sizeof(float));
}

}  // namespace ln
}  // namespace krs
#endif
