// Host-side planner of K20 (gru.hip): which kernel a call runs, its grid, its LDS.  Plain C++ with no device code, so
// it can be compiled and checked on a CPU (tests/host/gru_plan_check.cpp).
#ifndef KRS_GRU_PLAN_H_
#define KRS_GRU_PLAN_H_

#include <stddef.h>
#include <stdint.h>

namespace krs {
namespace gru {

constexpr int kFastRows = 32;      // batch rows of a fast-path workgroup: one MFMA block
constexpr int kFastMaxU = 128;
constexpr int kGenRows = 4;        // batch rows of a generic workgroup
constexpr int kGenThreads = 256;
constexpr int kMaxU = 1024;
constexpr int kPadBytes = 16;      // per LDS row of the fast path: 16-byte reads of 16 rows then cover all 64 banks
constexpr int64_t kLdsLimit = 160 * 1024;
constexpr int64_t kMaxGroups = 2147483647;   // grid.x

// (the values of KRS_GRU_* and krs_dtype in include/krs.h)
enum { kRouteNone = 0, kRouteFast = 1, kRouteGeneric = 2 };
enum { kF32 = 0, kBF16 = 1 };
enum { kOk = 0, kInvalid = -1, kUnsupported = -2 };

struct Plan {
  int status = kOk;         // kOk, kInvalid or kUnsupported
  const char* why = "";     // the limit a refusal names
  int kernel = kRouteNone;  // kRouteNone after a refusal or a no-op (b == 0 or l == 0)
  int upad = 0;             // fast: 32, 64 or 128; generic: 0
  int rows = 0;             // batch rows of one workgroup
  int threads = 0;          // fast: one wave per 32 units of upad; generic: 256
  int64_t groups = 0;       // workgroups of each sweep
  int64_t lds_fwd = 0;      // dynamic LDS bytes of the forward sweep
  int64_t lds_bwd = 0;      // ... of the backward sweep
};

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// fast path LDS: the recurrent kernel as bf16, 3 * upad rows of upad (forward: row = gate column, k contiguous) or upad
// rows of 3 * upad (backward: row = unit, gate columns contiguous), each row padded by kPadBytes; then the double-buffered
// A operand: 32 rows of upad (forward: h) or of 3 * upad (backward: da).
inline int64_t fast_lds_fwd(int upad) {
  return (int64_t)3 * upad * (upad * 2 + kPadBytes) + (int64_t)2 * kFastRows * (upad * 2 + kPadBytes);
}
inline int64_t fast_lds_bwd(int upad) {
  return (int64_t)upad * (3 * upad * 2 + kPadBytes) + (int64_t)2 * kFastRows * (3 * upad * 2 + kPadBytes) +
         (int64_t)kFastRows * sizeof(int);
}
// generic path LDS, fp32: forward h [2][rows][u]; backward dh [rows][u] + da [rows][3u] + first [rows]
inline int64_t gen_lds_fwd(int64_t u) { return (int64_t)2 * kGenRows * u * 4; }
inline int64_t gen_lds_bwd(int64_t u) { return (int64_t)4 * kGenRows * u * 4 + kGenRows * (int64_t)sizeof(int); }

inline Plan plan(int64_t b, int64_t l, int64_t u, int dtype) {
  Plan pl;
  if (b < 0 || l < 0 || u < 1) {
    pl.status = kInvalid, pl.why = "b >= 0, l >= 0, u >= 1";
    return pl;
  }
  if (dtype != kF32 && dtype != kBF16) {
    pl.status = kInvalid, pl.why = "dtype is KRS_F32 or KRS_BF16";
    return pl;
  }
  if (u > kMaxU) {
    pl.status = kUnsupported, pl.why = "u <= 1024";
    return pl;
  }
  if (l > kMaxGroups || cdiv(b, kGenRows) > kMaxGroups) {
    pl.status = kUnsupported, pl.why = "b / 4 and l <= 2^31 - 1";
    return pl;
  }
  if (b == 0 || l == 0) return pl;
  if (dtype == kBF16 && u <= kFastMaxU) {
    pl.kernel = kRouteFast;
    pl.upad = u <= 32 ? 32 : u <= 64 ? 64 : 128;
    pl.rows = kFastRows;
    pl.threads = 2 * pl.upad;
    pl.lds_fwd = fast_lds_fwd(pl.upad);
    pl.lds_bwd = fast_lds_bwd(pl.upad);
  } else {
    pl.kernel = kRouteGeneric;   // fp32 at any u, bf16 above 128: fp32 FMA, the state in LDS
    pl.rows = kGenRows;
    pl.threads = kGenThreads;
    pl.lds_fwd = gen_lds_fwd(u);
    pl.lds_bwd = gen_lds_bwd(u);
  }
  pl.groups = cdiv(b, pl.rows);
  return pl;
}

// the reserve: z, r, c, q of every step in the compute dtype, [b, l, 4u]
inline size_t reserve_bytes(int64_t b, int64_t l, int64_t u, int dtype) {
  if (b <= 0 || l <= 0 || u <= 0) return 0;
  return (size_t)b * (size_t)l * 4u * (size_t)u * (dtype == kBF16 ? 2u : 4u);
}

}  // namespace gru
}  // namespace krs
#endif
