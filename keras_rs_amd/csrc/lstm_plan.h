// Host-side planner of K25 (lstm.hip): which kernel a call runs, its grid, its LDS, and the bytes of the reserve.  Plain
// C++ with no device code, so it can be compiled and checked on a CPU (tests/host/lstm_plan_check.cpp).
#ifndef KRS_LSTM_PLAN_H_
#define KRS_LSTM_PLAN_H_

#include <stddef.h>
#include <stdint.h>

namespace krs {
namespace lstm {

constexpr int kFastRows = 32;      // batch rows of a fast-path workgroup: one MFMA block
constexpr int kFastMaxU = 128;
constexpr int kGenRows = 4;        // batch rows of a generic workgroup
constexpr int kGenThreads = 256;
constexpr int kMaxU = 1024;
constexpr int kPadBytes = 16;      // per LDS row of the fast path: 16-byte reads of 16 rows then cover all 64 banks
constexpr int64_t kLdsLimit = 160 * 1024;
constexpr int64_t kMaxGroups = 2147483647;   // grid.x

// (the values of KRS_LSTM_* and krs_dtype in include/krs.h)
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
  int bwd_kernel_vgprs = 0; // fast: registers a lane spends on its share of the recurrent kernel in the backward sweep
};

inline constexpr int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Fast path, forward: the recurrent kernel as bf16, 4 * upad rows (row = gate column, k contiguous) of upad, each row
// padded by kPadBytes; then the double-buffered A operand, h as bf16: 2 x 32 rows of upad.
inline constexpr int64_t fast_lds_fwd(int upad) {
  return (int64_t)4 * upad * (upad * 2 + kPadBytes) + (int64_t)2 * kFastRows * (upad * 2 + kPadBytes);
}
// Fast path, backward: the recurrent kernel is NOT in LDS.  Wave w holds rows 32 w .. 32 w + 31 of it (the B operand of
// da . U^T for the units it owns) in registers: 4 * upad gate columns of bf16 per row, half a row per lane, which is
// upad VGPRs a lane.  LDS holds the double-buffered A operand, da as bf16 (2 x 32 rows of 4 * upad), and the first
// valid step of the 32 rows.  (K20's layout -- the kernel AND da in LDS -- would need 199 680 B at upad = 128.)
inline constexpr int64_t fast_lds_bwd(int upad) {
  return (int64_t)2 * kFastRows * (4 * upad * 2 + kPadBytes) + (int64_t)kFastRows * (int64_t)sizeof(int);
}
inline constexpr int fast_bwd_kernel_vgprs(int upad) { return 4 * upad * 2 / 2 / 4; }
// generic path LDS, fp32: forward h [2][rows][u] + c [rows][u]; backward dh + dc [rows][u] each, da [rows][4u], first
inline constexpr int64_t gen_lds_fwd(int64_t u) { return (int64_t)3 * kGenRows * u * 4; }
inline constexpr int64_t gen_lds_bwd(int64_t u) { return (int64_t)6 * kGenRows * u * 4 + kGenRows * (int64_t)sizeof(int); }

static_assert(fast_lds_fwd(128) == 156672 && fast_lds_fwd(128) <= kLdsLimit, "forward at upad = 128: U and 2 x h");
static_assert(fast_lds_bwd(128) == 66688 && fast_lds_bwd(128) <= kLdsLimit, "backward at upad = 128: 2 x da and first");
static_assert(fast_bwd_kernel_vgprs(128) == 128, "backward at upad = 128: half of the 512 VGPRs of a 4-wave workgroup's lane");
static_assert(gen_lds_bwd(kMaxU) <= kLdsLimit && gen_lds_fwd(kMaxU) <= kLdsLimit, "generic at u = 1024");

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
    pl.bwd_kernel_vgprs = fast_bwd_kernel_vgprs(pl.upad);
  } else {
    pl.kernel = kRouteGeneric;   // fp32 at any u, bf16 above 128: fp32 FMA, the states in LDS
    pl.rows = kGenRows;
    pl.threads = kGenThreads;
    pl.lds_fwd = gen_lds_fwd(u);
    pl.lds_bwd = gen_lds_bwd(u);
  }
  pl.groups = cdiv(b, pl.rows);
  return pl;
}

// The reserve, one block per token (token (bi, t) at block bi * l + t).  bf16: i [u] and g [u] as bf16, then f [u],
// o [u] and the carried cell state c [u] as fp32 -- 16 u bytes; a gate near 1 stored as bf16 would lose its 1 - gate,
// which the backward multiplies by (f (1 - f), o (1 - o)), and c is carried over many steps.  fp32: i, g, f, o, c as
// fp32 -- 20 u bytes.
inline constexpr int64_t reserve_token_bytes(int64_t u, int dtype) { return (dtype == kBF16 ? 16 : 20) * u; }
inline size_t reserve_bytes(int64_t b, int64_t l, int64_t u, int dtype) {
  if (b <= 0 || l <= 0 || u <= 0) return 0;
  return (size_t)b * (size_t)l * (size_t)reserve_token_bytes(u, dtype);
}

}  // namespace lstm
}  // namespace krs
#endif
