// Host-side planner of K19 (seq_attention.hip): which kernel a call runs, its grids, its workspace, and the dropout
// hash.  Plain C++ with no device code, so it can be compiled and checked on a CPU (tests/host/seq_attn_plan_check.cpp).
#ifndef KRS_SEQ_ATTN_PLAN_H_
#define KRS_SEQ_ATTN_PLAN_H_

#include <stddef.h>
#include <stdint.h>

namespace krs {
namespace seqattn {

constexpr int kOwnRows = 128;      // owner rows of a fast-path workgroup: 4 waves x 32
constexpr int kTile = 32;          // streamed rows per step (one MFMA block)
constexpr int kMaxL = 4096;        // the generic kernels keep one row of scores in LDS; (i << 12) | j in the hash
constexpr int kMaxDh = 256;
constexpr int kFastMaxDh = 128;
constexpr int64_t kMaxGroups = 2147483647;   // grid.x

// (the values of KRS_SEQ_ATTN_* and krs_dtype in include/krs.h)
enum { kRouteNone = 0, kRouteFast = 1, kRouteGeneric = 2 };
enum { kF32 = 0, kBF16 = 1 };
enum { kOk = 0, kInvalid = -1, kUnsupported = -2 };

struct Plan {
  int status = kOk;         // kOk, kInvalid or kUnsupported
  const char* why = "";     // the limit a refusal names
  int kernel = kRouteNone;  // kRouteNone after a refusal or a no-op (b == 0 or l == 0)
  int dpad = 0;             // fast: 32, 64 or 128; generic: 0
  int vec = 0;              // fast: rows are whole 16-byte chunks on 16-byte boundaries
  int64_t oblocks = 0;      // fast: workgroups along the owner side of one (b, h)
  int64_t groups = 0;       // workgroups of each sweep
};

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// `aligned`: every operand base is on 16 bytes and every token stride is a multiple of 8 elements (the caller reads
// the pointer VALUES; the planner never sees memory).
inline Plan plan(int64_t b, int64_t h, int64_t l, int64_t dh, int dtype, bool aligned) {
  Plan pl;
  if (b < 0 || h < 1 || l < 0 || dh < 1) {
    pl.status = kInvalid, pl.why = "b >= 0, h >= 1, l >= 0, dh >= 1";
    return pl;
  }
  if (dtype != kF32 && dtype != kBF16) {
    pl.status = kInvalid, pl.why = "dtype is KRS_F32 or KRS_BF16";
    return pl;
  }
  if (l > kMaxL) {
    pl.status = kUnsupported, pl.why = "l <= 4096";
    return pl;
  }
  if (dh > kMaxDh) {
    pl.status = kUnsupported, pl.why = "dh <= 256";
    return pl;
  }
  if (b > kMaxGroups || h > kMaxGroups || b * h > kMaxGroups || b * h * l > kMaxGroups) {
    pl.status = kUnsupported, pl.why = "b * h * l <= 2^31 - 1 (the launch grid)";
    return pl;
  }
  if (b == 0 || l == 0) return pl;
  if (dtype == kBF16 && dh <= kFastMaxDh) {
    pl.kernel = kRouteFast;
    pl.dpad = dh <= 32 ? 32 : dh <= 64 ? 64 : 128;
    pl.vec = aligned && dh % 8 == 0;
    pl.oblocks = cdiv(l, kOwnRows);
    pl.groups = pl.oblocks * b * h;
  } else {
    pl.kernel = kRouteGeneric;   // fp32 at any dh, bf16 above 128: fp32 FMA, one workgroup per (b, h, row)
    pl.groups = b * h * l;
  }
  return pl;
}

inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }
// backward: delta [b, h, l] fp32.  The forward needs none.
inline size_t workspace_bytes(int64_t b, int64_t h, int64_t l) {
  if (b <= 0 || h <= 0 || l <= 0) return 0;
  return align256((size_t)b * (size_t)h * (size_t)l * sizeof(float));
}

// ---- the dropout mask: keep(i, j) <=> hash >= floor(p * 2^32), 32-bit integer operations only (include/krs.h) ----
#if defined(__HIPCC__)
#define KRS_SEQ_HD __host__ __device__ inline
#else
#define KRS_SEQ_HD inline
#endif
KRS_SEQ_HD uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
// bh = b_index * h + h_index
KRS_SEQ_HD uint32_t hash_base(uint32_t seed_lo, uint32_t seed_hi, uint32_t draw_lo, uint32_t draw_hi, uint32_t bh) {
  uint32_t x = mix32(seed_lo ^ 0x9e3779b9u);
  x = mix32(x ^ seed_hi);
  x = mix32(x ^ draw_lo);
  x = mix32(x ^ draw_hi);
  return mix32(x ^ bh);
}
KRS_SEQ_HD uint32_t hash_ij(uint32_t base, uint32_t i, uint32_t j) { return mix32(base + ((i << 12) | j)); }
inline uint32_t drop_threshold(float p) { return (uint32_t)((double)p * 4294967296.0); }

}  // namespace seqattn
}  // namespace krs
#endif
