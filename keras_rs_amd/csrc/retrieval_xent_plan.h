// Host-side geometry of K13 (retrieval_xent.hip): how the streamed side of a sweep is cut into slices and how much
// workspace the per-slice partials take.  Plain C++ with no device code, so it can be compiled and checked on a CPU.
#ifndef KRS_RETRIEVAL_XENT_PLAN_H_
#define KRS_RETRIEVAL_XENT_PLAN_H_

#include <stddef.h>
#include <stdint.h>

namespace krs {
namespace xent {

constexpr int kOwnRows = 128;        // owner rows of a workgroup: 4 waves x 32
constexpr int kTile = 32;            // streamed rows per step (one MFMA block)
constexpr int kTargetGroups = 512;   // workgroups wanted: two per CU
constexpr int kMinSlice = 64;        // shortest slice once the target is met (two steps)
constexpr int kMaxSlices = 1024;
constexpr int kMaxD = 256;

struct Sweep {
  int64_t oblocks;   // workgroups along the owner side
  int S;             // slices of the streamed side
  int64_t slice;     // streamed rows per slice (a multiple of kTile)
};

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// A sweep of `owner` rows against `streamed` rows.  The slice count depends on (b, n) alone; it is capped so that
// S * owner rows stays below 8 (b + n): the fp32 partials [S, owner, d] of one gradient then take at most
// 8 (b + n) d floats, those of both gradients 16 (b + n) d.
inline Sweep plan_sweep(int64_t owner, int64_t streamed, int64_t b, int64_t n) {
  Sweep sw;
  sw.oblocks = cdiv(owner, kOwnRows);
  int64_t s = cdiv(kTargetGroups, sw.oblocks);
  if (s > cdiv(streamed, kMinSlice)) s = cdiv(streamed, kMinSlice);
  if (s > 8 * (b + n) / owner) s = 8 * (b + n) / owner;
  if (s > kMaxSlices) s = kMaxSlices;
  if (s < 1) s = 1;
  sw.slice = cdiv(cdiv(streamed, s), kTile) * kTile;
  sw.S = (int)cdiv(streamed, sw.slice);
  return sw;
}

inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }

// forward: (m, Z, S, A) per slice and query;  gradients: fp32 [S, rows, d] per side that is split
inline size_t fwd_bytes(int64_t b, int64_t n) {
  const Sweep q = plan_sweep(b, n, b, n);
  return q.S > 1 ? align256((size_t)q.S * (size_t)b * 4 * sizeof(float)) : 0;
}
inline size_t dq_bytes(int64_t b, int64_t n, int64_t d) {
  const Sweep q = plan_sweep(b, n, b, n);
  return q.S > 1 ? align256((size_t)q.S * (size_t)b * (size_t)d * sizeof(float)) : 0;
}
inline size_t dc_bytes(int64_t b, int64_t n, int64_t d) {
  const Sweep c = plan_sweep(n, b, b, n);
  return c.S > 1 ? align256((size_t)c.S * (size_t)n * (size_t)d * sizeof(float)) : 0;
}
// K15 (krs_retrieval_rank): the positives' scores [b] fp32, then the slices' counts [S, b] int32 when the sweep is
// cut.  S b <= 8 (b + n), so this is at most 4 b + 32 (b + n) + 512 bytes.
inline size_t rank_pos_bytes(int64_t b) { return align256((size_t)b * sizeof(float)); }
inline size_t rank_bytes(int64_t b, int64_t n) {
  const Sweep q = plan_sweep(b, n, b, n);
  return rank_pos_bytes(b) + (q.S > 1 ? align256((size_t)q.S * (size_t)b * sizeof(int32_t)) : 0);
}
inline size_t workspace_bytes(int64_t b, int64_t n, int64_t d) {
  const size_t f = fwd_bytes(b, n), g = dq_bytes(b, n, d) + dc_bytes(b, n, d);
  return f > g ? f : g;
}

}  // namespace xent
}  // namespace krs
#endif
