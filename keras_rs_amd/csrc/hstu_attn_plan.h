// Host-side planner of K31 (hstu_attention.hip): which kernel a call runs, its grids, its LDS and the workspace of the
// position-bias gradient.  Plain C++17 with no HIP header, so it can be compiled and checked on a CPU.
#ifndef KRS_HSTU_ATTN_PLAN_H_
#define KRS_HSTU_ATTN_PLAN_H_

#include <stddef.h>
#include <stdint.h>

namespace krs {
namespace hstu {

constexpr int kOwnRows = 128;      // owner rows of a fast-route workgroup: 4 waves x 32
constexpr int kTile = 32;          // streamed rows per step (one MFMA block)
constexpr int kWindow = 160;       // bias entries of one step: 128 owners against 32 streamed rows span 159 offsets
constexpr int kMaxL = 4096;        // the generic kernels keep one row of weights in LDS
constexpr int kMaxDh = 256;
constexpr int kFastMaxDh = 128;
constexpr int kBinChunk = 64;      // offsets of one workgroup of the generic dpos sweep and of the reduce
constexpr int64_t kMaxGroups = 2147483647;   // grid.x

// (the values of KRS_HSTU_ATTN_* and krs_dtype in include/krs.h)
enum { kRouteNone = 0, kRouteFast = 1, kRouteGeneric = 2 };
enum { kF32 = 0, kBF16 = 1 };
enum { kOk = 0, kInvalid = -1, kUnsupported = -2 };

struct Plan {
  int status = kOk;         // kOk, kInvalid or kUnsupported
  const char* why = "";     // the limit a refusal names
  int kernel = kRouteNone;  // kRouteNone after a refusal or a no-op (b == 0 or l == 0)
  int dpad = 0;             // fast: 32, 64 or 128; generic: 0
  int vec = 0;              // fast: rows are whole 16-byte chunks on 16-byte boundaries
  int64_t oblocks = 0;      // fast: workgroups along the owner side of one (b, h); generic: 1
  int64_t groups = 0;       // workgroups of each sweep
  int lds_static = 0;       // LDS of the sweeps without the dpos tables
  int lds_dpos = 0;         // fast: dynamic LDS of the key-owner sweep when dpos is wanted (exchange tiles + bins)
  // dpos: one partial table of `bins` floats per `parts` workgroups, added in index order by the reduce launch
  int64_t bins = 0, parts = 0, dpos_groups = 0, reduce_groups = 0;
};

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// LDS of attn_kernel<DPAD>: two double-buffered tiles, the streamed rows' validity and the bias window
inline int fast_lds_static(int dpad) { return 4 * kTile * dpad * 2 + 2 * kTile * 4 + 2 * kWindow * 4; }
// bins of a fast-route workgroup: offsets i - j of 128 keys against whole query tiles, see hstu_attention.hip
inline int64_t fast_bins(int64_t l) { return cdiv(l, kTile) * kTile + kOwnRows; }
inline int fast_lds_dpos(int64_t l) { return (int)((4 * kTile * kTile + fast_bins(l)) * 4); }
// the widest generic kernel (dk / dv): two rows of dh floats and two of l floats at their limits
constexpr int kGenericLds = (2 * kMaxDh + 2 * kMaxL) * 4;

// `aligned`: every operand base is on 16 bytes and every token stride is a multiple of 8 elements (the caller reads
// the pointer VALUES; the planner never sees memory).  hb: rows of the position table, 0 when there is none.
inline Plan plan(int64_t b, int64_t h, int64_t l, int64_t dh, int dtype, bool aligned, int64_t hb) {
  Plan pl;
  if (b < 0 || h < 1 || l < 0 || dh < 1) {
    pl.status = kInvalid, pl.why = "b >= 0, h >= 1, l >= 0, dh >= 1";
    return pl;
  }
  if (dtype != kF32 && dtype != kBF16) {
    pl.status = kInvalid, pl.why = "dtype is KRS_F32 or KRS_BF16";
    return pl;
  }
  if (hb != 0 && hb != 1 && hb != h) {
    pl.status = kInvalid, pl.why = "hb is 1 or h (0 without a position table)";
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
    pl.lds_static = fast_lds_static(pl.dpad);
    if (hb) {
      pl.lds_dpos = fast_lds_dpos(l);
      pl.bins = fast_bins(l);
      pl.parts = pl.groups;
    }
  } else {
    pl.kernel = kRouteGeneric;   // fp32 at any dh, bf16 above 128: fp32 FMA, one workgroup per (b, h, row)
    pl.oblocks = 1;
    pl.groups = b * h * l;
    pl.lds_static = kGenericLds;
    if (hb) {
      pl.bins = 2 * l - 1;
      pl.parts = b * h;
      pl.dpos_groups = b * h * cdiv(pl.bins, kBinChunk);
    }
  }
  if (hb) pl.reduce_groups = hb * cdiv(2 * l - 1, kBinChunk);
  return pl;
}

inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }
// backward with dpos: the partial tables, fp32 [parts, bins].  Nothing else is kept: the forward needs none.
inline size_t workspace_bytes(const Plan& pl) {
  return pl.status == kOk ? align256((size_t)pl.parts * (size_t)pl.bins * sizeof(float)) : 0;
}

}  // namespace hstu
}  // namespace krs
#endif
