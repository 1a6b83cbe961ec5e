// The route of krs_sampled_softmax_fwd_bwd (sampled_softmax.hip, K30) as a pure function of the call: the route, DPAD,
// vector or element loads, the two grids, the token splits of the negatives sweep, the launches and the workspace
// layout.  Plain C++17 on krs.h, no HIP header: krs_sampled_softmax_plan_route answers from it without a GPU and
// tests/host/sampled_softmax_plan_check.cpp walks it under the sanitizers.  Pointers are read as VALUES.
// A plan guarantees:
//   * fast exactly when emb is bf16 and d <= 128, with DPAD the smallest of 32, 64, 128 that holds d;
//   * vec only when every 8-column chunk of an emb row and of a table row is one whole 16-byte piece;
//   * grid_tokens = g * ceil(lg / 128) (fast) or t (generic): one loss partial each;
//   * grid_negs = g * ceil(n / 128) * splits (fast) or g * n (generic);
//   * splits * split_tiles >= ceil(lg / 32) > (splits - 1) * split_tiles: no split without a token tile;
//   * the workspace pieces do not overlap and end at workspace_bytes.
#ifndef KRS_SAMPLED_SOFTMAX_PLAN_H_
#define KRS_SAMPLED_SOFTMAX_PLAN_H_

#include <cstddef>
#include <cstdint>

#include "../../include/krs.h"

namespace krs {
namespace ssm {

constexpr int64_t kMaxCount = 2147483647;
constexpr int kOwn = KRS_SAMPLED_SOFTMAX_OWN_ROWS;
constexpr int kTile = KRS_SAMPLED_SOFTMAX_TILE;
constexpr int kThreads = 256;
constexpr int64_t kWantGroups = 256;      // workgroups the negatives sweep asks for before it stops splitting: one per CU

struct Call {
  const void* emb = nullptr;
  int64_t ld_emb = 0;
  int emb_dtype = KRS_F32;
  const void* table = nullptr;
  int64_t ld_table = 0;
  int table_dtype = KRS_F32;
  int64_t vocab = 0;
  const void* pos = nullptr;
  const void* neg = nullptr;
  int itype = KRS_I32;
  const void* weight = nullptr;
  const void* pos_logq = nullptr;
  const void* neg_logq = nullptr;
  int64_t t = 0, g = 0, n = 0, d = 0;
  const void* lse = nullptr;
  const void* gpos = nullptr;
  const void* demb = nullptr;
  int64_t ld_demb = 0;
  const void* dneg = nullptr;
};

struct Plan {
  int status = KRS_OK;                     // KRS_OK or KRS_ERR_INVALID
  const char* why = "";                    // the limit a refusal names
  krs_sampled_softmax_route route = {};    // all zero after a refusal or when t == 0
  int64_t lg = 0;                          // tokens of a group
  int w_blocks = 0;                        // workgroups of the W pass (0 without weights)
  // workspace, in floats from its start: W partials, c [t], loss partials [grid_tokens], dneg partials
  size_t off_c = 0, off_loss = 0, off_dneg = 0, floats = 0;
};

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline bool on16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool stride16(int64_t ld, int dtype) { return ld % (dtype == KRS_BF16 ? 8 : 4) == 0; }
inline bool fast_route(int64_t d, int emb_dtype) {
  return emb_dtype == KRS_BF16 && d <= KRS_SAMPLED_SOFTMAX_FAST_MAX_DIM;
}

// the shape's part of a plan (no pointer is read): what the workspace depends on
inline void shape(Plan& pl, int64_t t, int64_t g, int64_t n, int64_t d, int emb_dtype) {
  const int64_t lg = t / g;
  pl.lg = lg;
  if (fast_route(d, emb_dtype)) {
    const int64_t tiles = cdiv(lg, kTile), base = g * cdiv(n, kOwn);
    int64_t splits = kWantGroups / base;
    if (splits > KRS_SAMPLED_SOFTMAX_MAX_SPLITS) splits = KRS_SAMPLED_SOFTMAX_MAX_SPLITS;
    if (splits > tiles) splits = tiles;
    if (splits < 1) splits = 1;
    const int64_t per = cdiv(tiles, splits);
    splits = cdiv(tiles, per);
    pl.route.kernel = KRS_SAMPLED_SOFTMAX_FAST;
    pl.route.dpad = d <= 32 ? 32 : d <= 64 ? 64 : 128;
    pl.route.grid_tokens = (int32_t)(g * cdiv(lg, kOwn));
    pl.route.grid_negs = (int32_t)(base * splits);
    pl.route.splits = (int32_t)splits;
    pl.route.split_tiles = (int32_t)per;
  } else {
    pl.route.kernel = KRS_SAMPLED_SOFTMAX_GENERIC;
    pl.route.grid_tokens = (int32_t)t;
    pl.route.grid_negs = (int32_t)(g * n);
    pl.route.splits = 1;
    pl.route.split_tiles = (int32_t)cdiv(lg, kTile);
  }
  pl.off_c = KRS_SAMPLED_BCE_W_BLOCKS;
  pl.off_loss = pl.off_c + (size_t)t;
  pl.off_dneg = (pl.off_loss + (size_t)pl.route.grid_tokens + 63) / 64 * 64;      // (256-byte boundary)
  pl.floats = pl.off_dneg + (pl.route.splits > 1 ? (size_t)pl.route.splits * (size_t)(g * n) * (size_t)d : 0);
}

inline const char* shape_refusal(int64_t t, int64_t g, int64_t n, int64_t d, int emb_dtype) {
  if (emb_dtype != KRS_F32 && emb_dtype != KRS_BF16) return "emb dtype (KRS_F32 or KRS_BF16)";
  if (n < 1 || n > KRS_SAMPLED_SOFTMAX_MAX_NEGATIVES) return "1 <= n <= 4096";
  if (d < 1 || d > KRS_SAMPLED_SOFTMAX_MAX_DIM) return "1 <= d <= 512";
  if (t < 0 || t > kMaxCount) return "0 <= t <= 2^31 - 1";
  if (g < 1 || t % g != 0) return "g >= 1 and t % g == 0";
  if (g > kMaxCount || g * n > kMaxCount) return "g * n <= 2^31 - 1";
  return nullptr;
}

inline Plan plan(const Call& c) {
  Plan pl;
  auto refuse = [&](const char* why) {
    pl = Plan();
    pl.status = KRS_ERR_INVALID, pl.why = why;
    return pl;
  };
  if (const char* why = shape_refusal(c.t, c.g, c.n, c.d, c.emb_dtype)) return refuse(why);
  if (c.table_dtype != KRS_F32 && c.table_dtype != KRS_BF16) return refuse("table dtype (KRS_F32 or KRS_BF16)");
  if (c.itype != KRS_I32 && c.itype != KRS_I64) return refuse("id type (KRS_I32 or KRS_I64)");
  if ((c.pos_logq == nullptr) != (c.neg_logq == nullptr)) return refuse("pos_logq and neg_logq given both or neither");
  if (c.vocab < 0) return refuse("vocab >= 0");
  if (c.ld_emb < c.d) return refuse("ld_emb >= d");
  if (c.ld_table < c.d) return refuse("ld_table >= d");
  if (c.ld_demb < c.d) return refuse("ld_demb >= d");
  if (c.t == 0) return pl;
  if (!c.emb || !c.table || !c.pos || !c.neg) return refuse("non-null emb, table, pos and neg");
  if (!c.lse || !c.gpos || !c.demb || !c.dneg) return refuse("non-null lse, gpos, demb and dneg");
  shape(pl, c.t, c.g, c.n, c.d, c.emb_dtype);
  if (pl.route.kernel == KRS_SAMPLED_SOFTMAX_FAST)
    pl.route.vec = c.d % 8 == 0 && on16(c.emb) && on16(c.table) && stride16(c.ld_emb, c.emb_dtype) &&
                   stride16(c.ld_table, c.table_dtype);
  if (c.weight) {
    const int64_t wb = cdiv(c.t, KRS_SAMPLED_BCE_W_THREADS);
    pl.w_blocks = (int)(wb > KRS_SAMPLED_BCE_W_BLOCKS ? KRS_SAMPLED_BCE_W_BLOCKS : wb);
  }
  pl.route.launches = (c.weight ? 1 : 0) + 2 + (pl.route.splits > 1 ? 1 : 0) + 1;
  return pl;
}

inline size_t workspace_bytes(int64_t t, int64_t g, int64_t n, int64_t d, int emb_dtype) {
  if (t <= 0 || shape_refusal(t, g, n, d, emb_dtype)) return 0;
  Plan pl;
  shape(pl, t, g, n, d, emb_dtype);
  return pl.floats * sizeof(float);
}

}  // namespace ssm
}  // namespace krs
#endif
