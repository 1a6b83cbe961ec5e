// The route of krs_sampled_bce_fwd_bwd (sampled_bce.hip) as a pure function of the call: the lanes of a token, the
// vector or the element route, the workgroups, the launches and the workspace.  Plain C++17 on krs.h, no HIP header:
// krs_sampled_bce_plan_route answers from it without a GPU.  Device pointers are read as VALUES (nullness, alignment).
// A plan guarantees:
//   * g is the smallest of 8, 16, 32, 64 with 8 * g >= d;
//   * the vector route only when every lane's 8 columns of emb, table and demb are whole 16-byte pieces;
//   * 1 <= blocks <= KRS_SAMPLED_BCE_MAX_BLOCKS and no workgroup without a token;
//   * launches = [W pass, with weights] + main + [finish when blocks > 1].
#ifndef KRS_SAMPLED_BCE_PLAN_H_
#define KRS_SAMPLED_BCE_PLAN_H_

#include <cstddef>
#include <cstdint>

#include "../../include/krs.h"

namespace krs {
namespace sbce {

constexpr int64_t kMaxTokens = 2147483647;
constexpr int kCols = 8;          // adjacent columns of a lane
constexpr int kChunk = 4;         // item rows in flight per token

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
  int64_t t = 0, d = 0, n = 0;
  const void* glog = nullptr;
  const void* demb = nullptr;
  int64_t ld_demb = 0;
};

struct Plan {
  int status = KRS_OK;                 // KRS_OK or KRS_ERR_INVALID
  const char* why = "";
  krs_sampled_bce_route route = {};    // all zero after a refusal or when t == 0
  int w_blocks = 0;                    // workgroups of the W pass (0 without weights)
};

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline bool on16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
// a row stride at which every lane's 8 columns start on 16 bytes
inline bool stride16(int64_t ld, int dtype) { return ld % (dtype == KRS_BF16 ? 8 : 4) == 0; }
inline int group_for(int64_t d) { return d <= 64 ? 8 : d <= 128 ? 16 : d <= 256 ? 32 : 64; }

inline Plan plan(const Call& c) {
  Plan pl;
  auto refuse = [&](const char* why) {
    pl.status = KRS_ERR_INVALID, pl.why = why;
    return pl;
  };
  if (c.emb_dtype != KRS_F32 && c.emb_dtype != KRS_BF16) return refuse("emb dtype");
  if (c.table_dtype != KRS_F32 && c.table_dtype != KRS_BF16) return refuse("table dtype");
  if (c.itype != KRS_I32 && c.itype != KRS_I64) return refuse("id type");
  if (c.d < 1 || c.d > KRS_SAMPLED_BCE_MAX_DIM) return refuse("d");
  if (c.n < 0 || c.n > KRS_SAMPLED_BCE_MAX_NEGATIVES) return refuse("n");
  if (c.t < 0 || c.t > kMaxTokens) return refuse("t");
  if (c.vocab < 0) return refuse("vocab");
  if (c.ld_emb < c.d) return refuse("ld_emb");
  if (c.ld_table < c.d) return refuse("ld_table");
  if (c.demb && c.ld_demb < c.d) return refuse("ld_demb");
  if (c.t == 0) return pl;
  if (!c.emb || !c.table || !c.pos || !c.glog || (c.n > 0 && !c.neg)) return refuse("null operand");
  const bool vec = c.d % kCols == 0 && on16(c.emb) && on16(c.table) && on16(c.demb) &&
                   stride16(c.ld_emb, c.emb_dtype) && stride16(c.ld_table, c.table_dtype) &&
                   (!c.demb || stride16(c.ld_demb, c.emb_dtype));
  const int g = group_for(c.d);
  const int64_t blocks = cdiv(c.t, KRS_SAMPLED_BCE_THREADS / g);
  pl.route.kernel = vec ? KRS_SAMPLED_BCE_VEC : KRS_SAMPLED_BCE_ELEM;
  pl.route.g = g;
  pl.route.blocks = (int)(blocks > KRS_SAMPLED_BCE_MAX_BLOCKS ? KRS_SAMPLED_BCE_MAX_BLOCKS : blocks);
  if (c.weight) {
    const int64_t wb = cdiv(c.t, KRS_SAMPLED_BCE_W_THREADS);
    pl.w_blocks = (int)(wb > KRS_SAMPLED_BCE_W_BLOCKS ? KRS_SAMPLED_BCE_W_BLOCKS : wb);
  }
  pl.route.launches = (c.weight ? 1 : 0) + 1 + (pl.route.blocks > 1 ? 1 : 0);
  return pl;
}

// the W pass's partials, then one partial per workgroup of the main pass
inline size_t workspace_bytes(int64_t t) {
  if (t <= 0) return 0;
  return (size_t)(KRS_SAMPLED_BCE_W_BLOCKS + KRS_SAMPLED_BCE_MAX_BLOCKS) * sizeof(float);
}

}  // namespace sbce
}  // namespace krs
#endif
