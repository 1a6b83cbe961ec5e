// krs_embed_bag_fwd's routing decision as a pure function of the call: kernel, lanes per row, the template switches of the
// pooled kernel, bags per group and the grid.  Plain C++17 on krs.h, no HIP header: tests/host/embed_fwd_plan_check.cpp
// walks it under the sanitizers and krs_embed_bag_fwd_plan_route answers from it without a GPU.  embed_bag_fwd.hip checks
// its pointers, plans here and launches exactly what the plan names; no shape condition lives anywhere else.
// A plan guarantees (the walk asserts it): lpr is the smallest of 8 / 16 / 32 / 64 that holds the row's 16-byte pieces; the
// generic kernel runs exactly the rows that are not whole pieces or exceed 1024 bytes; 1 <= bpg <= 16 on the pooled kernel;
// blocks x 4 waves cover every bag (unit) and blocks <= 2^31 - 1; every int the kernels recompute from batch fits.
#ifndef KRS_EMBED_FWD_PLAN_H_
#define KRS_EMBED_FWD_PLAN_H_

#include <climits>
#include <cstdint>

#include "../../include/krs.h"

namespace krs {
namespace eplan {

constexpr int kPieceBytes = 16, kMaxRowBytes = 1024;   // a lane moves one 16-byte piece; 64 lanes hold at most 1024 bytes
constexpr int kRowsMaxFeats = 128;                     // embed_gather_hot1_rows keeps its per-feature constants in LDS
constexpr int kMaxBpg = 16, kLookupsPerGroup = 32;     // embed_bag_fwd_vec stages at most 16 bag ends per group
constexpr int kHotRowBytes = 256;                      // LDS staging of hot rows: bf16 rows of 16 pieces only
constexpr int64_t kMaxBlocks = 0x7fffffffLL;
// the kernels recompute (batch + bags_per_wave - 1) / bags_per_wave and (batch + 63) / 64 in int; bags_per_wave <= 8 * 16
constexpr int kMaxBatch = INT_MAX - 8 * kMaxBpg;

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// One krs_embed_bag_fwd call as the decision sees it.  out_addr: the VALUE of `out` (read for nullness and alignment).
struct EmbedFwdCall {
  int n_feats = 0, batch = 0, dim = 0;
  int64_t nnz = 0, out_ld = 0;
  int table_dtype = KRS_F32, out_dtype = KRS_F32;
  bool has_offsets = false, has_weights = false;
  uint64_t out_addr = 0;
  int hot_rows_opt = 0;   // krs_embed_set_option(KRS_EMBED_OPT_HOTROWS, .): 0 | 64 | 128
};

struct EmbedFwdPlan {
  krs_embed_fwd_route route = {};   // all zero ("none") when nothing is launched: n_feats == 0, batch == 0 or a refused call
  int status = KRS_OK;              // before the first launch: KRS_OK, KRS_ERR_INVALID, KRS_ERR_UNSUPPORTED
  const char* why = "";             // the refusal in words
};

inline EmbedFwdPlan plan_embed_fwd(const EmbedFwdCall& c) {
  EmbedFwdPlan p;
  auto refuse = [&](int status, const char* why) { p = EmbedFwdPlan(); p.status = status; p.why = why; return p; };
  if (!c.out_addr) return refuse(KRS_ERR_INVALID, "null tables/feats/out");
  if (!(c.n_feats >= 0 && c.batch >= 0 && c.dim > 0 && c.nnz >= 0)) return refuse(KRS_ERR_INVALID, "negative size");
  if (!((c.table_dtype == KRS_F32 || c.table_dtype == KRS_BF16) && (c.out_dtype == KRS_F32 || c.out_dtype == KRS_BF16)))
    return refuse(KRS_ERR_INVALID, "bad dtype");
  if (c.n_feats == 0 || c.batch == 0) return p;
  if (c.batch > kMaxBatch) return refuse(KRS_ERR_UNSUPPORTED, "batch beyond the kernels' 32-bit bag arithmetic");
  krs_embed_fwd_route& rt = p.route;
  rt.table_dtype = c.table_dtype;
  rt.out_dtype = c.out_dtype;
  const int64_t n_bags = (int64_t)c.n_feats * c.batch;
  const int es_t = c.table_dtype == KRS_BF16 ? 2 : 4, es_o = c.out_dtype == KRS_BF16 ? 2 : 4;
  const int64_t row_bytes = (int64_t)c.dim * es_t;
  if (row_bytes % kPieceBytes != 0 || row_bytes > kMaxRowBytes) {
    // any dim / any alignment: one lpr-lane group per bag, one column per lane per pass
    int lpr = 1;
    while (lpr < c.dim && lpr < 64) lpr <<= 1;
    rt.kernel = KRS_EMBED_FWD_GENERIC;
    rt.lpr = lpr;
    rt.has_w = c.has_weights;
    rt.blocks = cdiv(n_bags, 256 / lpr);
  } else {
    const int pieces = (int)(row_bytes / kPieceBytes);
    rt.lpr = pieces <= 8 ? 8 : (pieces <= 16 ? 16 : (pieces <= 32 ? 32 : 64));
    // every bag has exactly one lookup on average (dense, unweighted): the pure-gather kernels
    if (!c.has_offsets && !c.has_weights && c.nnz == n_bags) {
      // sample-major walk where the raw pieces can be stored as they are: same element size, 16-byte aligned output rows
      const bool rows_ok = es_t == es_o && c.n_feats <= kRowsMaxFeats &&
                           ((c.out_addr | ((uint64_t)c.out_ld * (uint64_t)es_o)) & 15) == 0;
      rt.kernel = rows_ok ? KRS_EMBED_FWD_HOT1_ROWS : KRS_EMBED_FWD_HOT1;
      rt.blocks = rows_ok ? cdiv(cdiv(n_bags, 64), 4) : cdiv(cdiv(c.batch, 64) * c.n_feats, 4);
    } else {
      // ~16-32 lookups per group: enough row loads in flight per wave without making one group's stream long
      const int64_t mean_hot = c.nnz / n_bags > 0 ? c.nnz / n_bags : 1;
      const int64_t bpg = kLookupsPerGroup / mean_hot;
      rt.kernel = KRS_EMBED_FWD_VEC;
      rt.bpg = bpg < 1 ? 1 : (bpg > kMaxBpg ? kMaxBpg : (int)bpg);
      rt.has_w = c.has_weights;
      rt.stream = c.nnz < 2 * n_bags;   // bags of ~1 lookup: no row reuse to protect
      if (es_t == 2 && es_o == 2 && rt.lpr == 16 && c.hot_rows_opt > 0 && !c.has_weights && row_bytes == kHotRowBytes)
        rt.hot_rows = c.hot_rows_opt >= 128 ? 128 : 64;
      rt.blocks = cdiv(cdiv(c.batch, (int64_t)(64 / rt.lpr) * rt.bpg) * c.n_feats, 4);
    }
  }
  if (rt.blocks > kMaxBlocks) return refuse(KRS_ERR_UNSUPPORTED, "grid too large");
  return p;
}

}  // namespace eplan
}  // namespace krs
#endif
