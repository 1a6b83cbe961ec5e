// krs_embed_bag_fwd_q8's routing decision and krs_quantize_rows_q8's launch shape as pure functions of the call.  Plain
// C++17 on krs.h, no HIP header: tests/host/embed_fwd_q8_plan_check.cpp walks them under the sanitizers and
// krs_embed_bag_fwd_q8_plan_route answers from the first without a GPU.  embed_bag_fwd_q8.hip checks its pointers, plans
// here and launches exactly what the plan names.
// A lookup plan guarantees (the walk asserts it): the pooled kernel runs exactly the rows that are whole 16-byte pieces of
// at most 1024 bytes (an int8 element is a byte: dim % 16 == 0 && dim <= 1024), lpr is the smallest of 8 / 16 / 32 / 64
// that holds the pieces, 1 <= bpg <= 16; the generic kernel runs every other dim; blocks x 4 waves cover every bag and
// blocks <= 2^31 - 1; every int the kernels recompute from batch fits.
#ifndef KRS_EMBED_FWD_Q8_PLAN_H_
#define KRS_EMBED_FWD_Q8_PLAN_H_

#include <climits>
#include <cstdint>

#include "../../include/krs.h"

namespace krs {
namespace q8plan {

constexpr int kPieceBytes = 16, kMaxRowBytes = 1024;   // a lane moves one 16-byte piece = 16 int8 elements
constexpr int kMaxBpg = 16, kLookupsPerGroup = 32;     // embed_bag_fwd_q8_vec stages at most 16 bag ends per group
constexpr int64_t kMaxBlocks = 0x7fffffffLL;
// the kernel recomputes (batch + bags_per_wave - 1) / bags_per_wave in int; bags_per_wave <= 8 * 16
constexpr int kMaxBatch = INT_MAX - 8 * kMaxBpg;

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// One krs_embed_bag_fwd_q8 call as the decision sees it.  out_addr: the VALUE of `out` (read for nullness only: the
// kernels test the alignment of their stores themselves).
struct Q8FwdCall {
  int n_feats = 0, batch = 0, dim = 0;
  int64_t nnz = 0, out_ld = 0;
  int out_dtype = KRS_F32;
  bool has_offsets = false, has_weights = false;
  uint64_t out_addr = 0;
};

struct Q8FwdPlan {
  krs_embed_fwd_route route = {};   // all zero ("none") when nothing is launched: n_feats == 0, batch == 0 or a refused call
  int status = KRS_OK;              // before the first launch: KRS_OK, KRS_ERR_INVALID, KRS_ERR_UNSUPPORTED
  const char* why = "";             // the refusal in words
};

inline Q8FwdPlan plan_q8_fwd(const Q8FwdCall& c) {
  Q8FwdPlan p;
  auto refuse = [&](int status, const char* why) { p = Q8FwdPlan(); p.status = status; p.why = why; return p; };
  if (!c.out_addr) return refuse(KRS_ERR_INVALID, "null tables/feats/out");
  if (!(c.n_feats >= 0 && c.batch >= 0 && c.dim > 0 && c.nnz >= 0)) return refuse(KRS_ERR_INVALID, "negative size");
  if (!(c.out_dtype == KRS_F32 || c.out_dtype == KRS_BF16)) return refuse(KRS_ERR_INVALID, "bad dtype");
  if (c.n_feats == 0 || c.batch == 0) return p;
  if (c.batch > kMaxBatch) return refuse(KRS_ERR_UNSUPPORTED, "batch beyond the kernels' 32-bit bag arithmetic");
  krs_embed_fwd_route& rt = p.route;
  rt.table_dtype = KRS_I8;
  rt.out_dtype = c.out_dtype;
  rt.has_w = c.has_weights;
  const int64_t n_bags = (int64_t)c.n_feats * c.batch;
  if (c.dim % kPieceBytes != 0 || c.dim > kMaxRowBytes) {
    // any dim: one lpr-lane group per bag, one column per lane per pass
    int lpr = 1;
    while (lpr < c.dim && lpr < 64) lpr <<= 1;
    rt.kernel = KRS_EMBED_FWD_GENERIC;
    rt.lpr = lpr;
    rt.blocks = cdiv(n_bags, 256 / lpr);
  } else {
    const int pieces = c.dim / kPieceBytes;
    rt.lpr = pieces <= 8 ? 8 : (pieces <= 16 ? 16 : (pieces <= 32 ? 32 : 64));
    // ~16-32 lookups per group, as K1: enough row loads in flight per wave without making one group's stream long
    const int64_t mean_hot = c.nnz / n_bags > 0 ? c.nnz / n_bags : 1;
    const int64_t bpg = kLookupsPerGroup / mean_hot;
    rt.kernel = KRS_EMBED_FWD_VEC;
    rt.bpg = bpg < 1 ? 1 : (bpg > kMaxBpg ? kMaxBpg : (int)bpg);
    rt.blocks = cdiv(cdiv(c.batch, (int64_t)(64 / rt.lpr) * rt.bpg) * c.n_feats, 4);
  }
  if (rt.blocks > kMaxBlocks) return refuse(KRS_ERR_UNSUPPORTED, "grid too large");
  return p;
}

// krs_quantize_rows_q8: rows of up to kRegRowElems elements are held in registers by a group of `lanes` lanes, 16
// elements per lane (lanes = the smallest power of two >= ceil(dim / 16)); a longer row takes a wave and is read twice.
// `vec`: a lane's 16 elements are consecutive and move as 16-byte loads and one 16-byte store (dim % 16 == 0 and both
// base pointers 16-byte aligned); otherwise the group's lanes interleave element by element.
constexpr int kRegRowElems = 1024;
struct QuantizePlan {
  int lanes = 0;
  bool vec = false, two_pass = false;
  int64_t blocks = 0;   // workgroups of 256 threads = 256 / lanes rows
  int status = KRS_OK;
  const char* why = "";
};

inline QuantizePlan plan_quantize(int64_t vocab, int dim, int table_dtype, uint64_t table_addr, uint64_t q_addr,
                                  uint64_t step_addr) {
  QuantizePlan p;
  auto refuse = [&](int status, const char* why) { p = QuantizePlan(); p.status = status; p.why = why; return p; };
  if (!(vocab >= 0 && dim > 0)) return refuse(KRS_ERR_INVALID, "negative size");
  if (!(table_dtype == KRS_F32 || table_dtype == KRS_BF16)) return refuse(KRS_ERR_INVALID, "bad dtype");
  if (vocab > 0 && !(table_addr && q_addr && step_addr)) return refuse(KRS_ERR_INVALID, "null table/q/step");
  if (vocab > INT_MAX) return refuse(KRS_ERR_UNSUPPORTED, "more than INT32_MAX rows");
  if (vocab == 0) return p;
  if (dim > kRegRowElems) {
    p.lanes = 64;
    p.two_pass = true;
  } else {
    int lanes = 1;
    while (lanes * 16 < dim) lanes <<= 1;
    p.lanes = lanes;
    p.vec = dim % 16 == 0 && ((table_addr | q_addr) & 15) == 0;
  }
  p.blocks = cdiv(vocab, 256 / p.lanes);
  return p;
}

}  // namespace q8plan
}  // namespace krs
#endif
