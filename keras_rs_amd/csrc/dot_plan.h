// krs_dot_interaction_fwd's and krs_dot_interaction_bwd_accumulate's routing decision as a pure function of the call:
// the kernel, its template switches, the grid, the dynamic LDS request, the sample packing of the vector-ALU backward
// and the (i0, j0) launches of the block kernels.  Plain C++17 on krs.h, no HIP header: tests/host/dot_plan_check.cpp
// walks it under the sanitizers and krs_dot_interaction_plan_route answers from it without a GPU.  dot_interaction.hip
// plans here and launches exactly what the plan names; no shape condition lives anywhere else.  The host pointer TABLES
// (feats, ld, grad_feats, grad_feat_ld) are read; the device pointers in them are read as VALUES (nullness, alignment).
// A plan guarantees (the walk asserts it):
//   * vector-ALU backward: ng * 64 >= spw * ncols (every gradient column of the wave's samples is loaded),
//     spw * (1 << lps_log2) <= 64, 2 << lps_log2 covers min(dim, 128), ncols > 0, every byte offset fits 31 bits;
//   * MFMA backward: ng * 64 >= ncols, row strides in bytes fit 32 bits;
//   * lds_bytes is the kernel's own layout and never exceeds 64 KiB (no launch opts in to more; a CU has 160 KB);
//   * fr >= n_feats wherever a build provides for a fixed number of feature rows; ks * 32 == dim * es when ks > 0;
//   * the block launches cover every (i, j) pair the direction needs exactly once, first_j on the first launch of a row.
#ifndef KRS_DOT_PLAN_H_
#define KRS_DOT_PLAN_H_

#include <cstdint>
#include <vector>

#include "../../include/krs.h"

namespace krs {
namespace dplan {

constexpr int kMaxFast = 32;                    // feature rows of the MFMA and vector-ALU kernels
constexpr int kMaxGeneric = 64;                 // pointer-table length of the plain kernels
constexpr int kBlockI = 32, kBlockJ = 128;      // features per launch of the block kernels
constexpr int kFwdWaves = 4, kFwdMaxBlocks = 2048;       // dot_fwd_mfma_kernel: 256 threads, persistent
constexpr int kMfmaWaves = 2, kMfmaMaxBlocks = 2048;     // dot_bwd_mfma_kernel: 128 threads, persistent
constexpr int kValuMaxBlocks = 16384;                    // dot_bwd_valu_kernel: 64 threads, persistent
constexpr int kPlainMaxBlocks = 65536;                   // generic and block kernels: 256 threads, grid-stride
constexpr int kTabBytes = 64 * 16;              // the {pointer, stride} table both backward kernels keep in LDS
constexpr int kMfmaGsBytes = 2048, kMfmaStageBytes = 32 * 36 * 4;   // dot_bwd_mfma_kernel: Gs image, staging block
constexpr int kValuMultiNg = 16;                // gradient elements per lane of the MULTI build
constexpr int64_t kLaunchLds = 64 * 1024;       // what a launch may ask for without opting in
constexpr int64_t kCuLds = 160 * 1024;          // what a CU has

constexpr int tri_cols(int rows, bool self) { return self ? rows * (rows + 1) / 2 : rows * (rows - 1) / 2; }
// dot_bwd_valu_kernel<ES, FR, SELF, MULTI, ACC>: gradient elements per lane, dynamic LDS bytes for spw samples per wave
constexpr int valu_ng(int fr, bool self, bool multi) { return multi ? kValuMultiNg : (tri_cols(fr, self) + 63) / 64; }
constexpr int64_t valu_lds(int fr, bool self, int spw) { return kTabBytes + (int64_t)2 * spw * (tri_cols(fr, self) + 1) * 4; }
// dot_bwd_mfma_kernel<SELF, ACC, NG, 4>: X image bytes per wave, dynamic LDS bytes
constexpr int mfma_x_bytes(int dim) { return (dim + 127) / 128 * 8192; }
constexpr int64_t mfma_lds(int dim) { return kTabBytes + (int64_t)kMfmaWaves * (mfma_x_bytes(dim) + kMfmaGsBytes + kMfmaStageBytes); }

inline int64_t cdiv(int64_t a, int64_t b) { return a / b + (a % b != 0); }
inline int64_t sat_mul(int64_t a, int64_t b) { return (a != 0 && b > INT64_MAX / a) ? INT64_MAX : a * b; }   // a, b >= 0
inline int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

// One call as the decision sees it.  feats / ld / grad_feats / grad_feat_ld are the entry's HOST tables of n_feats
// entries; out_addr is the VALUE of `out` (forward) or `grad_out` (backward).
struct DotCall {
  bool backward = false;
  int n_feats = 0;
  int64_t batch = 0;
  int dim = 0, dtype = KRS_F32;
  bool self_interaction = false, skip_gather = false;
  uint64_t accumulate_mask = 0;             // backward only
  const void* const* feats = nullptr;
  const int64_t* ld = nullptr;
  void* const* grad_feats = nullptr;        // backward only
  const int64_t* grad_feat_ld = nullptr;    // backward only
  uint64_t out_addr = 0;
  int64_t out_ld = 0;
  bool force_valu = false;                  // KRS_DOT_BWD_VALU is set: the MFMA backward is not taken (read by the entry)
};

struct DotLaunch {   // one launch of a block kernel: features [i0, i0 + ni) against [j0, j0 + nj)
  int i0, ni, j0, nj, first_j;
  unsigned blocks;
};

struct DotPlan {
  krs_dot_route route = {};    // all zero ("none") when nothing is launched: batch == 0 or a refused call
  int status = KRS_OK;         // before the first launch: KRS_OK or KRS_ERR_INVALID
  const char* why = "";        // the refusal in words
  unsigned grid = 0, block = 0;     // one-launch routes
  int64_t lds_bytes = 0;            // dynamic LDS of the launch
  bool lds_opt_in = false;          // the launch must raise hipFuncAttributeMaxDynamicSharedMemorySize first (never, today)
  int lps_log2 = 0, spw = 0;        // vector-ALU backward: lanes per sample (log2), samples per wave
  int x_bytes = 0;                  // MFMA backward: X image bytes per wave
  uint64_t acc_mask = 0;            // accumulate_mask without the bits past n_feats
  std::vector<DotLaunch> launches;  // block kernels
};

inline bool aligned(const void* p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) % to) == 0; }
// (batch * ld + dim) * es < 2^31 without forming the product: what the vector-ALU backward's 32-bit offsets need
inline bool offsets_fit_31_bits(int64_t batch, int64_t ld, int dim, int es) {
  const int64_t lim = ((int64_t)1 << 31) / es;   // in elements
  return ld > 0 && dim < lim && batch <= (lim - 1 - dim) / ld;
}

inline DotPlan plan_dot(const DotCall& c) {
  DotPlan p;
  auto refuse = [&](int status, const char* why) { p = DotPlan(); p.status = status; p.why = why; return p; };
  if (!c.feats || !c.ld || !c.out_addr) return refuse(KRS_ERR_INVALID, "null argument");
  if (!(c.n_feats > 0 && c.batch >= 0 && c.dim > 0)) return refuse(KRS_ERR_INVALID, "bad sizes");
  if (!(c.dtype == KRS_F32 || c.dtype == KRS_BF16)) return refuse(KRS_ERR_INVALID, "bad dtype");
  for (int f = 0; f < c.n_feats; ++f)
    if (!c.feats[f]) return refuse(KRS_ERR_INVALID, "null feature pointer");
  if (c.backward) {
    if (!c.grad_feats || !c.grad_feat_ld) return refuse(KRS_ERR_INVALID, "null gradient outputs");
    for (int f = 0; f < c.n_feats; ++f)
      if (!c.grad_feats[f]) return refuse(KRS_ERR_INVALID, "null gradient pointer");
  }
  if (c.batch == 0) return p;

  const int F = c.n_feats, dim = c.dim, es = c.dtype == KRS_BF16 ? 2 : 4;
  const bool self = c.self_interaction, skip = c.skip_gather;
  krs_dot_route& rt = p.route;
  rt.dtype = c.dtype;
  rt.launches = 1;
  if (c.backward) p.acc_mask = F < 64 ? c.accumulate_mask & (((uint64_t)1 << F) - 1) : c.accumulate_mask;

  auto plan_blocks = [&]() {   // more than 64 features: one launch per (32 features i, 128 features j)
    rt.kernel = c.backward ? KRS_DOT_BWD_BLOCK : KRS_DOT_FWD_BLOCK;
    p.block = 256;
    for (int i0 = 0; i0 < F; i0 += kBlockI) {
      const int ni = F - i0 < kBlockI ? F - i0 : kBlockI;
      // forward without skip_gather: pairs with j > i are not part of the output
      const int j_end = (!c.backward && !skip) ? i0 + ni : F;
      for (int j0 = 0; j0 < j_end; j0 += kBlockJ) {
        const int nj = j_end - j0 < kBlockJ ? j_end - j0 : kBlockJ;
        const int64_t work = sat_mul(c.batch, (int64_t)ni * (c.backward ? dim : nj));
        p.launches.push_back(DotLaunch{i0, ni, j0, nj, j0 == 0, (unsigned)min64(cdiv(work, 256), kPlainMaxBlocks)});
        rt.blocks += p.launches.back().blocks;
      }
    }
    rt.launches = (int32_t)p.launches.size();
  };
  auto plan_generic = [&](int64_t work) {
    rt.kernel = c.backward ? KRS_DOT_BWD_GENERIC : KRS_DOT_FWD_GENERIC;
    rt.fr = kMaxGeneric;
    p.block = 256;
    p.grid = (unsigned)min64(cdiv(work, 256), kPlainMaxBlocks);
    rt.blocks = p.grid;
  };

  if (!c.backward) {
    // matrix cores: rows of whole 16-byte pieces, 16-byte aligned
    const int ve = 16 / es;
    bool fast = F <= kMaxFast && dim % ve == 0;
    for (int f = 0; fast && f < F; ++f) fast = aligned(c.feats[f], 16) && c.ld[f] % ve == 0;
    if (fast) {
      rt.kernel = KRS_DOT_FWD_MFMA;
      rt.ks = (es == 2 && dim == 128) ? 8 : ((es == 2 && dim == 64) ? 4 : 0);   // k steps known at compile time
      rt.fr = kMaxFast;
      p.block = 64 * kFwdWaves;
      p.grid = (unsigned)min64(cdiv(c.batch, kFwdWaves), kFwdMaxBlocks);
      rt.blocks = p.grid;
    } else if (F > kMaxGeneric) {
      plan_blocks();
    } else {
      plan_generic(sat_mul(c.batch, (int64_t)F * F));
    }
    return p;
  }

  const int ncols = F <= kMaxFast ? (skip ? F * F : tri_cols(F, self)) : 0;   // columns of the incoming gradient
  // matrix cores: bf16, rows of whole 32-column blocks (one 16-lane group loads a row: D <= 128), 16-byte aligned rows,
  // row strides whose bytes fit 32 bits
  bool mfma = es == 2 && F <= kMaxFast && dim % 32 == 0 && dim <= 128 && !c.force_valu && ncols > 0;
  for (int f = 0; mfma && f < F; ++f)
    mfma = aligned(c.feats[f], 16) && aligned(c.grad_feats[f], 16) && c.ld[f] % 8 == 0 && c.grad_feat_ld[f] % 8 == 0 &&
           c.ld[f] > 0 && c.grad_feat_ld[f] > 0 && c.ld[f] < ((int64_t)1 << 31) && c.grad_feat_ld[f] < ((int64_t)1 << 31);
  if (mfma) {
    rt.kernel = KRS_DOT_BWD_MFMA;
    rt.fr = kMaxFast;
    rt.self = self;
    rt.acc = p.acc_mask != 0;
    rt.ng = skip ? 16 : 9;    // 64 * 16 >= 32 * 32 columns of the [F, F] layout; 64 * 9 >= tri_cols(32, true) = 528
    p.x_bytes = mfma_x_bytes(dim);
    p.lds_bytes = mfma_lds(dim);
    p.block = 64 * kMfmaWaves;
    p.grid = (unsigned)min64(cdiv(c.batch, kMfmaWaves), kMfmaMaxBlocks);
    rt.lds_bytes = (int32_t)p.lds_bytes;
    rt.blocks = p.grid;
    return p;
  }
  // vector ALU: pairs of adjacent columns per lane (even D, rows aligned to a pair), 32-bit byte offsets, and at least
  // one gradient column (the kernel clamps its gradient loads to column ncols - 1)
  bool valu = F <= kMaxFast && dim % 2 == 0 && ncols > 0;
  for (int f = 0; valu && f < F; ++f)
    valu = aligned(c.feats[f], 2 * es) && aligned(c.grad_feats[f], 2 * es) && c.ld[f] % 2 == 0 && c.grad_feat_ld[f] % 2 == 0 &&
           offsets_fit_31_bits(c.batch, c.ld[f], dim, es) && offsets_fit_31_bits(c.batch, c.grad_feat_ld[f], dim, es);
  if (valu) {
    int lps_log2 = 0;
    while ((2 << lps_log2) < dim && lps_log2 < 6) ++lps_log2;     // lanes per sample: dim / 2 up to 64
    // samples per wave: what the lanes hold, what 16 gradient elements per lane cover, what 64 KiB of LDS hold (the
    // MULTI build stages 2 * spw rows of tri_cols(32, SELF) + 1 floats whatever F is: 15 samples with SELF, else 16)
    int spw = 64 >> lps_log2;
    if (spw > kValuMultiNg * 64 / ncols) spw = kValuMultiNg * 64 / ncols;
    const int lds_cap = (int)((kLaunchLds - kTabBytes) / (2 * 4 * (tri_cols(kMaxFast, self) + 1)));
    if (spw > lds_cap) spw = lds_cap;
    if (spw < 1) spw = 1;
    // one sample per wave: rows rounded up to 28 (the 26 + 1 features of DLRM) or 32, as long as the build's
    // ceil(tri_cols(FR, SELF) / 64) gradient elements per lane cover the incoming columns -- the [F, F] layout of
    // 23 and 24 (without SELF) or 25 and more features does not fit them.  Everything else takes the MULTI build.
    bool multi = spw > 1;
    int fr = kMaxFast;
    if (!multi) {
      fr = (F <= 28 && !skip) ? 28 : kMaxFast;
      if (valu_ng(fr, self, false) * 64 < ncols) { multi = true; fr = kMaxFast; }
    }
    rt.kernel = KRS_DOT_BWD_VALU;
    rt.fr = fr;
    rt.self = self;
    rt.multi = multi;
    rt.acc = p.acc_mask != 0;
    rt.ng = valu_ng(fr, self, multi);
    rt.lps_log2 = lps_log2;
    rt.spw = spw;
    p.lps_log2 = lps_log2;
    p.spw = spw;
    p.lds_bytes = valu_lds(fr, self, spw);
    p.block = 64;
    p.grid = (unsigned)min64(cdiv(c.batch, spw), kValuMaxBlocks);
    rt.lds_bytes = (int32_t)p.lds_bytes;
    rt.blocks = p.grid;
    return p;
  }
  if (F > kMaxGeneric) plan_blocks();
  else plan_generic(sat_mul(c.batch, (int64_t)F * dim));
  return p;
}

}  // namespace dplan
}  // namespace krs
#endif
