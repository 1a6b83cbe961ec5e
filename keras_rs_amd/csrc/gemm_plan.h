// krs_gemm's routing decision as a pure function of the call: kernel, splits along K, reduce kernel, grid, LDS bytes.
// Plain C++17 on krs.h, no HIP header: tests/host/gemm_plan_check.cpp walks it under the sanitizers and krs_gemm_plan_route
// answers from it without a GPU.  gemm.hip validates, plans here and launches; no shape condition lives anywhere else.
// A plan guarantees (the lattice walk asserts it): on pp256 / pp256_kstrided every split, the last included, is whole 32-k
// blocks and at least 4 of them; on pp64 whole 64-k blocks and at least 3; on tn_glds k and k_per_split are multiples of 64;
// glds is unsplit on whole 128-byte rows; splits > 1 exactly when a reduce kernel follows, within plan_workspace_bytes.
// Not guaranteed: on mfma, tn_glds and thin a trailing split may start past K (16 x 16 x 9000 tn bf16: 17 splits of 576,
// the last starts at 9216); those kernels bound every k they touch and write a zero slab for such a split.
#ifndef KRS_GEMM_PLAN_H_
#define KRS_GEMM_PLAN_H_

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/krs.h"

namespace krs {

inline bool al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

namespace gplan {

// every threshold, once
constexpr int kTile = 128, kRowBytes = 128;   // the 128 x 128 kernels; a tile row is 128 bytes of K (64 bf16 / 32 fp32)
constexpr int kLdsStride = kRowBytes + 16, kTileBytes = kTile * kLdsStride;   // register-staged tiles pad rows by 16 bytes
constexpr int kBigTile = 256, kCUs = 256;     // the ring kernels' tile (the L2 -> LDS path bounds these products); one round
constexpr int kFillTiles = 192;               // 256 x 256 tiles must cover most CUs (8192 x 512 is 64: 128 x 128 or a split ring)
constexpr int kRingBlock = 32, kRingDepth = 4;        // gemm_pp256_kernel: four stages of 32-k blocks, its tail drains three
constexpr int kRing64Block = 64, kRing64Depth = 3;    // gemm_pp64_kernel: 64-k pieces (whole 128-byte lines), at least three
constexpr int kRingMinK = 256;                // shorter contractions (per split, K-strided build) stay on 128 x 128 tiles
constexpr int kRingSplitMinK = 2048, kSplitMinK = 512;   // the K-contiguous ring splits a long K only, >= 512 per split
constexpr int kGldsMinK = 1024;               // K = 512 runs better register-staged: three workgroups per CU hide the epilogues
constexpr int kThinMax = 16, kThinMinK = 1024, kThinMaxSplits = 128;   // gemm_thin_kernel (13 inputs, 1 unit); 256 splits made
                                                                        // the reduce the longer kernel, 64 idled half the CUs
constexpr int kWgradMinK = 4096, kMaxSplits = 64;     // the weight-gradient cost rule starts at this K
constexpr int kGeneralMinK = 4096, kGeneralSplitK = 1024, kGeneralWgs = 1024;   // general rule: >= 1024 of K per split, ~4 wg / CU
constexpr int kRowdotMaxN = 8, kRowdotMinK = 32, kRowdotMinM = 1024, kRowdotRows = 16;   // gemm_rowdot_kernel (1-unit Dense)
constexpr int kSmallkMaxK = 16, kSmallkMaxN = 1024, kSmallkRows = 64, kSmallkMinMN = 1 << 16;   // B [K, N] fp32 in <= 64 KB LDS
constexpr size_t kRingLds = 4 * 32768, kRing64Lds = 5 * 32768, kGldsLds = 4 * kTile * kRowBytes;   // stages x (A + B)
constexpr int64_t kMaxGridThreads = 0xffffffffll, kMaxGridYZ = 65535;   // launch limits: threads along x, blocks along y / z
// The ring's LDS in the epilogue (every slot is dead): eight waves stage 32 x 68 floats of accumulators each from byte 0 on;
// under KRS_GEMM_SCHED_LDS_LANDING a wave's 32-row chunk of x and of x0 (32 rows x 128 bytes each) lands behind that.
constexpr size_t kEpiStageBytes = 8 * 32 * 68 * sizeof(float), kEpiLandWaveBytes = 2 * 32 * 128;
constexpr size_t kEpiLandBytes = 8 * kEpiLandWaveBytes;

// gemm_pp64_kernel's work items.  Workgroup b runs on XCD b % 8 and is that XCD's item b / 8 = tslot * splits + split; tile
// tslot of an XCD lies in its M panel g = tslot / nt (tile row g * 8 + XCD of C) at N tile j:
//   panel order   j = tslot % nt: the N tiles of a panel back to back, sharing A in the XCD's L2;
//   staggered     the same panels, but an odd panel starts half way round: j = (tslot % nt + nt / 2) % nt.
// Either way tslot -> (g, j) is a bijection onto [0, panels) x [0, nt): a rotation inside each panel (the lattice walk of
// tests/host/gemm_epi_schedule_check.cpp counts every tile once).  Which workgroup computes a tile changes speed, never bits.
struct RingTile { int64_t panel; int n_tile; };
constexpr RingTile ring_tile_of_slot(int64_t tslot, int nt, bool stagger) {
  const int64_t g = tslot / nt;
  int j = (int)(tslot - g * nt);
  if (stagger && (g & 1)) j = j + nt / 2 >= nt ? j + nt / 2 - nt : j + nt / 2;
  return RingTile{g, j};
}

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int64_t round_up(int64_t a, int64_t b) { return cdiv(a, b) * b; }

// One krs_gemm call as the decision sees it.  al_*: base pointer on 16 bytes; bias / x0 / u_out / r: epilogue operands present.
struct GemmCall {
  int64_t m = 0, n = 0, k = 0, lda = 0, ldb = 0, ldc = 0, ldx = 0, ldu = 0, ldr = 0;
  bool a_km = false, b_nk = false;
  int es = 2, out_dtype = KRS_BF16, act = KRS_ACT_NONE;   // es: bytes per input element (2 = bf16, 4 = fp32)
  bool al_a = true, al_b = true, al_c = true, al_bias = true, al_x0 = true, al_x = true, al_u = true, al_r = true;
  bool has_ep = false, bias = false, x0 = false, u_out = false, r = false;
  size_t workspace_bytes = 0;   // offered (0 with a NULL workspace)
  bool allow_split = true;      // false: one pass over K (the two-call form of krs_gemm_cross_bwd has no slab workspace)
  int pipe = 4;                 // KRS_GEMM_OPT_PIPELINE: 4 | 5 | 0
  bool tn128 = false;           // development switch KRS_GEMM_TN128: weight gradients on the 128 x 128 gemm_tn_glds_kernel
  bool x_is_x0 = false;         // the cross epilogue's x IS its x0 (one pointer, one stride: the first layer of a stack)
  int epi_sched = 0;            // KRS_GEMM_OPT_EPI_SCHEDULE: 0 | 1 | 2 | 3
};

// which epilogue operands a call brings and how they are aligned (ep NULL: no epilogue); pointer VALUES only
inline void set_epilogue(GemmCall& c, const krs_gemm_epilogue* ep) {
  if (!ep) return;
  c.has_ep = true; c.act = ep->act; c.bias = ep->bias != nullptr; c.al_bias = al16(ep->bias);
  c.x0 = ep->x0 != nullptr; c.al_x0 = al16(ep->x0); c.al_x = al16(ep->x); c.ldx = ep->ldx;
  c.x_is_x0 = c.x0 && ep->x == ep->x0;     // (x0 and x share ldx)
  c.u_out = ep->u_out != nullptr; c.al_u = al16(ep->u_out); c.ldu = ep->ldu;
  c.r = ep->r != nullptr; c.al_r = al16(ep->r); c.ldr = ep->ldr;
}

struct GemmPlan {
  krs_gemm_route route = {};    // all zero ("none") when nothing is launched: m == 0, n == 0 or a refused call
  int status = KRS_OK;          // before the first launch: KRS_OK, KRS_ERR_WORKSPACE (`need` bytes wanted), KRS_ERR_UNSUPPORTED
  size_t need = 0, lds = 0;     // slab bytes of the split; dynamic LDS bytes
  int64_t k_per_split = 0, grid[3] = {1, 1, 1}, reduce_grid = 0;
  int block = 256, mt = 0, nt = 0;   // threads per workgroup; the tile-count arguments of the ring and tn_glds kernels
};

inline bool thin_shape(int64_t m, int64_t n, int64_t k) { return k >= kThinMinK && std::min(m, n) <= kThinMax; }

// Split-K factor of a tile product and of gemm_thin_kernel (a_km only).  The caller rounds K per split up to tile rows.
inline int pick_splits(int64_t m, int64_t n, int64_t k, bool a_km, bool ring_ok) {
  if (a_km && thin_shape(m, n, k)) return (int)std::min<int64_t>(k / kSplitMinK, kThinMaxSplits);
  const int64_t t256 = cdiv(m, kBigTile) * cdiv(n, kBigTile);
  // Weight gradients on 256 x 256 tiles: minimise rounds over the CUs x (K per split + per-workgroup overhead) + slab
  // traffic (2 x 14 tiles of the C3 gradients: 9 splits = 252 workgroups in one round; 16 were 1.75 rounds and 113 MB of
  // slabs instead of 64).  Skipped: a count whose last split is empty or shorter than the ring, whose tail always drains.
  if (a_km && m >= kBigTile && n >= kBigTile && k % 64 == 0 && k >= kWgradMinK) {
    const double slab = (double)m * (double)n * 6.45e-5;   // slab write + read of one split, in k steps of a tile
    double best = 0;
    int best_s = 1;
    for (int s = 1; s <= kMaxSplits && k / s >= kSplitMinK; ++s) {
      const int64_t kps = round_up(cdiv(k, s), 64);
      if (k - (int64_t)(s - 1) * kps < kRingDepth * kRingBlock) continue;
      const double cost = (double)cdiv(t256 * s, kCUs) * (double)(kps + 256) + (s > 1 ? slab * s : 0.0);
      if (s == 1 || cost < best) { best = cost; best_s = s; }
    }
    return best_s;
  }
  // K-contiguous bf16 products with too few 256 x 256 tiles but a long K: the ring with K dealt to s workgroups per tile,
  // s x tiles ~ one round (half the operand bytes per flop of the 128 x 128 kernels; h = x U at M = 8192: 59 -> 4x us).
  // The last split takes what the 64-k rounding leaves and must still hold a ring.
  if (ring_ok && !a_km && m >= kBigTile && n >= kBigTile && k >= kRingSplitMinK && k % kRingBlock == 0 && t256 < kFillTiles) {
    auto fits = [&](int64_t q) {
      const int64_t last = k - (q - 1) * round_up(cdiv(k, q), 64);
      return k / q >= kSplitMinK && last >= kRingDepth * kRingBlock && last % kRingBlock == 0;
    };
    int64_t s = kCUs / t256;
    while (s > 1 && !fits(s)) --s;
    if (s > 1) return (int)s;
  }
  const int64_t tiles = cdiv(m, kTile) * cdiv(n, kTile), max_s = k / kGeneralSplitK;
  if (tiles >= kCUs || k < kGeneralMinK) return 1;
  int64_t s = std::min<int64_t>({cdiv(kGeneralWgs, tiles), max_s, kMaxSplits});
  if (s > 8) s = (s + 7) / 8 * 8;          // whole rounds over the 8 XCDs (gemm_tn_glds_kernel deals splits to XCDs)
  if (s > max_s) s = max_s / 8 * 8;
  return s < 1 ? 1 : (int)s;
}

// Slab bytes no krs_gemm of this shape exceeds: the largest need over the input dtypes and B layouts (they decide ring_ok).
inline size_t plan_workspace_bytes(int64_t m, int64_t n, int64_t k, bool a_km) {
  if (m <= 0 || n <= 0 || k <= 0) return 0;
  const int s = std::max(pick_splits(m, n, k, a_km, true), pick_splits(m, n, k, a_km, false));
  return s > 1 ? (size_t)s * (size_t)m * (size_t)n * sizeof(float) : 0;
}

// every epilogue operand allows 8-wide vector access
inline bool ep_vec(const GemmCall& c) {
  return c.n % 8 == 0 && c.ldc % 8 == 0 && c.al_c && (!c.bias || c.al_bias) &&
         (!c.x0 || (c.al_x0 && c.al_x && c.ldx % 8 == 0)) && (!c.u_out || (c.al_u && c.ldu % 8 == 0)) &&
         (!c.r || (c.al_r && c.ldr % 8 == 0));
}

// the MFMA tile kernels load 16-byte vectors: aligned bases and strides, the contiguous axis in whole vectors
inline bool tile_eligible(const GemmCall& c) {
  const int64_t va = 16 / c.es;
  return c.k > 0 && !(c.a_km && c.b_nk) && c.al_a && c.al_b && c.lda % va == 0 && c.ldb % va == 0 &&
         (c.a_km ? c.m : c.k) % va == 0 && (c.b_nk ? c.k : c.n) % va == 0;
}

inline GemmPlan plan_gemm(const GemmCall& c) {
  GemmPlan p;
  const int64_t m = c.m, n = c.n, k = c.k;
  p.k_per_split = k;
  if (m == 0 || n == 0) return p;
  krs_gemm_route& rt = p.route;
  rt.ep_vec = ep_vec(c);
  rt.splits = 1;
  auto refuse = [&](int status, size_t need) { p = GemmPlan(); p.status = status; p.need = need; return p; };
  auto split = [&](int s, int64_t unit) {      // false: the workspace does not hold s slabs
    p.need = (size_t)s * (size_t)m * (size_t)n * sizeof(float);
    if (c.workspace_bytes < p.need) return false;
    rt.splits = s;
    p.k_per_split = round_up(cdiv(k, s), unit);
    return true;
  };
  const bool tn = c.a_km && !c.b_nk, nt = !c.a_km && c.b_nk;
  if (tile_eligible(c)) {
    const int s = c.allow_split ? pick_splits(m, n, k, c.a_km, c.es == 2 && c.b_nk) : 1;
    if (s > 1 && !split(s, kRowBytes / c.es)) return refuse(KRS_ERR_WORKSPACE, p.need);
    const int64_t kps = p.k_per_split, last = k - (int64_t)(s - 1) * kps, t256 = cdiv(m, kBigTile) * cdiv(n, kBigTile);
    const bool big = c.es == 2 && c.pipe != 0 && m >= kBigTile && n >= kBigTile;   // 256 x 256 tiles: bf16, pipelines 4 / 5
    // the LDS-DMA kernels of K-contiguous operands (no staging registers, no ds_write traffic): unsplit, whole tile rows
    const bool dma = nt && s == 1 && k % (kRowBytes / c.es) == 0;
    // the ring on K-contiguous operands: unsplit where its tiles fill the chip, split wherever every split holds a ring
    if (big && nt && k >= kRingMinK && k % kRingBlock == 0 && kps % kRingBlock == 0 && last >= kRingDepth * kRingBlock &&
        (s > 1 || (dma && t256 >= kFillTiles))) {
      const bool k64 = c.pipe == 4 && k % kRing64Block == 0 && kps % kRing64Block == 0 && last >= kRing64Depth * kRing64Block;
      rt.kernel = k64 ? KRS_GEMM_KERNEL_PP64 : KRS_GEMM_KERNEL_PP256;
      p.nt = (int)cdiv(n, kBigTile);
      p.grid[0] = round_up(cdiv(m, kBigTile), 8) * p.nt * s;
      p.lds = k64 ? kRing64Lds : kRingLds;
    } else if (dma && k >= kGldsMinK) {
      rt.kernel = KRS_GEMM_KERNEL_GLDS;
      p.lds = kGldsLds;
    } else if (c.es == 2 && tn && k % 64 == 0 && kps % 64 == 0 && m >= 8 && n >= 8 && m % 8 == 0 && n % 8 == 0) {
      // bf16 weight gradients: tiles DMA'd as they lie, transposing LDS reads (K in whole 64-row tiles, whole vectors of C)
      const bool ring = big && !c.tn128 && kps >= kRingMinK;
      rt.kernel = ring ? KRS_GEMM_KERNEL_PP256_KSTRIDED : KRS_GEMM_KERNEL_TN_GLDS;
      p.mt = (int)cdiv(m, ring ? kBigTile : kTile), p.nt = (int)cdiv(n, ring ? kBigTile : kTile);
      p.grid[0] = ring ? round_up((int64_t)s * p.mt * p.nt, 8) : round_up(s, 8) * p.mt * p.nt;   // splits dealt to the 8 XCDs
      p.lds = ring ? kRingLds : kGldsLds;
    } else {
      rt.kernel = KRS_GEMM_KERNEL_MFMA;
      p.lds = 2 * kTileBytes;
    }
    if (p.lds == kRingLds || p.lds == kRing64Lds) p.block = 512;
    if (rt.kernel == KRS_GEMM_KERNEL_GLDS || rt.kernel == KRS_GEMM_KERNEL_MFMA) {
      p.grid[0] = (c.a_km ? cdiv(m, kTile) : round_up(cdiv(m, kTile), 8)) * cdiv(n, kTile);
      p.grid[2] = s;
    }
    // the specialised epilogue builds of these four kernels: bf16 output, vector access everywhere, no split-K
    if (rt.kernel != KRS_GEMM_KERNEL_PP256_KSTRIDED && rt.kernel != KRS_GEMM_KERNEL_TN_GLDS && c.has_ep && rt.ep_vec &&
        s == 1 && c.out_dtype == KRS_BF16 && n >= 8) {
      if (c.x0 && !c.r) rt.epilogue = 1;
      else if (c.r && !c.x0 && !c.bias && c.act == KRS_ACT_NONE) rt.epilogue = 2;
    }
    // the epilogue schedules of gemm_pp64_kernel's streaming builds (KRS_GEMM_OPT_EPI_SCHEDULE); the landing region lies
    // inside the ring's LDS (kEpiStageBytes + kEpiLandBytes <= kRing64Lds, asserted next to the kernel and by the lattice walk)
    if (rt.kernel == KRS_GEMM_KERNEL_PP64 && rt.epilogue != 0) {
      if ((c.epi_sched & 1) && rt.epilogue == 1) rt.schedule |= c.x_is_x0 ? KRS_GEMM_SCHED_X_IS_X0 : KRS_GEMM_SCHED_LDS_LANDING;
      if (c.epi_sched & 2) rt.schedule |= KRS_GEMM_SCHED_STAGGER;
    }
    const bool vec4 = !c.has_ep && c.out_dtype == KRS_F32 && n % 4 == 0 && c.ldc % 4 == 0 && c.al_c;
    if (s > 1) rt.reduce = vec4 ? KRS_GEMM_REDUCE_VEC4 : (rt.ep_vec ? KRS_GEMM_REDUCE_VEC8 : KRS_GEMM_REDUCE_SCALAR);
  } else if (tn && thin_shape(m, n, k)) {
    // weight gradients the tile kernels refuse, one tiny dimension: split when the workspace allows, never refused
    if (!split(pick_splits(m, n, k, true, false), 1)) p.need = 0;
    const int64_t n_thin = std::min(m, n);
    rt.kernel = KRS_GEMM_KERNEL_THIN;
    rt.thin_is_a = m <= n;
    rt.thin_width = n_thin <= 1 ? 1 : (n_thin <= 4 ? 4 : (n_thin <= 8 ? 8 : 16));
    p.grid[0] = cdiv(std::max(m, n), 256);
    p.grid[1] = rt.splits;
    if (rt.splits > 1) rt.reduce = KRS_GEMM_REDUCE_SCALAR;
  } else if (!c.a_km && n <= kRowdotMaxN && k >= kRowdotMinK && m >= kRowdotMinM) {
    rt.kernel = KRS_GEMM_KERNEL_ROWDOT;
    p.grid[0] = cdiv(m, kRowdotRows);
  } else if (!c.a_km && k <= kSmallkMaxK && n % 8 == 0 && n <= kSmallkMaxN && m * n >= kSmallkMinMN) {
    rt.kernel = KRS_GEMM_KERNEL_SMALLK;
    p.grid[0] = cdiv(m, kSmallkRows);
    p.lds = (size_t)k * n * sizeof(float);
  } else {
    rt.kernel = KRS_GEMM_KERNEL_GENERIC;
    p.grid[0] = cdiv(m * n, 256);
  }
  if (rt.reduce) p.reduce_grid = cdiv(m * (rt.reduce == KRS_GEMM_REDUCE_VEC4 ? n / 4 : rt.reduce == KRS_GEMM_REDUCE_VEC8 ? n / 8 : n), 256);
  if (p.grid[0] * p.block > kMaxGridThreads || p.reduce_grid * 256 > kMaxGridThreads || p.grid[1] > kMaxGridYZ || p.grid[2] > kMaxGridYZ)
    return refuse(KRS_ERR_UNSUPPORTED, 0);
  return p;
}

struct CrossBwdPlan {
  int route = KRS_CROSS_BWD_NONE, epilogue = 0;   // KRS_CROSS_BWD_*; the fused epilogue number 3 .. 10, else 0
  bool stagger = false;                           // fused on the 64-k ring under KRS_GEMM_OPT_EPI_SCHEDULE 2 / 3
  GemmPlan product;                               // fused: grid, LDS bytes and nt of the ring launch
};

// krs_gemm_cross_bwd / krs_gemm_dense_bwd.  cb.product: the plan of the call the two-call form would make (nt, R as the
// epilogue's residual, C = g_out, allow_split = false); x0, u, dz, dx0, u_upper lie on `ld` (al_streams: all on 16 bytes).
// Fused exactly where plan_gemm gave that product a ring kernel -- the same predicate, not a restatement -- and every
// stream is vector-accessible; the ring (64-k under pipeline 4, 32-k under 5) is the one plan_gemm named.
inline void plan_cross_bwd(CrossBwdPlan& cb, bool has_r, int64_t ld, bool al_streams, bool dense, bool store_g, bool has_dx0,
                           bool dx0_accumulate, bool has_u_upper, int epi_sched = 0) {
  const krs_gemm_route& rt = cb.product.route;
  cb.route = rt.kernel == KRS_GEMM_KERNEL_PP64 ? KRS_CROSS_BWD_PP64 : KRS_CROSS_BWD_PP256;
  cb.epilogue = 0;
  if ((rt.kernel != KRS_GEMM_KERNEL_PP64 && rt.kernel != KRS_GEMM_KERNEL_PP256) || rt.splits != 1 || !rt.ep_vec || ld % 8 != 0 ||
      !al_streams)
    cb.route = rt.kernel == KRS_GEMM_KERNEL_NONE ? KRS_CROSS_BWD_NONE : KRS_CROSS_BWD_TWO_CALL;
  else if (dense) cb.epilogue = store_g ? 10 : 9;
  else if (has_u_upper) cb.epilogue = 7;
  else if (has_r) cb.epilogue = dx0_accumulate ? 4 : 3;
  else cb.epilogue = !has_dx0 ? 8 : (dx0_accumulate ? 6 : 5);
  cb.stagger = cb.route == KRS_CROSS_BWD_PP64 && (epi_sched & 2);
}

}  // namespace gplan
}  // namespace krs
#endif
