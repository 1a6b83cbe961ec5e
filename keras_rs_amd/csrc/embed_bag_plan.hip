// K2 -- the PLAN of the index-scatter gradient of the fused embedding bag: everything that depends on the ids alone.
// The apply kernels that consume it are in embed_bag_bwd.hip; the two share the workspace layout of krs_bag_plan.h.
//
// Plan (once per batch of ids, independent of the gradient values):
//   keys[p] = tables[t(f)].row_base + ids[p]   (u32; invalid ids -> 0xffffffff)
//   vals[p] = (bag(p) << 32) | p               (u64)
//   stable LSD radix sort of (keys, vals) over ceil(log2(total_rows)) bits (namespace rs below: own kernels;
//   dense bags whose tables form contiguous runs of positions are sorted per table, over the id bits alone).
//   head flags -> exclusive scan -> segment list (first sorted position of every run of equal
//   keys), and the work items of the segments longer than kLongSeg lookups.
// Equal keys keep their input order, so the apply kernels sum a row's contributions in ascending p
//   => run-to-run bit-identical.
#include <algorithm>

#include "krs_bag_plan.h"

namespace krs {
// krs_embed_set_option(KRS_EMBED_OPT_PLAN, v): 0 = table-segmented sort where the layout allows it (default), 1 = always the global sort
int g_plan_variant = 0;
// krs_embed_set_option(KRS_EMBED_OPT_RANK, v): how a scatter pass ranks the keys of a round (rs::count_rank below) -- 0 = by the
// LDS counts, ballots only for rounds with many collisions (default), 1 = always ballots (A/B), 2 = always by the counts
int g_rank_mode = 0;
namespace {

// ---- plan: the sort (LSD radix sort of (row key, bag << 32 | position) pairs, written for this plan) -----------
// Digits of up to 10 bits, ceil(bits / 10) passes over ceil(log2(total_rows + 1)) key bits (C3: 25 bits = 3 passes,
// against 4 passes of 8 bits over the same bits in a general-purpose device sort).  One pass = per-tile digit
// histogram -> exclusive scan of the [digit][tile] counts (krs_scan.h) -> stable scatter.  A tile is 4096 consecutive
// lookups, one workgroup; wave w owns the w-th quarter, so the (wave, round, lane) order IS the input order and
// the ranks below keep equal keys in input order (stability = ascending position inside a row's segment = a fixed
// summation order in the apply kernels).  Dense bags: the first pass computes keys and values from the ids on the
// fly (no key generation kernel, no round trip of 12 bytes per lookup through HBM).
// Two sorts are built from the pieces below: the GLOBAL one (hist_kernel / scatter_kernel: any bags, 64-bit payload)
// and the one SEGMENTED BY TABLE (hist_seg_kernel / scatter_seg_kernel: dense bags, 32-bit payload).  They differ in
// how a tile is found, how its keys are loaded and what the last pass writes; everything else is shared.
namespace rs {
constexpr int kHistThreads = 256, kHistItems = kTile / kHistThreads;
constexpr int kThreads = 512, kWaves = kThreads / 64, kItems = kTile / kThreads;   // scatter: 8 waves x 512 lookups
constexpr int kGenFeats = 256;   // features whose descriptors the generating pass caches in LDS

struct Gen {   // key generation for dense bags (first pass)
  const krs_table* tables;
  const krs_feature* feats;
  int n_feats;
  const void* ids;
  int id64;
  int batch;
  int* err_flag;
};

// per-feature constants of the generating pass, in LDS (padded to 16 bytes: the kernels' LDS sizes stay multiples of 16)
struct alignas(16) GenLds {
  uint32_t base[kGenFeats + 1];   // first lookup position of the feature (nnz < 2^31)
  uint32_t hot[kGenFeats];
  uint32_t row_base[kGenFeats];   // total_rows < 2^32 (checked by the plan)
  uint32_t vocab[kGenFeats];
};
__device__ __forceinline__ void load_gen(const Gen& gen, int64_t nnz, GenLds& g, int n_threads) {
  for (int i = threadIdx.x; i <= gen.n_feats; i += n_threads) {
    if (i < gen.n_feats) {
      const krs_feature ft = gen.feats[i];
      const krs_table tb = gen.tables[ft.table];
      g.base[i] = (uint32_t)ft.ids_base;
      g.hot[i] = (uint32_t)ft.hot;
      g.row_base[i] = (uint32_t)tb.row_base;
      g.vocab[i] = (uint32_t)tb.vocab;
    } else {
      g.base[i] = (uint32_t)nnz;
    }
  }
}
// feature of lookup position q; dense bags, features laid out one after the other
__device__ __forceinline__ int gen_feature(const GenLds& g, int n_feats, uint32_t q) {
  int lo = 0, hi = n_feats;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (g.base[mid] <= q) lo = mid; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ uint64_t gen_value(const Gen& gen, const GenLds& g, int f, uint32_t q) {
  const uint32_t bag = (uint32_t)f * (uint32_t)gen.batch + (q - g.base[f]) / g.hot[f];
  return ((uint64_t)bag << 32) | (uint64_t)q;
}
// (key, value) of lookup position q; false = the id is out of range (key = kInvalidKey)
__device__ __forceinline__ bool generate(const Gen& gen, const GenLds& g, uint32_t q, uint32_t& key, uint64_t& val) {
  const int f = gen_feature(g, gen.n_feats, q);
  const int64_t id = ld_index(gen.ids, gen.id64, q);
  const bool valid = id >= 0 && id < (int64_t)g.vocab[f];
  key = valid ? g.row_base[f] + (uint32_t)id : kInvalidKey;
  val = gen_value(gen, g, f, q);
  return valid;
}

__device__ __forceinline__ int digit_of(uint32_t key, int shift, int bins) { return (int)((key >> shift) & (bins - 1)); }

// Which tile workgroup b takes.  Workgroups are dealt round-robin to the chip's eight XCDs (each with an L2 of its own), so b
// and b + 8 share one; they take CONSECUTIVE tiles: a digit's pieces of neighbouring tiles -- runs of about four keys = 16
// bytes with 1024 digits -- and the neighbouring 4-byte counters of the [digit][tile] matrix then meet in one L2 and
// leave it as whole lines.  The grid is tile_grid(tiles) = 8 * ceil(tiles / 8) workgroups; those whose tile lies past the
// end exit.  A bijection on the tiles whatever the placement: where a workgroup runs changes the speed only.
// (Multi-hot C3 plan, table-segmented: 533 -> 411 us; docs/measurement_log.md, K2 plan ranking.)
__device__ __forceinline__ uint32_t tile_of_block(uint32_t b, uint32_t tiles) { return (b & 7) * ((tiles + 7) / 8) + (b >> 3); }
inline unsigned tile_grid(unsigned tiles) { return (tiles + 7) / 8 * 8; }

// ---- histogram pass: the tile's digit counts, in LDS, to the tile's column of the [digit][tile] count matrix ----
__device__ __forceinline__ void hist_zero(int (&h)[kMaxBins], int bins) {
  for (int i = threadIdx.x; i < bins; i += kHistThreads) h[i] = 0;
}
__device__ __forceinline__ void hist_add(int (&h)[kMaxBins], uint32_t key, int shift, int bins) {
  atomicAdd(&h[digit_of(key, shift, bins)], 1);
}
// col / stride: the tile's column of the count matrix.  bad: this thread met an out-of-range id (the histogram pass
// that reads the ids reports them; the scatter pass of the same data does not look)
__device__ __forceinline__ void hist_finish(const int (&h)[kMaxBins], int bins, int32_t* col, int64_t stride, bool bad,
                                            int* err_flag) {
  if (bad && err_flag) atomicOr(err_flag, KRS_FLAG_ID_OUT_OF_RANGE);
  __syncthreads();
  for (int i = threadIdx.x; i < bins; i += kHistThreads) col[(int64_t)i * stride] = h[i];
}

// ---- scatter pass: LDS of one tile; V = the payload that travels with a key ----
// (74 KB with a 64-bit payload: two workgroups (16 waves) per CU; 16-byte aligned: wtot is read with 128-bit loads)
template <typename V>
struct alignas(16) TileLds {
  uint16_t cnt[kWaves][kMaxBins];   // per wave: elements of each digit seen so far -> (wave, digit) start
  uint16_t tile_excl[kMaxBins];     // first slot of every digit in the tile's sorted image
  int gbase[kMaxBins];              // first output slot of the tile's elements of every digit
  uint32_t skey[kTile];             // the tile, sorted by digit (stable): consecutive threads then
  V sval[kTile];                    // write consecutive output slots inside a digit's run
  int wtot[kWaves];
};
template <typename V>
__device__ __forceinline__ void zero_counts(TileLds<V>& s) {
  for (int i = threadIdx.x; i < kWaves * kMaxBins; i += kThreads) (&s.cnt[0][0])[i] = 0;
}
// Lanes of this round whose key has this lane's digit: one ballot per digit bit (gfx950 has no match_any).
__device__ __forceinline__ unsigned long long digit_peers(int d, bool live, int bits) {
  unsigned long long peers = __ballot(live);
  for (int b = 0; b < bits; ++b) {
    const unsigned long long m = __ballot((d >> b) & 1);
    peers &= ((d >> b) & 1) ? m : ~m;
  }
  return peers;
}
// One round of ballot ranking: the rank of this lane's key among the keys of the same digit that its wave has seen so
// far (`mine` = the wave's row of cnt; dead lanes take no part and get 0).  `bits` ballots per round, and the rounds of a
// wave are a serial chain through the leader's read-modify-write of the counter.
__device__ __forceinline__ int ballot_rank(uint32_t key, bool live, int shift, int bits, volatile uint16_t* mine,
                                           int lane) {
  const int d = digit_of(key, shift, 1 << bits);
  const unsigned long long peers = digit_peers(d, live, bits);
  int r = 0, c = 0;
  if (live) {
    r = __popcll(peers & ((1ULL << lane) - 1ULL));
    const int leader = __ffsll((long long)peers) - 1;
    if (lane == leader) {
      c = mine[d];
      mine[d] = (uint16_t)(c + __popcll(peers));
    }
    c = __shfl(c, leader, 64);
  }
  __builtin_amdgcn_wave_barrier();
  return c + r;
}
// Count-and-fix ranking of all the thread's rounds: the same ranks and the same final counters as kItems calls of
// ballot_rank, found from the counters themselves.  The wave's row of cnt is read as 32-bit words (digit d = half d & 1
// of word d >> 1; a wave sees at most 512 keys of a tile, so a half never carries into the other).  A round reads its
// lanes' words, adds one to the digit's half with an LDS add that returns nothing, and reads the words again: the adds
// of one instruction commute, so what the second read sees does not depend on the order in which the hardware serves
// the lanes.  The first read holds c, the digit's count before the round; the difference n, the live lanes of the
// round with that digit.  n == 1 (nearly every key when the digit is wide): rank = c, no ballot.  n > 1: one ballot
// per collided group of the round, lanes ranked in ascending order = input order (stable).  A wave's LDS instructions
// execute in order, so all rounds' instructions are issued back to back (a later round's first read sees the earlier
// rounds' adds) and waited for once.  `fallback`: a round in which more groups may have collided than its digit has
// bits is ranked by digit_peers instead (narrow digits, tiny vocabularies, hot rows); never both forms in one round.
typedef uint32_t __attribute__((may_alias)) cnt_word;
__device__ __forceinline__ void count_rank(const uint32_t (&key)[kItems], int64_t first, int64_t end, int shift, int bits,
                                           bool fallback, uint16_t* mine, int lane, int (&rank)[kItems]) {
  cnt_word* word = reinterpret_cast<cnt_word*>(mine);
  uint32_t before[kItems], after[kItems];
#pragma unroll
  for (int it = 0; it < kItems; ++it) {
    const int d = digit_of(key[it], shift, 1 << bits);
    const bool live = first + it * 64 < end;
    cnt_word* w = word + (d >> 1);
    before[it] = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    __builtin_amdgcn_wave_barrier();
    // (dead lanes add 0: no change of the execution mask between the LDS instructions)
    __hip_atomic_fetch_add(w, live ? 1u << (16 * (d & 1)) : 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    __builtin_amdgcn_wave_barrier();
    after[it] = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    __builtin_amdgcn_wave_barrier();
  }
  const unsigned long long below = (1ULL << lane) - 1ULL;
#pragma unroll
  for (int it = 0; it < kItems; ++it) {
    const int d = digit_of(key[it], shift, 1 << bits);
    const bool live = first + it * 64 < end;
    const int c = (int)((before[it] >> (16 * (d & 1))) & 0xffffu);
    const int n = (int)((after[it] >> (16 * (d & 1))) & 0xffffu) - c;
    int r = c;
    unsigned long long pend = __ballot(live && n > 1);   // lanes of collided groups
    if (fallback && __popcll(pend) / 2 > bits) {
      r = c + __popcll(digit_peers(d, live, bits) & below);
    } else {
      while (pend) {
        const int leader = __ffsll((long long)pend) - 1;
        const int dl = __builtin_amdgcn_readlane(d, leader);
        const unsigned long long peers = __ballot(live && d == dl);
        if (d == dl) r = c + __popcll(peers & below);
        pend &= ~peers;
      }
    }
    rank[it] = live ? r : 0;
  }
}
// The ranks of the thread's keys (positions first + it * 64, live below end) by the form that `mode` (g_rank_mode) asks for.
__device__ __forceinline__ void rank_keys(const uint32_t (&key)[kItems], int64_t first, int64_t end, int shift, int bits,
                                          int mode, uint16_t* mine, int lane, int (&rank)[kItems]) {
  if (mode == 1) {
#pragma unroll
    for (int it = 0; it < kItems; ++it) rank[it] = ballot_rank(key[it], first + it * 64 < end, shift, bits, mine, lane);
  } else {
    count_rank(key, first, end, shift, bits, mode == 0, mine, lane, rank);
  }
}
// Once every wave has ranked its keys: digit totals of the tile -> exclusive scan over the digits (bins <= 1024 = 2 per
// thread) -> tile_excl, the (wave, digit) starts (in place of the counts) and gbase from the tile's column (col /
// stride) of the scanned count matrix.
template <typename V>
__device__ __forceinline__ void digit_bases(TileLds<V>& s, int bins, const int32_t* col, int64_t stride) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  int tot[2], run = 0;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int i = threadIdx.x * 2 + k;
    tot[k] = 0;
    if (i < bins)
      for (int w = 0; w < kWaves; ++w) tot[k] += s.cnt[w][i];
    run += tot[k];
  }
  int x = run;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) s.wtot[wave] = x;
  __syncthreads();
  int excl = x - run;
  for (int w = 0; w < wave; ++w) excl += s.wtot[w];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int i = threadIdx.x * 2 + k;
    if (i < bins) {
      s.tile_excl[i] = (uint16_t)excl;
      s.gbase[i] = col[(int64_t)i * stride];
      int o = excl;
      for (int w = 0; w < kWaves; ++w) {
        const int t = s.cnt[w][i];
        s.cnt[w][i] = (uint16_t)o;
        o += t;
      }
      excl += tot[k];
    }
  }
  __syncthreads();
}
// The thread's ranked elements (positions first + it * 64, live below end) to their slots of the tile's sorted image.
template <typename V>
__device__ __forceinline__ void stage_tile(TileLds<V>& s, const uint32_t (&key)[kItems], const V (&val)[kItems],
                                           const int (&rank)[kItems], int64_t first, int64_t end, int shift, int bins) {
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int it = 0; it < kItems; ++it) {
    if (first + it * 64 < end) {
      const int lp = s.cnt[wave][digit_of(key[it], shift, bins)] + rank[it];
      s.skey[lp] = key[it];
      s.sval[lp] = val[it];
    }
  }
  __syncthreads();
}
// output slot of staged element i, whose digit is d
template <typename V>
__device__ __forceinline__ int out_slot(const TileLds<V>& s, int i, int d) {
  return s.gbase[d] + (i - (int)s.tile_excl[d]);
}

// ---- the global sort ----------------------------------------------------------------------------------------
struct Pass {
  const uint32_t* keys_in;     // null in a generating pass
  const uint64_t* vals_in;
  uint32_t* keys_out;
  uint64_t* vals_out;
  int32_t* counts;             // [bins][tiles]: histogram, then exclusive offsets
  int64_t nnz;
  int n_tiles;
  int shift, bits;
  int rank;                    // g_rank_mode
  Gen gen;
};

template <bool GEN>
__global__ __launch_bounds__(kHistThreads) void hist_kernel(const Pass p) {
  __shared__ int h[kMaxBins];
  __shared__ GenLds g;
  const uint32_t tile = tile_of_block(blockIdx.x, p.n_tiles);
  if (tile >= (uint32_t)p.n_tiles) return;
  const int bins = 1 << p.bits;
  hist_zero(h, bins);
  if constexpr (GEN) load_gen(p.gen, p.nnz, g, kHistThreads);
  __syncthreads();
  const int64_t base = (int64_t)tile * kTile;
  bool bad = false;
  for (int it = 0; it < kHistItems; ++it) {
    const int64_t q = base + it * kHistThreads + threadIdx.x;
    if (q < p.nnz) {
      uint32_t key;
      if constexpr (GEN) {
        uint64_t v;
        bad |= !generate(p.gen, g, (uint32_t)q, key, v);
      } else {
        key = p.keys_in[q];
      }
      hist_add(h, key, p.shift, bins);
    }
  }
  hist_finish(h, bins, p.counts + tile, p.n_tiles, bad, p.gen.err_flag);
}

template <bool GEN>
__global__ __launch_bounds__(kThreads) void scatter_kernel(const Pass p) {
  __shared__ TileLds<uint64_t> s;
  __shared__ GenLds g;
  const uint32_t tile = tile_of_block(blockIdx.x, p.n_tiles);
  if (tile >= (uint32_t)p.n_tiles) return;
  const int bins = 1 << p.bits;
  zero_counts(s);
  if constexpr (GEN) load_gen(p.gen, p.nnz, g, kThreads);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t tile0 = (int64_t)tile * kTile;
  const int64_t first = tile0 + (int64_t)wave * (kTile / kWaves) + lane;
  uint32_t key[kItems];
  uint64_t val[kItems];
  int rank[kItems];
#pragma unroll
  for (int it = 0; it < kItems; ++it) {
    const int64_t q = first + it * 64;
    const bool live = q < p.nnz;
    key[it] = kInvalidKey;
    val[it] = 0;
    if (live) {
      if constexpr (GEN) {
        generate(p.gen, g, (uint32_t)q, key[it], val[it]);
      } else {
        key[it] = p.keys_in[q];
        val[it] = p.vals_in[q];
      }
    }
  }
  rank_keys(key, first, p.nnz, p.shift, p.bits, p.rank, s.cnt[wave], lane, rank);
  digit_bases(s, bins, p.counts + tile, p.n_tiles);
  stage_tile(s, key, val, rank, first, p.nnz, p.shift, bins);
  const int n_here = (int)min<int64_t>(kTile, p.nnz - tile0);
#pragma unroll
  for (int it = 0; it < kItems; ++it) {
    const int i = it * kThreads + threadIdx.x;
    if (i < n_here) {
      const uint32_t k = s.skey[i];
      const int pos = out_slot(s, i, digit_of(k, p.shift, bins));
      p.keys_out[pos] = k;
      p.vals_out[pos] = s.sval[i];
    }
  }
}

// ---- the same sort, SEGMENTED BY TABLE (round 3) ------------------------------------------------------------
// Dense bags arrive feature-major, so the lookups of one table already form ONE contiguous run of positions (when
// the features of a table are neighbours and tables ascend with the features -- what DistributedEmbedding builds).
// Sorting by the global row then needs no pass over the table bits: every table's run is an independent PROBLEM,
// sorted in place by the id alone -- ceil(log2(max vocab + 1)) bits, 20 at C3 = TWO passes instead of three -- and
// the problems' sorted runs, one after the other, are exactly the global order.  Tiles never straddle problems
// (a problem's last tile may be partial); the count matrix is laid out [problem][digit][tile of the problem], so
// ONE exclusive scan over it still yields every tile's output offsets (a problem's lookups stay inside its run).
// Intermediate passes carry (local key, position) = 8 bytes per lookup instead of (key, bag << 32 | position) = 12;
// the LAST pass writes what the apply kernels read: the global key (row_base + id; all ones for an invalid id) and
// the 64-bit value, whose bag is recomputed from the position (feature constants in LDS, as the first pass does).
// Per lookup 40 bytes move instead of 76.  Out-of-range ids sort to the END OF THEIR TABLE'S RUN (sentinel = all
// ones in the key bits), not to the end of the array: the apply kernels skip invalid segments wherever they are;
// the compact (sparse) form, whose output is indexed by segment, keeps the global sort.
// (Measured and not kept: sorting each feature's lookups by row id alone when every feature has its own table -- the
//  lookups arrive grouped by feature, so two 10-bit passes replace the three 9/8/8-bit ones at 26 x 1 M rows: 602 us
//  either way; the scatter pass pays per key BIT (ballots), 20 against 25, and the per-feature tile bookkeeping and the
//  wider count matrix took the difference back.)
struct Seg {
  int n;                                  // problems
  uint32_t lookup_start[kMaxProb + 1];    // first lookup position of problem i; [n] = nnz
  uint32_t tile_start[kMaxProb + 1];      // first tile of problem i; [n] = tiles in all
  uint32_t row_base[kMaxProb];            // global row of the table's row 0
};
struct SegPass {
  const uint32_t* keys_in;     // FIRST pass: null (keys come from the ids)
  const uint32_t* pos_in;
  uint32_t* keys_out;          // LAST pass: global keys
  uint32_t* pos_out;           // intermediate passes
  uint64_t* vals_out;          // LAST pass
  int32_t* counts;
  int64_t nnz;
  int shift, bits, key_bits;
  int rank;                    // g_rank_mode
  Gen gen;
  Seg seg;
};
// where workgroup `tile` works
struct SegTile {
  int pr;             // its problem
  int64_t t0, end;    // its lookup positions
  int32_t* col;       // its column of the problem's [digit][tile] block of the count matrix
  uint32_t stride;    // = tiles of the problem
};
__device__ __forceinline__ SegTile seg_tile(const SegPass& p, uint32_t tile) {
  const Seg& sg = p.seg;
  int lo = 0, hi = sg.n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (sg.tile_start[mid] <= tile) lo = mid; else hi = mid;
  }
  SegTile t;
  t.pr = lo;
  const uint32_t tl = tile - sg.tile_start[lo];
  t.stride = sg.tile_start[lo + 1] - sg.tile_start[lo];
  t.t0 = (int64_t)sg.lookup_start[lo] + (int64_t)tl * kTile;
  t.end = min<int64_t>(t.t0 + kTile, sg.lookup_start[lo + 1]);
  t.col = p.counts + ((int64_t)1 << p.bits) * sg.tile_start[lo] + tl;
  return t;
}
// FIRST pass: the local keys of the thread's ITEMS positions first + it * STRIDE of tile t (key = the id, or all ones
// in the key bits when it is out of range), positions clamped to the tile.  All ids are requested before the first is
// looked at.  Returns whether one of the thread's positions inside the tile is out of range.
template <int ITEMS, int STRIDE>
__device__ __forceinline__ bool seg_first_keys(const SegPass& p, const GenLds& g, const SegTile& t, int64_t first,
                                               uint32_t (&key)[ITEMS], uint32_t (&pos)[ITEMS]) {
  int64_t idv[ITEMS];
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) idv[it] = ld_index(p.gen.ids, p.gen.id64, min<int64_t>(first + it * STRIDE, t.end - 1));
  // (a tile lies inside ONE feature almost always -- tiles never straddle tables, and a table's features are few: the
  //  per-key search over the feature bases is then one search per tile; round 5)
  const int f_lo = gen_feature(g, p.gen.n_feats, (uint32_t)t.t0), f_hi = gen_feature(g, p.gen.n_feats, (uint32_t)(t.end - 1));
  bool bad = false;
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) {
    const int64_t q = min<int64_t>(first + it * STRIDE, t.end - 1);
    const int f = f_lo == f_hi ? f_lo : gen_feature(g, p.gen.n_feats, (uint32_t)q);
    const bool valid = idv[it] >= 0 && idv[it] < (int64_t)g.vocab[f];
    key[it] = valid ? (uint32_t)idv[it] : (1u << p.key_bits) - 1u;
    pos[it] = (uint32_t)q;
    bad = bad || (!valid && first + it * STRIDE < t.end);
  }
  return bad;
}

// (Round 5 measured one workgroup per EIGHT consecutive tiles here, so that a digit's counters leave as 32 contiguous bytes:
//  the write counter of this kernel fell from 121 MB to 14 MB per launch -- one tile's 1024 counters are 1024 scattered
//  4-byte stores into the [digit][tile] matrix -- and the plan got SLOWER, 558 -> 582 us with 1024-thread groups (1815 us
//  with 256-thread ones): the kernel wants its 3400 independent workgroups.  tile_of_block keeps them and puts the eight
//  neighbouring columns into one L2 instead: 40 -> 26 us in the second pass.)
template <bool FIRST>
__global__ __launch_bounds__(kHistThreads) void hist_seg_kernel(const SegPass p) {
  __shared__ int h[kMaxBins];
  __shared__ GenLds g;
  const uint32_t tile = tile_of_block(blockIdx.x, p.seg.tile_start[p.seg.n]);
  if (tile >= p.seg.tile_start[p.seg.n]) return;
  const int bins = 1 << p.bits;
  hist_zero(h, bins);
  if constexpr (FIRST) load_gen(p.gen, p.nnz, g, kHistThreads);
  __syncthreads();
  const SegTile t = seg_tile(p, tile);
  const int64_t first = t.t0 + threadIdx.x;
  bool bad = false;
  uint32_t key[kHistItems];
  if constexpr (FIRST) {
    uint32_t pos[kHistItems];
    bad = seg_first_keys<kHistItems, kHistThreads>(p, g, t, first, key, pos);
  } else {
#pragma unroll
    for (int it = 0; it < kHistItems; ++it) key[it] = p.keys_in[min<int64_t>(first + it * kHistThreads, t.end - 1)];
  }
#pragma unroll
  for (int it = 0; it < kHistItems; ++it)
    if (first + it * kHistThreads < t.end) hist_add(h, key[it], p.shift, bins);
  hist_finish(h, bins, t.col, t.stride, bad, p.gen.err_flag);
}

template <bool FIRST, bool LAST>
__global__ __launch_bounds__(kThreads) void scatter_seg_kernel(const SegPass p) {
  __shared__ TileLds<uint32_t> s;   // the payload is the lookup's position
  __shared__ GenLds g;
  const uint32_t tile = tile_of_block(blockIdx.x, p.seg.tile_start[p.seg.n]);
  if (tile >= p.seg.tile_start[p.seg.n]) return;
  const int bins = 1 << p.bits;
  zero_counts(s);
  if constexpr (FIRST || LAST) load_gen(p.gen, p.nnz, g, kThreads);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const SegTile t = seg_tile(p, tile);
  const int64_t first = t.t0 + (int64_t)wave * (kTile / kWaves) + lane;
  uint32_t key[kItems], pos[kItems];
  int rank[kItems];
  // all of the thread's keys are requested before the first is ranked (addresses clamped to the tile, dead slots
  // masked afterwards): one exposed memory latency per tile instead of one per round of the ranking loop below,
  // whose LDS counter updates form a dependent chain the loads could not be scheduled across
  if constexpr (FIRST) {
    seg_first_keys<kItems, 64>(p, g, t, first, key, pos);
  } else {
#pragma unroll
    for (int it = 0; it < kItems; ++it) {
      const int64_t q = min<int64_t>(first + it * 64, t.end - 1);
      key[it] = p.keys_in[q];
      pos[it] = p.pos_in[q];
    }
  }
#pragma unroll
  for (int it = 0; it < kItems; ++it) {
    const bool live = first + it * 64 < t.end;
    if (!live) { key[it] = 0xffffffffu; pos[it] = 0; }
  }
  rank_keys(key, first, t.end, p.shift, p.bits, p.rank, s.cnt[wave], lane, rank);
  digit_bases(s, bins, t.col, t.stride);
  stage_tile(s, key, pos, rank, first, t.end, p.shift, bins);
  const int n_here = (int)(t.end - t.t0);
  const uint32_t sentinel = (1u << p.key_bits) - 1u, rb = p.seg.row_base[t.pr];
  // (last pass: a key's original position lies anywhere in its TABLE's run; a table looked up by one feature -- the usual
  //  case -- needs one search per tile instead of one per key)
  int pf_lo = 0, pf_hi = 1;
  if constexpr (LAST) {
    pf_lo = gen_feature(g, p.gen.n_feats, p.seg.lookup_start[t.pr]);
    pf_hi = gen_feature(g, p.gen.n_feats, p.seg.lookup_start[t.pr + 1] - 1);
  }
#pragma unroll
  for (int it = 0; it < kItems; ++it) {
    const int i = it * kThreads + threadIdx.x;
    if (i < n_here) {
      const uint32_t k = s.skey[i], q = s.sval[i];
      const int o = out_slot(s, i, digit_of(k, p.shift, bins));
      if constexpr (LAST) {
        const int f = pf_lo == pf_hi ? pf_lo : gen_feature(g, p.gen.n_feats, q);
        p.keys_out[o] = k == sentinel ? kInvalidKey : rb + k;
        p.vals_out[o] = gen_value(p.gen, g, f, q);
      } else {
        p.keys_out[o] = k;
        p.pos_out[o] = q;
      }
    }
  }
}

// ---- host side of both sorts ----
// Bits that tell the values 0 .. n apart: 2^bits - 1 > every valid key, so all ones still sorts last.
inline unsigned key_bits(int64_t n) {
  unsigned bits = 1;
  while (bits < 32 && (1ULL << bits) <= (uint64_t)n) ++bits;
  return bits;
}
// ceil(bits / kMaxBits) passes, low digit first, the bits spread evenly over them
struct Schedule {
  int passes;
  int bits[4], shift[4];
};
inline Schedule pass_schedule(unsigned bits) {
  Schedule s;
  s.passes = (int)((bits + kMaxBits - 1) / kMaxBits);
  unsigned done = 0;
  for (int ps = 0; ps < s.passes; ++ps) {
    s.bits[ps] = (int)((bits - done + (s.passes - ps) - 1) / (s.passes - ps));
    s.shift[ps] = (int)done;
    done += (unsigned)s.bits[ps];
  }
  return s;
}
inline Gen make_gen(const krs_table* tables, const krs_feature* feats, int n_feats, const void* ids, int id_type,
                    int batch, int* err_flag) {
  Gen g;
  g.tables = tables; g.feats = feats; g.n_feats = n_feats; g.ids = ids;
  g.id64 = id_type == KRS_I64; g.batch = batch; g.err_flag = err_flag;
  return g;
}
}  // namespace rs

// ---- plan: key generation ---------------------------------------------------
struct KeyParams {
  const krs_table* tables;
  const krs_feature* feats;
  int n_feats;
  const void* ids;
  int id64;
  const void* offsets;
  int off64;
  int batch;
  uint32_t* keys;
  uint64_t* vals;
  int* err_flag;
};

// 16 lanes per bag; lanes stride over the bag's positions (coalesced writes).
__global__ __launch_bounds__(256) void bag_keys_kernel(const KeyParams p) {
  const int64_t bag = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int sub = threadIdx.x & 15;
  if (bag >= (int64_t)p.n_feats * p.batch) return;
  const int f = (int)(bag / p.batch);
  const int b = (int)(bag - (int64_t)f * p.batch);
  const krs_feature ft = p.feats[f];
  const krs_table tb = p.tables[ft.table];
  int64_t s, e;
  if (p.offsets) {
    s = ld_index(p.offsets, p.off64, bag);
    e = ld_index(p.offsets, p.off64, bag + 1);
  } else {
    s = ft.ids_base + (int64_t)b * ft.hot;
    e = s + ft.hot;
  }
  int oob = 0;
  for (int64_t q = s + sub; q < e; q += 16) {
    const int64_t id = ld_index(p.ids, p.id64, q);
    uint32_t key = kInvalidKey;
    if (id >= 0 && id < tb.vocab)
      key = (uint32_t)(tb.row_base + id);
    else
      oob = 1;
    p.keys[q] = key;
    p.vals[q] = ((uint64_t)bag << 32) | (uint64_t)(uint32_t)q;
  }
  if (oob && p.err_flag) atomicOr(p.err_flag, KRS_FLAG_ID_OUT_OF_RANGE);
}

// ---- plan: segment list ---------------------------------------------------------
// Segment list (first sorted position of every run of equal keys) by block-wise compaction: heads are counted
// per block of 4096 keys, the block counts are scanned by one workgroup, and a second pass over the keys writes
// every head's position at (block offset + rank inside the block).  Two reads of the sorted keys and one
// compact write -- the flag / index arrays of a flags -> device-wide scan -> scatter pipeline (five launches,
// 0.5 GB of traffic at 14 M lookups) are not materialised.  A trailing run of invalid keys is a segment too.
constexpr int kSegTile = 4096, kSegItems = 16;   // 256 threads x 16 consecutive keys
__device__ __forceinline__ uint32_t seg_head_mask(const uint32_t* keys, int64_t nnz, int64_t t0) {
  if (t0 >= nnz) return 0u;
  uint32_t prev = t0 > 0 ? keys[t0 - 1] : ~keys[0];   // position 0 is a head
  uint32_t mask = 0u;
  if (t0 + kSegItems <= nnz) {
    const uint4* v = reinterpret_cast<const uint4*>(keys + t0);   // t0 is a multiple of 16: 64-byte aligned
#pragma unroll
    for (int q = 0; q < kSegItems / 4; ++q) {
      const uint4 k = v[q];
      mask |= (uint32_t)(k.x != prev) << (4 * q);
      mask |= (uint32_t)(k.y != k.x) << (4 * q + 1);
      mask |= (uint32_t)(k.z != k.y) << (4 * q + 2);
      mask |= (uint32_t)(k.w != k.z) << (4 * q + 3);
      prev = k.w;
    }
  } else {
    for (int k = 0; t0 + k < nnz; ++k) {
      const uint32_t cur = keys[t0 + k];
      mask |= (uint32_t)(cur != prev) << k;
      prev = cur;
    }
  }
  return mask;
}
__global__ __launch_bounds__(256) void seg_count_kernel(const uint32_t* keys, int64_t nnz, int32_t* block_heads) {
  __shared__ int total;
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  int c = __popc(seg_head_mask(keys, nnz, (int64_t)blockIdx.x * kSegTile + threadIdx.x * kSegItems));
  for (int o = 32; o; o >>= 1) c += __shfl_down(c, o, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(&total, c);   // integer: order does not matter
  __syncthreads();
  if (threadIdx.x == 0) block_heads[blockIdx.x] = total;
}
__global__ __launch_bounds__(256) void seg_emit_kernel(const uint32_t* keys, int64_t nnz, const int32_t* block_off,
                                                       uint32_t* seg_start, uint32_t* n_seg) {
  __shared__ int wsum[4];
  const int64_t t0 = (int64_t)blockIdx.x * kSegTile + threadIdx.x * kSegItems;
  const uint32_t mask = seg_head_mask(keys, nnz, t0);
  const int c = __popc(mask), lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int x = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) wsum[wave] = x;
  __syncthreads();
  uint32_t off = (uint32_t)block_off[blockIdx.x] + (uint32_t)(x - c);
  for (int w = 0; w < wave; ++w) off += (uint32_t)wsum[w];
  uint32_t m = mask;
  while (m) {
    const int k = __ffs(m) - 1;
    m &= m - 1;
    seg_start[off++] = (uint32_t)(t0 + k);
  }
  if (t0 < nnz && t0 + kSegItems >= nnz) *n_seg = off;   // the thread that holds the last key
}
__global__ void long_list_kernel(const uint32_t* seg_start, const uint32_t* n_seg, int64_t nnz, uint32_t* counters,
                                 LongItem* items, MultiSeg* multi) {
  // counters[0] = work items, [1] = partial rows handed out, [2] = multi-chunk segments
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t ns = *n_seg;
  if (u >= ns) return;
  const int64_t e = u + 1 < ns ? (int64_t)seg_start[u + 1] : nnz;
  const int64_t len = e - (int64_t)seg_start[u];
  if (len <= kLongSeg) return;
  const uint32_t nch = (uint32_t)((len + kChunk - 1) / kChunk);
  const uint32_t base = atomicAdd(counters, nch);
  uint32_t pb = 0xffffffffu;
  if (nch > 1) {
    pb = atomicAdd(counters + 1, nch);
    multi[atomicAdd(counters + 2, 1u)] = MultiSeg{(uint32_t)u, pb, nch};
  }
  for (uint32_t c = 0; c < nch; ++c) items[base + c] = LongItem{(uint32_t)u, c, nch > 1 ? pb + c : 0xffffffffu};
}

// Table-segmented sort (rs::scatter_seg_kernel) when the host descriptors are given and the lookups are laid out for
// it: dense bags, the features of a table neighbours, tables (and their row bases) ascending with the features.
// Returns true when it has enqueued the sort; false = the caller runs the global sort.
bool plan_sort_by_table(const PlanLayout& l, const rs::Temp& tmp, const rs::Gen& gen, const krs_table* tables_host,
                        int n_tables, const krs_feature* feats_host, int64_t nnz, hipStream_t st) {
  if (!tables_host || !feats_host || gen.n_feats > rs::kGenFeats || n_tables <= 0) return false;
  rs::SegPass sp;
  rs::Seg& sg = sp.seg;
  sg.n = 0;
  int64_t pos = 0, max_vocab = 0;
  int prev_table = -1;
  for (int f = 0; f < gen.n_feats; ++f) {
    const krs_feature& ft = feats_host[f];
    if (ft.hot < 1 || ft.ids_base != pos || ft.table < prev_table || ft.table >= n_tables) return false;
    if (ft.table != prev_table) {
      if (sg.n == rs::kMaxProb) return false;
      const krs_table& tb = tables_host[ft.table];
      if (prev_table >= 0 && tb.row_base < tables_host[prev_table].row_base + tables_host[prev_table].vocab) return false;
      sg.lookup_start[sg.n] = (uint32_t)pos;
      sg.row_base[sg.n] = (uint32_t)tb.row_base;
      max_vocab = std::max<int64_t>(max_vocab, tb.vocab);
      ++sg.n;
      prev_table = ft.table;
    }
    pos += (int64_t)gen.batch * ft.hot;
  }
  if (pos != nnz || sg.n == 0) return false;
  sg.lookup_start[sg.n] = (uint32_t)nnz;
  uint32_t tiles = 0;
  for (int i = 0; i < sg.n; ++i) {
    sg.tile_start[i] = tiles;
    tiles += (uint32_t)ceil_div((int64_t)sg.lookup_start[i + 1] - sg.lookup_start[i], rs::kTile);
  }
  sg.tile_start[sg.n] = tiles;
  if (tiles == 0) return false;
  // key = id, plus one pattern (all ones) for an out-of-range id
  const unsigned bits = rs::key_bits(max_vocab);
  if (bits > 31) return false;
  const rs::Schedule sch = rs::pass_schedule(bits);
  sp.counts = tmp.counts; sp.nnz = nnz; sp.key_bits = (int)bits; sp.rank = g_rank_mode;
  sp.gen = gen;
  // intermediate (key, position) pairs ping-pong between I0 = (keys_in, vals_in as u32) and I1 = (keys_sorted,
  // vals_sorted as u32); the LAST pass reads I0 and writes the final (keys_sorted, vals_sorted): the pass before it
  // writes I0, the one before that I1, ...
  uint32_t* k0 = l.keys_in; uint32_t* q0 = reinterpret_cast<uint32_t*>(l.vals_in);
  uint32_t* k1 = l.keys_sorted; uint32_t* q1 = reinterpret_cast<uint32_t*>(l.vals_sorted);
  for (int ps = 0; ps < sch.passes; ++ps) {
    const bool first = ps == 0, last = ps == sch.passes - 1;
    sp.bits = sch.bits[ps];
    sp.shift = sch.shift[ps];
    const bool out_is_i0 = ((sch.passes - 2 - ps) % 2) == 0;        // (meaningless for the last pass)
    const bool in_is_i0 = ((sch.passes - 1 - ps) % 2) == 0;         // the last pass reads I0
    sp.keys_in = first ? nullptr : (in_is_i0 ? k0 : k1);
    sp.pos_in = first ? nullptr : (in_is_i0 ? q0 : q1);
    sp.keys_out = last ? l.keys_sorted : (out_is_i0 ? k0 : k1);
    sp.pos_out = last ? nullptr : (out_is_i0 ? q0 : q1);
    sp.vals_out = last ? l.vals_sorted : nullptr;
    if (first) hipLaunchKernelGGL(rs::hist_seg_kernel<true>, dim3(rs::tile_grid(tiles)), dim3(rs::kHistThreads), 0, st, sp);
    else hipLaunchKernelGGL(rs::hist_seg_kernel<false>, dim3(rs::tile_grid(tiles)), dim3(rs::kHistThreads), 0, st, sp);
    scan::exclusive(tmp.counts, tmp.counts, (int64_t)(1 << sp.bits) * tiles, tmp.sums, nullptr, st);
    if (first && last) hipLaunchKernelGGL((rs::scatter_seg_kernel<true, true>), dim3(rs::tile_grid(tiles)), dim3(rs::kThreads), 0, st, sp);
    else if (first) hipLaunchKernelGGL((rs::scatter_seg_kernel<true, false>), dim3(rs::tile_grid(tiles)), dim3(rs::kThreads), 0, st, sp);
    else if (last) hipLaunchKernelGGL((rs::scatter_seg_kernel<false, true>), dim3(rs::tile_grid(tiles)), dim3(rs::kThreads), 0, st, sp);
    else hipLaunchKernelGGL((rs::scatter_seg_kernel<false, false>), dim3(rs::tile_grid(tiles)), dim3(rs::kThreads), 0, st, sp);
  }
  return true;
}

// Global sort (rs::scatter_kernel) of the (row key, bag << 32 | position) pairs over the significant bits of total_rows.
int plan_sort_global(const PlanLayout& l, const rs::Temp& tmp, const rs::Gen& gen, const void* offsets, int off_type,
                     int64_t nnz, int64_t total_rows, hipStream_t st) {
  const rs::Schedule sch = rs::pass_schedule(rs::key_bits(total_rows));
  // ping-pong between (keys_in, vals_in) and (keys_sorted, vals_sorted); the LAST pass must write the sorted pair
  // dense bags: keys are generated inside the first pass (feature constants cached in LDS)
  const bool gen_first = offsets == nullptr && gen.n_feats <= rs::kGenFeats;
  bool to_sorted = (sch.passes % 2) == 1;    // where the first pass writes
  if (!gen_first) {
    // CSR bags (or very many features): the key kernel walks the bags
    KeyParams kp;
    kp.tables = gen.tables; kp.feats = gen.feats; kp.n_feats = gen.n_feats; kp.ids = gen.ids; kp.id64 = gen.id64;
    kp.offsets = offsets; kp.off64 = off_type == KRS_I64; kp.batch = gen.batch; kp.err_flag = gen.err_flag;
    kp.keys = to_sorted ? l.keys_in : l.keys_sorted;
    kp.vals = to_sorted ? l.vals_in : l.vals_sorted;
    const int64_t n_bags = (int64_t)gen.n_feats * gen.batch;
    // lookup positions outside every bag (offsets[n_bags] < nnz: the padded tail of a static-capacity exchange)
    // must not carry stale keys: all ones = the invalid key, which sorts behind every row and is skipped
    KRS_HIP(hipMemsetAsync(kp.keys, 0xff, (size_t)nnz * sizeof(uint32_t), st));
    hipLaunchKernelGGL(bag_keys_kernel, dim3((unsigned)ceil_div(n_bags, 16)), dim3(256), 0, st, kp);
    KRS_CHECK_LAUNCH("bag_keys_kernel");
  }
  rs::Pass p;
  p.nnz = nnz;
  p.n_tiles = (int)ceil_div(nnz, rs::kTile);
  p.counts = tmp.counts;
  p.rank = g_rank_mode;
  p.gen = gen;
  for (int ps = 0; ps < sch.passes; ++ps) {
    p.bits = sch.bits[ps];
    p.shift = sch.shift[ps];
    const bool generating = gen_first && ps == 0;
    p.keys_in = generating ? nullptr : (to_sorted ? l.keys_in : l.keys_sorted);
    p.vals_in = generating ? nullptr : (to_sorted ? l.vals_in : l.vals_sorted);
    p.keys_out = to_sorted ? l.keys_sorted : l.keys_in;
    p.vals_out = to_sorted ? l.vals_sorted : l.vals_in;
    if (generating) hipLaunchKernelGGL(rs::hist_kernel<true>, dim3(rs::tile_grid((unsigned)p.n_tiles)), dim3(rs::kHistThreads), 0, st, p);
    else hipLaunchKernelGGL(rs::hist_kernel<false>, dim3(rs::tile_grid((unsigned)p.n_tiles)), dim3(rs::kHistThreads), 0, st, p);
    scan::exclusive(tmp.counts, tmp.counts, (int64_t)(1 << p.bits) * p.n_tiles, tmp.sums, nullptr, st);
    if (generating) hipLaunchKernelGGL(rs::scatter_kernel<true>, dim3(rs::tile_grid((unsigned)p.n_tiles)), dim3(rs::kThreads), 0, st, p);
    else hipLaunchKernelGGL(rs::scatter_kernel<false>, dim3(rs::tile_grid((unsigned)p.n_tiles)), dim3(rs::kThreads), 0, st, p);
    to_sorted = !to_sorted;
  }
  return KRS_OK;
}

// Which sort produced the plan is recorded IN the workspace (PlanLayout::sort_mode, written by the plan call on its
// stream): krs_embed_bag_bwd_sparse reports n_unique = -1 for a table-segmented plan wherever the workspace has been
// copied to.  (Round 3 also kept a host map keyed by the workspace address; an allocator hands freed addresses out
// again, so a stale entry could refuse a good plan -- removed)
int plan_impl(const krs_table* tables, const krs_table* tables_host, int n_tables, const krs_feature* feats,
              const krs_feature* feats_host, int n_feats, const void* ids, int id_type, const void* offsets,
              int off_type, int batch, int64_t nnz, int64_t total_rows, void* workspace, size_t workspace_bytes,
              int* err_flag, void* stream) {
  KRS_REQUIRE(tables && feats && (ids || nnz == 0), "embed_bag_bwd_plan: null argument");
  KRS_REQUIRE(n_feats > 0 && batch > 0 && nnz >= 0, "embed_bag_bwd_plan: bad sizes");
  KRS_REQUIRE(total_rows > 0 && total_rows < 0xffffffffLL, "embed_bag_bwd_plan: total_rows must fit 32-bit keys");
  KRS_REQUIRE(nnz < 0x7fffffffLL && (int64_t)n_feats * batch < 0xffffffffLL,
              "embed_bag_bwd_plan: nnz must stay below 2^31 and the bag count below 2^32");
  if (nnz == 0) return KRS_OK;
  KRS_REQUIRE(workspace, "embed_bag_bwd_plan: null workspace");
  const PlanLayout l = plan_layout(workspace, nnz, true);
  if (workspace_bytes < l.total_bytes)
    return fail(KRS_ERR_WORKSPACE, "embed_bag_bwd_plan: workspace %zu < %zu bytes", workspace_bytes, l.total_bytes);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const rs::Temp tmp = rs::carve_temp(l.temp, nnz);
  const rs::Gen gen = rs::make_gen(tables, feats, n_feats, ids, id_type, batch, err_flag);
  const bool by_table = offsets == nullptr && g_plan_variant == 0 &&
                        plan_sort_by_table(l, tmp, gen, tables_host, n_tables, feats_host, nnz, st);
  if (!by_table)
    if (int rc = plan_sort_global(l, tmp, gen, offsets, off_type, nnz, total_rows, st)) return rc;
  KRS_CHECK_LAUNCH("embed_bag_bwd_plan: radix sort");
  // segment list: heads per block -> one-workgroup scan of the block counts -> head positions
  const unsigned nb = (unsigned)ceil_div(nnz, 256);
  const unsigned nsb = (unsigned)ceil_div(nnz, kSegTile);
  hipLaunchKernelGGL(seg_count_kernel, dim3(nsb), dim3(256), 0, st, l.keys_sorted, nnz, tmp.sums2);
  hipLaunchKernelGGL(scan::block_kernel, dim3(1), dim3(1024), 0, st, tmp.sums2, (int64_t)nsb, (int64_t*)nullptr);
  hipLaunchKernelGGL(seg_emit_kernel, dim3(nsb), dim3(256), 0, st, l.keys_sorted, nnz, tmp.sums2, l.seg_start, l.n_seg);
  KRS_CHECK_LAUNCH("seg_emit_kernel");
  // segments too long for one lane group (at most nnz / kLongSeg of them)
  KRS_HIP(hipMemsetAsync(l.n_long, 0, 3 * sizeof(uint32_t), st));
  KRS_HIP(hipMemsetAsync(l.sort_mode, by_table ? 1 : 0, sizeof(uint32_t), st));
  hipLaunchKernelGGL(long_list_kernel, dim3(nb), dim3(256), 0, st, l.seg_start, l.n_seg, nnz, l.n_long, l.long_list,
                     l.multi_list);
  KRS_CHECK_LAUNCH("long_list_kernel");
  return KRS_OK;
}

}  // namespace
}  // namespace krs

using namespace krs;

extern "C" size_t krs_embed_bag_bwd_workspace_bytes(int64_t nnz) {
  if (nnz < 0) return 0;
  return plan_layout(nullptr, nnz, true).total_bytes;
}

extern "C" int krs_embed_bag_bwd_plan(const krs_table* tables, const krs_feature* feats, int n_feats,
                                      const void* ids, int id_type, const void* offsets, int off_type,
                                      int batch, int64_t nnz, int64_t total_rows, void* workspace,
                                      size_t workspace_bytes, int* err_flag, void* stream) {
  return plan_impl(tables, nullptr, 0, feats, nullptr, n_feats, ids, id_type, offsets, off_type, batch, nnz, total_rows,
                   workspace, workspace_bytes, err_flag, stream);
}

extern "C" int krs_embed_bag_bwd_plan_tables(const krs_table* tables, const krs_table* tables_host, int n_tables,
                                             const krs_feature* feats, const krs_feature* feats_host, int n_feats,
                                             const void* ids, int id_type, int batch, int64_t nnz, int64_t total_rows,
                                             void* workspace, size_t workspace_bytes, int* err_flag, void* stream) {
  KRS_REQUIRE(tables_host && feats_host && n_tables > 0, "embed_bag_bwd_plan_tables: null host descriptors");
  return plan_impl(tables, tables_host, n_tables, feats, feats_host, n_feats, ids, id_type, nullptr, KRS_I32, batch, nnz,
                   total_rows, workspace, workspace_bytes, err_flag, stream);
}
