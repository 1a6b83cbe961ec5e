// What the K2 plan (embed_bag_plan.hip) and the K2 apply kernels (embed_bag_bwd.hip) must agree on: the layout of the
// plan workspace and the records the plan leaves in it.  Nothing else of the plan is visible to the apply side.
#ifndef KRS_BAG_PLAN_H_
#define KRS_BAG_PLAN_H_

#include "krs_common.h"
#include "krs_scan.h"

namespace krs {
namespace {   // (internal linkage, as in the sources that include this: every object compiles its own copy)

constexpr uint32_t kInvalidKey = 0xffffffffu;
constexpr int kLongSeg = 128;   // segments longer than this are summed by whole workgroups
constexpr int kChunk = 2048;    // ... in chunks of this many lookups, one workgroup each
constexpr int kPartialBytes = 2048;  // fp32 partial row of a chunk (row bytes <= 1024 on the vector path)

// one workgroup's share of a long segment
struct LongItem {
  uint32_t seg;       // segment index
  uint32_t chunk;     // which kChunk-sized piece of it
  uint32_t partial;   // slot in the partial-row buffer, or ~0u when the segment is a single chunk
};
// a long segment that spans several chunks: its partial rows are summed in chunk order afterwards
struct MultiSeg {
  uint32_t seg, partial_base, n_chunks;
};

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

namespace rs {
// the sort's tile shape, as far as the workspace depends on it (the kernels are in embed_bag_plan.hip)
constexpr int kTile = 4096, kMaxBits = 10, kMaxBins = 1 << kMaxBits;
constexpr int kMaxProb = 128;    // tables (problems) of the table-segmented sort

// the sort's temporaries, carved out of PlanLayout::temp
struct Temp {
  int32_t* counts;   // [bins][tiles]: per-tile digit histogram, then exclusive offsets
  int32_t* sums;     // scan workspace of the count matrix
  int32_t* sums2;    // block counts of the segment list
  size_t bytes;
};
inline Temp carve_temp(void* temp, int64_t nnz) {
  const int64_t tiles = ceil_div(nnz > 0 ? nnz : 1, kTile) + kMaxProb;   // (every problem may end in a partial tile)
  char* p = reinterpret_cast<char*>(temp);
  size_t o = 0;
  Temp t;
  t.counts = reinterpret_cast<int32_t*>(p + o); o += align_up((size_t)kMaxBins * tiles * sizeof(int32_t), 256);
  t.sums = reinterpret_cast<int32_t*>(p + o); o += align_up(scan::workspace_bytes((int64_t)kMaxBins * tiles), 256);
  t.sums2 = reinterpret_cast<int32_t*>(p + o); o += align_up(scan::workspace_bytes(nnz), 256);
  t.bytes = o;
  return t;
}
inline size_t temp_bytes(int64_t nnz) { return carve_temp(nullptr, nnz).bytes; }
}  // namespace rs

struct PlanLayout {
  uint32_t* keys_in;      // dead after the sort -> reused as head flags
  uint32_t* keys_sorted;
  uint64_t* vals_in;      // dead after the sort -> its second half is reused as seg_start
  uint64_t* vals_sorted;
  uint32_t* seg_start;    // = vals_in, next n words: first sorted position of every segment
  uint32_t* n_seg;        // number of segments (a trailing run of invalid keys counts as one)
  uint32_t* n_long;       // number of LongItems (device scalar); [1] partial rows handed out; [2] MultiSegs
  // 0 = global sort (out-of-range lookups form ONE trailing run), != 0 = table-segmented sort (they end every TABLE's
  // run).  Written by the plan on its stream; count_unique_kernel reads it and reports n_unique = -1 when it is not 0
  uint32_t* sort_mode;
  LongItem* long_list;    // work items of the segments longer than kLongSeg (any order)
  MultiSeg* multi_list;   // segments longer than kChunk
  float* partials;        // [<= 2 * nnz / kChunk + 2] fp32 partial rows, kPartialBytes apart
  void* temp;
  size_t temp_bytes;
  size_t total_bytes;
};

inline PlanLayout plan_layout(void* ws, int64_t nnz, bool need_temp = false) {
  PlanLayout l;
  char* p = reinterpret_cast<char*>(ws);
  size_t o = 0;
  const size_t n = (size_t)(nnz > 0 ? nnz : 1);
  l.keys_in = reinterpret_cast<uint32_t*>(p + o); o += align_up(n * 4, 256);
  l.keys_sorted = reinterpret_cast<uint32_t*>(p + o); o += align_up(n * 4, 256);
  l.vals_in = reinterpret_cast<uint64_t*>(p + o); o += align_up(n * 8 + 8, 256);
  l.vals_sorted = reinterpret_cast<uint64_t*>(p + o); o += align_up(n * 8, 256);
  l.n_seg = reinterpret_cast<uint32_t*>(p + o);
  l.n_long = l.n_seg + 1;
  l.sort_mode = l.n_seg + 8; o += 256;
  // every long segment has <= len / kChunk + 1 items; there are <= n / kLongSeg long segments
  l.long_list = reinterpret_cast<LongItem*>(p + o); o += align_up((n / kLongSeg + n / kChunk + 2) * sizeof(LongItem), 256);
  l.multi_list = reinterpret_cast<MultiSeg*>(p + o); o += align_up((n / kChunk + 2) * sizeof(MultiSeg), 256);
  l.partials = reinterpret_cast<float*>(p + o); o += align_up((2 * (n / kChunk) + 2) * (size_t)kPartialBytes, 256);
  l.seg_start = reinterpret_cast<uint32_t*>(l.vals_in) + n;
  l.temp = p + o;
  l.temp_bytes = need_temp ? rs::temp_bytes(nnz) : 0;
  l.total_bytes = o + l.temp_bytes;
  return l;
}

}  // namespace
}  // namespace krs
#endif
