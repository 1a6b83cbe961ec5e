// The device hash table of K26 (vocab.hip) as pure host arithmetic: the table's size, the home slot of a key and the
// route of krs_vocab_lookup as a function of the call.  Plain C++17 on krs.h, no HIP header: krs_vocab_table_bytes,
// krs_vocab_home_slot and krs_vocab_plan_route answer from it without a GPU, and the kernels call the same home_slot.
// Device pointers are read as VALUES (nullness, alignment).  A plan guarantees:
//   * slots is a multiple of 8 and >= 2 * n_tokens (load <= 0.5), so a probe chain always meets an empty slot;
//   * the LDS route only when slots * 16 bytes fit one workgroup's LDS, and under KRS_VOCAB_AUTO only when kLdsAuto
//     holds and the call has kLdsMinIds ids or more (measured: it never pays, so kLdsAuto is false);
//   * vector access only when ids and out start on 16 bytes and a lane's ids and indices are whole 16-byte pieces;
//   * 1 <= blocks, and blocks * kThreads * ids_per_lane < n + kThreads * ids_per_lane on the global route.
#ifndef KRS_VOCAB_PLAN_H_
#define KRS_VOCAB_PLAN_H_

#include <cstddef>
#include <cstdint>

#include "../../include/krs.h"

#if defined(__HIPCC__)
#define KRS_VOCAB_HD __host__ __device__
#else
#define KRS_VOCAB_HD
#endif

namespace krs {
namespace vocab {

constexpr int64_t kEmpty = INT64_MIN;      // the key word of an empty slot; the TOKEN INT64_MIN lives in the side slot
constexpr int kHeaderWords = KRS_VOCAB_HEADER_BYTES / 8;
constexpr int kCount = 0, kSideUsed = 1, kSidePayload = 2;      // header words (the rest are zero)
constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1 << 20;
constexpr int64_t kLdsBytes = 160 * 1024;                        // a gfx950 workgroup's LDS
constexpr int64_t kLdsMaxSlots = kLdsBytes / KRS_VOCAB_SLOT_BYTES;   // 10240 slots: vocabularies up to 5120 tokens
constexpr int kLdsIdsPerLane = 4;
constexpr int kLdsMaxBlocks = 256;                               // one workgroup a CU: each holds the whole table
// The global route's ids per lane: their first probes are in flight together.  Measured with scripts/bench_vocab.py
// (section ipl; docs/measurement_log.md, K26) at 2^22 uniform int64 ids: vocabulary 2^20: 92.4 / 100.0 / 111.6 /
// 127.1 us at 1 / 2 / 4 / 8 ids a lane, vocabulary 40 M: 121.9 / 125.9 / 138.3 / 158.3 us.  One id a lane wins both:
// eight waves a SIMD already keep more probes in flight than a lane's second id adds, and one id a lane keeps the id
// loads and index stores of a wave on consecutive addresses.
constexpr int kGlobalIdsPerLane = 1;
// The LDS route stages slots * 16 bytes per workgroup before its first probe, and a workgroup walks kLdsMinIds ids or
// more (blocks = n / kLdsMinIds, at most one a CU): below that many ids in the call one workgroup would stage the
// table for a handful of ids.  Measured against the global route at vocabulary 2^10 (scripts/bench_vocab.py, section
// crossover; docs/measurement_log.md, K26): 2^8 ids 11.7 / 11.7 us (LDS / global), 2^10 11.5 / 11.7, 2^12 27.1 / 11.0,
// 2^14 31.6 / 12.2, 2^16 30.7 / 12.9, 2^22 114.0 / 51.5 -- the two ties are the launch floor, and from 2^12 ids on the
// LDS route LOSES by 2.2x or more: a 16 KB table is L2-resident for the global route anyway, and n / 4096 workgroups
// leave most CUs idle.
// It wins at no measured point, so KRS_VOCAB_AUTO never takes it (kLdsAuto); route_hint KRS_VOCAB_LDS still runs it.
constexpr int64_t kLdsMinIds = 4096;
constexpr bool kLdsAuto = false;

// splitmix64's finalizer, then multiply-high onto [0, slots): written down in krs.h (K26)
KRS_VOCAB_HD inline uint64_t mix(uint64_t x) {
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}
KRS_VOCAB_HD inline int64_t home_slot(int64_t key, int64_t slots) {
  const uint64_t h = mix((uint64_t)key);
#if defined(__HIP_DEVICE_COMPILE__)
  return (int64_t)__umul64hi(h, (uint64_t)slots);
#else
  return (int64_t)(uint64_t)(((unsigned __int128)h * (uint64_t)slots) >> 64);
#endif
}

// floor modulus (Keras' rule for an integer OOV token): the result has the sign of m > 0
KRS_VOCAB_HD inline int64_t floormod(int64_t a, int64_t m) {
  const int64_t r = a % m;
  return r < 0 ? r + m : r;
}

inline int64_t slots_for(int64_t n_tokens) {
  if (n_tokens < 0 || n_tokens > (INT64_MAX >> 6)) return 0;
  const int64_t s = (2 * n_tokens + 7) / 8 * 8;
  return s < 8 ? 8 : s;
}
inline size_t table_bytes(int64_t n_tokens) {
  const int64_t s = slots_for(n_tokens);
  return s ? (size_t)KRS_VOCAB_HEADER_BYTES + (size_t)s * KRS_VOCAB_SLOT_BYTES : 0;
}

struct Call {
  int64_t slots = 0, n = 0;
  const void* table = nullptr;
  const void* ids = nullptr;
  const void* out = nullptr;
  int ids_itype = KRS_I64, out_itype = KRS_I64;
  int num_oov = 1;
  int route_hint = KRS_VOCAB_AUTO, ids_per_lane = 0;
};

struct Plan {
  int status = KRS_OK;
  const char* why = "";
  krs_vocab_route route = {};
};

inline bool on16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool itype_ok(int t) { return t == KRS_I32 || t == KRS_I64; }
inline bool slots_ok(int64_t slots) { return slots >= 8 && slots % 8 == 0 && slots <= (INT64_MAX >> 6); }

inline Plan plan(const Call& c) {
  Plan pl;
  auto refuse = [&](const char* why) {
    pl.status = KRS_ERR_INVALID, pl.why = why;
    return pl;
  };
  if (!slots_ok(c.slots)) return refuse("slots (a multiple of 8, at least 8)");
  if (!itype_ok(c.ids_itype)) return refuse("ids_itype");
  if (!itype_ok(c.out_itype)) return refuse("out_itype");
  if (c.n < 0) return refuse("n");
  if (c.num_oov < 0) return refuse("num_oov_indices");
  if (c.route_hint < KRS_VOCAB_AUTO || c.route_hint > KRS_VOCAB_GLOBAL) return refuse("route_hint");
  const int ipl = c.ids_per_lane;
  if (ipl != 0 && ipl != 1 && ipl != 2 && ipl != 4 && ipl != 8) return refuse("ids_per_lane (0, 1, 2, 4 or 8)");
  if (c.route_hint == KRS_VOCAB_LDS && c.slots > kLdsMaxSlots) return refuse("route_hint (the table does not fit in LDS)");
  if (!c.table) return refuse("null table");
  if (!on16(c.table)) return refuse("table alignment (16 bytes)");
  if (c.n == 0) return pl;
  if (!c.ids || !c.out) return refuse("null ids or out");
  const bool lds = c.route_hint == KRS_VOCAB_LDS ||
                   (c.route_hint == KRS_VOCAB_AUTO && kLdsAuto && c.slots <= kLdsMaxSlots && c.n >= kLdsMinIds);
  krs_vocab_route& r = pl.route;
  r.route = lds ? KRS_VOCAB_LDS : KRS_VOCAB_GLOBAL;
  r.ids_per_lane = lds ? kLdsIdsPerLane : (ipl ? ipl : kGlobalIdsPerLane);
  const int in_bytes = r.ids_per_lane * (c.ids_itype == KRS_I64 ? 8 : 4);
  const int out_bytes = r.ids_per_lane * (c.out_itype == KRS_I64 ? 8 : 4);
  r.vec = on16(c.ids) && on16(c.out) && in_bytes % 16 == 0 && out_bytes % 16 == 0;
  r.lds_bytes = lds ? (int32_t)(c.slots * KRS_VOCAB_SLOT_BYTES) : 0;
  r.slots = c.slots;
  const int64_t per_block = (int64_t)kThreads * r.ids_per_lane;
  if (lds) {
    const int64_t g = c.n / kLdsMinIds;
    r.blocks = g < 1 ? 1 : (g > kLdsMaxBlocks ? kLdsMaxBlocks : g);
  } else {
    const int64_t g = (c.n + per_block - 1) / per_block;
    r.blocks = g > kMaxBlocks ? kMaxBlocks : g;      // (the kernel strides over the grid)
  }
  return pl;
}

// krs_vocab_export: the spans of the table its workgroups compact, and the workspace that carries their counts
constexpr int kExportMaxBlocks = 1024;
inline int64_t export_blocks(int64_t slots) {
  const int64_t g = (slots + kThreads - 1) / kThreads;
  return g < 1 ? 1 : (g > kExportMaxBlocks ? kExportMaxBlocks : g);
}
inline size_t export_workspace_bytes(int64_t slots) {
  return slots_ok(slots) ? (size_t)export_blocks(slots) * sizeof(int64_t) : 0;
}

}  // namespace vocab
}  // namespace krs
#endif
