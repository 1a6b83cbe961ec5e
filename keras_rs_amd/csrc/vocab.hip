// K26 -- the vocabulary in front of K1: raw int64 tokens to row numbers through an open-addressing hash table on the
// device (keras.layers.IntegerLookup / StringLookup, output_mode "int"), the counting that builds a vocabulary
// (`adapt`) on the same table, and its compaction.
//
// The table is include/krs.h's (K26): a 128-byte header, then 16-byte slots {key, payload}; linear probing from
// vocab::home_slot with wrap-around; load <= 0.5, so a chain always ends at an empty slot.  One probe is one 16-byte
// load -- a lookup is a random-access, latency-bound walk, K1's one-hot regime -- and the two lookup routes differ in
// where that load goes:
//   * lookup_lds_kernel: the table fits a workgroup's 160 KB of LDS.  Every workgroup stages it once with 16-byte
//     loads (coalesced, served by L2 after the first workgroup) and probes with ds_read_b128; ids and indices move 16
//     bytes a lane.
//   * lookup_global_kernel<IPL>: a lane owns IPL consecutive ids.  All IPL home slots are loaded before the first is
//     examined, so a wave has 64 * IPL independent 16-byte loads in flight; only then does a chain continue.
// krs_vocab_upsert is the only writer: a slot is claimed with a 64-bit atomicCAS on its key word, a count is an integer
// atomicAdd.  Counts are integers, so the table's contents do not depend on the order the lanes arrive in (which SLOT
// a key of a colliding pair gets does; a lookup finds it either way, and `export` hands out slot order).
#include "krs_common.h"
#include "vocab_plan.h"

namespace krs {
namespace {

using vocab::kEmpty;
using vocab::kHeaderWords;
using vocab::kThreads;
typedef unsigned long long u64;

struct Slot {      // one 16-byte probe
  int64_t key, payload;
};
__device__ __forceinline__ Slot as_slot(const uint4& v) {
  Slot s;
  s.key = (int64_t)((u64)v.x | (u64)v.y << 32);
  s.payload = (int64_t)((u64)v.z | (u64)v.w << 32);
  return s;
}

// ---- element / 16-byte access of a lane's N ids and indices -------------------------------------------------------
template <bool W64, int N>
__device__ __forceinline__ void load_ids(const void* ids, int64_t first, int64_t n, bool vec, int64_t (&k)[N]) {
  if (vec && first + N <= n) {
    if constexpr (W64) {
      const uint4* p = reinterpret_cast<const uint4*>(reinterpret_cast<const int64_t*>(ids) + first);
#pragma unroll
      for (int i = 0; i < N / 2; ++i) {
        const uint4 v = p[i];
        k[2 * i] = (int64_t)((u64)v.x | (u64)v.y << 32);
        k[2 * i + 1] = (int64_t)((u64)v.z | (u64)v.w << 32);
      }
    } else {
      const uint4* p = reinterpret_cast<const uint4*>(reinterpret_cast<const int32_t*>(ids) + first);
#pragma unroll
      for (int i = 0; i < N / 4; ++i) {
        const uint4 v = p[i];
        k[4 * i] = (int32_t)v.x, k[4 * i + 1] = (int32_t)v.y, k[4 * i + 2] = (int32_t)v.z, k[4 * i + 3] = (int32_t)v.w;
      }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < N; ++i) k[i] = first + i < n ? ld_index(ids, W64, first + i) : 0;
}

template <bool W64, int N>
__device__ __forceinline__ void store_out(void* out, int64_t first, int64_t n, bool vec, const int64_t (&r)[N]) {
  if (vec && first + N <= n) {
    if constexpr (W64) {
      uint4* p = reinterpret_cast<uint4*>(reinterpret_cast<int64_t*>(out) + first);
#pragma unroll
      for (int i = 0; i < N / 2; ++i)
        p[i] = make_uint4((uint32_t)r[2 * i], (uint32_t)((u64)r[2 * i] >> 32), (uint32_t)r[2 * i + 1],
                          (uint32_t)((u64)r[2 * i + 1] >> 32));
    } else {
      uint4* p = reinterpret_cast<uint4*>(reinterpret_cast<int32_t*>(out) + first);
#pragma unroll
      for (int i = 0; i < N / 4; ++i)
        p[i] = make_uint4((uint32_t)r[4 * i], (uint32_t)r[4 * i + 1], (uint32_t)r[4 * i + 2], (uint32_t)r[4 * i + 3]);
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    if (first + i < n) {
      if constexpr (W64) reinterpret_cast<int64_t*>(out)[first + i] = r[i];
      else reinterpret_cast<int32_t*>(out)[first + i] = (int32_t)r[i];
    }
  }
}

// ---- lookup ---------------------------------------------------------------------------------------------------
struct LookupArgs {
  const int64_t* header;
  const uint4* slots;      // [n_slots]
  const void* ids;
  void* out;
  int* err_flag;
  int64_t n_slots, n, mask_token;
  int has_mask, num_oov, vec;
};

// the index of a token that is NOT the mask: `hit` with its payload, or Keras' OOV rule
__device__ __forceinline__ int64_t index_of(const LookupArgs& a, int64_t key, bool hit, int64_t payload, bool& oov) {
  if (hit) return a.has_mask + a.num_oov + payload;
  if (a.num_oov == 1) return a.has_mask;
  if (a.num_oov > 1) return a.has_mask + vocab::floormod(key, a.num_oov);
  oov = true;
  return -1;
}

// the chain of `key` from slot s on, whose content `cur` is already here.  LDS: probes read the staged copy.
template <bool LDS>
__device__ __forceinline__ bool walk_chain(const LookupArgs& a, const uint4* lds, int64_t key, int64_t s, Slot cur,
                                           int64_t& payload) {
  if (key == kEmpty) {     // the one token the slots cannot hold: the header's side slot
    payload = a.header[vocab::kSidePayload];
    return a.header[vocab::kSideUsed] != 0;
  }
  for (int64_t probes = 0; probes < a.n_slots; ++probes) {      // (bounded: a full table cannot spin)
    if (cur.key == key) {
      payload = cur.payload;
      return true;
    }
    if (cur.key == kEmpty) return false;
    s = s + 1 == a.n_slots ? 0 : s + 1;
    if constexpr (LDS) cur = as_slot(lds[s]);
    else cur = as_slot(a.slots[s]);
  }
  return false;
}

template <int IPL, bool IN64, bool OUT64>
__global__ __launch_bounds__(kThreads) void lookup_global_kernel(const LookupArgs a) {
  bool oov = false;
  const int64_t items = (a.n + IPL - 1) / IPL;
  for (int64_t it = (int64_t)blockIdx.x * kThreads + threadIdx.x; it < items; it += (int64_t)gridDim.x * kThreads) {
    const int64_t first = it * IPL;
    int64_t key[IPL], home[IPL], res[IPL];
    uint4 probe[IPL];
    load_ids<IN64, IPL>(a.ids, first, a.n, a.vec, key);
#pragma unroll
    for (int i = 0; i < IPL; ++i) home[i] = vocab::home_slot(key[i], a.n_slots);
#pragma unroll
    for (int i = 0; i < IPL; ++i) probe[i] = a.slots[home[i]];      // IPL loads in flight before the first is read
#pragma unroll
    for (int i = 0; i < IPL; ++i) {
      if (a.has_mask && key[i] == a.mask_token) {
        res[i] = 0;
        continue;
      }
      int64_t payload = 0;
      const bool hit = walk_chain<false>(a, nullptr, key[i], home[i], as_slot(probe[i]), payload);
      bool miss = false;
      res[i] = index_of(a, key[i], hit, payload, miss);
      oov |= miss && first + i < a.n;
    }
    store_out<OUT64, IPL>(a.out, first, a.n, a.vec, res);
  }
  if (oov && a.err_flag) atomicOr(a.err_flag, KRS_FLAG_OOV_TOKEN);
}

template <bool IN64, bool OUT64>
__global__ __launch_bounds__(kThreads) void lookup_lds_kernel(const LookupArgs a) {
  constexpr int IPL = vocab::kLdsIdsPerLane;
  extern __shared__ __attribute__((aligned(16))) uint4 staged[];      // [n_slots]
  for (int64_t s = threadIdx.x; s < a.n_slots; s += kThreads) staged[s] = a.slots[s];
  __syncthreads();
  bool oov = false;
  const int64_t items = (a.n + IPL - 1) / IPL;
  for (int64_t it = (int64_t)blockIdx.x * kThreads + threadIdx.x; it < items; it += (int64_t)gridDim.x * kThreads) {
    const int64_t first = it * IPL;
    int64_t key[IPL], res[IPL];
    load_ids<IN64, IPL>(a.ids, first, a.n, a.vec, key);
#pragma unroll
    for (int i = 0; i < IPL; ++i) {
      if (a.has_mask && key[i] == a.mask_token) {
        res[i] = 0;
        continue;
      }
      const int64_t home = vocab::home_slot(key[i], a.n_slots);
      int64_t payload = 0;
      const bool hit = walk_chain<true>(a, staged, key[i], home, as_slot(staged[home]), payload);
      bool miss = false;
      res[i] = index_of(a, key[i], hit, payload, miss);
      oov |= miss && first + i < a.n;
    }
    store_out<OUT64, IPL>(a.out, first, a.n, a.vec, res);
  }
  if (oov && a.err_flag) atomicOr(a.err_flag, KRS_FLAG_OOV_TOKEN);
}

// ---- the writer -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void clear_kernel(int64_t* table, int64_t n_slots) {
  const int64_t words = kHeaderWords + 2 * n_slots;
  for (int64_t w = (int64_t)blockIdx.x * kThreads + threadIdx.x; w < words; w += (int64_t)gridDim.x * kThreads)
    table[w] = w >= kHeaderWords && ((w - kHeaderWords) & 1) == 0 ? kEmpty : 0;
}

template <bool ADD>
__global__ __launch_bounds__(kThreads) void upsert_kernel(int64_t* table, int64_t n_slots, const void* keys, int k64,
                                                          const int64_t* payloads, int64_t n, int* err_flag) {
  u64* header = reinterpret_cast<u64*>(table);
  u64* slots = header + kHeaderWords;      // slot s: key at 2s, payload at 2s + 1
  int raise = 0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const int64_t key = ld_index(keys, k64, i);
    const u64 value = (u64)(payloads ? payloads[i] : (ADD ? 1 : i));
    u64* payload_word = nullptr;
    bool claimed = false;
    if (key == kEmpty) {
      claimed = atomicCAS(header + vocab::kSideUsed, (u64)0, (u64)1) == 0;
      payload_word = header + vocab::kSidePayload;
    } else {
      int64_t s = vocab::home_slot(key, n_slots);
      for (int64_t probes = 0; probes < n_slots && !payload_word; ++probes) {
        u64* key_word = slots + 2 * s;
        u64 seen = __hip_atomic_load(key_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (seen == (u64)kEmpty) {
          seen = atomicCAS(key_word, (u64)kEmpty, (u64)key);
          claimed = seen == (u64)kEmpty;
          if (claimed) seen = (u64)key;
        }
        if (seen == (u64)key) payload_word = key_word + 1;
        s = s + 1 == n_slots ? 0 : s + 1;
      }
    }
    if (!payload_word) {
      raise |= KRS_FLAG_TABLE_FULL;
      continue;
    }
    if (claimed) atomicAdd(header + vocab::kCount, (u64)1);
    if constexpr (ADD) {
      atomicAdd(payload_word, value);
    } else {
      if (claimed) *payload_word = value;      // the claimer alone writes the payload
      else raise |= KRS_FLAG_DUPLICATE_TOKEN;
    }
  }
  if (raise && err_flag) atomicOr(err_flag, raise);
}

// ---- export: occupied slots in slot order -------------------------------------------------------------------------
// workgroup j owns the slots [j * span, (j + 1) * span); pass 1 counts them, pass 2 places them after the counts of
// the workgroups before it
__device__ __forceinline__ int block_sum(int v, int* wave_sums) {      // every thread gets the workgroup's sum
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if (lane == 0) wave_sums[wave] = v;
  __syncthreads();
  int s = 0;
  for (int w = 0; w < kThreads / 64; ++w) s += wave_sums[w];
  return s;
}

__global__ __launch_bounds__(kThreads) void export_count_kernel(const uint4* slots, int64_t n_slots, int64_t span,
                                                                int64_t* counts) {
  __shared__ int wave_sums[kThreads / 64];
  const int64_t lo = (int64_t)blockIdx.x * span, hi = lo + span < n_slots ? lo + span : n_slots;
  int mine = 0;
  for (int64_t s = lo + threadIdx.x; s < hi; s += kThreads) mine += as_slot(slots[s]).key != kEmpty;
  const int total = block_sum(mine, wave_sums);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void export_write_kernel(const int64_t* header, const uint4* slots,
                                                                int64_t n_slots, int64_t span, const int64_t* counts,
                                                                int64_t* keys, int64_t* payloads, int64_t cap,
                                                                int64_t* out_count) {
  __shared__ int wave_sums[kThreads / 64];
  __shared__ int wave_base[kThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t at = 0;
  for (int j = 0; j < (int)blockIdx.x; ++j) at += counts[j];      // (<= 1024 words, the same in every thread)
  const int64_t lo = (int64_t)blockIdx.x * span, hi = lo + span < n_slots ? lo + span : n_slots;
  for (int64_t t0 = lo; t0 < hi; t0 += kThreads) {      // a tile of kThreads slots, in slot order
    const int64_t s = t0 + threadIdx.x;
    Slot v = {kEmpty, 0};
    if (s < hi) v = as_slot(slots[s]);
    const bool used = v.key != kEmpty;
    const u64 ballot = __ballot(used);
    const int rank = __popcll(ballot & (((u64)1 << lane) - 1));
    __syncthreads();
    if (lane == 0) wave_sums[wave] = __popcll(ballot);
    __syncthreads();
    if (threadIdx.x == 0) {
      int run = 0;
      for (int w = 0; w < kThreads / 64; ++w) wave_base[w] = run, run += wave_sums[w];
    }
    __syncthreads();
    const int64_t pos = at + wave_base[wave] + rank;
    if (used && pos < cap) keys[pos] = v.key, payloads[pos] = v.payload;
    int tile = 0;
    for (int w = 0; w < kThreads / 64; ++w) tile += wave_sums[w];
    at += tile;
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {      // `at` is now the number of occupied slots
    if (header[vocab::kSideUsed] != 0) {
      if (at < cap) keys[at] = kEmpty, payloads[at] = header[vocab::kSidePayload];
      ++at;
    }
    *out_count = at;
  }
}

thread_local krs_vocab_route g_route = {};

vocab::Call call_of(const void* table, int64_t slots, const void* ids, int ids_itype, int64_t n, int num_oov,
                    const void* out, int out_itype, int route_hint, int ids_per_lane) {
  vocab::Call c;
  c.table = table, c.slots = slots, c.ids = ids, c.ids_itype = ids_itype, c.n = n, c.num_oov = num_oov;
  c.out = out, c.out_itype = out_itype, c.route_hint = route_hint, c.ids_per_lane = ids_per_lane;
  return c;
}

int refuse(const char* what, const vocab::Plan& pl, const vocab::Call& c) {
  return fail(pl.status, "%s: bad %s (table %p, slots %lld, ids %p itype %d, n %lld, num_oov %d, out %p itype %d, "
              "route_hint %d, ids_per_lane %d)", what, pl.why, c.table, (long long)c.slots, c.ids, c.ids_itype,
              (long long)c.n, c.num_oov, c.out, c.out_itype, c.route_hint, c.ids_per_lane);
}

template <int IPL>
void launch_global(const krs_vocab_route& r, bool in64, bool out64, const LookupArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)r.blocks), block(kThreads);
  if (in64 && out64) hipLaunchKernelGGL((lookup_global_kernel<IPL, true, true>), grid, block, 0, st, a);
  else if (in64) hipLaunchKernelGGL((lookup_global_kernel<IPL, true, false>), grid, block, 0, st, a);
  else if (out64) hipLaunchKernelGGL((lookup_global_kernel<IPL, false, true>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((lookup_global_kernel<IPL, false, false>), grid, block, 0, st, a);
}

template <bool IN64, bool OUT64>
int launch_lds(const krs_vocab_route& r, const LookupArgs& a, hipStream_t st) {
  auto kern = lookup_lds_kernel<IN64, OUT64>;
  static bool raised = false;      // once per build, to the whole LDS: no runtime call is left for a captured step
  if (!raised) {
    KRS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)vocab::kLdsBytes));
    raised = true;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)r.blocks), dim3(kThreads), (size_t)r.lds_bytes, st, a);
  return KRS_OK;
}

int grid_for(int64_t work) {
  const int64_t g = (work + kThreads - 1) / kThreads;
  return (int)(g < 1 ? 1 : (g > 65536 ? 65536 : g));
}

}  // namespace
}  // namespace krs

extern "C" size_t krs_vocab_table_bytes(int64_t n_tokens) { return krs::vocab::table_bytes(n_tokens); }

extern "C" int64_t krs_vocab_home_slot(int64_t key, int64_t slots) {
  return slots > 0 ? krs::vocab::home_slot(key, slots) : -1;
}

extern "C" size_t krs_vocab_export_workspace_bytes(int64_t slots) { return krs::vocab::export_workspace_bytes(slots); }

extern "C" int krs_vocab_last_route(krs_vocab_route* route) {
  if (route) *route = krs::g_route;
  return krs::g_route.route;
}

extern "C" int krs_vocab_plan_route(const void* table, int64_t slots, const void* ids, int ids_itype, int64_t n,
                                    int num_oov, const void* out, int out_itype, int route_hint, int ids_per_lane,
                                    krs_vocab_route* route) {
  using namespace krs;
  const vocab::Call call = call_of(table, slots, ids, ids_itype, n, num_oov, out, out_itype, route_hint, ids_per_lane);
  const vocab::Plan pl = vocab::plan(call);
  if (route) *route = pl.route;
  return pl.status == KRS_OK ? KRS_OK : refuse("krs_vocab_plan_route", pl, call);
}

extern "C" int krs_vocab_upsert(void* table, int64_t slots, const void* keys, int keys_itype, const int64_t* payloads,
                                int64_t n, int mode, int init, int* err_flag, void* stream) {
  using namespace krs;
  const char* what = "krs_vocab_upsert";
  KRS_REQUIRE(table && vocab::on16(table), "%s: table %p must be a device buffer on a 16-byte boundary", what, table);
  KRS_REQUIRE(vocab::slots_ok(slots), "%s: slots %lld must be a multiple of 8, at least 8", what, (long long)slots);
  KRS_REQUIRE(vocab::itype_ok(keys_itype), "%s: bad keys_itype %d", what, keys_itype);
  KRS_REQUIRE(mode == KRS_VOCAB_SET || mode == KRS_VOCAB_ADD, "%s: bad mode %d", what, mode);
  KRS_REQUIRE(n >= 0, "%s: n %lld is negative", what, (long long)n);
  KRS_REQUIRE(n == 0 || keys, "%s: null keys with n %lld", what, (long long)n);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int64_t* t = reinterpret_cast<int64_t*>(table);
  if (init)
    hipLaunchKernelGGL(clear_kernel, dim3(grid_for(vocab::kHeaderWords + 2 * slots)), dim3(kThreads), 0, st, t, slots);
  if (n > 0) {
    const dim3 grid(grid_for(n)), block(kThreads);
    const int k64 = keys_itype == KRS_I64;
    if (mode == KRS_VOCAB_ADD)
      hipLaunchKernelGGL(upsert_kernel<true>, grid, block, 0, st, t, slots, keys, k64, payloads, n, err_flag);
    else
      hipLaunchKernelGGL(upsert_kernel<false>, grid, block, 0, st, t, slots, keys, k64, payloads, n, err_flag);
  }
  KRS_CHECK_LAUNCH(what);
  return KRS_OK;
}

extern "C" int krs_vocab_lookup(const void* table, int64_t slots, const void* ids, int ids_itype, int64_t n,
                                int has_mask, int64_t mask_token, int num_oov, void* out, int out_itype, int* err_flag,
                                int route_hint, int ids_per_lane, void* stream) {
  using namespace krs;
  const char* what = "krs_vocab_lookup";
  g_route = {};
  const vocab::Call call = call_of(table, slots, ids, ids_itype, n, num_oov, out, out_itype, route_hint, ids_per_lane);
  const vocab::Plan pl = vocab::plan(call);
  if (pl.status != KRS_OK) return refuse(what, pl, call);
  if (n == 0) return KRS_OK;
  const krs_vocab_route& r = pl.route;
  LookupArgs a = {};
  a.header = reinterpret_cast<const int64_t*>(table);
  a.slots = reinterpret_cast<const uint4*>(a.header + vocab::kHeaderWords);
  a.ids = ids, a.out = out, a.err_flag = err_flag;
  a.n_slots = slots, a.n = n, a.mask_token = mask_token;
  a.has_mask = has_mask != 0, a.num_oov = num_oov, a.vec = r.vec;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool in64 = ids_itype == KRS_I64, out64 = out_itype == KRS_I64;
  if (r.route == KRS_VOCAB_LDS) {
    int rc;
    if (in64 && out64) rc = launch_lds<true, true>(r, a, st);
    else if (in64) rc = launch_lds<true, false>(r, a, st);
    else if (out64) rc = launch_lds<false, true>(r, a, st);
    else rc = launch_lds<false, false>(r, a, st);
    if (rc != KRS_OK) return rc;
  } else if (r.ids_per_lane == 1) {
    launch_global<1>(r, in64, out64, a, st);
  } else if (r.ids_per_lane == 2) {
    launch_global<2>(r, in64, out64, a, st);
  } else if (r.ids_per_lane == 4) {
    launch_global<4>(r, in64, out64, a, st);
  } else {
    launch_global<8>(r, in64, out64, a, st);
  }
  KRS_CHECK_LAUNCH(what);
  g_route = r;
  return KRS_OK;
}

extern "C" int krs_vocab_export(const void* table, int64_t slots, int64_t* keys, int64_t* payloads, int64_t cap,
                                int64_t* out_count, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace krs;
  const char* what = "krs_vocab_export";
  KRS_REQUIRE(table && vocab::on16(table), "%s: table %p must be a device buffer on a 16-byte boundary", what, table);
  KRS_REQUIRE(vocab::slots_ok(slots), "%s: slots %lld must be a multiple of 8, at least 8", what, (long long)slots);
  KRS_REQUIRE(cap >= 0 && out_count && (cap == 0 || (keys && payloads)),
              "%s: null outputs (keys %p, payloads %p, cap %lld, out_count %p)", what, (void*)keys, (void*)payloads,
              (long long)cap, (void*)out_count);
  const size_t need = vocab::export_workspace_bytes(slots);
  if (!workspace || workspace_bytes < need)
    return fail(KRS_ERR_WORKSPACE, "%s: workspace of %zu bytes at %p, %zu needed", what, workspace_bytes, workspace,
                need);
  const int64_t blocks = vocab::export_blocks(slots);
  const int64_t span = (slots + blocks - 1) / blocks;
  const int64_t* header = reinterpret_cast<const int64_t*>(table);
  const uint4* sl = reinterpret_cast<const uint4*>(header + vocab::kHeaderWords);
  int64_t* counts = reinterpret_cast<int64_t*>(workspace);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(export_count_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, sl, slots, span, counts);
  hipLaunchKernelGGL(export_write_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, header, sl, slots, span,
                     counts, keys, payloads, cap, out_count);
  KRS_CHECK_LAUNCH(what);
  return KRS_OK;
}
