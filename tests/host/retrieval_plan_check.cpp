// Walks a lattice of krs_topk_rows / krs_retrieval_topk / krs_retrieval_topk_q8 / krs_retrieval_mine calls through the
// planner (keras_rs_amd/csrc/retrieval_plan.h; it and gemm_plan.h, which it takes krs_gemm's workspace from, compile
// without HIP) and checks what every plan promises the kernels it names: stage 1's geometry, the queue bound, the LDS
// request against the kernel's own layout, the grids, the workspace sections, the query chunks of the two-step path and
// the selection route with its launch count.  The expectations are restated here from retrieval.hip's kernels, not taken
// from the planner's helpers.
// Stand-alone: tests/test_retrieval_routes_host.py builds it with the host compiler and -fsanitize=address,undefined (a
// signed overflow anywhere in the planner stops it) and runs it as a child process.  Exit 0 = every invariant held;
// otherwise the first offending calls of each invariant are printed and the exit status is 1.
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

#include "../../keras_rs_amd/csrc/retrieval_plan.h"

using namespace krs::rplan;

static std::map<std::string, long> g_failed;
static long g_checks = 0, g_plans = 0, g_kernel[4] = {}, g_select[4] = {}, g_vec[2] = {}, g_multi_chunk = 0, g_refused = 0;

static void report(const char* what, const Call& c, const Plan& p) {
  if (++g_failed[what] > 3) return;
  const krs_retrieval_route& rt = p.route;
  std::printf("FAILED %s: variant=%d b=%lld n=%lld d=%lld k=%d es=%d ldc=%lld c=%llx budget=%lld -> status=%d kernel=%d vec=%d "
              "S=%d qtiles=%d slice=%lld row_bytes=%d lds=%d blocks=%lld select=%d len=%lld P=%lld launches=%d chunks=%lld "
              "chunk_rows=%lld total=%lld\n",
              what, c.variant, (long long)c.b, (long long)c.n, (long long)c.d, c.k, c.es, (long long)c.ldc,
              (unsigned long long)c.c_addr, (long long)c.slab_budget, p.status, rt.kernel, rt.vec, rt.S, rt.qtiles,
              (long long)rt.slice, rt.row_bytes, rt.lds_bytes, (long long)rt.blocks, rt.select, (long long)rt.select_len,
              (long long)rt.select_p, rt.select_launches, (long long)rt.chunks, (long long)rt.chunk_rows, (long long)p.total);
}

#define CHECK(cond, what) do { ++g_checks; if (!(cond)) report(what, c, p); } while (0)

static bool is_none(const krs_retrieval_route& rt) {
  const krs_retrieval_route none = {};
  return std::memcmp(&rt, &none, sizeof rt) == 0;
}
static __int128 up256(__int128 v) { return (v + 255) / 256 * 256; }
static int64_t pow2_ge(int64_t v) {
  int64_t p = 1;
  while (p < v) p *= 2;
  return p;
}

// the selection of `rows` rows of `len` pairs, as select_rows and its kernels need it
static void check_select(const Call& c, const Plan& p, int64_t rows, int64_t len) {
  const Select& s = p.sel;
  const krs_retrieval_route& rt = p.route;
  CHECK(rt.select == s.route && rt.select_len == s.len && rt.select_p == s.P && rt.select_launches == s.launches,
        "the record's selection is the plan's");
  CHECK(s.len == len, "the selection runs over the row length");
  CHECK((s.route == KRS_SELECT_LDS) == (len <= 2048), "LDS sort exactly when a row fits 2048 slots");
  if (s.route < 0 || s.route > 3) return;
  ++g_select[s.route];
  if (s.route == KRS_SELECT_LDS) {
    // topk_small_kernel sorts n = s.sort_n slots of a __shared__ uint64_t[2048]
    CHECK(s.P == pow2_ge(len) && s.sort_n == s.P && s.P <= 2048 && s.launches == 1, "the LDS sort's slots");
    CHECK(select_list_bytes(rows, s) == 0, "the LDS route needs no list");
    CHECK(rows <= kMaxGrid, "topk_small_kernel's grid");
    return;
  }
  CHECK(s.P == pow2_ge(c.k) && s.P >= c.k && s.P < 2 * (int64_t)c.k, "P is the power of two at or above k");
  CHECK((s.route == KRS_SELECT_RADIX_MERGE) == (s.P > 2048), "merged in global memory exactly when P > 2048");
  CHECK(s.sort_n == (s.P < 2048 ? s.P : 2048) && s.P % s.sort_n == 0, "a sort block is min(P, 2048) slots");
  // the launches as select_rows made them before it had a plan
  int launches = 2;   // radix_select_kernel, sort_block_kernel(0)
  const int64_t n = s.P < 2048 ? s.P : 2048;
  int global_levels = 0;
  for (int64_t kk = 2 * n; kk <= s.P; kk *= 2) {
    for (int64_t j = kk / 2; j >= n; j /= 2) ++launches;
    ++launches;
    ++global_levels;
  }
  ++launches;         // emit_kernel
  CHECK(s.launches == launches, "the launch count is the loop's");
  CHECK((global_levels > 0) == (s.route == KRS_SELECT_RADIX_MERGE), "global merge levels only on the merge route");
  // what for_each_sort_launch visits: first the full block sort, every level ends with a block pass, steps have j >= n
  int visited = 0, bad_order = 0;
  int64_t last_kk = -1, last_j = -1;
  for_each_sort_launch(s, [&](int64_t kk, int64_t j) {
    if (visited == 0 && (kk != 0 || j != 0)) ++bad_order;
    if (visited > 0 && (kk < 2 * n || kk > s.P || (kk & (kk - 1)))) ++bad_order;
    if (j != 0 && (j < n || j >= kk || (j & (j - 1)))) ++bad_order;
    if (j != 0 && last_kk == kk && last_j != 2 * j) ++bad_order;      // halving inside a level
    if (j != 0 && last_kk != kk && j != kk / 2) ++bad_order;          // a level starts at kk / 2
    if (j == 0 && visited > 0 && !(last_kk == kk && last_j == n)) ++bad_order;   // the block pass takes over below n
    last_kk = kk;
    last_j = j;
    ++visited;
  });
  CHECK(visited == launches - 2 && bad_order == 0, "the sort launches are a bitonic network's, in order");
  CHECK(select_list_bytes(rows, s) == rows * s.P * 8, "a list of P pairs per row");
  const __int128 sblocks = (__int128)rows * (s.P / n), steps = ((__int128)rows * (s.P / 2) + 255) / 256,
                 emits = ((__int128)rows * c.k + 255) / 256;
  CHECK(rows <= kMaxGrid && sblocks <= kMaxGrid && (global_levels == 0 || steps <= kMaxGrid) && emits <= kMaxGrid,
        "a selection grid exceeds 32 bits on a served call");
}

static void check(const Call& c) {
  const Plan p = plan_retrieval(c);
  ++g_plans;
  const krs_retrieval_route& rt = p.route;
  if (p.status != KRS_OK || c.b == 0) {
    CHECK(is_none(rt) && p.total == 0 && p.blocks == 0 && p.chunks == 0, "a call that launches nothing has a route record");
    CHECK(p.status == KRS_OK || p.status == KRS_ERR_UNSUPPORTED, "a refusal is KRS_ERR_UNSUPPORTED");
    if (p.status != KRS_OK) {
      ++g_refused;
      // a refusal is for size alone: a grid past 32 bits or bytes past 63
      const __int128 rows_p = (__int128)c.b * pow2_ge(c.k);
      CHECK(c.b > (1 << 20) && rows_p * 8 > ((__int128)1 << 40), "a call of ordinary size is refused");
    }
    return;
  }
  CHECK(rt.kernel >= KRS_RETR_FUSED && rt.kernel <= KRS_RETR_ROWS, "no kernel for a call that has work");
  if (rt.kernel < 1 || rt.kernel > 3) return;
  ++g_kernel[rt.kernel];
  CHECK(rt.variant == c.variant && rt.es == c.es, "variant and element size");
  CHECK(p.total >= 0 && p.total < INT64_MAX, "the workspace total");

  if (c.variant == KRS_RETR_VARIANT_ROWS) {
    CHECK(rt.kernel == KRS_RETR_ROWS, "krs_topk_rows selects rows");
    CHECK(rt.vec == 0 && rt.S == 0 && rt.qtiles == 0 && rt.slice == 0 && rt.row_bytes == 0 && rt.lds_bytes == 0 &&
          rt.blocks == 0 && rt.chunks == 0 && rt.chunk_rows == 0, "fields that do not apply are 0");
    check_select(c, p, c.b, c.n);
    CHECK(p.off_merge == 0 && p.total == select_list_bytes(c.b, p.sel), "the row lists are the whole workspace");
    CHECK(p.total == (c.n <= 2048 ? 0 : c.b * pow2_ge(c.k) * 8), "krs_topk_rows_workspace_bytes");
    return;
  }

  const bool fused = c.k <= 128 && c.d <= 512;
  CHECK((rt.kernel == KRS_RETR_FUSED) == fused, "fused exactly when k <= 128 and d <= 512");
  if (rt.kernel == KRS_RETR_FUSED) {
    const int64_t S = p.S, slice = p.slice, qtiles = p.qtiles;
    CHECK(rt.S == p.S && rt.qtiles == p.qtiles && rt.slice == p.slice && rt.row_bytes == p.row_bytes &&
          rt.lds_bytes == p.lds_bytes && rt.blocks == p.blocks && rt.vec == (int)p.vec && rt.chunks == 0 &&
          rt.chunk_rows == 0, "the record's stage 1 is the plan's");
    CHECK(slice > 0 && slice % 128 == 0, "slice % 128 == 0");
    CHECK(S >= 8 && S % 8 == 0, "S % 8 == 0");
    CHECK(S * slice >= c.n, "S * slice >= n");
    CHECK((S - 8) * slice < c.n, "(S - 8) * slice < n");
    CHECK(qtiles * 32 >= c.b && (qtiles - 1) * 32 < c.b, "the query tiles cover b");
    CHECK(c.k + 128 <= 256, "k + kCB <= kQueue");
    CHECK(slice <= INT32_MAX && S * slice < ((int64_t)1 << 33), "slice offsets stay small");
    // stage1_body's K loop: whole 32-byte steps that cover d elements, at most 8 per trip times the trips it makes
    CHECK(p.row_bytes % 32 == 0 && p.row_bytes >= c.d * c.es && p.row_bytes - 32 < c.d * c.es, "row_bytes");
    // stage1_body's own layout of the dynamic LDS
    int64_t lds = 32 * ((int64_t)p.row_bytes + 16);        // qt [kQM][lstride]
    lds += (int64_t)32 * 256 * 8;                           // queue [kQM][cap]
    lds += 32 * 4;                                          // cnt
    lds += 32 * 4;                                          // thr
    if (c.variant == KRS_RETR_VARIANT_Q8) lds += 32 * 4;    // qstep
    if (c.variant == KRS_RETR_VARIANT_MINE) {
      CHECK(lds % 8 == 0, "the positives' ids sit on 8 bytes");
      lds += 32 * 8 + 32 * 4;                               // pid, posr
    }
    CHECK(p.lds_bytes == lds, "lds_bytes is the kernel's own layout");
    CHECK(p.lds_bytes < 160 * 1024, "lds_bytes stays below 160 KiB");
    CHECK(p.blocks == S * qtiles && p.blocks <= kMaxGrid, "the stage-1 grid");
    // slot >> 3 of the last workgroup names the last (slice group, query tile): every (slice, tile) has a workgroup
    CHECK(((p.blocks - 1) >> 3) / qtiles * 8 + 7 == S - 1, "the grid deals every slice to an XCD");
    const bool vec = (c.d * c.es) % 16 == 0 && (c.ldc * c.es) % 16 == 0 && c.c_addr % 16 == 0;
    CHECK(p.vec == vec, "VEC exactly when rows are whole 16-byte chunks on a 16-byte boundary");
    ++g_vec[p.vec];
    check_select(c, p, c.b, S * c.k);
    CHECK(p.sel.route == KRS_SELECT_LDS || (p.sel.route == KRS_SELECT_RADIX && p.sel.P <= 128), "stage 1's lists never need the global merge");
    // sections: slice lists, merge lists, then (q8) the quantized rows and their steps
    const int64_t lists = c.b * S * c.k * 8, merge = select_list_bytes(c.b, p.sel);
    CHECK(p.off_lists == 0 && p.off_merge % 256 == 0 && p.off_merge >= lists, "the merge lists follow the slice lists");
    __int128 want = up256(lists) + up256(merge);
    if (c.variant == KRS_RETR_VARIANT_Q8) {
      CHECK(p.off_qq % 256 == 0 && p.off_qq >= p.off_merge + merge, "the quantized rows follow the merge lists");
      CHECK(p.off_qstep % 256 == 0 && p.off_qstep >= p.off_qq + c.b * p.row_bytes, "the steps follow the quantized rows");
      CHECK(p.total >= p.off_qstep + c.b * 4, "the steps fit");
      want += up256((__int128)c.b * p.row_bytes) + up256((__int128)c.b * 4);
    } else {
      CHECK(p.total >= p.off_merge + merge, "the merge lists fit");
    }
    CHECK((__int128)p.total == want, "the sections sum to *_workspace_bytes");
    return;
  }

  CHECK(c.variant == KRS_RETR_VARIANT_TOPK, "only krs_retrieval_topk has a two-step path");
  CHECK(rt.vec == 0 && rt.S == 0 && rt.qtiles == 0 && rt.slice == 0 && rt.row_bytes == 0 && rt.lds_bytes == 0 && rt.blocks == 0,
        "fields that do not apply are 0");
  const int64_t bc = p.chunk_rows, chunks = p.chunks;
  CHECK(rt.chunks == chunks && rt.chunk_rows == bc, "the record's chunks are the plan's");
  CHECK(bc >= 1 && bc <= c.b && chunks >= 1, "a chunk has at least one row");
  CHECK((__int128)(chunks - 1) * bc < c.b && (__int128)chunks * bc >= c.b, "the chunks tile [0, b)");
  if (chunks > 1) ++g_multi_chunk;
  int64_t covered = 0;
  bool tiled = true;
  const int64_t walk = chunks < 64 ? chunks : 64;          // the head of the list, then its tail
  for (int64_t i = 0; i < walk; ++i) {
    tiled = tiled && chunk_row0(p, i) == covered && chunk_len(p, i, c.b) >= 1 && chunk_len(p, i, c.b) <= bc;
    covered += chunk_len(p, i, c.b);
  }
  if (chunks == walk) tiled = tiled && covered == c.b;
  else tiled = tiled && chunk_row0(p, chunks - 1) + chunk_len(p, chunks - 1, c.b) == c.b && chunk_len(p, chunks - 1, c.b) >= 1;
  CHECK(tiled, "every chunk starts where the last one ended");
  check_select(c, p, bc, c.n);
  const __int128 per_row = (__int128)c.n * 4 + (c.n <= 2048 ? 0 : pow2_ge(c.k) * 8);
  CHECK(bc == 1 || per_row * bc <= c.slab_budget, "a chunk's slab and lists stay within the budget");
  CHECK(bc == c.b || per_row * (bc + 1) > c.slab_budget, "a chunk is as long as the budget allows");
  const int64_t slab = bc * c.n * 4, merge = select_list_bytes(bc, p.sel);
  CHECK(p.off_slab == 0 && p.off_merge % 256 == 0 && p.off_merge >= slab, "the lists follow the slab");
  CHECK(p.off_gemm % 256 == 0 && p.off_gemm >= p.off_merge + merge, "krs_gemm's workspace follows the lists");
  CHECK(p.gemm_bytes % 256 == 0 && p.total == p.off_gemm + p.gemm_bytes, "krs_gemm's workspace ends the workspace");
  CHECK((size_t)p.gemm_bytes >= krs::gplan::plan_workspace_bytes(bc, c.n, c.d, false), "a full chunk's GEMM workspace");
  const int64_t tail = c.b - (chunks - 1) * bc;
  CHECK((size_t)p.gemm_bytes >= krs::gplan::plan_workspace_bytes(tail, c.n, c.d, false), "the tail chunk's GEMM workspace");
  CHECK((__int128)p.total == up256(slab) + up256(merge) + p.gemm_bytes, "the sections sum to *_workspace_bytes");
}

int main() {
  const int64_t kBig = ((int64_t)1 << 31) - 1;
  const int64_t bs[] = {0, 1, 31, 32, 33, 130, 4097, 65536, kBig};
  const int ks[] = {1, 2, 3, 4, 5, 64, 85, 86, 127, 128, 129, 2048, 2049, 4097};
  const int64_t budgets[] = {kSlabBudget, 1, 4096, 300000, (int64_t)1 << 40};
  const uint64_t base = 0x7f0000100000ull;
  for (int64_t b : bs)
    for (int k : ks) {
      const int64_t ns[] = {1, k, 127, 128, 129, 255, 8192, 65536, 65537, 131072, 131073, ((int64_t)1 << 20) + 37, kBig};
      for (int64_t n : ns) {
        if (k > n) continue;
        Call c;
        c.b = b; c.n = n; c.k = k;
        c.variant = KRS_RETR_VARIANT_ROWS;
        c.d = 0; c.es = 4; c.ldc = n; c.c_addr = base;
        check(c);
        for (int64_t d = 1; d <= 520; ++d) {
          c.d = d; c.ldc = d; c.c_addr = base;
          for (int es : {2, 4}) {
            c.variant = KRS_RETR_VARIANT_TOPK;
            c.es = es;
            if (fused_path(d, k)) {
              check(c);
            } else {
              for (int64_t budget : budgets) {
                c.slab_budget = budget;
                check(c);
              }
              c.slab_budget = kSlabBudget;
            }
            if (fused_path(d, k) && k <= n - 1) {
              c.variant = KRS_RETR_VARIANT_MINE;
              check(c);
            }
          }
          if (fused_path(d, k)) {
            c.variant = KRS_RETR_VARIANT_Q8;
            c.es = 1;
            check(c);
          }
        }
      }
    }
  // wide rows, where krs_gemm splits K and asks for a workspace that depends on the chunk's rows: the shorter tail chunk
  // may ask for more than a full one
  long tail_larger = 0;
  for (int64_t b : {33, 70, 130, 1000, 4097})
    for (int64_t n : {255, 3000, 8192, 65537})
      for (int64_t d : {1024, 4096, 16384, 65536})
        for (int k : {10, 129, 200})
          for (int64_t rows : {1, 7, 16, 32, 100, 128, 1000}) {
            Call c;
            c.variant = KRS_RETR_VARIANT_TOPK;
            c.b = b; c.n = n; c.d = d; c.k = k; c.es = 2; c.ldc = d; c.c_addr = base;
            c.slab_budget = rows * (n * 4 + (n <= 2048 ? 0 : 256 * 8));
            check(c);
            const Plan p = plan_retrieval(c);
            if (p.chunks > 1 && b % p.chunk_rows &&
                krs::gplan::plan_workspace_bytes(b % p.chunk_rows, n, d, false) > krs::gplan::plan_workspace_bytes(p.chunk_rows, n, d, false))
              ++tail_larger;
          }
  if (tail_larger == 0) {
    std::printf("FAILED the walk met no tail chunk whose krs_gemm workspace exceeds a full chunk's\n");
    ++g_failed["coverage"];
  }
  // the three ways of losing VEC at every width: a misaligned base, an odd row stride, (the width itself is the third)
  for (int64_t d = 1; d <= 520; ++d)
    for (int es : {1, 2, 4})
      for (int way = 0; way < 4; ++way) {
        if (d > 512) continue;
        Call c;
        c.variant = es == 1 ? KRS_RETR_VARIANT_Q8 : KRS_RETR_VARIANT_TOPK;
        c.b = 33; c.n = 255; c.d = d; c.k = 10; c.es = es;
        c.ldc = way == 2 ? d + 1 : (way == 3 ? d + 3 : d);
        c.c_addr = base + (way == 1 || way == 3 ? (uint64_t)es : 0);
        check(c);
      }
  long failed = 0;
  for (const auto& kv : g_failed) failed += kv.second;
  std::printf("%ld plans: fused %ld, slab %ld (multi-chunk %ld), rows %ld; select lds %ld radix %ld merge %ld; vec %ld element %ld; "
              "refused %ld\n", g_plans, g_kernel[1], g_kernel[2], g_multi_chunk, g_kernel[3], g_select[1], g_select[2],
              g_select[3], g_vec[1], g_vec[0], g_refused);
  const bool covered = g_kernel[1] && g_kernel[2] && g_kernel[3] && g_select[1] && g_select[2] && g_select[3] && g_vec[0] &&
                       g_vec[1] && g_multi_chunk;
  if (!covered) {
    std::printf("FAILED the walk did not reach every route\n");
    ++failed;
  }
  if (failed) std::printf("%ld checks, %ld failed checks\n", g_checks, failed);
  else std::printf("%ld 0 failed checks\n", g_checks);
  return failed ? 1 : 0;
}
