// Walks krs::ln::plan (keras_rs_amd/csrc/ln_plan.h, which includes seq_attn_plan.h for the dropout hash; no other
// project header) over a grid of (n, d, dtype, aligned) and checks what every plan promises the K22 kernels that read
// it.  Stand-alone: tests/test_layer_norm_host.py builds it with the host compiler and -fsanitize=address,undefined and
// runs it as a child process.  After the walk it prints one line "status kernel lanes per_lane vec rows_per_pass
// rows_per_group groups workspace_bytes" per "n d dtype aligned" tuple of its command line (four numbers each), then,
// for "hash seed draw row column" tuples, the dropout hash, then the tally.  Exit 0 = every invariant held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../keras_rs_amd/csrc/ln_plan.h"

using namespace krs::ln;

static std::map<std::string, long> g_failed;
static long g_plans = 0;
static std::map<int, long> g_builds;

#define CHECK(cond, what)                                                                                      \
  do {                                                                                                         \
    if (!(cond) && ++g_failed[what] <= 3)                                                                      \
      std::printf("FAILED %s: n=%lld d=%lld dtype=%d aligned=%d\n", what, (long long)n, (long long)d, dtype,   \
                  (int)aligned);                                                                               \
  } while (0)

static void check(int64_t n, int64_t d, int dtype, bool aligned) {
  const Plan pl = plan(n, d, dtype, aligned);
  ++g_plans;
  const bool bad = n < 0 || d < 1 || (dtype != kF32 && dtype != kBF16);
  CHECK((pl.status == kInvalid) == bad, "invalid exactly for a bad shape or dtype");
  if (pl.status != kOk) {
    CHECK(pl.kernel == kRouteNone && pl.groups == 0 && pl.lanes_per_row == 0, "a refused call has no route");
    CHECK(pl.why && std::strlen(pl.why) > 0, "a refusal names its limit");
    if (pl.status == kUnsupported) CHECK(d > kMaxD || n > kMaxN, "unsupported only beyond a limit");
    if (n < 0 || d < 1 || d > kMaxD || n > kMaxN) CHECK(workspace_bytes(n, d) == 0, "a refused shape needs no workspace");
    return;
  }
  CHECK(d <= kMaxD && n <= kMaxN, "an accepted call is within the limits");
  if (n == 0) {
    CHECK(pl.kernel == kRouteNone && pl.groups == 0, "an empty call launches nothing");
    CHECK(workspace_bytes(n, d) == 0, "an empty call needs no workspace");
    return;
  }
  const int chunk = dtype == kBF16 ? 8 : 4;
  ++g_builds[(dtype * 2 + pl.vec) * 100 + pl.per_lane];
  CHECK(pl.vec == (aligned && d % chunk == 0), "16-byte accesses only on whole aligned chunks");
  CHECK(pl.kernel == (pl.vec ? kRouteVec : kRouteElem), "the route is the vec claim");
  const int lanes = pl.lanes_per_row;
  CHECK(lanes == 8 || lanes == 16 || lanes == 32 || lanes == 64, "8, 16, 32 or 64 lanes own a row");
  CHECK(pl.per_lane == 8 || pl.per_lane == 16 || pl.per_lane == 32 || pl.per_lane == 64, "8, 16, 32 or 64 registers a lane");
  CHECK((int64_t)lanes * pl.per_lane >= d, "the lanes hold the row");
  CHECK(pl.per_lane >= chunk && pl.per_lane % chunk == 0, "a lane holds whole chunks");
  CHECK(lanes == 64 || pl.per_lane == 8, "more than 8 registers a lane only when the whole wave owns the row");
  CHECK(lanes == kMinLanes || (int64_t)(lanes / 2) * pl.per_lane < d, "no fewer lanes would hold the row");
  CHECK(pl.per_lane == 8 || (int64_t)lanes * (pl.per_lane / 2) < d, "no fewer registers would hold the row");
  CHECK(pl.rows_per_pass == kThreads / lanes, "a workgroup has 256 / lanes rows in flight");
  CHECK(pl.rows_per_group >= pl.rows_per_pass && pl.rows_per_group % pl.rows_per_pass == 0, "a workgroup owns whole passes");
  CHECK(pl.groups >= 1 && pl.groups <= kMaxGroups, "grid within the bound of the partials");
  CHECK(pl.groups * pl.rows_per_group >= n && (pl.groups - 1) * pl.rows_per_group < n, "the workgroups cover n exactly");
  const Plan other = plan(n, d, dtype == kBF16 ? kF32 : kBF16, !aligned);
  CHECK(other.groups == pl.groups && other.lanes_per_row == lanes && other.per_lane == pl.per_lane,
        "the layout depends on n and d alone (so does the workspace)");
  const size_t ws = workspace_bytes(n, d);
  CHECK(ws >= (size_t)pl.groups * 2 * (size_t)d * 4 && ws % 256 == 0 && ws < (size_t)pl.groups * 2 * (size_t)d * 4 + 256,
        "workspace holds two fp32 rows of d per workgroup");
}

int main(int argc, char** argv) {
  const std::vector<int64_t> ns = {-1, 0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 257, 8191, 8192, 8193, 65536, 819200,
                                   (int64_t)1 << 24, 2147483647, (int64_t)1 << 31, (int64_t)1 << 40};
  const std::vector<int64_t> ds = {0, 1, 2, 7, 8, 50, 63, 64, 65, 100, 128, 129, 255, 256, 257, 511, 512, 513, 1000, 1024,
                                   1025, 1999, 2048, 2049, 4095, 4096, 4097, (int64_t)1 << 33};
  for (int64_t n : ns)
    for (int64_t d : ds)
      for (int dtype : {0, 1, 2, -1})
        for (int aligned = 0; aligned < 2; ++aligned) check(n, d, dtype, aligned != 0);
  int i = 1;
  while (i < argc) {
    if (std::strcmp(argv[i], "hash") == 0 && i + 4 < argc) {
      const uint64_t seed = std::strtoull(argv[i + 1], nullptr, 10), draw = std::strtoull(argv[i + 2], nullptr, 10);
      const uint32_t base = hash_base((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)draw, (uint32_t)(draw >> 32),
                                      (uint32_t)std::strtoull(argv[i + 3], nullptr, 10));
      std::printf("%u\n", mix32(base + (uint32_t)std::strtoull(argv[i + 4], nullptr, 10)));
      i += 5;
    } else if (i + 3 < argc) {
      const int64_t n = std::atoll(argv[i]), d = std::atoll(argv[i + 1]);
      const Plan pl = plan(n, d, std::atoi(argv[i + 2]), std::atoi(argv[i + 3]) != 0);
      std::printf("%d %d %d %d %d %d %lld %lld %zu\n", pl.status, pl.kernel, pl.lanes_per_row, pl.per_lane, pl.vec,
                  pl.rows_per_pass, (long long)pl.rows_per_group, (long long)pl.groups, workspace_bytes(n, d));
      i += 4;
    } else {
      std::printf("usage: ln_plan_check [n d dtype aligned | hash seed draw row column]...\n");
      return 2;
    }
  }
  long total = 0;
  if (g_builds.size() != 16) { std::printf("the grid reached %zu of the 16 (dtype, vec, per_lane) builds\n", g_builds.size()); ++total; }
  if (drop_threshold(0.0f) != 0u || drop_threshold(0.5f) != 0x80000000u) { std::printf("drop_threshold\n"); ++total; }
  for (const auto& f : g_failed) { std::printf("%ld x %s\n", f.second, f.first.c_str()); total += f.second; }
  std::printf("%ld plans, %ld failed checks\n", g_plans, total);
  return total ? 1 : 0;
}
