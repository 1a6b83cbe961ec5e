// Walks krs::dwalk::plan (keras_rs_amd/csrc/dense_walk_plan.h; it includes include/krs.h and no other project header)
// over m in 1..20000 (every m to 5000, sparse above) x n in 1..9000 (sparse) x both dtypes x aligned / misaligned
// operands x the three entries with a row walk, and checks what every plan promises the kernels that read it.
// Stand-alone: tests/test_dense_walk_host.py builds it with the host compiler and -fsanitize=address,undefined and runs
// it as a child process.  After the walk it prints one line "status kernel v acc two_stage rows_per_block strips chunks
// grid_y workspace_bytes" per "entry m n dtype ld misalign want_dbias has_workspace dx0_accumulate" tuple of its command
// line (nine numbers each: ld is the one leading dimension, misalign the byte offset of the operand's base), then the
// tally.  Exit 0 = every invariant held.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "../../keras_rs_amd/csrc/dense_walk_plan.h"

using namespace krs::dwalk;

static std::map<std::string, long> g_failed;
static long g_plans = 0, g_walked = 0;
static std::map<int, long> g_routes;

#define CHECK(cond, what)                                                                                       \
  do {                                                                                                          \
    if (!(cond) && ++g_failed[what] <= 3)                                                                       \
      std::printf("FAILED %s: entry=%d m=%lld n=%lld dtype=%d aligned=%d\n", what, entry, (long long)m,         \
                  (long long)n, dtype, (int)aligned);                                                           \
  } while (0)

static Plan ask(int entry, int64_t m, int64_t n, int dtype, int64_t ld, uintptr_t base, bool dbias, bool ws, bool acc) {
  const void* ptrs[2] = {reinterpret_cast<const void*>(base), nullptr};
  Call c;
  c.entry = entry; c.m = m; c.n = n; c.dtype = dtype; c.ld = &ld; c.n_ld = entry == KRS_DENSE_WALK_COLSUM ? 0 : 1;
  c.ptrs = ptrs; c.n_ptrs = 2; c.want_dbias = dbias; c.has_workspace = ws; c.dx0_accumulate = acc;
  return plan(c);
}

static bool is_none(const krs_dense_walk_route& r) {
  return !r.kernel && !r.v && !r.acc && !r.two_stage && !r.rows_per_block && !r.reserved && !r.strips && !r.chunks && !r.grid_y;
}

// the rows the kernels' own index arithmetic gives each chunk: every row exactly once, no read-ahead row outside [0, m)
static bool rows_once(const krs_dense_walk_route& r, int64_t m) {
  const int64_t slots = r.kernel == KRS_DENSE_WALK_VEC ? r.grid_y * kWavesPerGroup : r.grid_y;
  int64_t next = 0;
  for (int64_t s = 0; s < slots; ++s) {
    const int64_t r0 = s * r.rows_per_block, r1 = std::min<int64_t>(m, r0 + r.rows_per_block);
    if (s < r.chunks ? (r0 != next || r1 <= r0) : r1 > r0) return false;    // live chunks in order; idle waves own nothing
    if (r1 > r0) next = r1;
    for (int a = 0; a < 2; ++a) {                                           // the clamped rows of the read-ahead
      const int64_t ra = std::max<int64_t>(std::min(r0 + a, r1 - 1), 0);
      if (ra < 0 || ra >= m) return false;
    }
  }
  return next == m;
}

static void check(int entry, int64_t m, int64_t n, int dtype, bool aligned, bool literal) {
  const int v = dtype == KRS_BF16 ? 8 : 4;
  const Plan pl = ask(entry, m, n, dtype, n, aligned ? 4096 : 4096 + (dtype == KRS_BF16 ? 2 : 4), true, true, true);
  ++g_plans;
  CHECK(pl.status == KRS_OK, "an ordinary shape is accepted");
  const krs_dense_walk_route& r = pl.route;
  const bool vec = entry != KRS_DENSE_WALK_COLSUM && aligned && n % v == 0;
  ++g_routes[entry * 100 + dtype * 10 + r.kernel];
  CHECK(r.kernel == (vec ? KRS_DENSE_WALK_VEC : KRS_DENSE_WALK_SCALAR), "vector exactly on whole aligned 16-byte pieces");
  CHECK(r.v == (vec ? v : 1), "v is the 16-byte width or 1");
  CHECK(r.acc == (vec && entry == KRS_DENSE_WALK_CROSS_BWD), "the ACC build is the cross vector kernel's");
  CHECK(r.two_stage == 1 && r.reserved == 0, "a workspace gives the two-stage sums");
  CHECK(r.strips >= 1 && r.strips * 64 * r.v >= n && (r.strips - 1) * 64 * r.v < n, "the strips cover n exactly");
  CHECK(r.rows_per_block >= 1 && r.chunks >= 1, "a chunk has rows");
  CHECK((int64_t)r.rows_per_block * r.chunks >= m && (int64_t)r.rows_per_block * (r.chunks - 1) < m,
        "rows_per_block * chunks >= m > rows_per_block * (chunks - 1)");
  CHECK(r.chunks <= cdiv(kTargetBlocks, r.strips) && r.chunks <= m, "no more chunks than the target or the rows");
  if (vec) CHECK(r.grid_y * 4 >= r.chunks && (r.grid_y - 1) * 4 < r.chunks, "grid_y * 4 >= chunks on the vector route");
  else CHECK(r.grid_y == r.chunks, "grid_y is the chunks on the scalar route");
  CHECK(r.grid_y <= 65535 && r.strips <= 2147483647, "the grid is launchable");
  CHECK(workspace_bytes(m, n) >= (size_t)r.grid_y * (size_t)n * sizeof(float), "the workspace covers grid_y * n floats");
  if (literal) {
    ++g_walked;
    CHECK(rows_once(r, m), "every row is in exactly one chunk");
  }
  // the same walk whatever is asked of it: outputs wanted and the workspace do not move the geometry
  const Plan bare = ask(entry, m, n, dtype, n, aligned ? 4096 : 4096 + (dtype == KRS_BF16 ? 2 : 4), false, false, false);
  CHECK(bare.route.rows_per_block == r.rows_per_block && bare.route.chunks == r.chunks && bare.route.grid_y == r.grid_y &&
            bare.route.strips == r.strips && bare.route.kernel == r.kernel, "the geometry depends on m, n and the route alone");
  CHECK(bare.route.acc == 0 && bare.route.two_stage == 0, "nothing asked, nothing claimed");
  // a leading dimension off the 16-byte grid leaves the vector route, one on it stays
  if (vec) {
    CHECK(ask(entry, m, n, dtype, n + v, 4096, true, true, false).route.kernel == KRS_DENSE_WALK_VEC, "ld = n + v stays vector");
    CHECK(ask(entry, m, n, dtype, n + 3, 4096, true, true, false).route.kernel == KRS_DENSE_WALK_SCALAR, "ld = n + 3 leaves it");
    CHECK(ask(entry, m, n, dtype, n + 1, 4096, true, true, false).route.kernel == KRS_DENSE_WALK_SCALAR, "ld = n + 1 leaves it");
  }
}

static void refusals() {
  const int entry = -1, dtype = 0;
  const int64_t m = 0, n = 0;
  const bool aligned = true;
  const int B = KRS_DENSE_WALK_CROSS_BWD;
  auto refused = [](const Plan& p, int status) { return p.status == status && is_none(p.route) && p.why && p.why[0]; };
  CHECK(refused(ask(-1, 4, 4, 0, 4, 0, 0, 0, 0), KRS_ERR_INVALID) && refused(ask(4, 4, 4, 0, 4, 0, 0, 0, 0), KRS_ERR_INVALID), "unknown entry");
  CHECK(refused(ask(B, -1, 4, 0, 4, 0, 0, 0, 0), KRS_ERR_INVALID) && refused(ask(B, 4, -1, 0, 4, 0, 0, 0, 0), KRS_ERR_INVALID), "negative size");
  CHECK(refused(ask(B, 4, 8, 0, 7, 0, 0, 0, 0), KRS_ERR_INVALID), "ld below n");
  CHECK(refused(ask(B, 4, 8, 2, 8, 0, 0, 0, 0), KRS_ERR_INVALID) && refused(ask(B, 4, 8, -1, 8, 0, 0, 0, 0), KRS_ERR_INVALID), "bad dtype");
  CHECK(refused(ask(B, (int64_t)1 << 31, 8, 0, 8, 0, 0, 0, 0), KRS_ERR_UNSUPPORTED), "m above 2^31 - 1");
  CHECK(ask(B, 2147483647, 8, 0, 8, 0, 0, 0, 0).status == KRS_OK, "m = 2^31 - 1 is planned");
  for (int e = 0; e < 4; ++e) {
    const Plan a = ask(e, 0, 8, 0, 8, 0, 1, 1, 1), b = ask(e, 8, 0, 0, 8, 0, 1, 1, 1);
    CHECK(a.status == KRS_OK && b.status == KRS_OK && is_none(a.route) && is_none(b.route), "an empty call launches nothing");
  }
  CHECK(workspace_bytes(0, 8) == 0 && workspace_bytes(8, 0) == 0 && workspace_bytes(-1, 8) == 0, "an empty shape needs no workspace");
  const Plan f = ask(KRS_DENSE_WALK_CROSS_FWD, 100, 64, 1, 64, 4096, 1, 1, 1);
  CHECK(f.route.kernel == KRS_DENSE_WALK_VEC && f.route.v == 8 && !f.route.rows_per_block && !f.route.chunks && !f.route.grid_y &&
            !f.route.strips && !f.route.acc && !f.route.two_stage, "the forward records kernel and v alone");
  CHECK(ask(KRS_DENSE_WALK_CROSS_FWD, 100, 60, 1, 60, 4096, 0, 0, 0).route.v == 1, "the forward's scalar kernel");
}

int main(int argc, char** argv) {
  std::vector<int64_t> ms, ns;
  for (int64_t m = 1; m <= 5000; ++m) ms.push_back(m);
  for (int64_t m = 5001; m <= 20000; m += (m % 1000 < 8 || m % 1024 < 4) ? 1 : 97) ms.push_back(m);
  for (int64_t n = 1; n <= 9000; ++n)
    if (n <= 130 || n % 256 <= 1 || n % 256 == 255 || n % 512 == 8 || n % 520 == 4 || n % 1000 == 250) ns.push_back(n);
  for (int entry : {KRS_DENSE_WALK_CROSS_BWD, KRS_DENSE_WALK_DENSE_ACT_BWD, KRS_DENSE_WALK_COLSUM})
    for (int64_t m : ms)
      for (int64_t n : ns)
        for (int dtype : {KRS_F32, KRS_BF16})
          for (int aligned = 0; aligned < 2; ++aligned) {
            if (entry != KRS_DENSE_WALK_CROSS_BWD && m > 300 && m % 3) continue;   // (the entries share the geometry)
            check(entry, m, n, dtype, aligned != 0, m <= 70 || (m + n) % 41 == 0);
          }
  refusals();
  for (int i = 1; i + 8 < argc; i += 9) {
    const Plan pl = ask(std::atoi(argv[i]), std::atoll(argv[i + 1]), std::atoll(argv[i + 2]), std::atoi(argv[i + 3]),
                        std::atoll(argv[i + 4]), 4096 + (uintptr_t)std::atoll(argv[i + 5]), std::atoi(argv[i + 6]) != 0,
                        std::atoi(argv[i + 7]) != 0, std::atoi(argv[i + 8]) != 0);
    const krs_dense_walk_route& r = pl.route;
    std::printf("%d %d %d %d %d %d %lld %lld %lld %zu\n", pl.status, r.kernel, r.v, r.acc, r.two_stage, r.rows_per_block,
                (long long)r.strips, (long long)r.chunks, (long long)r.grid_y,
                workspace_bytes(std::atoll(argv[i + 1]), std::atoll(argv[i + 2])));
  }
  if ((argc - 1) % 9) { std::printf("usage: dense_walk_plan_check [entry m n dtype ld misalign want_dbias has_workspace dx0_accumulate]...\n"); return 2; }
  long total = 0;
  // 2 vector-capable entries x 2 dtypes x 2 kernels + the column sum's scalar kernel at 2 dtypes
  if (g_routes.size() != 10) { std::printf("the grid reached %zu of the 10 (entry, dtype, kernel) routes\n", g_routes.size()); ++total; }
  for (const auto& f : g_failed) { std::printf("%ld x %s\n", f.second, f.first.c_str()); total += f.second; }
  std::printf("%ld plans, %ld walked row by row, %ld failed checks\n", g_plans, g_walked, total);
  return total ? 1 : 0;
}
