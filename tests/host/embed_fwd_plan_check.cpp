// Walks a grid of krs_embed_bag_fwd calls through the planner (keras_rs_amd/csrc/embed_fwd_plan.h, the only project
// header this program includes -- it compiles without HIP) and checks what every plan promises the kernel it names.
// Stand-alone: tests/test_embed_fwd_routes_host.py builds it with the host compiler and -fsanitize=address,undefined (a
// signed overflow anywhere in the planner stops it) and runs it as a child process.  Exit 0 = every invariant held;
// otherwise the first offending calls of each invariant are printed and the exit status is 1.
#include <climits>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../../keras_rs_amd/csrc/embed_fwd_plan.h"

using namespace krs::eplan;

static std::map<std::string, long> g_failed;
static long g_plans = 0, g_kernel[5] = {}, g_hot = 0, g_refused_batch = 0, g_refused_grid = 0;

static void report(const char* what, const EmbedFwdCall& c, const EmbedFwdPlan& p) {
  if (++g_failed[what] > 3) return;
  const krs_embed_fwd_route& rt = p.route;
  std::printf("FAILED %s: n_feats=%d batch=%d dim=%d nnz=%lld dtypes=%d/%d offsets=%d weights=%d out=%llx ld=%lld opt=%d -> "
              "status=%d kernel=%d lpr=%d has_w=%d stream=%d hot_rows=%d bpg=%d blocks=%lld\n",
              what, c.n_feats, c.batch, c.dim, (long long)c.nnz, c.table_dtype, c.out_dtype, (int)c.has_offsets,
              (int)c.has_weights, (unsigned long long)c.out_addr, (long long)c.out_ld, c.hot_rows_opt, p.status, rt.kernel,
              rt.lpr, rt.has_w, rt.stream, rt.hot_rows, rt.bpg, (long long)rt.blocks);
}

#define CHECK(cond, what) do { if (!(cond)) report(what, c, p); } while (0)

static void check(const EmbedFwdCall& c) {
  const EmbedFwdPlan p = plan_embed_fwd(c);
  ++g_plans;
  const krs_embed_fwd_route& rt = p.route;
  const krs_embed_fwd_route none = {};
  const bool is_none = rt.kernel == none.kernel && rt.lpr == 0 && rt.has_w == 0 && rt.stream == 0 && rt.hot_rows == 0 &&
                       rt.bpg == 0 && rt.table_dtype == 0 && rt.out_dtype == 0 && rt.blocks == 0;
  if (p.status != KRS_OK || c.n_feats == 0 || c.batch == 0) {
    CHECK(is_none, "a call that launches nothing has a route record");
    // a valid call is refused for exactly two reasons
    if (p.status == KRS_ERR_UNSUPPORTED) {
      if (c.batch > INT_MAX - 128) ++g_refused_batch; else ++g_refused_grid;
    }
    CHECK(p.status == KRS_OK || p.status == KRS_ERR_UNSUPPORTED, "a valid call is refused as invalid");
    CHECK(p.status == KRS_OK || p.why[0] != 0, "a refusal without words");
    return;
  }
  CHECK(c.batch <= INT_MAX - 128, "batch beyond the kernels' int arithmetic is planned");
  const int es_t = c.table_dtype == KRS_BF16 ? 2 : 4, es_o = c.out_dtype == KRS_BF16 ? 2 : 4;
  const int64_t row_bytes = (int64_t)c.dim * es_t, n_bags = (int64_t)c.n_feats * c.batch;
  const bool generic = row_bytes % 16 != 0 || row_bytes > 1024;
  CHECK(rt.kernel >= KRS_EMBED_FWD_VEC && rt.kernel <= KRS_EMBED_FWD_GENERIC, "no kernel for a call that has work");
  if (rt.kernel >= 0 && rt.kernel < 5) ++g_kernel[rt.kernel];
  CHECK((rt.kernel == KRS_EMBED_FWD_GENERIC) == generic, "generic exactly when the row is not whole pieces of at most 1024 bytes");
  CHECK(rt.table_dtype == c.table_dtype && rt.out_dtype == c.out_dtype, "dtype pair");
  CHECK(rt.blocks >= 1 && rt.blocks <= 0x7fffffffLL, "grid beyond the launch limit");
  if (generic) {
    CHECK(rt.lpr >= 1 && rt.lpr <= 64 && (rt.lpr & (rt.lpr - 1)) == 0 && (rt.lpr >= c.dim || rt.lpr == 64) &&
          (rt.lpr == 1 || rt.lpr / 2 < c.dim), "generic: lpr is the smallest power of two >= dim, at most 64");
    CHECK(rt.blocks * (256 / rt.lpr) >= n_bags && (rt.blocks - 1) * (256 / rt.lpr) < n_bags, "generic: blocks cover the bags");
    CHECK(rt.has_w == (int)c.has_weights && !rt.stream && !rt.hot_rows && !rt.bpg, "generic: pooled-kernel fields set");
    return;
  }
  const int64_t pieces = row_bytes / 16;
  CHECK((rt.lpr == 8 || rt.lpr == 16 || rt.lpr == 32 || rt.lpr == 64) && rt.lpr >= pieces && (rt.lpr == 8 || rt.lpr / 2 < pieces),
        "lpr is the smallest of 8 / 16 / 32 / 64 that holds the pieces");
  const bool one_hot = !c.has_offsets && !c.has_weights && c.nnz == n_bags;
  CHECK((rt.kernel != KRS_EMBED_FWD_VEC) == one_hot, "a gather kernel exactly for one unweighted dense lookup per bag");
  if (one_hot) {
    const bool rows_ok = es_t == es_o && c.n_feats <= 128 && c.out_addr % 16 == 0 &&
                         ((uint64_t)c.out_ld * (uint64_t)es_o) % 16 == 0;   // (mod 2^64 keeps mod 16)
    CHECK((rt.kernel == KRS_EMBED_FWD_HOT1_ROWS) == rows_ok, "sample-major gather off its conditions");
    CHECK(!rt.has_w && !rt.stream && !rt.hot_rows && !rt.bpg, "gather: pooled-kernel fields set");
    if (rows_ok) CHECK(rt.blocks * 4 * 64 >= n_bags && (rt.blocks - 1) * 4 * 64 < n_bags, "hot1_rows: waves cover the units");
    else {
      const int64_t waves = ((int64_t)c.batch + 63) / 64 * c.n_feats;
      CHECK(rt.blocks * 4 >= waves && (rt.blocks - 1) * 4 < waves, "hot1: waves cover the bags");
    }
    return;
  }
  CHECK(rt.bpg >= 1 && rt.bpg <= 16, "1 <= bpg <= 16");
  const int64_t mean = c.nnz / n_bags;
  CHECK(rt.bpg == (mean <= 2 ? 16 : (mean > 32 ? 1 : 32 / mean)), "bpg = clamp(32 / mean bag length, 1, 16)");
  const int64_t bags_per_wave = (int64_t)(64 / rt.lpr) * rt.bpg;
  CHECK(bags_per_wave <= 128 && (int64_t)c.batch + bags_per_wave - 1 <= INT_MAX, "the kernel's int bag arithmetic overflows");
  const int64_t waves_per_feat = ((int64_t)c.batch + bags_per_wave - 1) / bags_per_wave, waves = waves_per_feat * c.n_feats;
  CHECK(waves_per_feat * bags_per_wave >= c.batch && rt.blocks * 4 >= waves && (rt.blocks - 1) * 4 < waves, "vec: waves cover the bags");
  CHECK(rt.has_w == (int)c.has_weights && rt.stream == (int)(c.nnz < 2 * n_bags), "vec: HAS_W / STREAM");
  const bool hot = c.hot_rows_opt > 0 && !c.has_weights && es_t == 2 && es_o == 2 && row_bytes == 256;
  CHECK(rt.hot_rows == (hot ? c.hot_rows_opt : 0), "vec: hot rows off their gate");
  if (rt.hot_rows) ++g_hot;
}

int main() {
  const std::vector<int> dims = {1, 2, 3, 4, 5, 7, 8, 9, 12, 16, 20, 24, 32, 33, 36, 40, 64, 68, 72, 96, 128, 132, 136, 160, 192, 255, 256,
                                 257, 260, 264, 320, 508, 512, 513, 516, 520, 1024, 4096, INT_MAX};
  const std::vector<int> feats = {0, 1, 2, 3, 26, 127, 128, 129, 1000, 65536, INT_MAX};
  const std::vector<int> batches = {0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 4096, 16384, 1 << 20, INT_MAX - 1000, INT_MAX - 129,
                                    INT_MAX - 128, INT_MAX - 127, INT_MAX - 1, INT_MAX};
  const uint64_t base = 0x7f0000100000ull;
  for (int dim : dims)
    for (int n_feats : feats)
      for (int batch : batches) {
        const int64_t n_bags = (int64_t)n_feats * batch;
        // nnz around every threshold of the mean bag length, and the largest value
        std::vector<int64_t> nnzs = {0, 1, n_bags - 1, n_bags, n_bags + 1, 2 * n_bags - 1, 2 * n_bags};
        if (n_bags < (int64_t)1 << 56) {
          for (int64_t m : {3, 9, 16, 17, 32, 33, 40}) nnzs.push_back(m * n_bags);
          nnzs.push_back(5 * n_bags + 3);
          nnzs.push_back(33 * n_bags - 1);
        }
        nnzs.push_back(INT64_MAX);
        for (int64_t nnz : nnzs) {
          if (nnz < 0) continue;
          for (int form = 0; form < 4 * 4 * 4 * 3; ++form) {
            EmbedFwdCall c;
            c.n_feats = n_feats; c.batch = batch; c.dim = dim; c.nnz = nnz;
            c.table_dtype = form & 1 ? KRS_BF16 : KRS_F32; c.out_dtype = form & 2 ? KRS_BF16 : KRS_F32;
            c.has_offsets = (form >> 2) & 1; c.has_weights = (form >> 3) & 1;
            const int align = (form >> 4) & 3;      // aligned | base off 2 bytes | odd row stride | a huge row stride
            c.out_addr = base + (align == 1 ? 2 : 0);
            c.out_ld = align == 2 ? (int64_t)n_feats * dim + 1 : (align == 3 ? INT64_MAX : ((int64_t)n_feats * dim + 7) / 8 * 8);
            c.hot_rows_opt = (form >> 6) == 0 ? 0 : ((form >> 6) == 1 ? 64 : 128);
            check(c);
          }
        }
      }
  // what the entry refuses as invalid, with no record
  {
    EmbedFwdCall ok;
    ok.n_feats = 2; ok.batch = 100; ok.dim = 128; ok.nnz = 600; ok.out_addr = base; ok.out_ld = 256;
    std::vector<EmbedFwdCall> bad(7, ok);
    bad[0].out_addr = 0; bad[1].n_feats = -1; bad[2].batch = -1; bad[3].dim = 0; bad[4].nnz = -1; bad[5].table_dtype = 2;
    bad[6].out_dtype = -1;
    for (const EmbedFwdCall& c : bad) {
      const EmbedFwdPlan p = plan_embed_fwd(c);
      ++g_plans;
      CHECK(p.status == KRS_ERR_INVALID && p.route.kernel == KRS_EMBED_FWD_NONE && p.route.blocks == 0 && p.route.lpr == 0,
            "an invalid call is not refused");
    }
  }
  long total = 0;
  for (int kern = 1; kern <= 4; ++kern)
    if (!g_kernel[kern]) { std::printf("the grid never reached kernel %d\n", kern); ++total; }
  if (!g_hot) { std::printf("the grid never reached the hot-rows build\n"); ++total; }
  if (!g_refused_batch) { std::printf("the grid never reached the batch refusal\n"); ++total; }
  if (!g_refused_grid) { std::printf("the grid never reached the grid refusal\n"); ++total; }
  for (const auto& f : g_failed) { std::printf("%ld x %s\n", f.second, f.first.c_str()); total += f.second; }
  std::printf("%ld plans, %ld failed checks\n", g_plans, total);
  return total ? 1 : 0;
}
