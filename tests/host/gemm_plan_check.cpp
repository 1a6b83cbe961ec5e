// Walks a lattice of krs_gemm calls through the planner (keras_rs_amd/csrc/gemm_plan.h, the only project header this
// program includes) and checks what every plan promises the kernel it names.  Stand-alone: tests/test_gemm_routes_host.py
// builds it with the host compiler and -fsanitize=address,undefined and runs it as a child process.  Exit 0 = every
// invariant held; otherwise the first offending calls of each invariant are printed and the exit status is 1.
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../../keras_rs_amd/csrc/gemm_plan.h"

using namespace krs::gplan;

static std::map<std::string, long> g_failed;
static long g_plans = 0, g_kernel[11] = {}, g_fused = 0;   // how often each kernel family / the fused backward was planned

static void report(const char* what, const GemmCall& c, const GemmPlan& p) {
  if (++g_failed[what] > 3) return;
  std::printf("FAILED %s: %s %s m=%lld n=%lld k=%lld pipe=%d allow_split=%d al_a=%d al_c=%d ws=%zu -> kernel=%d splits=%d "
              "k_per_split=%lld reduce=%d status=%d need=%zu grid=%lld,%lld,%lld\n",
              what, c.a_km ? "tn" : (c.b_nk ? "nt" : "nn"), c.es == 2 ? "bf16" : "f32", (long long)c.m, (long long)c.n,
              (long long)c.k, c.pipe, (int)c.allow_split, (int)c.al_a, (int)c.al_c, c.workspace_bytes, p.route.kernel,
              p.route.splits, (long long)p.k_per_split, p.route.reduce, p.status, p.need, (long long)p.grid[0],
              (long long)p.grid[1], (long long)p.grid[2]);
}

#define CHECK(cond, what) do { if (!(cond)) report(what, c, p); } while (0)

static void check(const GemmCall& c, const GemmPlan& p) {
  ++g_plans;
  const krs_gemm_route& rt = p.route;
  const int64_t m = c.m, n = c.n, k = c.k, s = rt.splits, kps = p.k_per_split, last = k - (s - 1) * kps;
  // the workspace the query sizes is enough for every call of the shape: never refused, never more slabs than it holds
  CHECK(p.status != KRS_ERR_WORKSPACE, "a call with the query's workspace is refused");
  if (p.status != KRS_OK || m == 0 || n == 0) {
    CHECK(rt.kernel == KRS_GEMM_KERNEL_NONE && rt.splits == 0, "a call that launches nothing has a route record");
    return;
  }
  CHECK(s >= 1 && (s > 1) == (rt.reduce != KRS_GEMM_REDUCE_NONE), "splits > 1 exactly when a reduce kernel follows");
  CHECK(s == 1 || (size_t)s * m * n * sizeof(float) <= plan_workspace_bytes(m, n, k, c.a_km), "slabs beyond the query");
  CHECK(s == 1 || c.allow_split || rt.kernel == KRS_GEMM_KERNEL_THIN, "a split although allow_split is false");
  const int64_t block = p.block;
  CHECK(block == (rt.kernel == KRS_GEMM_KERNEL_PP64 || rt.kernel == KRS_GEMM_KERNEL_PP256 || rt.kernel == KRS_GEMM_KERNEL_PP256_KSTRIDED ? 512 : 256), "workgroup size");
  CHECK(p.grid[0] >= 1 && p.grid[0] * block <= 0xffffffffll && p.grid[1] >= 1 && p.grid[1] <= 65535 && p.grid[2] >= 1 &&
        p.grid[2] <= 65535 && p.reduce_grid * 256 <= 0xffffffffll && (p.reduce_grid > 0) == (s > 1), "grid beyond the launch limits");
  const bool nt = !c.a_km && c.b_nk, tn = c.a_km && !c.b_nk;
  if (rt.kernel >= 0 && rt.kernel <= 10) ++g_kernel[rt.kernel];
  switch (rt.kernel) {
    case KRS_GEMM_KERNEL_PP256:
    case KRS_GEMM_KERNEL_PP256_KSTRIDED:
      CHECK(k % 32 == 0 && kps % 32 == 0 && last % 32 == 0 && last >= 4 * 32 && kps >= 4 * 32, "32-k ring: a split under 4 whole blocks");
      CHECK(c.es == 2 && m >= 256 && n >= 256 && c.pipe != 0, "32-k ring: minimums");
      CHECK(rt.kernel == KRS_GEMM_KERNEL_PP256 ? nt : (tn && m % 8 == 0 && n % 8 == 0 && k % 64 == 0 && kps % 64 == 0), "32-k ring: layout");
      CHECK(p.lds == 131072 && p.nt == (n + 255) / 256, "32-k ring: launch arguments");
      break;
    case KRS_GEMM_KERNEL_PP64:
      CHECK(k % 64 == 0 && kps % 64 == 0 && last % 64 == 0 && last >= 3 * 64 && kps >= 3 * 64, "64-k ring: a split under 3 whole blocks");
      CHECK(c.es == 2 && nt && m >= 256 && n >= 256 && c.pipe == 4 && p.lds == 163840, "64-k ring: minimums");
      break;
    case KRS_GEMM_KERNEL_TN_GLDS:
      CHECK(k % 64 == 0 && kps % 64 == 0, "tn_glds: K not in whole 64-row tiles");
      CHECK(c.es == 2 && tn && m >= 8 && n >= 8 && m % 8 == 0 && n % 8 == 0 && p.lds == 65536, "tn_glds: minimums");
      break;
    case KRS_GEMM_KERNEL_GLDS:
      CHECK(s == 1 && nt && (k * c.es) % 128 == 0 && k >= 1024 && p.lds == 65536, "glds: split, or K not in whole 128-byte rows");
      break;
    case KRS_GEMM_KERNEL_MFMA:
      CHECK(s == 1 || kps % (128 / c.es) == 0, "mfma: split not in whole tile rows");
      break;
    case KRS_GEMM_KERNEL_THIN:
      CHECK(tn && std::min(m, n) <= 16 && k >= 1024 && rt.thin_width >= std::min(m, n) && rt.thin_is_a == (m <= n), "thin: minimums");
      break;
    case KRS_GEMM_KERNEL_ROWDOT:
      CHECK(!c.a_km && s == 1 && n <= 8 && m >= 1024 && k >= 32, "rowdot: minimums");
      break;
    case KRS_GEMM_KERNEL_SMALLK:
      CHECK(!c.a_km && s == 1 && n % 8 == 0 && (size_t)k * n * 4 <= 65536 && p.lds == (size_t)k * n * 4, "smallk: B beyond 64 KB of LDS");
      break;
    case KRS_GEMM_KERNEL_GENERIC:
      CHECK(s == 1, "generic: split");
      break;
    default:
      CHECK(false, "no kernel for a product that has work");
  }
  const bool tile = rt.kernel >= KRS_GEMM_KERNEL_MFMA && rt.kernel <= KRS_GEMM_KERNEL_PP64;
  CHECK(tile == tile_eligible(c), "a tile kernel for an operand it cannot vector-load (or none for one it can)");
  CHECK(rt.epilogue == 0 || (tile && s == 1 && rt.ep_vec && c.out_dtype == KRS_BF16), "epilogue build 1 / 2 off its conditions");
}

// the fused cross backward rides on the product's own plan: fused only where krs_gemm itself (split allowed, the query's
// workspace) would run the same product unsplit on the same ring kernel
static void check_cross_bwd(GemmCall c) {
  c.allow_split = false;
  c.workspace_bytes = 0;
  for (int streams = 0; streams < 2; ++streams) {
    CrossBwdPlan cb;
    cb.product = plan_gemm(c);
    plan_cross_bwd(cb, c.r, c.n, streams != 0, !c.r, true, true, false, false);
    GemmCall g = c;
    g.allow_split = true;
    g.workspace_bytes = plan_workspace_bytes(c.m, c.n, c.k, false);
    const GemmPlan p = plan_gemm(g);
    ++g_plans;
    if (cb.product.status != KRS_OK) { CHECK(cb.route == KRS_CROSS_BWD_NONE, "cross_bwd: a route for a refused product"); continue; }
    const bool fused = cb.route == KRS_CROSS_BWD_PP64 || cb.route == KRS_CROSS_BWD_PP256;
    CHECK(fused || (cb.route == KRS_CROSS_BWD_TWO_CALL && cb.epilogue == 0), "cross_bwd: neither fused nor two-call");
    if (!fused) continue;
    ++g_fused;
    CHECK(streams && p.route.splits == 1 && p.route.kernel == (cb.route == KRS_CROSS_BWD_PP64 ? KRS_GEMM_KERNEL_PP64 : KRS_GEMM_KERNEL_PP256),
          "cross_bwd: fused where krs_gemm would not run the product unsplit on that ring");
    CHECK(cb.epilogue == (c.r ? 3 : 10) && p.route.ep_vec && c.es == 2, "cross_bwd: epilogue number");
  }
}

int main() {
  const std::vector<int64_t> mn = {1, 3, 7, 8, 13, 16, 17, 64, 130, 136, 255, 256, 264, 520, 1032, 2056, 3456, 8192, 12296, 65536};
  // K: around every threshold for every (m, n); the fine sweep (every multiple of 8 up to 8192, of 32 up to 70000) for the
  // pairs below, which sit on both sides of each m / n threshold -- the whole cross product would run for minutes
  const std::vector<int64_t> k_edges = {0, 1, 5, 8, 15, 16, 17, 24, 31, 32, 33, 40, 63, 64, 72, 77, 128, 136, 192, 200, 255,
      256, 264, 288, 320, 448, 511, 512, 520, 1000, 1023, 1024, 1030, 1056, 1088, 2047, 2048, 2080, 2112, 4095, 4096, 4100,
      4104, 4288, 4352, 4672, 6144, 8192, 9000, 24576, 65536, 69984, 70000};
  std::vector<int64_t> k_fine = {0, 1, 9, 77, 1031, 4099, 69999};
  for (int64_t k = 8; k <= 8192; k += 8) k_fine.push_back(k);
  for (int64_t k = 8192 + 32; k <= 70000; k += 32) k_fine.push_back(k);
  const std::vector<std::pair<int64_t, int64_t>> fine_pairs = {{256, 256}, {255, 256}, {256, 264}, {264, 520}, {520, 520},
      {1032, 520}, {2056, 1032}, {3456, 520}, {8192, 520}, {520, 8192}, {16, 16}, {13, 520}, {520, 7}, {130, 136}, {12296, 256},
      {65536, 256}, {17, 2056}};
  auto walk = [&](int64_t m, int64_t n, const std::vector<int64_t>& ks) {
    long form = 0;
    for (int64_t k : ks)
      for (int layout = 0; layout < 3; ++layout)
        for (int es = 2; es <= 4; es += 2)
          for (int pipe : {0, 4, 5})
            for (int allow = 0; allow < 2; ++allow)
              for (int align = 0; align < 3; ++align, ++form) {     // all bases aligned | A off 16 bytes | C off 16 bytes
                GemmCall c;
                c.m = m; c.n = n; c.k = k; c.a_km = layout == 2; c.b_nk = layout == 1; c.es = es; c.pipe = pipe;
                c.allow_split = allow != 0; c.al_a = align != 1; c.al_c = align != 2;
                c.lda = c.a_km ? m : k; c.ldb = c.b_nk ? k : n; c.ldc = c.ldx = c.ldu = c.ldr = n;
                c.out_dtype = es == 4 || form % 5 == 0 ? KRS_F32 : KRS_BF16;
                c.has_ep = form % 4 != 0; c.bias = form % 4 == 1; c.x0 = form % 4 == 2; c.r = form % 4 == 3;   // null | bias | cross | residual
                c.tn128 = form % 7 == 0;
                c.workspace_bytes = plan_workspace_bytes(m, n, k, c.a_km);
                check(c, plan_gemm(c));
                if (layout == 1 && allow && k > 0 && !c.bias && !c.x0) check_cross_bwd(c);
              }
  };
  for (int64_t m : mn)
    for (int64_t n : mn) walk(m, n, k_edges);
  for (const auto& pr : fine_pairs) walk(pr.first, pr.second, k_fine);
  // without a workspace a split tile product is refused and leaves no record; nothing else is
  for (int64_t m : mn)
    for (int64_t n : mn)
      for (int64_t k : k_edges)
        for (int layout = 0; layout < 3; ++layout) {
          GemmCall c;
          c.m = m; c.n = n; c.k = k; c.a_km = layout == 2; c.b_nk = layout == 1;
          c.lda = c.a_km ? m : k; c.ldb = c.b_nk ? k : n; c.ldc = n;
          const GemmPlan p = plan_gemm(c);
          ++g_plans;
          CHECK(p.status == KRS_OK ? p.route.splits == 1 && p.need == 0
                                   : p.route.kernel == KRS_GEMM_KERNEL_NONE &&
                                         (p.status == KRS_ERR_WORKSPACE ? p.need > 0 : p.status == KRS_ERR_UNSUPPORTED),
                "without a workspace: neither unsplit nor refused");
        }
  long total = 0;
  for (int kern = 1; kern <= 10; ++kern)
    if (!g_kernel[kern]) { std::printf("the lattice never reached kernel %d\n", kern); ++total; }
  if (!g_fused) { std::printf("the lattice never reached the fused cross backward\n"); ++total; }
  for (const auto& f : g_failed) { std::printf("%ld x %s\n", f.second, f.first.c_str()); total += f.second; }
  std::printf("%ld plans, %ld failed checks\n", g_plans, total);
  return total ? 1 : 0;
}
