// Walks what keras_rs_amd/csrc/gemm_plan.h promises about the epilogue schedules of gemm_pp64_kernel
// (KRS_GEMM_OPT_EPI_SCHEDULE, the `schedule` field of krs_gemm_route) -- the only project header this program includes.
// Stand-alone: tests/test_gemm_epi_schedule_host.py builds it with the host compiler and -fsanitize=address,undefined and
// runs it as a child process.  Exit 0 = every invariant held; otherwise the first offenders of each are printed, exit 1.
//   * the schedule option changes nothing of a plan but the schedule bits, and option 0 sets none;
//   * bits appear only on the unsplit 64-k ring with epilogue build 1 or 2; LDS_LANDING and X_IS_X0 only with build 1, never
//     together, X_IS_X0 exactly when the call's x is its x0;
//   * the landing region lies inside the LDS bytes of a plan that names LDS_LANDING, behind the accumulator staging;
//   * the work-item order of the kernel, in panel order and staggered, gives every (tile, split) to exactly one workgroup
//     of the grid the planner launches.
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../../keras_rs_amd/csrc/gemm_plan.h"

using namespace krs::gplan;

static std::map<std::string, long> g_failed;
static long g_plans = 0, g_orders = 0, g_seen[8] = {};

static void fail(const char* what, const std::string& where) {
  if (++g_failed[what] <= 3) std::printf("FAILED %s: %s\n", what, where.c_str());
}

static std::string describe(const GemmCall& c) {
  char buf[256];
  std::snprintf(buf, sizeof buf, "m=%lld n=%lld k=%lld pipe=%d sched=%d x_is_x0=%d x0=%d r=%d bias=%d odt=%d ws=%zu",
                (long long)c.m, (long long)c.n, (long long)c.k, c.pipe, c.epi_sched, (int)c.x_is_x0, (int)c.x0, (int)c.r,
                (int)c.bias, c.out_dtype, c.workspace_bytes);
  return buf;
}

#define CHECK(cond, what) do { if (!(cond)) fail(what, describe(c)); } while (0)

static void check_plan(GemmCall c) {
  c.epi_sched = 0;
  const GemmPlan ref = plan_gemm(c);
  CHECK(ref.route.schedule == 0, "schedule bits under option 0");
  for (int sched = 1; sched <= 3; ++sched) {
    c.epi_sched = sched;
    const GemmPlan p = plan_gemm(c);
    const krs_gemm_route& rt = p.route;
    ++g_plans;
    CHECK(p.status == ref.status && rt.kernel == ref.route.kernel && rt.splits == ref.route.splits && rt.reduce == ref.route.reduce &&
              rt.epilogue == ref.route.epilogue && rt.ep_vec == ref.route.ep_vec && p.lds == ref.lds && p.nt == ref.nt &&
              p.grid[0] == ref.grid[0] && p.grid[1] == ref.grid[1] && p.grid[2] == ref.grid[2] && p.k_per_split == ref.k_per_split,
          "the schedule option changed the route");
    const int s = rt.schedule;
    if (s >= 0 && s < 8) ++g_seen[s];
    const bool streaming = rt.kernel == KRS_GEMM_KERNEL_PP64 && rt.splits == 1 && (rt.epilogue == 1 || rt.epilogue == 2);
    CHECK(s == 0 || streaming, "schedule bits off the unsplit 64-k ring's builds 1 / 2");
    CHECK((s & ~(KRS_GEMM_SCHED_LDS_LANDING | KRS_GEMM_SCHED_STAGGER | KRS_GEMM_SCHED_X_IS_X0)) == 0, "unknown schedule bits");
    CHECK(((s & KRS_GEMM_SCHED_STAGGER) != 0) == (streaming && (sched & 2)), "stagger off its option");
    const bool land = s & KRS_GEMM_SCHED_LDS_LANDING, one = s & KRS_GEMM_SCHED_X_IS_X0;
    CHECK(!(land && one), "LDS landing together with the x == x0 build");
    CHECK((land || one) == (streaming && rt.epilogue == 1 && (sched & 1)), "landing / x == x0 off the cross build or its option");
    CHECK(!one || (c.x0 && c.x_is_x0), "the x == x0 build for a call whose x is not its x0");
    CHECK(!land || !c.x_is_x0, "LDS landing for a call whose x is its x0");
    CHECK(!land || (kEpiStageBytes + kEpiLandBytes <= p.lds && kEpiLandBytes == 8 * 2 * 4 * 1024), "the landing region leaves the plan's LDS");
  }
}

// the kernel's own arithmetic: workgroup b of the grid -> (tile row, tile column, split), or nothing for a row beyond mt
static void check_order(int mt, int nt, int splits, bool stagger) {
  ++g_orders;
  const int64_t grid = round_up(mt, 8) * nt * splits;
  std::vector<int> hits((size_t)mt * nt * splits, 0);
  char where[96];
  std::snprintf(where, sizeof where, "mt=%d nt=%d splits=%d stagger=%d", mt, nt, splits, (int)stagger);
  for (int64_t b = 0; b < grid; ++b) {
    const int64_t xcd = b & 7, slot_id = b >> 3, tslot = slot_id / splits;
    const int split = (int)(slot_id - tslot * splits);
    const RingTile t = ring_tile_of_slot(tslot, nt, stagger);
    const int64_t m_tile = t.panel * 8 + xcd;
    if (t.n_tile < 0 || t.n_tile >= nt || t.panel < 0) { fail("a tile column outside the panel", where); return; }
    if (!stagger && t.n_tile != tslot % nt) { fail("panel order is not tslot % nt", where); return; }
    if (m_tile >= mt) continue;
    ++hits[((size_t)m_tile * nt + t.n_tile) * splits + split];
  }
  for (int h : hits)
    if (h != 1) { fail("a (tile, split) computed by no workgroup or by two", where); return; }
}

int main() {
  static_assert(kEpiStageBytes == 8 * 32 * 68 * 4 && kEpiStageBytes + kEpiLandBytes <= kRing64Lds, "landing region");
  const std::vector<int64_t> ms = {255, 256, 3500, 3584, 12296, 49152, 65536}, ns = {8, 256, 264, 3456, 3464, 4104};
  const std::vector<int64_t> ks = {64, 128, 192, 200, 256, 320, 448, 512, 1024, 2112, 3456};
  long form = 0;
  for (int64_t m : ms)
    for (int64_t n : ns)
      for (int64_t k : ks)
        for (int pipe : {0, 4, 5})
          for (int ep = 0; ep < 6; ++ep)                 // null | bias | cross | cross, x == x0 | residual | cross + residual
            for (int odt : {KRS_BF16, KRS_F32})
              for (int align = 0; align < 2; ++align, ++form) {
                GemmCall c;
                c.m = m; c.n = n; c.k = k; c.b_nk = true; c.pipe = pipe; c.out_dtype = odt;
                c.lda = c.ldb = k; c.ldc = c.ldx = c.ldu = c.ldr = n;
                c.has_ep = ep != 0; c.bias = ep == 1 || (ep >= 2 && form % 2); c.x0 = ep == 2 || ep == 3 || ep == 5;
                c.x_is_x0 = ep == 3; c.r = ep >= 4; c.u_out = c.x0 && form % 3 == 0; c.al_x = align == 0;
                if (c.x_is_x0) c.al_x0 = c.al_x;
                c.workspace_bytes = form % 5 ? plan_workspace_bytes(m, n, k, false) : 0;
                check_plan(c);
              }
  for (int mt = 1; mt <= 40; ++mt)
    for (int nt = 1; nt <= 20; ++nt)
      for (int splits : {1, 2, 3, 5})
        for (int stagger = 0; stagger < 2; ++stagger) check_order(mt, nt, splits, stagger != 0);
  long total = 0;
  const int L = KRS_GEMM_SCHED_LDS_LANDING, S = KRS_GEMM_SCHED_STAGGER, X = KRS_GEMM_SCHED_X_IS_X0;
  for (int s : {L, S, X, L | S, X | S})
    if (!g_seen[s]) { std::printf("the lattice never reached schedule %d\n", s); ++total; }
  for (const auto& f : g_failed) { std::printf("%ld x %s\n", f.second, f.first.c_str()); total += f.second; }
  std::printf("%ld plans, %ld tile orders, %ld failed checks\n", g_plans, g_orders, total);
  return total ? 1 : 0;
}
