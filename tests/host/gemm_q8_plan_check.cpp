// Walks a lattice of krs_gemm_q8 calls through the planner (keras_rs_amd/csrc/gemm_q8_plan.h, which builds on gemm_plan.h;
// no other project header) and checks what every plan promises the kernel it names.  Stand-alone:
// tests/test_gemm_q8_host.py builds it with the host compiler and -fsanitize=address,undefined and runs it as a child
// process.  Exit 0 = every invariant held; otherwise the first offending calls of each invariant are printed, exit status 1.
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../../keras_rs_amd/csrc/gemm_q8_plan.h"

using namespace krs;
using gplan::GemmCall;
using q8plan::Q8Plan;

static std::map<std::string, long> g_failed;
static long g_plans = 0, g_kernel[4] = {}, g_refused = 0, g_cross = 0;

static void report(const char* what, const GemmCall& c, const Q8Plan& p) {
  if (++g_failed[what] > 3) return;
  std::printf("FAILED %s: m=%lld n=%lld k=%lld lda=%lld ldw=%lld ldc=%lld al_a=%d al_w=%d al_c=%d -> kernel=%d ep_vec=%d "
              "k_tail=%d status=%d grid=%lld block=%d lds=%zu nt=%d\n",
              what, (long long)c.m, (long long)c.n, (long long)c.k, (long long)c.lda, (long long)c.ldb, (long long)c.ldc,
              (int)c.al_a, (int)c.al_b, (int)c.al_c, p.route.kernel, p.route.ep_vec, p.route.k_tail, p.status,
              (long long)p.grid, p.block, p.lds, p.nt);
}

#define CHECK(cond, what) do { if (!(cond)) report(what, c, p); } while (0)

static void check(const GemmCall& c, const Q8Plan& p) {
  ++g_plans;
  const krs_gemm_q8_route& rt = p.route;
  const int64_t m = c.m, n = c.n, k = c.k;
  CHECK(p.status == KRS_OK || p.status == KRS_ERR_UNSUPPORTED, "a status the entry does not document");
  // every refusal is decided here, before any launch: it names its limit and carries no kernel, grid or LDS
  if (p.status != KRS_OK) {
    ++g_refused;
    CHECK(rt.kernel == KRS_GEMM_Q8_KERNEL_NONE && rt.ep_vec == 0 && rt.k_tail == 0 && rt.epilogue == 0 && p.grid == 0 && p.lds == 0,
          "a refused call has a route record");
    CHECK(p.why && p.why[0], "a refusal without a message");
    CHECK(k > q8plan::kMaxK || m > INT32_MAX || n > INT32_MAX || (m > 0 && n > 0), "a refusal without a cause");
    return;
  }
  CHECK(k <= q8plan::kMaxK, "a contraction that can overflow int32 was accepted");
  if (m == 0 || n == 0) {
    CHECK(rt.kernel == KRS_GEMM_Q8_KERNEL_NONE && p.grid == 0, "an empty product has a route record");
    return;
  }
  CHECK(rt.kernel >= KRS_GEMM_Q8_KERNEL_GENERIC && rt.kernel <= KRS_GEMM_Q8_KERNEL_RING, "no kernel for a product with work");
  if (rt.kernel >= 0 && rt.kernel <= 3) ++g_kernel[rt.kernel];
  CHECK(p.grid >= 1 && p.grid * p.block <= 0xffffffffll, "grid beyond the launch limits");
  const bool vec16 = c.al_a && c.al_b && c.lda % 16 == 0 && c.ldb % 16 == 0 && k % 16 == 0 && k > 0;
  // ep_vec promises 8-wide access to every epilogue operand
  if (rt.ep_vec) {
    CHECK(n % 8 == 0 && c.ldc % 8 == 0 && c.al_c && (!c.bias || c.al_bias), "ep_vec: C or bias");
    CHECK(!c.x0 || (c.al_x0 && c.al_x && c.ldx % 8 == 0), "ep_vec: x0 / x");
    CHECK(!c.u_out || (c.al_u && c.ldu % 8 == 0), "ep_vec: u_out");
    CHECK(!c.r || (c.al_r && c.ldr % 8 == 0), "ep_vec: r");
  }
  switch (rt.kernel) {
    case KRS_GEMM_Q8_KERNEL_RING:
      CHECK(vec16, "ring: 16-byte loads on an operand that does not allow them");
      CHECK(k % 128 == 0 && k / 128 >= 3, "ring: not whole pieces, or fewer than three");
      CHECK(m >= 256 && n >= 256, "ring: a dimension below its tile");
      CHECK(gplan::cdiv(m, 256) * gplan::cdiv(n, 256) >= q8plan::kFillTiles, "ring: below the chip-fill bar");
      CHECK(p.block == 512 && p.lds == 163840 && p.nt == (n + 255) / 256, "ring: launch arguments");
      // the kernel maps workgroup id -> (M tile = (id >> 3) / nt * 8 + (id & 7), N tile = (id >> 3) % nt): every tile once
      CHECK(p.grid == (gplan::cdiv(m, 256) + 7) / 8 * 8 * p.nt, "ring: grid does not cover the tiles");
      CHECK(rt.k_tail == 0, "ring: k_tail set");
      // the cross build loads x0 / x and stores C / u_out as bf16 vectors, unconditionally
      CHECK(rt.epilogue == (c.has_ep && rt.ep_vec && c.out_dtype == KRS_BF16 && c.x0 && !c.r ? 1 : 0), "ring: epilogue build");
      if (rt.epilogue == 1) ++g_cross;
      break;
    case KRS_GEMM_Q8_KERNEL_TILE128:
      CHECK(vec16, "tile128: 16-byte loads on an operand that does not allow them");
      CHECK(p.block == 256 && p.lds == 2 * 128 * 144, "tile128: launch arguments");
      CHECK(p.lds >= 4 * 32 * 68 * 4, "tile128: the epilogue's staging does not fit");
      CHECK(p.grid == (gplan::cdiv(m, 128) + 7) / 8 * 8 * gplan::cdiv(n, 128), "tile128: grid does not cover the tiles");
      CHECK(rt.k_tail == (k % 128 != 0) && rt.epilogue == 0, "tile128: k_tail / epilogue");
      // not the ring although the ring's conditions hold?
      CHECK(!(m >= 256 && n >= 256 && k % 128 == 0 && k >= 384 &&
              gplan::cdiv(m, 256) * gplan::cdiv(n, 256) >= q8plan::kFillTiles), "tile128 for a ring shape");
      break;
    default:
      CHECK(!vec16, "generic for a tile-eligible call");
      CHECK(p.block == 256 && p.lds == 0 && p.grid == gplan::cdiv(m * n, 256), "generic: launch arguments");
      CHECK(rt.k_tail == 0 && rt.epilogue == 0, "generic: k_tail / epilogue set");
  }
}

int main() {
  const std::vector<int64_t> ms = {0, 1, 7, 127, 128, 129, 255, 256, 257, 1000, 12035, 24575, 48896, 49152, 65536, 1 << 22,
                                   (1ll << 31) - 1, 1ll << 31};
  const std::vector<int64_t> ns = {0, 1, 8, 13, 127, 128, 129, 255, 256, 257, 512, 776, 1024, 3456, 1 << 20, (1ll << 31) - 1,
                                   1ll << 31};
  const std::vector<int64_t> ks = {0, 1, 13, 15, 16, 17, 32, 48, 127, 128, 144, 256, 383, 384, 400, 512, 640, 3456, 131072 - 128,
                                   131072, 131073, 1 << 20};
  for (int64_t m : ms)
    for (int64_t n : ns)
      for (int64_t k : ks)
        for (int pad = 0; pad < 4; ++pad)          // 0: dense rows; 1: lda + 16; 2: lda + 8 (breaks alignment); 3: ldw + 4
          for (int al = 0; al < 4; ++al)           // bit 0: aq off 16 bytes, bit 1: wq off
            for (int ep = 0; ep < 4; ++ep) {       // 0: none; 1: bias; 2: cross + u_out; 3: residual, C off 16 bytes
              GemmCall c;
              c.m = m; c.n = n; c.k = k; c.es = 1; c.a_km = false; c.b_nk = true; c.out_dtype = (m + n + k) & 1 ? KRS_BF16 : KRS_F32;
              c.lda = k + (pad == 1 ? 16 : pad == 2 ? 8 : 0);
              c.ldb = k + (pad == 3 ? 4 : 0);
              c.ldc = n + (pad == 1 ? 8 : 0);
              c.al_a = !(al & 1); c.al_b = !(al & 2);
              c.has_ep = ep != 0; c.bias = ep == 1 || ep == 2;
              c.x0 = c.u_out = ep == 2; c.ldx = c.ldu = n; c.al_u = pad != 2;
              c.r = ep == 3; c.ldr = n + (pad == 3 ? 1 : 0); c.al_c = ep != 3;
              const Q8Plan p = q8plan::plan_gemm_q8(c);
              check(c, p);
            }
  std::printf("%ld plans: generic %ld, tile128 %ld, ring %ld (cross build %ld), refused %ld\n", g_plans, g_kernel[1],
              g_kernel[2], g_kernel[3], g_cross, g_refused);
  bool thin = false;
  for (int i = 1; i <= 3; ++i) thin = thin || g_kernel[i] == 0;
  if (thin || g_refused == 0 || g_cross == 0 || g_cross == g_kernel[3]) {
    std::printf("FAILED the lattice does not reach every kernel, both ring builds and a refusal\n");
    return 1;
  }
  long failed = 0;
  for (const auto& f : g_failed) failed += f.second;
  std::printf("%ld failed checks\n", failed);
  return failed ? 1 : 0;
}
