// Walks a grid of krs_embed_bag_fwd_q8 and krs_quantize_rows_q8 calls through their planner
// (keras_rs_amd/csrc/embed_fwd_q8_plan.h, the only project header this program includes -- it compiles without HIP) and
// checks what every plan promises the kernel it names.  Stand-alone: tests/test_embed_q8_host.py builds it with the host
// compiler and -fsanitize=address,undefined (a signed overflow anywhere in the planner stops it) and runs it as a child
// process.  Exit 0 = every invariant held; otherwise the first offending calls of each invariant are printed and the exit
// status is 1.
#include <climits>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../../keras_rs_amd/csrc/embed_fwd_q8_plan.h"

using namespace krs::q8plan;

static std::map<std::string, long> g_failed;
static long g_plans = 0, g_kernel[5] = {}, g_refused_batch = 0, g_refused_grid = 0, g_qvec = 0, g_qscalar = 0, g_qlong = 0;

static void report(const char* what, const Q8FwdCall& c, const Q8FwdPlan& p) {
  if (++g_failed[what] > 3) return;
  const krs_embed_fwd_route& rt = p.route;
  std::printf("FAILED %s: n_feats=%d batch=%d dim=%d nnz=%lld out_dtype=%d offsets=%d weights=%d -> status=%d kernel=%d "
              "lpr=%d has_w=%d bpg=%d blocks=%lld\n",
              what, c.n_feats, c.batch, c.dim, (long long)c.nnz, c.out_dtype, (int)c.has_offsets, (int)c.has_weights,
              p.status, rt.kernel, rt.lpr, rt.has_w, rt.bpg, (long long)rt.blocks);
}

#define CHECK(cond, what) do { if (!(cond)) report(what, c, p); } while (0)

static void check(const Q8FwdCall& c) {
  const Q8FwdPlan p = plan_q8_fwd(c);
  ++g_plans;
  const krs_embed_fwd_route& rt = p.route;
  const bool is_none = rt.kernel == 0 && rt.lpr == 0 && rt.has_w == 0 && rt.stream == 0 && rt.hot_rows == 0 && rt.bpg == 0 &&
                       rt.table_dtype == 0 && rt.out_dtype == 0 && rt.blocks == 0;
  if (p.status != KRS_OK || c.n_feats == 0 || c.batch == 0) {
    CHECK(is_none, "a call that launches nothing has a route record");
    if (p.status == KRS_ERR_UNSUPPORTED) {
      if (c.batch > INT_MAX - 128) ++g_refused_batch; else ++g_refused_grid;
    }
    CHECK(p.status == KRS_OK || p.status == KRS_ERR_UNSUPPORTED, "a valid call is refused as invalid");
    CHECK(p.status == KRS_OK || p.why[0] != 0, "a refusal without words");
    return;
  }
  CHECK(c.batch <= INT_MAX - 128, "batch beyond the kernels' int arithmetic is planned");
  const int64_t n_bags = (int64_t)c.n_feats * c.batch;
  const bool generic = c.dim % 16 != 0 || c.dim > 1024;
  CHECK(rt.kernel == KRS_EMBED_FWD_VEC || rt.kernel == KRS_EMBED_FWD_GENERIC, "no q8 kernel for a call that has work");
  if (rt.kernel >= 0 && rt.kernel < 5) ++g_kernel[rt.kernel];
  CHECK((rt.kernel == KRS_EMBED_FWD_GENERIC) == generic, "generic exactly when dim is not whole pieces of at most 1024 bytes");
  CHECK(rt.table_dtype == KRS_I8 && rt.out_dtype == c.out_dtype, "dtype pair");
  CHECK(rt.blocks >= 1 && rt.blocks <= 0x7fffffffLL, "grid beyond the launch limit");
  CHECK(rt.has_w == (int)c.has_weights && !rt.stream && !rt.hot_rows, "has_w / fields the q8 kernels do not have");
  if (generic) {
    CHECK(rt.lpr >= 1 && rt.lpr <= 64 && (rt.lpr & (rt.lpr - 1)) == 0 && (rt.lpr >= c.dim || rt.lpr == 64) &&
          (rt.lpr == 1 || rt.lpr / 2 < c.dim), "generic: lpr is the smallest power of two >= dim, at most 64");
    CHECK(rt.blocks * (256 / rt.lpr) >= n_bags && (rt.blocks - 1) * (256 / rt.lpr) < n_bags, "generic: blocks cover the bags");
    CHECK(!rt.bpg, "generic: bpg set");
    return;
  }
  const int pieces = c.dim / 16;
  CHECK((rt.lpr == 8 || rt.lpr == 16 || rt.lpr == 32 || rt.lpr == 64) && rt.lpr >= pieces && (rt.lpr == 8 || rt.lpr / 2 < pieces),
        "lpr is the smallest of 8 / 16 / 32 / 64 that holds the pieces");
  CHECK(rt.bpg >= 1 && rt.bpg <= 16, "1 <= bpg <= 16");
  const int64_t mean = c.nnz / n_bags;
  CHECK(rt.bpg == (mean <= 2 ? 16 : (mean > 32 ? 1 : 32 / mean)), "bpg = clamp(32 / mean bag length, 1, 16)");
  const int64_t bags_per_wave = (int64_t)(64 / rt.lpr) * rt.bpg;
  CHECK(bags_per_wave <= 128 && (int64_t)c.batch + bags_per_wave - 1 <= INT_MAX, "the kernel's int bag arithmetic overflows");
  const int64_t waves_per_feat = ((int64_t)c.batch + bags_per_wave - 1) / bags_per_wave, waves = waves_per_feat * c.n_feats;
  CHECK(waves_per_feat * bags_per_wave >= c.batch && rt.blocks * 4 >= waves && (rt.blocks - 1) * 4 < waves, "vec: waves cover the bags");
}

static void check_quantize(int64_t vocab, int dim, int dtype, uint64_t table, uint64_t q, uint64_t step) {
  const QuantizePlan p = plan_quantize(vocab, dim, dtype, table, q, step);
  ++g_plans;
  auto bad = [&](const char* what) {
    if (++g_failed[what] <= 3)
      std::printf("FAILED %s: vocab=%lld dim=%d dtype=%d -> status=%d lanes=%d vec=%d two_pass=%d blocks=%lld\n", what,
                  (long long)vocab, dim, dtype, p.status, p.lanes, (int)p.vec, (int)p.two_pass, (long long)p.blocks);
  };
  if (vocab > INT_MAX) { if (p.status != KRS_ERR_UNSUPPORTED || p.blocks) bad("more than INT32_MAX rows are planned"); return; }
  if (p.status != KRS_OK) { bad("a valid quantize call is refused"); return; }
  if (vocab == 0) { if (p.blocks) bad("an empty table launches"); return; }
  if (!(p.lanes >= 1 && p.lanes <= 64 && (p.lanes & (p.lanes - 1)) == 0)) { bad("lanes is not a power of two in 1 .. 64"); return; }
  const int64_t rows_per_block = 256 / p.lanes;
  if (!(p.blocks >= 1 && p.blocks <= 0x7fffffffLL && p.blocks * rows_per_block >= vocab && (p.blocks - 1) * rows_per_block < vocab))
    bad("quantize: blocks do not cover the rows");
  if (p.two_pass != (dim > 1024)) bad("two passes exactly for rows longer than 1024 elements");
  if (!p.two_pass && !((int64_t)p.lanes * 16 >= dim && (p.lanes == 1 || (int64_t)(p.lanes / 2) * 16 < dim)))
    bad("lanes x 16 registers do not hold the row, or twice as many as needed");
  if (p.vec && !(dim % 16 == 0 && table % 16 == 0 && q % 16 == 0 && !p.two_pass)) bad("16-byte moves off their alignment");
  if (!p.two_pass && dim % 16 == 0 && table % 16 == 0 && q % 16 == 0 && !p.vec) bad("aligned rows without 16-byte moves");
  if (p.two_pass) ++g_qlong; else if (p.vec) ++g_qvec; else ++g_qscalar;
}

int main() {
  const std::vector<int> dims = {1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 20, 24, 32, 33, 48, 64, 96, 112, 128, 129, 144, 160, 255,
                                 256, 257, 272, 320, 496, 512, 513, 528, 1008, 1023, 1024, 1025, 1040, 4096, INT_MAX};
  const std::vector<int> feats = {0, 1, 2, 3, 26, 127, 128, 129, 1000, 65536, INT_MAX};
  const std::vector<int> batches = {0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 4096, 16384, 1 << 20, INT_MAX - 1000, INT_MAX - 129,
                                    INT_MAX - 128, INT_MAX - 127, INT_MAX - 1, INT_MAX};
  const uint64_t base = 0x7f0000100000ull;
  for (int dim : dims)
    for (int n_feats : feats)
      for (int batch : batches) {
        const int64_t n_bags = (int64_t)n_feats * batch;
        std::vector<int64_t> nnzs = {0, 1, n_bags - 1, n_bags, n_bags + 1, 2 * n_bags - 1, 2 * n_bags};
        if (n_bags < (int64_t)1 << 56) {
          for (int64_t m : {3, 9, 16, 17, 32, 33, 40}) nnzs.push_back(m * n_bags);
          nnzs.push_back(5 * n_bags + 3);
          nnzs.push_back(33 * n_bags - 1);
        }
        nnzs.push_back(INT64_MAX);
        for (int64_t nnz : nnzs) {
          if (nnz < 0) continue;
          for (int form = 0; form < 2 * 2 * 2 * 2; ++form) {
            Q8FwdCall c;
            c.n_feats = n_feats; c.batch = batch; c.dim = dim; c.nnz = nnz;
            c.out_dtype = form & 1 ? KRS_BF16 : KRS_F32;
            c.has_offsets = (form >> 1) & 1; c.has_weights = (form >> 2) & 1;
            c.out_addr = base + ((form >> 3) & 1 ? 2 : 0);
            c.out_ld = (form >> 3) & 1 ? INT64_MAX : (int64_t)n_feats * dim;
            check(c);
          }
        }
      }
  // what the entry refuses as invalid, with no record
  {
    Q8FwdCall ok;
    ok.n_feats = 2; ok.batch = 100; ok.dim = 128; ok.nnz = 600; ok.out_addr = base; ok.out_ld = 256;
    std::vector<Q8FwdCall> bad(7, ok);
    bad[0].out_addr = 0; bad[1].n_feats = -1; bad[2].batch = -1; bad[3].dim = 0; bad[4].nnz = -1; bad[5].out_dtype = KRS_I8;
    bad[6].out_dtype = -1;
    for (const Q8FwdCall& c : bad) {
      const Q8FwdPlan p = plan_q8_fwd(c);
      ++g_plans;
      CHECK(p.status == KRS_ERR_INVALID && p.route.kernel == KRS_EMBED_FWD_NONE && p.route.blocks == 0 && p.route.lpr == 0 &&
            p.route.table_dtype == 0, "an invalid call is not refused");
    }
  }
  // the quantizer's launch shape
  for (int dim : dims)
    for (int64_t vocab : {(int64_t)0, (int64_t)1, (int64_t)3, (int64_t)4, (int64_t)5, (int64_t)67, (int64_t)255, (int64_t)256,
                          (int64_t)257, (int64_t)1 << 20, (int64_t)INT_MAX - 1, (int64_t)INT_MAX, (int64_t)INT_MAX + 1, INT64_MAX})
      for (int form = 0; form < 8; ++form)
        check_quantize(vocab, dim, form & 1 ? KRS_BF16 : KRS_F32, base + (form & 2 ? 4 : 0), base + 0x1000000 + (form & 4 ? 1 : 0),
                       base + 0x2000000);
  {
    long bad = 0;
    bad += plan_quantize(-1, 8, KRS_F32, base, base, base).status != KRS_ERR_INVALID;
    bad += plan_quantize(4, 0, KRS_F32, base, base, base).status != KRS_ERR_INVALID;
    bad += plan_quantize(4, 8, KRS_I8, base, base, base).status != KRS_ERR_INVALID;
    bad += plan_quantize(4, 8, KRS_F32, 0, base, base).status != KRS_ERR_INVALID;
    bad += plan_quantize(4, 8, KRS_F32, base, 0, base).status != KRS_ERR_INVALID;
    bad += plan_quantize(4, 8, KRS_F32, base, base, 0).status != KRS_ERR_INVALID;
    if (bad) { std::printf("%ld invalid quantize calls were not refused\n", bad); g_failed["invalid quantize call"] += bad; }
    g_plans += 6;
  }
  long total = 0;
  for (int kern : {(int)KRS_EMBED_FWD_VEC, (int)KRS_EMBED_FWD_GENERIC})
    if (!g_kernel[kern]) { std::printf("the grid never reached kernel %d\n", kern); ++total; }
  if (g_kernel[KRS_EMBED_FWD_HOT1] || g_kernel[KRS_EMBED_FWD_HOT1_ROWS]) { std::printf("a gather kernel was planned: there is none\n"); ++total; }
  if (!g_refused_batch) { std::printf("the grid never reached the batch refusal\n"); ++total; }
  if (!g_refused_grid) { std::printf("the grid never reached the grid refusal\n"); ++total; }
  if (!g_qvec || !g_qscalar || !g_qlong) { std::printf("the grid never reached one of the quantizer's three forms\n"); ++total; }
  for (const auto& f : g_failed) { std::printf("%ld x %s\n", f.second, f.first.c_str()); total += f.second; }
  std::printf("%ld plans, %ld failed checks\n", g_plans, total);
  return total ? 1 : 0;
}
