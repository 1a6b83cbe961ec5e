// Walks a lattice of krs_dot_interaction_fwd / _bwd_accumulate calls through the planner (keras_rs_amd/csrc/dot_plan.h,
// the only project header this program includes -- it compiles without HIP) and checks what every plan promises the
// kernel it names: the gradient columns a lane loads, the LDS request against the kernel's own layout and the launch
// limit, the sample packing, the grids, the 32-bit offsets, and the tiling of the block launches.
// Stand-alone: tests/test_dot_interaction_routes_host.py builds it with the host compiler and
// -fsanitize=address,undefined (a signed overflow anywhere in the planner stops it) and runs it as a child process.
// Exit 0 = every invariant held; otherwise the first offending calls of each invariant are printed and the exit status is 1.
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../keras_rs_amd/csrc/dot_plan.h"

using namespace krs::dplan;

static std::map<std::string, long> g_failed;
static long g_plans = 0, g_kernel[8] = {}, g_multi_spw1 = 0, g_capped = 0;

static void report(const char* what, const DotCall& c, const DotPlan& p) {
  if (++g_failed[what] > 3) return;
  const krs_dot_route& rt = p.route;
  std::printf("FAILED %s: %s F=%d B=%lld D=%d dtype=%d self=%d skip=%d mask=%llx feat0=%llx ld0=%lld force_valu=%d -> status=%d "
              "kernel=%d ks=%d fr=%d self=%d multi=%d acc=%d ng=%d lps_log2=%d spw=%d launches=%d lds_bytes=%d blocks=%lld\n",
              what, c.backward ? "bwd" : "fwd", c.n_feats, (long long)c.batch, c.dim, c.dtype, (int)c.self_interaction,
              (int)c.skip_gather, (unsigned long long)c.accumulate_mask, (unsigned long long)(uintptr_t)c.feats[0],
              (long long)c.ld[0], (int)c.force_valu, p.status, rt.kernel, rt.ks, rt.fr, rt.self, rt.multi, rt.acc, rt.ng,
              rt.lps_log2, rt.spw, rt.launches, rt.lds_bytes, (long long)rt.blocks);
}

#define CHECK(cond, what) do { if (!(cond)) report(what, c, p); } while (0)

static bool is_none(const krs_dot_route& rt) {
  const krs_dot_route none = {};
  return std::memcmp(&rt, &none, sizeof rt) == 0;
}

static void check(const DotCall& c) {
  const DotPlan p = plan_dot(c);
  ++g_plans;
  const krs_dot_route& rt = p.route;
  if (p.status != KRS_OK || c.batch == 0) {
    CHECK(is_none(rt) && p.launches.empty() && p.grid == 0, "a call that launches nothing has a route record");
    CHECK(p.status == KRS_OK, "a valid call is refused");
    return;
  }
  const int F = c.n_feats, D = c.dim, es = c.dtype == KRS_BF16 ? 2 : 4;
  const bool self = c.self_interaction, skip = c.skip_gather;
  const int64_t ncols = skip ? (int64_t)F * F : (self ? (int64_t)F * (F + 1) / 2 : (int64_t)F * (F - 1) / 2);
  const uint64_t mask = F < 64 ? c.accumulate_mask & (((uint64_t)1 << F) - 1) : c.accumulate_mask;
  CHECK(rt.kernel >= KRS_DOT_FWD_MFMA && rt.kernel <= KRS_DOT_BWD_BLOCK, "no kernel for a call that has work");
  if (rt.kernel < 0 || rt.kernel > 7) return;
  ++g_kernel[rt.kernel];
  CHECK((rt.kernel >= KRS_DOT_BWD_MFMA) == c.backward, "direction");
  CHECK(rt.dtype == c.dtype, "dtype");
  CHECK(p.acc_mask == (c.backward ? mask : 0), "accumulate_mask is trimmed to the features");
  CHECK(rt.lds_bytes == p.lds_bytes && p.lds_bytes >= 0, "the record's lds_bytes is the launch's");
  CHECK(p.lds_bytes <= 160 * 1024, "more LDS than a CU has");
  CHECK(p.lds_bytes <= 65536 || p.lds_opt_in, "more than 64 KiB of dynamic LDS without opting in");
  const bool block_kernel = rt.kernel == KRS_DOT_FWD_BLOCK || rt.kernel == KRS_DOT_BWD_BLOCK;
  CHECK(block_kernel ? rt.fr == 0 : rt.fr >= F, "fr >= n_feats");
  CHECK(block_kernel == (F > 64), "the block kernels run exactly the calls of more than 64 features");
  if (!block_kernel) {
    CHECK(rt.launches == 1 && p.launches.empty(), "one launch");
    CHECK(p.grid >= 1 && rt.blocks == p.grid, "the record's blocks is the grid");
  }
  const bool fast_bwd = rt.kernel == KRS_DOT_BWD_MFMA || rt.kernel == KRS_DOT_BWD_VALU;
  if (!fast_bwd) CHECK(!rt.self && !rt.multi && !rt.acc && !rt.ng && !rt.lps_log2 && !rt.spw && !rt.lds_bytes, "backward-build fields set");
  if (rt.kernel != KRS_DOT_FWD_MFMA) CHECK(rt.ks == 0, "ks off the forward MFMA kernel");

  switch (rt.kernel) {
    case KRS_DOT_FWD_MFMA: {
      const int ve = 16 / es;
      CHECK(rt.fr == 32 && p.block == 256, "forward MFMA: 32 rows, four waves");
      CHECK(rt.ks == 0 || rt.ks * 32 == D * es, "KS * 32 == dim * es");
      CHECK(rt.ks == (es == 2 && D == 128 ? 8 : (es == 2 && D == 64 ? 4 : 0)), "KS is 8 at bf16 dim 128, 4 at bf16 dim 64");
      CHECK(D % ve == 0, "forward MFMA: rows are whole 16-byte pieces");
      for (int f = 0; f < F; ++f)
        CHECK((uintptr_t)c.feats[f] % 16 == 0 && c.ld[f] % ve == 0, "forward MFMA: 16-byte aligned rows");
      CHECK(p.grid <= 2048 && (p.grid == 2048 || (int64_t)p.grid * 4 >= c.batch) && ((int64_t)p.grid - 1) * 4 < c.batch,
            "forward MFMA: grid");
      break;
    }
    case KRS_DOT_BWD_MFMA: {
      CHECK(es == 2 && D % 32 == 0 && D <= 128 && !c.force_valu, "MFMA backward off its shapes");
      CHECK(rt.fr == 32 && p.block == 128 && rt.self == (int)self && rt.acc == (int)(mask != 0), "MFMA backward: build");
      CHECK((rt.ng == 9 || rt.ng == 16) && (int64_t)rt.ng * 64 >= ncols && ncols > 0, "MFMA backward: ng * 64 >= ncols");
      CHECK(p.x_bytes >= 32 * D * 2 && p.x_bytes % 8192 == 0, "MFMA backward: the X image holds 32 rows");
      CHECK(p.lds_bytes == 1024 + 2 * ((int64_t)p.x_bytes + 2048 + 32 * 36 * 4), "MFMA backward: LDS layout");
      for (int f = 0; f < F; ++f) {
        CHECK((uintptr_t)c.feats[f] % 16 == 0 && (uintptr_t)c.grad_feats[f] % 16 == 0 && c.ld[f] % 8 == 0 && c.grad_feat_ld[f] % 8 == 0,
              "MFMA backward: 16-byte aligned rows");
        CHECK(c.ld[f] > 0 && c.grad_feat_ld[f] > 0 && c.ld[f] * 2 < ((int64_t)1 << 32) && c.grad_feat_ld[f] * 2 < ((int64_t)1 << 32),
              "MFMA backward: row strides in bytes fit 32 bits");
      }
      CHECK(p.grid <= 2048 && (p.grid == 2048 || (int64_t)p.grid * 2 >= c.batch) && ((int64_t)p.grid - 1) * 2 < c.batch,
            "MFMA backward: grid");
      break;
    }
    case KRS_DOT_BWD_VALU: {
      const int tri = self ? rt.fr * (rt.fr + 1) / 2 : rt.fr * (rt.fr - 1) / 2;
      CHECK(D % 2 == 0 && ncols > 0, "vector-ALU backward off its shapes");
      CHECK((rt.fr == 28 || rt.fr == 32) && (!rt.multi || rt.fr == 32) && (rt.fr == 32 || (F <= 28 && !skip)), "vector-ALU backward: FR");
      CHECK(rt.self == (int)self && rt.acc == (int)(mask != 0) && p.block == 64, "vector-ALU backward: build");
      CHECK(rt.ng == (rt.multi ? 16 : (tri + 63) / 64), "vector-ALU backward: ng is the build's NG");
      CHECK(rt.spw >= 1 && (rt.multi || rt.spw == 1), "vector-ALU backward: one sample per wave off the MULTI build");
      CHECK((int64_t)rt.ng * 64 >= (int64_t)rt.spw * ncols, "vector-ALU backward: ng * 64 >= spw * ncols");
      CHECK(rt.lps_log2 >= 0 && rt.lps_log2 <= 6 && rt.spw * (1 << rt.lps_log2) <= 64, "vector-ALU backward: spw * lps <= 64");
      CHECK((2 << rt.lps_log2) >= (D < 128 ? D : 128), "vector-ALU backward: 2 * lps covers min(dim, 128)");
      CHECK(p.lds_bytes == 1024 + (int64_t)2 * rt.spw * (tri + 1) * 4, "vector-ALU backward: LDS layout");
      CHECK(p.spw == rt.spw && p.lps_log2 == rt.lps_log2, "vector-ALU backward: launch arguments");
      for (int f = 0; f < F; ++f) {
        CHECK((uintptr_t)c.feats[f] % (2 * es) == 0 && (uintptr_t)c.grad_feats[f] % (2 * es) == 0 && c.ld[f] % 2 == 0 &&
              c.grad_feat_ld[f] % 2 == 0, "vector-ALU backward: rows aligned to a pair of columns");
        const __int128 a = ((__int128)c.batch * c.ld[f] + D) * es, g = ((__int128)c.batch * c.grad_feat_ld[f] + D) * es;
        CHECK(c.ld[f] > 0 && c.grad_feat_ld[f] > 0 && a < ((__int128)1 << 31) && g < ((__int128)1 << 31),
              "vector-ALU backward: byte offsets fit 31 bits");
      }
      CHECK(p.grid <= 16384 && (p.grid == 16384 || (int64_t)p.grid * rt.spw >= c.batch) && ((int64_t)p.grid - 1) * rt.spw < c.batch,
            "vector-ALU backward: grid");
      if (rt.multi && rt.spw == 1) ++g_multi_spw1;
      if (rt.spw < (64 >> rt.lps_log2) && (int64_t)(rt.spw + 1) * ncols <= 1024) ++g_capped;
      break;
    }
    case KRS_DOT_FWD_GENERIC:
    case KRS_DOT_BWD_GENERIC: {
      CHECK(rt.fr == 64 && p.block == 256, "generic: 64 pointer slots, 256 threads");
      const __int128 work = (__int128)c.batch * F * (c.backward ? D : F);
      CHECK(p.grid <= 65536 && (p.grid == 65536 || (__int128)p.grid * 256 >= work) && ((__int128)p.grid - 1) * 256 < work, "generic: grid");
      break;
    }
    default: {   // block kernels
      CHECK(rt.launches == (int)p.launches.size() && rt.launches >= 1 && p.block == 256, "block: launches");
      std::vector<int> seen((size_t)F * F, 0);
      int64_t blocks = 0;
      int row = -1, next_j = 0;
      for (const DotLaunch& l : p.launches) {
        CHECK(l.ni >= 1 && l.ni <= 32 && l.nj >= 1 && l.nj <= 128 && l.i0 >= 0 && l.j0 >= 0 && l.i0 + l.ni <= F && l.j0 + l.nj <= F,
              "block: a launch outside the features or its pointer tables");
        if (l.i0 != row) { CHECK(l.i0 > row && l.i0 % 32 == 0, "block: rows of launches ascend"); row = l.i0; next_j = 0; }
        CHECK(l.j0 == next_j && l.first_j == (int)(l.j0 == 0), "block: chunks ascend from 0, first_j exactly on the first");
        next_j = l.j0 + l.nj;
        const __int128 work = (__int128)c.batch * l.ni * (c.backward ? D : l.nj);
        CHECK(l.blocks >= 1 && l.blocks <= 65536 && (l.blocks == 65536 || (__int128)l.blocks * 256 >= work), "block: grid");
        blocks += l.blocks;
        if (l.i0 + l.ni <= F && l.j0 + l.nj <= F && l.i0 >= 0 && l.j0 >= 0)
          for (int i = l.i0; i < l.i0 + l.ni; ++i)
            for (int j = l.j0; j < l.j0 + l.nj; ++j) ++seen[(size_t)i * F + j];
      }
      CHECK(blocks == rt.blocks, "block: the record's blocks is the sum of the grids");
      bool once = true;
      for (int i = 0; i < F && once; ++i)
        for (int j = 0; j < F && once; ++j) {
          const bool needed = c.backward || skip || j <= i;   // the forward gather writes the lower triangle only
          once = needed ? seen[(size_t)i * F + j] == 1 : seen[(size_t)i * F + j] <= 1;
        }
      CHECK(once, "block: the launches tile every (i, j) pair exactly once");
    }
  }
}

int main() {
  std::vector<int> dims;
  for (int d = 2; d <= 300; d += 2) dims.push_back(d);
  for (int d : {1, 3, 5, 7, 9, 31, 33, 63, 127, 129, 255, 299}) dims.push_back(d);
  const int64_t batches[] = {0, 1, 5, 100000};
  const uint64_t masks[] = {0, 0xaaaaaaaaaaaaaaaaull, 1ull << 63};
  const uint64_t base = 0x7f0000100000ull, gbase = 0x7e0000100000ull;
  std::vector<const void*> feats(140);
  std::vector<void*> gfeats(140);
  std::vector<int64_t> ld(140), gld(140);
  long variant = 0;
  for (int F = 1; F <= 140; ++F)
    for (int D : dims)
      for (int dtype : {KRS_F32, KRS_BF16})
        // 0: views of one concat buffer; 1: separate tensors, padded rows; 2: base 4 bytes off; 3: odd row stride;
        // 4: base 8 bytes off; 5: rows 2^30 elements apart; 6: 2^31 - 8; 7: 2^31
        for (int layout = 0; layout < 8; ++layout) {
          // past the fast kernels only the tiling and the grids are left to decide: a few dims and layouts there; the
          // far-apart rows at the dims where the kernel changes with them
          const bool key_dim = D == 2 || D == 3 || D == 32 || D == 128 || D == 130 || D == 300;
          if ((F > 34 && !(key_dim && (layout == 0 || layout == 3))) || (layout >= 4 && !key_dim)) continue;
          const int es = dtype == KRS_BF16 ? 2 : 4;
          const int64_t wide = ((int64_t)F * D + 7) / 8 * 8;
          for (int f = 0; f < F; ++f) {
            const uint64_t off = layout == 0 ? (uint64_t)f * D * es : (uint64_t)f * (1ull << 36);
            const uint64_t shift = layout == 2 ? 4 : (layout == 4 ? 8 : 0);
            feats[f] = reinterpret_cast<const void*>(base + off + shift);
            gfeats[f] = reinterpret_cast<void*>(gbase + off + shift);
            ld[f] = layout == 0 ? wide : (layout == 3 ? (D | 1) + 2
                                  : (layout == 5 ? (int64_t)1 << 30 : (layout == 6 ? ((int64_t)1 << 31) - 8
                                  : (layout == 7 ? (int64_t)1 << 31 : (D + 15) / 8 * 8))));
            gld[f] = ld[f];
          }
          for (int mode = 0; mode < 4; ++mode)
            for (int64_t batch : batches) {
              DotCall c;
              c.n_feats = F; c.batch = batch; c.dim = D; c.dtype = dtype;
              c.self_interaction = mode & 1; c.skip_gather = (mode & 2) != 0;
              c.feats = feats.data(); c.ld = ld.data(); c.out_addr = 0x7d0000100000ull;
              c.out_ld = (int64_t)F * F + 3;
              check(c);
              c.backward = true; c.grad_feats = gfeats.data(); c.grad_feat_ld = gld.data();
              // every mask without the switch; the switch with two of them, taking turns
              for (uint64_t m : masks) { c.accumulate_mask = m; c.force_valu = false; check(c); }
              c.force_valu = true;
              c.accumulate_mask = masks[variant++ % 3];
              check(c);
            }
        }
  // what the entries refuse as invalid, with no record
  {
    const void* f2[2] = {reinterpret_cast<const void*>(base), reinterpret_cast<const void*>(base + 4096)};
    void* g2[2] = {reinterpret_cast<void*>(gbase), reinterpret_cast<void*>(gbase + 4096)};
    const int64_t l2[2] = {128, 128};
    DotCall ok;
    ok.backward = true; ok.n_feats = 2; ok.batch = 100; ok.dim = 128; ok.dtype = KRS_BF16; ok.feats = f2; ok.ld = l2;
    ok.grad_feats = g2; ok.grad_feat_ld = l2; ok.out_addr = 0x7d0000100000ull; ok.out_ld = 1;
    std::vector<DotCall> bad(9, ok);
    const void* fnull[2] = {f2[0], nullptr};
    void* gnull[2] = {nullptr, g2[1]};
    bad[0].feats = nullptr; bad[1].ld = nullptr; bad[2].out_addr = 0; bad[3].n_feats = 0; bad[4].batch = -1; bad[5].dim = 0;
    bad[6].dtype = KRS_I8; bad[7].feats = fnull; bad[8].grad_feats = gnull;
    bad.push_back(ok); bad.back().grad_feats = nullptr;
    bad.push_back(ok); bad.back().grad_feat_ld = nullptr;
    for (const DotCall& c : bad) {
      const DotPlan p = plan_dot(c);
      ++g_plans;
      if (!(p.status == KRS_ERR_INVALID && is_none(p.route) && p.why[0] != 0)) {
        std::printf("FAILED an invalid call is not refused: status=%d kernel=%d\n", p.status, p.route.kernel);
        ++g_failed["an invalid call is not refused"];
      }
    }
    const DotPlan p = plan_dot(ok);
    if (p.status != KRS_OK || p.route.kernel != KRS_DOT_BWD_MFMA) ++g_failed["the valid call beside the invalid ones"];
  }
  long total = 0;
  for (int kern = 1; kern <= 7; ++kern)
    if (!g_kernel[kern]) { std::printf("the lattice never reached kernel %d\n", kern); ++total; }
  if (!g_multi_spw1) { std::printf("the lattice never reached the MULTI build with one sample per wave\n"); ++total; }
  if (!g_capped) { std::printf("the lattice never reached a sample count capped by the LDS request\n"); ++total; }
  for (const auto& f : g_failed) { std::printf("%ld x %s\n", f.second, f.first.c_str()); total += f.second; }
  std::printf("%ld plans, %ld failed checks\n", g_plans, total);
  return total ? 1 : 0;
}
