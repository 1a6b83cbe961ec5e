// Walks krs::seqattn::plan (keras_rs_amd/csrc/seq_attn_plan.h, the only project header this program includes) over a grid
// of (b, h, l, dh, dtype, aligned) and checks what every plan promises the K19 kernels that read it.  Stand-alone:
// tests/test_seq_attention_host.py builds it with the host compiler and -fsanitize=address,undefined and runs it as a
// child process.  After the walk it prints one line "status kernel dpad vec oblocks groups" per "b h l dh dtype aligned"
// tuple of its command line (six numbers each), then, for "hash seed draw bh i j" tuples, the dropout hash, then the
// tally.  Exit 0 = every invariant held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../keras_rs_amd/csrc/seq_attn_plan.h"

using namespace krs::seqattn;

static std::map<std::string, long> g_failed;
static long g_plans = 0;
static std::map<int, long> g_routes;

#define CHECK(cond, what)                                                                                          \
  do {                                                                                                             \
    if (!(cond) && ++g_failed[what] <= 3)                                                                          \
      std::printf("FAILED %s: b=%lld h=%lld l=%lld dh=%lld dtype=%d aligned=%d\n", what, (long long)b, (long long)h, \
                  (long long)l, (long long)dh, dtype, (int)aligned);                                               \
  } while (0)

static void check(int64_t b, int64_t h, int64_t l, int64_t dh, int dtype, bool aligned) {
  const Plan pl = plan(b, h, l, dh, dtype, aligned);
  ++g_plans;
  const bool bad_shape = b < 0 || h < 1 || l < 0 || dh < 1 || (dtype != kF32 && dtype != kBF16);
  CHECK((pl.status == kInvalid) == bad_shape, "invalid exactly for a bad shape or dtype");
  if (pl.status != kOk) {
    CHECK(pl.kernel == kRouteNone && pl.groups == 0, "a refused call has no route");
    CHECK(pl.why && std::strlen(pl.why) > 0, "a refusal names its limit");
    if (pl.status == kUnsupported)
      CHECK(l > kMaxL || dh > kMaxDh || b > kMaxGroups || h > kMaxGroups || b * h > kMaxGroups || b * h * l > kMaxGroups,
            "unsupported only beyond a limit");
    return;
  }
  CHECK(l <= kMaxL && dh <= kMaxDh, "an accepted call is within the limits");
  if (b == 0 || l == 0) {
    CHECK(pl.kernel == kRouteNone && pl.groups == 0, "an empty call launches nothing");
    return;
  }
  ++g_routes[pl.kernel * 1000 + pl.dpad * 2 + pl.vec];
  CHECK(pl.groups >= 1 && pl.groups <= kMaxGroups, "grid within the launch limit");
  if (pl.kernel == kRouteFast) {
    CHECK(dtype == kBF16 && dh <= kFastMaxDh, "the fast route is bf16 at dh <= 128");
    CHECK((pl.dpad == 32 || pl.dpad == 64 || pl.dpad == 128) && pl.dpad >= dh && (pl.dpad == 32 || pl.dpad / 2 < dh),
          "dpad is the smallest of 32, 64, 128 that holds dh");
    CHECK(pl.vec == (aligned && dh % 8 == 0), "whole-chunk loads only on whole aligned chunks");
    CHECK(pl.oblocks * kOwnRows >= l && (pl.oblocks - 1) * kOwnRows < l, "owner blocks cover l exactly");
    CHECK(pl.groups == pl.oblocks * b * h, "one workgroup per owner block and (b, h)");
  } else {
    CHECK(pl.kernel == kRouteGeneric && pl.dpad == 0 && pl.vec == 0, "the generic route has no dpad");
    CHECK(dtype == kF32 || dh > kFastMaxDh, "bf16 at dh <= 128 never takes the generic route");
    CHECK(pl.groups == b * h * l, "one workgroup per (b, h, row)");
  }
  CHECK(workspace_bytes(b, h, l) >= (size_t)(b * h * l) * 4 && workspace_bytes(b, h, l) % 256 == 0, "workspace holds delta");
}

int main(int argc, char** argv) {
  const std::vector<int64_t> bs = {-1, 0, 1, 3, 4096, 65536, (int64_t)1 << 21, (int64_t)1 << 31, (int64_t)1 << 40};
  const std::vector<int64_t> hs = {0, 1, 2, 3, 16, (int64_t)1 << 20, (int64_t)1 << 32};
  const std::vector<int64_t> ls = {-1, 0, 1, 31, 32, 33, 127, 128, 129, 200, 1024, 4095, 4096, 4097, (int64_t)1 << 33};
  const std::vector<int64_t> dhs = {0, 1, 8, 31, 32, 33, 50, 64, 65, 127, 128, 129, 160, 255, 256, 257, (int64_t)1 << 33};
  for (int64_t b : bs)
    for (int64_t h : hs)
      for (int64_t l : ls)
        for (int64_t dh : dhs)
          for (int dtype : {0, 1, 2, -1})
            for (int aligned = 0; aligned < 2; ++aligned) check(b, h, l, dh, dtype, aligned != 0);
  int i = 1;
  while (i < argc) {
    if (std::strcmp(argv[i], "hash") == 0 && i + 5 < argc) {
      const uint64_t seed = std::strtoull(argv[i + 1], nullptr, 10), draw = std::strtoull(argv[i + 2], nullptr, 10);
      const uint32_t base = hash_base((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)draw, (uint32_t)(draw >> 32),
                                      (uint32_t)std::strtoull(argv[i + 3], nullptr, 10));
      std::printf("%u\n", hash_ij(base, (uint32_t)std::atoll(argv[i + 4]), (uint32_t)std::atoll(argv[i + 5])));
      i += 6;
    } else if (i + 5 < argc) {
      const Plan pl = plan(std::atoll(argv[i]), std::atoll(argv[i + 1]), std::atoll(argv[i + 2]), std::atoll(argv[i + 3]),
                           std::atoi(argv[i + 4]), std::atoi(argv[i + 5]) != 0);
      std::printf("%d %d %d %d %lld %lld\n", pl.status, pl.kernel, pl.dpad, pl.vec, (long long)pl.oblocks,
                  (long long)pl.groups);
      i += 6;
    } else {
      std::printf("usage: seq_attn_plan_check [b h l dh dtype aligned | hash seed draw bh i j]...\n");
      return 2;
    }
  }
  long total = 0;
  if (g_routes.size() != 7) { std::printf("the grid reached %zu of the 7 (route, dpad, vec) builds\n", g_routes.size()); ++total; }
  if (drop_threshold(0.0f) != 0u || drop_threshold(0.5f) != 0x80000000u) { std::printf("drop_threshold\n"); ++total; }
  for (const auto& f : g_failed) { std::printf("%ld x %s\n", f.second, f.first.c_str()); total += f.second; }
  std::printf("%ld plans, %ld failed checks\n", g_plans, total);
  return total ? 1 : 0;
}
