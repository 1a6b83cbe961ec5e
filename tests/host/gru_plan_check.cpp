// Walks krs::gru::plan (keras_rs_amd/csrc/gru_plan.h, the only project header this program includes) over a grid of
// (b, l, u, dtype) and checks what every plan promises the K20 kernels that read it.  Stand-alone:
// tests/test_gru_host.py builds it with the host compiler and -fsanitize=address,undefined and runs it as a child
// process.  After the walk it prints one line "status kernel upad rows threads groups lds_fwd lds_bwd" per
// "b l u dtype" tuple of its command line (four numbers each), then the tally.  Exit 0 = every invariant held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../keras_rs_amd/csrc/gru_plan.h"

using namespace krs::gru;

static std::map<std::string, long> g_failed;
static long g_plans = 0;
static std::map<int, long> g_routes;

#define CHECK(cond, what)                                                                                         \
  do {                                                                                                            \
    if (!(cond) && ++g_failed[what] <= 3)                                                                         \
      std::printf("FAILED %s: b=%lld l=%lld u=%lld dtype=%d\n", what, (long long)b, (long long)l, (long long)u,    \
                  dtype);                                                                                         \
  } while (0)

static void check(int64_t b, int64_t l, int64_t u, int dtype) {
  const Plan pl = plan(b, l, u, dtype);
  ++g_plans;
  const bool bad_shape = b < 0 || l < 0 || u < 1 || (dtype != kF32 && dtype != kBF16);
  CHECK((pl.status == kInvalid) == bad_shape, "invalid exactly for a bad shape or dtype");
  if (pl.status != kOk) {
    CHECK(pl.kernel == kRouteNone && pl.groups == 0, "a refused call has no route");
    CHECK(pl.why && std::strlen(pl.why) > 0, "a refusal names its limit");
    if (pl.status == kUnsupported)
      CHECK(u > kMaxU || l > kMaxGroups || cdiv(b, kGenRows) > kMaxGroups, "unsupported only beyond a limit");
    return;
  }
  CHECK(u <= kMaxU, "an accepted call is within the limits");
  if (b == 0 || l == 0) {
    CHECK(pl.kernel == kRouteNone && pl.groups == 0, "an empty call launches nothing");
    return;
  }
  ++g_routes[pl.kernel * 1000 + pl.upad];
  CHECK(pl.groups >= 1 && pl.groups <= kMaxGroups, "grid within the launch limit");
  CHECK(pl.rows >= 1 && pl.rows * pl.groups >= b && pl.rows * (pl.groups - 1) < b, "rows x workgroups cover b exactly");
  CHECK(pl.lds_fwd > 0 && pl.lds_fwd <= kLdsLimit && pl.lds_bwd > 0 && pl.lds_bwd <= kLdsLimit, "LDS within 160 KiB");
  CHECK(pl.threads >= 64 && pl.threads <= 256 && pl.threads % 64 == 0, "whole waves, 256 threads at most");
  if (pl.kernel == kRouteFast) {
    CHECK(dtype == kBF16 && u <= kFastMaxU, "the fast route is bf16 at u <= 128");
    CHECK((pl.upad == 32 || pl.upad == 64 || pl.upad == 128) && pl.upad >= u && (pl.upad == 32 || pl.upad / 2 < u),
          "upad is the smallest of 32, 64, 128 that holds u");
    CHECK(pl.rows == kFastRows && pl.threads == 2 * pl.upad, "32 rows, one wave per 32 units");
    // the recurrent kernel, the double-buffered A tile (and the backward's first-valid table) all fit
    CHECK(pl.lds_fwd >= (int64_t)3 * pl.upad * pl.upad * 2 + (int64_t)2 * kFastRows * pl.upad * 2, "forward LDS holds U and h");
    CHECK(pl.lds_bwd >= (int64_t)3 * pl.upad * pl.upad * 2 + (int64_t)2 * kFastRows * 3 * pl.upad * 2 + kFastRows * 4,
          "backward LDS holds U, da and first");
    CHECK((pl.upad * 2 + kPadBytes) % 16 == 0 && (3 * pl.upad * 2 + kPadBytes) % 16 == 0, "LDS rows keep 16-byte alignment");
    CHECK(((pl.upad * 2 + kPadBytes) / 4) % 64 % 8 == 4 && ((3 * pl.upad * 2 + kPadBytes) / 4) % 64 % 8 == 4,
          "16 rows of 16-byte reads cover all 64 banks");
  } else {
    CHECK(pl.kernel == kRouteGeneric && pl.upad == 0, "the generic route has no upad");
    CHECK(dtype == kF32 || u > kFastMaxU, "bf16 at u <= 128 never takes the generic route");
    CHECK(pl.rows == kGenRows && pl.threads == kGenThreads, "4 rows, 256 threads");
    CHECK(pl.lds_fwd >= 2 * kGenRows * u * 4 && pl.lds_bwd >= 4 * kGenRows * u * 4 + kGenRows * 4,
          "generic LDS holds the state, dh and da");
  }
  if (b <= 65536 && l <= 65536)
    CHECK(reserve_bytes(b, l, u, dtype) == (size_t)(b * l * 4 * u) * (dtype == kBF16 ? 2 : 4), "the reserve is [b, l, 4u]");
}

int main(int argc, char** argv) {
  const std::vector<int64_t> bs = {-1, 0, 1, 3, 31, 32, 33, 65, 4096, (int64_t)1 << 21, (int64_t)1 << 33, (int64_t)1 << 40};
  const std::vector<int64_t> ls = {-1, 0, 1, 2, 7, 33, 200, 4096, (int64_t)1 << 31, (int64_t)1 << 33};
  const std::vector<int64_t> us = {0, 1, 8, 31, 32, 33, 50, 64, 65, 127, 128, 129, 160, 200, 256, 1023, 1024, 1025,
                                   (int64_t)1 << 33};
  for (int64_t b : bs)
    for (int64_t l : ls)
      for (int64_t u : us)
        for (int dtype : {0, 1, 2, -1}) check(b, l, u, dtype);
  int i = 1;
  while (i < argc) {
    if (i + 3 < argc) {
      const Plan pl = plan(std::atoll(argv[i]), std::atoll(argv[i + 1]), std::atoll(argv[i + 2]), std::atoi(argv[i + 3]));
      std::printf("%d %d %d %d %d %lld %lld %lld\n", pl.status, pl.kernel, pl.upad, pl.rows, pl.threads,
                  (long long)pl.groups, (long long)pl.lds_fwd, (long long)pl.lds_bwd);
      i += 4;
    } else {
      std::printf("usage: gru_plan_check [b l u dtype]...\n");
      return 2;
    }
  }
  long total = 0;
  if (g_routes.size() != 4) { std::printf("the grid reached %zu of the 4 (route, upad) builds\n", g_routes.size()); ++total; }
  if (reserve_bytes(0, 5, 8, kBF16) != 0 || reserve_bytes(2, 0, 8, kF32) != 0) { std::printf("reserve_bytes of nothing\n"); ++total; }
  for (const auto& f : g_failed) { std::printf("%ld x %s\n", f.second, f.first.c_str()); total += f.second; }
  std::printf("%ld plans, %ld failed checks\n", g_plans, total);
  return total ? 1 : 0;
}
