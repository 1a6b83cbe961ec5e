// Walks plan_sweep (keras_rs_amd/csrc/retrieval_xent_plan.h, the only project header this program includes) over a grid
// of (b, n) and checks what every plan promises the K13 kernels that read it.  Stand-alone:
// tests/test_retrieval_xent_cases_host.py builds it with the host compiler and -fsanitize=address,undefined and runs it
// as a child process.  After the walk it prints one line "oblocks S slice" per "owner streamed b n" tuple of its command
// line (four numbers each), then the tally.  Exit 0 = every invariant held; otherwise the first offending plans of each
// invariant are printed and the exit status is 1.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "../../keras_rs_amd/csrc/retrieval_xent_plan.h"

using namespace krs::xent;

static std::map<std::string, long> g_failed;
static long g_plans = 0, g_sliced = 0;

static void report(const char* what, int64_t owner, int64_t streamed, int64_t b, int64_t n, const Sweep& sw) {
  if (++g_failed[what] > 3) return;
  std::printf("FAILED %s: owner=%lld streamed=%lld b=%lld n=%lld -> oblocks=%lld S=%d slice=%lld\n", what,
              (long long)owner, (long long)streamed, (long long)b, (long long)n, (long long)sw.oblocks, sw.S,
              (long long)sw.slice);
}

#define CHECK(cond, what) do { if (!(cond)) report(what, owner, streamed, b, n, sw); } while (0)

static void check_sweep(int64_t owner, int64_t streamed, int64_t b, int64_t n) {
  const Sweep sw = plan_sweep(owner, streamed, b, n);
  ++g_plans;
  if (sw.S > 1) ++g_sliced;
  CHECK(sw.oblocks == (owner + kOwnRows - 1) / kOwnRows, "owner blocks of kOwnRows rows");
  CHECK(sw.slice >= kTile && sw.slice % kTile == 0, "a slice is not whole tiles");
  CHECK(sw.S >= 1 && sw.S <= kMaxSlices, "slice count outside 1 .. kMaxSlices");
  CHECK((int64_t)sw.S * sw.slice >= streamed, "the slices do not cover the streamed side");
  CHECK((int64_t)(sw.S - 1) * sw.slice < streamed, "an empty slice");
  CHECK(sw.S == 1 || (int64_t)sw.S * owner <= 8 * (b + n), "partials beyond 8 (b + n) rows");
  CHECK(sw.oblocks * sw.S <= 0xffffffffll, "grid beyond the launch limit");
}

static void check_bytes(int64_t b, int64_t n, int64_t d) {
  const Sweep sw = plan_sweep(b, n, b, n), swc = plan_sweep(n, b, b, n);      // (report() prints the fwd/dq sweep)
  const int64_t owner = b, streamed = n;
  const size_t f = fwd_bytes(b, n), q = dq_bytes(b, n, d), c = dc_bytes(b, n, d), w = workspace_bytes(b, n, d);
  ++g_plans;
  CHECK((f > 0) == (sw.S > 1) && (q > 0) == (sw.S > 1) && (c > 0) == (swc.S > 1), "bytes exactly where a sweep is sliced");
  CHECK(f % 256 == 0 && q % 256 == 0 && c % 256 == 0, "a partial region off 256 bytes");
  CHECK(f >= (sw.S > 1 ? (size_t)sw.S * (size_t)b * 16 : 0), "forward partials beyond their bytes");
  CHECK(q >= (sw.S > 1 ? (size_t)sw.S * (size_t)b * (size_t)d * 4 : 0), "dq partials beyond their bytes");
  CHECK(c >= (swc.S > 1 ? (size_t)swc.S * (size_t)n * (size_t)d * 4 : 0), "dc partials beyond their bytes");
  CHECK(w >= f && w >= q + c && (w == f || w == q + c), "workspace_bytes is not the larger of forward and backward");
  CHECK(q + c <= (size_t)16 * (size_t)(b + n) * (size_t)d * 4 + 512, "gradient partials beyond 16 (b + n) d floats");
}

int main(int argc, char** argv) {
  std::vector<int64_t> sides = {1, 4096, 65535, 65536, (int64_t)1 << 20, (int64_t)1 << 24};
  for (int64_t v : {32, 64, 128})
    for (int64_t e = -1; e <= 1; ++e) sides.push_back(v + e);
  for (int64_t b : sides)
    for (int64_t n : sides) {
      check_sweep(b, n, b, n);      // forward and dq: the queries own
      check_sweep(n, b, b, n);      // dc: the candidates own
      for (int64_t d : {1, 5, 40, 256}) check_bytes(b, n, d);
    }
  if ((argc - 1) % 4 != 0) {
    std::printf("usage: xent_plan_check [owner streamed b n]...\n");
    return 2;
  }
  for (int i = 1; i + 3 < argc; i += 4) {
    const Sweep sw = plan_sweep(std::atoll(argv[i]), std::atoll(argv[i + 1]), std::atoll(argv[i + 2]), std::atoll(argv[i + 3]));
    std::printf("%lld %d %lld\n", (long long)sw.oblocks, sw.S, (long long)sw.slice);
  }
  long total = 0;
  if (!g_sliced) { std::printf("the grid never reached a sliced sweep\n"); ++total; }
  for (const auto& f : g_failed) { std::printf("%ld x %s\n", f.second, f.first.c_str()); total += f.second; }
  std::printf("%ld plans, %ld failed checks\n", g_plans, total);
  return total ? 1 : 0;
}
