// Walks krs::ssm::plan (csrc/sampled_softmax_plan.h) over a grid of shapes and checks what its header promises; with
// arguments, prints the plan of each call "t g n d emb_dtype table_dtype aligned" as
// "status kernel dpad vec grid_tokens grid_negs splits split_tiles launches workspace_bytes".
#include <cstdio>
#include <cstdlib>

#include "../../keras_rs_amd/csrc/sampled_softmax_plan.h"

static int failed = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      ++failed;                                                              \
      std::printf("line %d: %s (t %lld g %lld n %lld d %lld)\n", __LINE__, #cond, (long long)c.t, (long long)c.g, \
                  (long long)c.n, (long long)c.d);                           \
    }                                                                        \
  } while (0)

static krs::ssm::Call call_of(int64_t t, int64_t g, int64_t n, int64_t d, int edt, int tdt, bool aligned) {
  krs::ssm::Call c;
  void* at = reinterpret_cast<void*>(static_cast<uintptr_t>(aligned ? 1 << 20 : (1 << 20) + 4));
  c.emb = c.table = at;
  c.pos = c.neg = c.lse = c.gpos = c.demb = c.dneg = reinterpret_cast<void*>(static_cast<uintptr_t>(1 << 20));
  c.emb_dtype = edt, c.table_dtype = tdt, c.vocab = 1000;
  c.t = t, c.g = g, c.n = n, c.d = d, c.ld_emb = c.ld_table = c.ld_demb = d;
  return c;
}

static void check(const krs::ssm::Call& c) {
  using namespace krs::ssm;
  const Plan pl = plan(c);
  const krs_sampled_softmax_route& r = pl.route;
  CHECK(pl.status == KRS_OK);
  const int64_t lg = c.t / c.g, tiles = cdiv(lg, kTile);
  const bool fast = c.emb_dtype == KRS_BF16 && c.d <= 128;
  CHECK(r.kernel == (fast ? KRS_SAMPLED_SOFTMAX_FAST : KRS_SAMPLED_SOFTMAX_GENERIC));
  CHECK(pl.lg == lg && r.splits >= 1 && r.splits <= KRS_SAMPLED_SOFTMAX_MAX_SPLITS);
  CHECK((int64_t)r.splits * r.split_tiles >= tiles && (int64_t)(r.splits - 1) * r.split_tiles < tiles);
  if (fast) {
    CHECK(r.dpad >= c.d && (r.dpad == 32 || r.dpad == 64 || r.dpad == 128) && (r.dpad == 32 || r.dpad / 2 < c.d));
    CHECK(r.grid_tokens == c.g * cdiv(lg, kOwn) && r.grid_negs == c.g * cdiv(c.n, kOwn) * r.splits);
    CHECK(!r.vec || (c.d % 8 == 0 && on16(c.emb)));
  } else {
    CHECK(r.dpad == 0 && r.vec == 0 && r.splits == 1 && r.grid_tokens == c.t && r.grid_negs == c.g * c.n);
  }
  CHECK(pl.off_c >= KRS_SAMPLED_BCE_W_BLOCKS && pl.off_loss >= pl.off_c + (size_t)c.t);
  CHECK(pl.off_dneg >= pl.off_loss + (size_t)r.grid_tokens && pl.off_dneg % 64 == 0);
  CHECK(pl.floats == pl.off_dneg + (r.splits > 1 ? (size_t)r.splits * c.g * c.n * c.d : 0));
  CHECK(workspace_bytes(c.t, c.g, c.n, c.d, c.emb_dtype) == pl.floats * sizeof(float));
  CHECK(r.launches == 3 + (r.splits > 1));
}

int main(int argc, char** argv) {
  if (argc > 1) {
    if ((argc - 1) % 7 != 0) {
      std::printf("usage: sampled_softmax_plan_check [t g n d emb_dtype table_dtype aligned]...\n");
      return 2;
    }
    for (int i = 1; i < argc; i += 7) {
      const krs::ssm::Call c = call_of(std::atoll(argv[i]), std::atoll(argv[i + 1]), std::atoll(argv[i + 2]),
                                       std::atoll(argv[i + 3]), std::atoi(argv[i + 4]), std::atoi(argv[i + 5]),
                                       std::atoi(argv[i + 6]) != 0);
      const krs::ssm::Plan pl = krs::ssm::plan(c);
      const krs_sampled_softmax_route& r = pl.route;
      std::printf("%d %d %d %d %d %d %d %d %d %zu\n", pl.status, r.kernel, r.dpad, r.vec, r.grid_tokens, r.grid_negs,
                  r.splits, r.split_tiles, r.launches,
                  krs::ssm::workspace_bytes(c.t, c.g, c.n, c.d, c.emb_dtype));
    }
  } else {
    const int64_t gs[] = {1, 3, 8, 4096}, lgs[] = {1, 31, 32, 33, 128, 129, 1024, 4097};
    const int64_t ns[] = {1, 31, 128, 129, 4096}, ds[] = {1, 8, 32, 33, 50, 64, 65, 128, 129, 512};
    for (int64_t g : gs)
      for (int64_t lg : lgs)
        for (int64_t n : ns)
          for (int64_t d : ds)
            for (int dt = 0; dt < 4; ++dt)
              for (int al = 0; al < 2; ++al) check(call_of(g * lg, g, n, d, dt & 1, dt >> 1, al != 0));
    krs::ssm::Call c = call_of(2147483647, 1, 4096, 512, KRS_F32, KRS_F32, true);      // the largest call
    check(c);
    c = call_of(0, 1, 1, 1, KRS_F32, KRS_F32, true);
    CHECK(krs::ssm::plan(c).status == KRS_OK && krs::ssm::plan(c).route.kernel == 0);
  }
  std::printf("%d failed checks\n", failed);
  return failed ? 1 : 0;
}
