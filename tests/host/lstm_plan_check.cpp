// Prints krs::lstm::plan (keras_rs_amd/csrc/lstm_plan.h, the only project header this program includes) for every
// "b l u dtype" tuple of its command line, one line each:
//   status kernel upad rows threads groups lds_fwd lds_bwd bwd_kernel_vgprs reserve_bytes why
// Stand-alone: tests/test_lstm_host.py builds it with the host compiler and -fsanitize=address,undefined, runs it as a
// child process and checks the lines.
#include <cstdio>
#include <cstdlib>

#include "../../keras_rs_amd/csrc/lstm_plan.h"

int main(int argc, char** argv) {
  if ((argc - 1) % 4 != 0) {
    std::printf("usage: lstm_plan_check [b l u dtype]...\n");
    return 2;
  }
  for (int i = 1; i + 3 < argc; i += 4) {
    const int64_t b = std::atoll(argv[i]), l = std::atoll(argv[i + 1]), u = std::atoll(argv[i + 2]);
    const int dtype = std::atoi(argv[i + 3]);
    const krs::lstm::Plan pl = krs::lstm::plan(b, l, u, dtype);
    std::printf("%d %d %d %d %d %lld %lld %lld %d %zu %s\n", pl.status, pl.kernel, pl.upad, pl.rows, pl.threads,
                (long long)pl.groups, (long long)pl.lds_fwd, (long long)pl.lds_bwd, pl.bwd_kernel_vgprs,
                krs::lstm::reserve_bytes(b, l, u, dtype), pl.why);
  }
  return 0;
}
