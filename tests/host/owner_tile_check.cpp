// Checks the index arithmetic of keras_rs_amd/csrc/krs_owner_tile.h (part A, the only project code this program sees:
// it is compiled without HIP) for DPAD = 32, 64, 128, 256 -- the contract that the K13 - K15 and K19 kernels rely on:
//   * tile_off<DPAD> maps (row < 32, ch < DPAD / 8) one to one onto the 16-byte slots of [0, 32 DPAD 2);
//   * acc_row over (r < 16, fhalf < 2) is a permutation of 0 .. 31;
//   * the score chain's A operand -- lane reads chunk 2 ks + (lane >> 5) of tile row lane & 31 -- stays inside the tile
//     and, over the 64 lanes and DPAD / 16 k-steps, reads every slot exactly once;
//   * for every (dt, s2) the gather's two 8-byte reads of the 64 lanes lie inside the tile on 8-byte boundaries and
//     cover rows 16 s2 .. 16 s2 + 15 x columns 32 dt .. 32 dt + 31 exactly once: the rows pack16 puts into k-step s2;
//     gather_at equals the arithmetic retrieval_xent.hip and seq_attention.hip keep written out.
// It does not emulate the transposed read's lane shuffle; that stays with the GPU matrix tests.  Stand-alone:
// tests/test_owner_tile_host.py builds it with the host compiler and -fsanitize=address,undefined and runs it as a
// child process.  Exit 0 = every check held.
#include <cstdio>
#include <vector>

#include "../../keras_rs_amd/csrc/krs_owner_tile.h"

using namespace krs;

static long g_checks = 0, g_failed = 0;

#define CHECK(cond, ...)                       \
  do {                                         \
    ++g_checks;                                \
    if (!(cond) && ++g_failed <= 20) {         \
      std::printf("FAILED " __VA_ARGS__);      \
      std::printf("\n");                       \
    }                                          \
  } while (0)

static_assert(kOwnerTile == 32, "one 32 x 32 MFMA block");
static_assert(acc_row(0, 0) == 0 && acc_row(15, 1) == 31 && acc_row(4, 0) == 8 && acc_row(3, 1) == 7, "acc_row");
static_assert(tile_off<128>(0, 0) == 0 && tile_off<128>(1, 0) == 256 + 16 * 4, "tile_off is usable in constant expressions");

template <int DPAD>
static void check_tile() {
  constexpr int CH = DPAD / 8, BYTES = kOwnerTile * DPAD * 2;

  // the image: a bijection onto the 16-byte slots
  std::vector<int> slot_of(BYTES / 16, -1);
  for (int row = 0; row < kOwnerTile; ++row)
    for (int ch = 0; ch < CH; ++ch) {
      const int off = tile_off<DPAD>(row, ch);
      CHECK(off % 16 == 0, "DPAD %d: tile_off(%d, %d) = %d is not on 16 bytes", DPAD, row, ch, off);
      CHECK(off >= 0 && off + 16 <= BYTES, "DPAD %d: tile_off(%d, %d) = %d leaves the tile", DPAD, row, ch, off);
      if (off % 16 || off < 0 || off + 16 > BYTES) continue;
      CHECK(slot_of[off / 16] < 0, "DPAD %d: tile_off(%d, %d) = %d is also chunk %d", DPAD, row, ch, off, slot_of[off / 16]);
      slot_of[off / 16] = row * CH + ch;
    }
  for (int s = 0; s < BYTES / 16; ++s) CHECK(slot_of[s] >= 0, "DPAD %d: slot %d holds no chunk", DPAD, s);

  // the score chain's A operand
  std::vector<int> reads(BYTES / 16, 0);
  for (int ks = 0; ks < DPAD / 16; ++ks)
    for (int lane = 0; lane < 64; ++lane) {
      const int frow = lane & 31, ch = 2 * ks + (lane >> 5);
      CHECK(ch < CH, "DPAD %d: k-step %d of lane %d reads chunk %d of %d", DPAD, ks, lane, ch, CH);
      const int off = tile_off<DPAD>(frow, ch);
      CHECK(off >= 0 && off + 16 <= BYTES, "DPAD %d: k-step %d of lane %d reads at %d", DPAD, ks, lane, off);
      if (off >= 0 && off + 16 <= BYTES) ++reads[off / 16];
    }
  for (int s = 0; s < BYTES / 16; ++s) CHECK(reads[s] == 1, "DPAD %d: the score chain reads slot %d %d times", DPAD, s, reads[s]);

  // the gather of the second product's B operand
  for (int dt = 0; dt < DPAD / 32; ++dt)
    for (int s2 = 0; s2 < 2; ++s2) {
      std::vector<int> seen(kOwnerTile * DPAD, 0);      // fetches of element (row, column)
      for (int lane = 0; lane < 64; ++lane)
        for (int which = 0; which < 2; ++which) {
          const GatherAt g = gather_at(dt, s2, lane, which);
          const bool inside = g.row >= 0 && g.row < kOwnerTile && g.ch >= 0 && g.ch < CH && (g.byte == 0 || g.byte == 8);
          CHECK(inside, "DPAD %d dt %d s2 %d lane %d read %d: row %d chunk %d byte %d", DPAD, dt, s2, lane, which, g.row,
                g.ch, g.byte);
          if (!inside) continue;
          // (the form xent_kernel and attn_kernel keep written out in their gathers)
          const int li = lane & 15, tq = li >> 2, tp = li & 3, chalf = (lane >> 4) & 1, r0 = 16 * s2 + 4 * (lane >> 5);
          CHECK(g.row == r0 + 8 * which + tq && g.ch == 4 * dt + 2 * chalf + (tp >> 1) && g.byte == 8 * (tp & 1),
                "DPAD %d dt %d s2 %d lane %d read %d differs from the written-out form", DPAD, dt, s2, lane, which);
          const int off = tile_off<DPAD>(g.row, g.ch) + g.byte;
          CHECK(off % 8 == 0 && off >= 0 && off + 8 <= BYTES, "DPAD %d dt %d s2 %d lane %d read %d: at %d", DPAD, dt, s2,
                lane, which, off);
          // (the 8 bytes are 4 consecutive columns of one row, whatever the image does with whole chunks)
          for (int x = 0; x < 4; ++x) ++seen[g.row * DPAD + g.ch * 8 + g.byte / 2 + x];
        }
      for (int row = 0; row < kOwnerTile; ++row)
        for (int col = 0; col < DPAD; ++col) {
          const bool wanted = row >= 16 * s2 && row < 16 * s2 + 16 && col >= 32 * dt && col < 32 * dt + 32;
          CHECK(seen[row * DPAD + col] == (wanted ? 1 : 0), "DPAD %d dt %d s2 %d: element (%d, %d) is fetched %d times",
                DPAD, dt, s2, row, col, seen[row * DPAD + col]);
        }
      // the rows of k-step s2 are pack16's: element j of lane half fhalf is tile row 16 s2 + acc_row(j, fhalf)
      std::vector<int> rows(kOwnerTile, 0);
      for (int fhalf = 0; fhalf < 2; ++fhalf)
        for (int j = 0; j < 8; ++j) ++rows[16 * s2 + acc_row(j, fhalf)];
      for (int row = 0; row < kOwnerTile; ++row)
        CHECK(rows[row] == (row >= 16 * s2 && row < 16 * s2 + 16 ? 1 : 0), "s2 %d: pack16 holds row %d %d times", s2, row,
              rows[row]);
    }
}

int main() {
  std::vector<int> rows(kOwnerTile, 0);
  for (int fhalf = 0; fhalf < 2; ++fhalf)
    for (int r = 0; r < 16; ++r) {
      const int row = acc_row(r, fhalf);
      CHECK(row >= 0 && row < kOwnerTile, "acc_row(%d, %d) = %d", r, fhalf, row);
      if (row >= 0 && row < kOwnerTile) ++rows[row];
    }
  for (int row = 0; row < kOwnerTile; ++row) CHECK(rows[row] == 1, "acc_row reaches row %d %d times", row, rows[row]);
  // a lane's two gather reads belong to its own half: rows acc_row(j, lane >> 5) of the k-step
  for (int lane = 0; lane < 64; ++lane)
    for (int which = 0; which < 2; ++which) {
      const GatherAt g = gather_at(0, 1, lane, which);
      CHECK(g.row == 16 + acc_row(4 * which, lane >> 5) + ((lane & 15) >> 2), "lane %d read %d takes row %d", lane, which,
            g.row);
    }
  check_tile<32>();
  check_tile<64>();
  check_tile<128>();
  check_tile<256>();
  std::printf("%ld checks, %ld failed checks\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
