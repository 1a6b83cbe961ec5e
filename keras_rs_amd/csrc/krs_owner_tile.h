// What the "owner on the lane" kernels share (K13 - K15 in retrieval_xent.hip, K19 in seq_attention.hip; the
// accumulator-row rule also serves retrieval.hip and gru.hip).  A new kernel that borrows the body starts from this header.
//
// The body: a wave owns 32 rows of one side, whose bf16 rows live in registers as the B operand of the score product;
// the other side streams through LDS in tiles of kOwnerTile rows.  One v_mfma_f32_32x32x16_bf16 chain scores the tile
// against the owners: lane (lane & 31) holds owner (lane & 31), and its 16 accumulator registers hold the tile rows
// acc_row(r, lane >> 5).  What the kernel makes of the 16 values, rounded pairwise to bf16 (pack16), is the A operand
// of a second product whose B operand is gathered from an LDS tile in that same row order (gather_at, lds_read_tr16).
//
// The tile image serves both kinds of read, the 16-byte row reads of the score chain and the transposed 8-byte reads
// of the gather: 16-byte chunk ch of row r of a 128-column block sits at 256 r + 16 (ch ^ (((r & 3) << 2) | ((r >> 2)
// & 3))), a 256-column tile is two such blocks, and a narrower tile masks the XOR to its row (tile_off).
//
// Part A is index arithmetic in plain C++17, checked on a CPU by tests/host/owner_tile_check.cpp; part B is device code.
// The header holds the leaves.  The two composite pieces -- the score chain over tile_off(lane & 31, 2 ks + (lane >> 5))
// and the gather over gather_at -- stay written out in xent_kernel and attn_kernel: as shared functions, and even with
// gather_at alone taken from here, hipcc rescheduled those kernels and timed rows ran slower (docs/measurement_log.md
// section 28).  Both kernels write gather_at's three integers out by hand; the host check states what they must equal.
#ifndef KRS_OWNER_TILE_H_
#define KRS_OWNER_TILE_H_

#if defined(__HIPCC__)
#include "krs_common.h"
#define KRS_OT_HD __host__ __device__ __forceinline__ constexpr
#else
#define KRS_OT_HD inline constexpr
#endif

namespace krs {

// ---- part A: where things are ----------------------------------------------------------------------------------------
constexpr int kOwnerTile = 32;   // streamed rows of a tile, and owner rows of a wave: one 32 x 32 MFMA block

// MFMA C/D layout of a 32 x 32 block: column = lane & 31, and register r of lane half fhalf = lane >> 5 is this row
KRS_OT_HD int acc_row(int r, int fhalf) { return (r & 3) + 8 * (r >> 2) + 4 * fhalf; }

// byte offset of 16-byte chunk ch of row `row` in the LDS image of a [kOwnerTile][DPAD] bf16 tile
template <int DPAD>
KRS_OT_HD int tile_off(int row, int ch) {
  constexpr int CH = DPAD / 8, CHB = CH < 16 ? CH : 16;
  const int swz = (((row & 3) << 2) | ((row >> 2) & 3)) & (CHB - 1);
  return (ch / CHB) * (kOwnerTile * CHB * 16) + row * (CHB * 16) + 16 * ((ch % CHB) ^ swz);
}

// The gather of the second product's B operand for k-step s2 (tile rows 16 s2 .. 16 s2 + 15, the rows pack16 puts into
// that step) and column tile dt (columns 32 dt .. 32 dt + 31): every lane makes two transposed reads, `which` = 0 and 1,
// of the 8 bytes at tile_off<DPAD>(row, ch) + byte, and takes them as elements 0, 1 and 2, 3 of the operand.
struct GatherAt {
  int row, ch, byte;
};
KRS_OT_HD GatherAt gather_at(int dt, int s2, int lane, int which) {
  const int li = lane & 15, tq = li >> 2, tp = li & 3, chalf = (lane >> 4) & 1, fhalf = lane >> 5;
  return GatherAt{16 * s2 + 8 * which + 4 * fhalf + tq, 4 * dt + 2 * chalf + (tp >> 1), 8 * (tp & 1)};
}

#if defined(__HIPCC__)
// ---- part B: device code ---------------------------------------------------------------------------------------------
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr float kNegInf = -__builtin_inff();

// 8 bf16 of a row from element e0 (`at` points at that element), zero beyond d and for a row that does not exist.
// VEC: every row is whole 16-byte chunks on 16-byte boundaries (d % 8 == 0 included), so a chunk is whole or absent.
template <bool VEC>
__device__ __forceinline__ u32x4 load_chunk(const uint16_t* at, int e0, int d, bool valid) {
  u32x4 v = {0u, 0u, 0u, 0u};
  if (!valid || e0 >= d) return v;
  if constexpr (VEC) {
    return *reinterpret_cast<const u32x4*>(at);
  } else {
    uint32_t h[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) h[x] = e0 + x < d ? at[x] : 0u;
    v = (u32x4){h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
    return v;
  }
}

// 16 per-lane values (by accumulator register), rounded pairwise to bf16 (round to nearest even): registers 8 s2 ..
// 8 s2 + 7 are k-step s2 of the second product's A operand, element j being tile row 16 s2 + acc_row(j, lane >> 5)
__device__ __forceinline__ void pack16(const float* sv, u32x4* pa) {
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2)
    pa[s2] = (u32x4){pack_bf16x2(sv[8 * s2], sv[8 * s2 + 1]), pack_bf16x2(sv[8 * s2 + 2], sv[8 * s2 + 3]),
                     pack_bf16x2(sv[8 * s2 + 4], sv[8 * s2 + 5]), pack_bf16x2(sv[8 * s2 + 6], sv[8 * s2 + 7])};
}

// ds_read_b64_tr_b16 at an LDS address: 4 bf16 of this lane's column, one from each of 4 rows
__device__ __forceinline__ u32x2 lds_read_tr16(const char* at) {
  return __builtin_bit_cast(u32x2,
                            __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(at)));
}

}  // namespace
#endif  // __HIPCC__

}  // namespace krs
#undef KRS_OT_HD
#endif
