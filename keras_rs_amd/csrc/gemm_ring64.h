// The main loop of the 256 x 256 ring on whole 128-byte lines: one copy, written in bytes, for gemm_pp64_kernel (gemm.hip:
// bf16, a line is 64 k) and gemm_q8_ring_kernel (gemm_q8.hip: int8, a line is 128 k).  A caller brings its accumulators, the
// MFMA that takes a lane's 16-byte fragment pair, and its epilogue.
//
// Same tile (256 x 256, eight waves as 2 x 4, 128 x 64 per wave), same ping-pong of the two wave groups and same k order
// per accumulator as gemm_pp256_kernel (the bf16 results are bit-identical to it) -- what changes is the operand stream: a
// piece is 256 rows x 128 bytes = 32 KB and every row of it is one whole 128-byte line (gemm_pp256_kernel's 64-byte pieces
// fetch each line of A / B in two halves, one K block apart: twice the requests on the per-CU L2 -> LDS path, which is what
// bounds the long-K products -- 1920 cycles per 32-k block against 1024 of MFMA; scripts/exp/gemm_probe3 measured the stream
// alone at 137 us with whole lines against 174).
//   LDS: FIVE 32 KB slots (160 KB, the whole CU), piece i (A of block kb = 2 kb, B = 2 kb + 1) in slot i % 5: while block kb
//   is read from two slots, pieces 2kb+2 .. 2kb+4 are landed / in flight in the other three.  Block kb is consumed in four
//   phases of 32 bytes of K (one MFMA per fragment pair each) and issues piece 2kb+3 in its phases 0, 1 and piece 2kb+4 in
//   its phases 2, 3 (two instructions per wave per phase, as the 64-byte ring); the slot of 2kb+3 held A(kb-1), read last in
//   phase 3 of block kb-1 -- that phase waits for its fragment reads before its first barrier, so the restage is ordered
//   behind them by a barrier whichever wave group issues it.  One counted wait per block (phase 3: vmcnt(2) = the half of piece
//   2kb+4 issued so far may stay in flight), the reads of block kb+1 come a phase later.
//   Row image: 128-byte pitch, 16-byte chunk c of row r at physical chunk c ^ ((r >> 1) & 7): the four 16-lane groups of a
//   ds_read_b128 (rows {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, +32) then cover the sixteen slots of the 256-byte bank row
//   once.  The DMA writes lanes linearly (8 lanes = one row), so the swizzle is applied to the SOURCE chunk: the eight lanes
//   of a row still fetch one whole line.  Rows beyond M / N are clamped to the last row (their results are never stored).
#ifndef KRS_GEMM_RING64_H_
#define KRS_GEMM_RING64_H_

#include "gemm_device.h"

namespace krs {
namespace {

namespace ring64 {
constexpr int SLOT = 32768;
constexpr int NSLOT = 5;
}  // namespace ring64

// Rows m0.. of A and n0.. of B (both K-contiguous, ES bytes per element) from element kbeg on, `nb` whole 128-byte blocks of
// K: the host guarantees nb >= 3, bases on 16 bytes and row strides in whole 16-byte chunks.  `smem` = the workgroup's
// NSLOT * SLOT bytes of dynamic LDS; lane / wave as the calling kernel holds them (wave uniform).
//   mma(i, j, fa, fb)   one MFMA on the wave's accumulator (i, j): 32-row chunk i of its 128 rows, 32-column half j of its
//                       64 columns, 16 bytes of K per lane;
//   tail()              runs once, in block nb-2 behind the last piece's DMA: what it loads from memory (NPF instructions)
//                       is younger than every piece, so the waits that follow leave NPF loads in flight.
// On return every wave has passed the loop's last barrier and its DMA has landed: the slots are dead.
template <int ES, int NPF, class Mma, class Tail>
__device__ __forceinline__ void ring64_main_loop(char* smem, const GemmParams& p, int64_t m0, int64_t n0, int64_t kbeg,
                                                 int64_t nb, int lane, int wave, Mma mma, Tail tail) {
  typedef const __attribute__((address_space(1))) void* gptr;
  typedef __attribute__((address_space(3))) void* lptr;
  const int grp = wave >> 2;
  const int wm = grp, wn = wave & 3;

  // DMA sources: instruction q = wave*4 + i fills rows q*8 .. q*8+7 of a piece, lane = row*8 + physical chunk
  const char* ap[4];
  const char* bp[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = (wave * 4 + i) * 8 + (lane >> 3);
    const int c = (lane & 7) ^ ((r >> 1) & 7);
    ap[i] = p.a + (min(m0 + r, p.m - 1) * p.lda + kbeg) * ES + c * 16;
    bp[i] = p.b + (min(n0 + r, p.n - 1) * p.ldb + kbeg) * ES + c * 16;
  }
  const int dma_off = wave * 4096;      // + i*1024
  auto issue_one = [&](const char* (&src)[4], int slot, int i) {
    __builtin_amdgcn_global_load_lds((gptr)src[i], (lptr)(smem + slot * ring64::SLOT + dma_off + i * 1024), 16, 0, 0);
    src[i] += 128;
  };
  auto issue_half = [&](const char* (&src)[4], int slot, int half) {
    issue_one(src, slot, half * 2);
    issue_one(src, slot, half * 2 + 1);
  };
  // fragment addresses inside a slot (phase hk: ^ hk*32)
  const int frow = lane & 31, fhalf = lane >> 5, key = (frow >> 1) & 7;
  const int a_lane = (wm * 128 + frow) * 128 + ((fhalf ^ key) << 4);
  const int b_lane = (wn * 64 + frow) * 128 + ((fhalf ^ key) << 4);
  auto load_frags = [&](int sa, int sb, int hk, u32x4(&fa)[4], u32x4(&fb)[2]) {
    const char* pa = smem + sa * ring64::SLOT;
    const char* pb = smem + sb * ring64::SLOT;
    const int x = hk * 32;
#pragma unroll
    for (int j = 0; j < 2; ++j) fb[j] = *reinterpret_cast<const u32x4*>(pb + (b_lane ^ x) + j * 4096);
#pragma unroll
    for (int i = 0; i < 4; ++i) fa[i] = *reinterpret_cast<const u32x4*>(pa + (a_lane ^ x) + i * 4096);
  };

  auto mfma8 = [&](const u32x4(&fa)[4], const u32x4(&fb)[2]) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) mma(i, j, fa[i], fb[j]);
    __builtin_amdgcn_s_setprio(0);
  };
  // the compute segment with the two LDS-DMA instructions of this phase's half piece (`src` / `slot`) behind its 2nd and 5th
  // MFMA: in the load segment they (60-185 cycles each) made it the longer of the two segments -- h = x U 195 -> 189 us, the
  // cross product 440 -> 430; where among the MFMAs they sit does not matter (profiles/r6_gemm_k64_dma_in_compute_ab.txt)
  auto mfma8_dma = [&](const u32x4(&fa)[4], const u32x4(&fb)[2], const char* (&src)[4], int slot, int half) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        mma(i, j, fa[i], fb[j]);
        if (i * 2 + j == 1) { __builtin_amdgcn_sched_barrier(0); issue_one(src, slot, half * 2); __builtin_amdgcn_sched_barrier(0); }
        if (i * 2 + j == 4) { __builtin_amdgcn_sched_barrier(0); issue_one(src, slot, half * 2 + 1); __builtin_amdgcn_sched_barrier(0); }
      }
    __builtin_amdgcn_s_setprio(0);
  };
  // one phase of a block that issues half a piece
  auto phase = [&](int sa, int sb, int hk, const char* (&src)[4], int slot, int half, bool last_of_block) {
    u32x4 fa[4], fb[2];
    load_frags(sa, sb, hk, fa, fb);
    if (last_of_block) {
      // pieces 2kb+2, 2kb+3 have landed (read from the next phase on); the first half of piece 2kb+4 may stay in flight (its
      // second half is issued behind this wait)
      pp_vmcnt<2>();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this block's last reads are done before the barrier: its A slot is restaged next
    }
    pp_barrier();
    mfma8_dma(fa, fb, src, slot, half);
    pp_barrier();
  };
  auto step5 = [](int v, int by) { v += by; return v >= ring64::NSLOT ? v - ring64::NSLOT : v; };

  // prologue: pieces 0 (A0), 1 (B0), 2 (A1) whole; block 0's operands must have landed, piece 2 may fly on
  issue_half(ap, 0, 0); issue_half(ap, 0, 1);
  issue_half(bp, 1, 0); issue_half(bp, 1, 1);
  issue_half(ap, 2, 0); issue_half(ap, 2, 1);
  pp_vmcnt<4>();
  pp_barrier();
  if (grp == 1) pp_barrier();  // rows 128..255 run one segment behind rows 0..127
  int sa = 0, sb = 1, s3 = 3, s4 = 4;   // slots of pieces 2kb, 2kb+1, 2kb+3, 2kb+4
  for (int64_t kb = 0; kb + 2 < nb; ++kb) {   // steady state: pieces 2kb+3 (B of kb+1) and 2kb+4 (A of kb+2) are issued
    phase(sa, sb, 0, bp, s3, 0, false);
    phase(sa, sb, 1, bp, s3, 1, false);
    phase(sa, sb, 2, ap, s4, 0, false);
    phase(sa, sb, 3, ap, s4, 1, true);
    sa = step5(sa, 2); sb = step5(sb, 2); s3 = step5(s3, 2); s4 = step5(s4, 2);
  }
  // block nb-2: only B(nb-1) = piece 2kb+3 is left to issue; the caller's tail loads are requested behind it
  {
    phase(sa, sb, 0, bp, s3, 0, false);
    phase(sa, sb, 1, bp, s3, 1, false);
    u32x4 fa[4], fb[2];
    load_frags(sa, sb, 2, fa, fb);
    tail();
    pp_barrier();
    mfma8(fa, fb);
    pp_barrier();
    load_frags(sa, sb, 3, fa, fb);
    pp_vmcnt<NPF>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    pp_barrier();
    mfma8(fa, fb);
    pp_barrier();
    sa = step5(sa, 2); sb = step5(sb, 2);
  }
  // block nb-1: nothing in flight but the tail's loads
#pragma unroll
  for (int hk = 0; hk < 4; ++hk) {
    u32x4 fa[4], fb[2];
    load_frags(sa, sb, hk, fa, fb);
    pp_barrier();
    mfma8(fa, fb);
    pp_barrier();
  }
  if (grp == 0) pp_barrier();
  lds_dma_retired<NPF>();
}

}  // namespace
}  // namespace krs
#endif
