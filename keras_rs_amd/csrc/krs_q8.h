// The row quantizer's arithmetic (include/krs.h, K16), shared by krs_quantize_rows_q8 (embed_bag_fwd_q8.hip) and the query
// quantizer of krs_retrieval_topk_q8 (retrieval.hip), so that both produce the same bits.
#ifndef KRS_Q8_H_
#define KRS_Q8_H_

#include "krs_common.h"

namespace krs {

__device__ __forceinline__ bool nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// the arithmetic of include/krs.h (K16): correctly rounded divisions, round half to even, clip to +-127
__device__ __forceinline__ void row_scales(float a, float& inv, float& step) {
  const float d = a + 1e-7f;
  inv = __fdiv_rn(127.0f, d);
  step = __fdiv_rn(d, 127.0f);
}
__device__ __forceinline__ int quantize1(float x, float inv) {
  return (int)fminf(fmaxf(rintf(__fmul_rn(x, inv)), -127.0f), 127.0f);
}

}  // namespace krs
#endif
