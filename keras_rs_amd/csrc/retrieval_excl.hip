// K27 -- per-query exclusion lists inside K8's fused top-k: krs_retrieval_topk_excl and krs_retrieval_topk_q8_excl
// (include/krs.h, K27).
//
// What a served recommender asks for: the best k candidates of each query among those the user has not seen.  The lists
// are [b, e] candidate row indices.  Three kernels of this file and one build of K8's stage 1 do it:
//   * excl_prepare_kernel     one workgroup per query row: the row into LDS as sort keys, krs_list.h's bitonic sort, then
//                             the ascending row, the count of its valid entries and the row's cursor at the start of every
//                             candidate slice into the workspace.  Stage 1 consumes this copy; the caller's tensor is read
//                             here and nowhere else.
//   * stage1_body<.., EXCL>   retrieval.hip's stage 1 with the step mask (its comment there): the owners of the tile rows
//                             walk their sorted lists alongside the candidate loop, one list entry per visit.
//   * excl_slab_kernel        the slab path: marks the excluded scores of a query chunk in the fp32 slab, between krs_gemm
//                             and the selection, which reads a mark as "no candidate" (MarkedSlabSrc).
// This file is a translation unit of its own: it takes the shared device code, the selection and the planner glue by
// including retrieval.hip without its entry points.
#define KRS_RETRIEVAL_NO_ENTRIES
#include "retrieval.hip"

namespace krs {
void retrieval_set_route(const krs_retrieval_route& route);   // retrieval.hip: the record krs_retrieval_last_route reads

namespace {
using rplan::kExclMax;

// sort key of a list entry: descending keys are ascending indices, and 0 (an ignored entry) sorts last
__device__ __forceinline__ uint64_t excl_key(int32_t v, int64_t n) {
  return v >= 0 && (int64_t)v < n ? (uint64_t)(0x7fffffff - v) + 1 : 0;
}
__device__ __forceinline__ int32_t excl_index(uint64_t key) { return (int32_t)(0x7fffffff - (int64_t)(key - 1)); }

// grid: b workgroups of kListThreads.  P = the power of two at or above e (<= kSortMax).  S == 0 (slab path): no cursors.
__global__ __launch_bounds__(kListThreads) void excl_prepare_kernel(const int32_t* excl, int64_t ldx, int e, int P,
                                                                    int64_t n, int S, int64_t slice, int32_t* list,
                                                                    int32_t* count, int32_t* start) {
  __shared__ uint64_t s[kSortMax];
  __shared__ int s_count;
  const int64_t row = blockIdx.x;
  const int tid = threadIdx.x;
  for (int i = tid; i < P; i += kListThreads) s[i] = i < e ? excl_key(excl[row * ldx + i], n) : 0;
  if (tid == 0) s_count = 0;
  __syncthreads();
  bitonic_sort(s, P, P, 0);                     // (ends with a barrier)
  // the valid entries are s[0 .. m): the one thread that sees the boundary owns the count
  for (int i = tid; i < P; i += kListThreads)
    if (s[i] != 0 && (i + 1 == P || s[i + 1] == 0)) s_count = i + 1;
  for (int i = tid; i < e; i += kListThreads) list[row * e + i] = s[i] != 0 ? excl_index(s[i]) : -1;
  __syncthreads();
  const int m = s_count;
  if (tid == 0) count[row] = m;
  // start[row, sl] = entries below sl * slice: one binary search in LDS per slice, not per candidate
  for (int sl = tid; sl < S; sl += kListThreads) {
    const int64_t first = (int64_t)sl * slice;
    int lo = 0, hi = m;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if ((int64_t)excl_index(s[mid]) < first) lo = mid + 1;
      else hi = mid;
    }
    start[row * S + sl] = lo;
  }
}

// the slab path: thread t = (row of the chunk, list entry j) writes the mark over that row's score of the excluded
// candidate.  A repeated entry is written by its first occurrence only (the list is sorted: one owner per word).
__global__ __launch_bounds__(256) void excl_slab_kernel(const int32_t* list, const int32_t* count, int e, int64_t row0,
                                                        int64_t rows, uint32_t* slab, int64_t n) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows * e) return;
  const int64_t r = t / e;
  const int j = (int)(t % e);
  const int32_t* l = list + (row0 + r) * e;
  if (j >= count[row0 + r]) return;
  const int32_t idx = l[j];
  if (j > 0 && l[j - 1] == idx) return;
  slab[r * n + idx] = kExclMark;
}

template <int ES, bool VEC>
__global__ __launch_bounds__(256) void retr_stage1_excl_kernel(const Stage1 p, const Excl ex) {
  stage1_body<ES, VEC, false, false, 0, true>(p, Mine{}, Q8Scale{}, Ivf{}, Ah{}, ex);
}
template <bool VEC>
__global__ __launch_bounds__(256) void retr_stage1_q8_excl_kernel(const Stage1 p, const Q8Scale q8, const Excl ex) {
  stage1_body<1, VEC, false, false, 0, true>(p, Mine{}, q8, Ivf{}, Ah{}, ex);
}

// the list arguments both entries check before anything else of theirs (e == 0 never gets here)
inline int excl_check(const char* who, const int32_t* excl, int64_t ldx, int64_t e) {
  KRS_REQUIRE(e > 0, "%s: e = %lld is negative", who, (long long)e);
  KRS_REQUIRE(ldx >= e, "%s: exclusion row stride %lld below e = %lld", who, (long long)ldx, (long long)e);
  KRS_REQUIRE(excl, "%s: null exclusion list with e = %lld", who, (long long)e);
  return KRS_OK;
}
// excl_prepare_kernel with the plan's sections; the Excl operand of stage 1
inline int excl_prepare(const rplan::Plan& pl, const int32_t* excl, int64_t ldx, int64_t e, int64_t b, int64_t n, char* ws,
                        hipStream_t st, Excl& ex) {
  int32_t* list = reinterpret_cast<int32_t*>(ws + pl.off_xlist);
  int32_t* count = reinterpret_cast<int32_t*>(ws + pl.off_xcount);
  int32_t* start = pl.route.kernel == KRS_RETR_FUSED ? reinterpret_cast<int32_t*>(ws + pl.off_xstart) : nullptr;
  hipLaunchKernelGGL(excl_prepare_kernel, dim3((unsigned)b), dim3(kListThreads), 0, st, excl, ldx, (int)e,
                     (int)rplan::pow2_at_least(e), n, start ? pl.S : 0, pl.slice, list, count, start);
  KRS_CHECK_LAUNCH("excl_prepare_kernel");
  ex = Excl{list, e, count, start};
  return KRS_OK;
}
}  // namespace
}  // namespace krs

extern "C" size_t krs_retrieval_topk_excl_workspace_bytes(int64_t b, int64_t n, int64_t d, int k, int dtype, int64_t e) {
  using namespace krs;
  if (e == 0) return krs_retrieval_topk_workspace_bytes(b, n, d, k, dtype);
  if (b <= 0 || n <= 0 || d <= 0 || k < 1 || e < 0) return 0;
  return (size_t)rplan::plan_retrieval(
             make_call(KRS_RETR_VARIANT_TOPK_EXCL, dtype == KRS_BF16 ? 2 : 4, nullptr, d, b, n, d, k, e))
      .total;
}

extern "C" int krs_retrieval_topk_excl(const void* q, int64_t ldq, const void* c, int64_t ldc, const int32_t* ids,
                                       int dtype, int64_t b, int64_t n, int64_t d, int k, void* out_scores,
                                       int32_t* out_ids, void* workspace, size_t workspace_bytes, void* stream,
                                       const int32_t* excl, int64_t ldx, int64_t e) {
  using namespace krs;
  if (e == 0)
    return krs_retrieval_topk(q, ldq, c, ldc, ids, dtype, b, n, d, k, out_scores, out_ids, workspace, workspace_bytes,
                              stream);
  const char* who = "krs_retrieval_topk_excl";
  retrieval_set_route(krs_retrieval_route{});
  const int rx = excl_check(who, excl, ldx, e);
  if (rx != KRS_OK) return rx;
  rplan::Plan pl;
  const int rc = check_and_plan(KRS_RETR_VARIANT_TOPK_EXCL, q, ldq, c, ldc, dtype, b, n, d, k, pl, e);
  if (rc != KRS_OK || b == 0) return rc;
  KRS_REQUIRE(out_ids, "%s: null operand", who);
  const size_t need = (size_t)pl.total;
  if (!workspace || workspace_bytes < need)
    return fail(KRS_ERR_WORKSPACE, "%s: needs %zu workspace bytes, got %zu", who, need, workspace_bytes);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* ws = reinterpret_cast<char*>(workspace);
  uint64_t* list = reinterpret_cast<uint64_t*>(ws + pl.off_merge);
  Excl ex;
  const int rp = excl_prepare(pl, excl, ldx, e, b, n, ws, st, ex);
  if (rp != KRS_OK) return rp;

  if (pl.route.kernel == KRS_RETR_FUSED) {
    const Stage1 p = stage1_args(pl, q, ldq, c, ldc, b, n, d, k, ws);
    KRS_STAGE1_BUILD(retr_stage1_excl_kernel, p, ex)
    KRS_CHECK_LAUNCH("retr_stage1_excl_kernel");
    // a row with fewer than k survivors ends in padding pairs: index -1, score -inf
    const Out out{out_ids, out_scores, dtype, ids, k, 0, n};
    const int rs = select_rows(PairSrc{p.out, pl.sel.len}, b, pl.sel, k, out, list, st);
    if (rs == KRS_OK) retrieval_set_route(pl.route);
    return rs;
  }

  // two-step path: krs_gemm into the chunk's slab, the marks, then the row selection over the marked slab
  float* slab = reinterpret_cast<float*>(ws + pl.off_slab);
  for (int64_t i = 0; i < pl.chunks; ++i) {
    const int64_t r0 = rplan::chunk_row0(pl, i), rows = rplan::chunk_len(pl, i, b);
    const int rg = krs_gemm(reinterpret_cast<const char*>(q) + r0 * ldq * pl.route.es, ldq, 0, c, ldc, 1, slab, n, rows, n,
                            d, dtype, KRS_F32, nullptr, ws + pl.off_gemm, (size_t)pl.gemm_bytes, stream);
    if (rg != KRS_OK) return rg;
    hipLaunchKernelGGL(excl_slab_kernel, dim3((unsigned)ceil_div(rows * e, 256)), dim3(256), 0, st, ex.list, ex.count,
                       (int)e, r0, rows, reinterpret_cast<uint32_t*>(slab), n);
    KRS_CHECK_LAUNCH("excl_slab_kernel");
    const MarkedSlabSrc src{reinterpret_cast<const uint32_t*>(slab), n};
    const Out out{out_ids, out_scores, dtype, ids, k, r0, n};
    const int rs = select_rows(src, rows, pl.sel, k, out, list, st);
    if (rs != KRS_OK) return rs;
  }
  retrieval_set_route(pl.route);
  return KRS_OK;
}

extern "C" size_t krs_retrieval_topk_q8_excl_workspace_bytes(int64_t b, int64_t n, int64_t d, int k, int64_t e) {
  using namespace krs;
  if (e == 0) return krs_retrieval_topk_q8_workspace_bytes(b, n, d, k);
  if (b <= 0 || n <= 0 || d <= 0 || k < 1 || e < 0 || !rplan::fused_path(d, k)) return 0;
  return (size_t)rplan::plan_retrieval(make_call(KRS_RETR_VARIANT_Q8_EXCL, 1, nullptr, d, b, n, d, k, e)).total;
}

extern "C" int krs_retrieval_topk_q8_excl(const void* q, int64_t ldq, int q_dtype, const int8_t* cq, int64_t ldc,
                                          const float* cstep, const int32_t* ids, int64_t b, int64_t n, int64_t d, int k,
                                          void* out_scores, int out_dtype, int32_t* out_ids, int* err_flag,
                                          void* workspace, size_t workspace_bytes, void* stream, const int32_t* excl,
                                          int64_t ldx, int64_t e) {
  using namespace krs;
  if (e == 0)
    return krs_retrieval_topk_q8(q, ldq, q_dtype, cq, ldc, cstep, ids, b, n, d, k, out_scores, out_dtype, out_ids,
                                 err_flag, workspace, workspace_bytes, stream);
  const char* who = "krs_retrieval_topk_q8_excl";
  retrieval_set_route(krs_retrieval_route{});
  KRS_REQUIRE(out_dtype == KRS_F32 || out_dtype == KRS_BF16, "%s: bad output dtype", who);
  const int rx = excl_check(who, excl, ldx, e);
  if (rx != KRS_OK) return rx;
  rplan::Plan pl;
  const int rc = check_and_plan(KRS_RETR_VARIANT_Q8_EXCL, q, ldq, cq, ldc, q_dtype, b, n, d, k, pl, e);
  if (rc != KRS_OK || b == 0) return rc;
  KRS_REQUIRE(cstep && out_ids, "%s: null operand", who);
  const size_t need = (size_t)pl.total;
  if (!workspace || workspace_bytes < need)
    return fail(KRS_ERR_WORKSPACE, "%s: needs %zu workspace bytes, got %zu", who, need, workspace_bytes);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* ws = reinterpret_cast<char*>(workspace);
  int8_t* qq = reinterpret_cast<int8_t*>(ws + pl.off_qq);
  float* qstep = reinterpret_cast<float*>(ws + pl.off_qstep);
  Excl ex;
  const int rp = excl_prepare(pl, excl, ldx, e, b, n, ws, st, ex);
  if (rp != KRS_OK) return rp;

  hipLaunchKernelGGL(quantize_queries_q8_kernel, dim3((unsigned)ceil_div(b, 4)), dim3(256), 0, st, q, ldq, q_dtype, b,
                     (int)d, pl.row_bytes, qq, qstep, err_flag);
  KRS_CHECK_LAUNCH("quantize_queries_q8_kernel");
  const Stage1 p = stage1_args(pl, qq, pl.row_bytes, cq, ldc, b, n, d, k, ws);
  const Q8Scale q8{cstep, qstep};
  if (pl.vec) KRS_STAGE1_LAUNCH(retr_stage1_q8_excl_kernel<true>, p, q8, ex)
  else KRS_STAGE1_LAUNCH(retr_stage1_q8_excl_kernel<false>, p, q8, ex)
  KRS_CHECK_LAUNCH("retr_stage1_q8_excl_kernel");
  const Out out{out_ids, out_scores, out_dtype, ids, k, 0, n};
  const int rs = select_rows(PairSrc{p.out, pl.sel.len}, b, pl.sel, k, out, reinterpret_cast<uint64_t*>(ws + pl.off_merge), st);
  if (rs == KRS_OK) retrieval_set_route(pl.route);
  return rs;
}
