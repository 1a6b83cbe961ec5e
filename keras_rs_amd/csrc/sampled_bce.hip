// K29 -- the sampled-item binary cross-entropy of a sequence model (SASRec's training loss): for every token the rows
// of its positive and its N sampled negative items are gathered ONCE and leave the logits' dot products, the BCE with
// logits, the logit gradients glog and the gradient to the sequence embedding.  Neither the [T, 1 + N, d] block of
// gathered rows nor the logits are ever stored; the table gradient is K2's (krs_embed_bag_bwd_dense with glog as the
// per-lookup weights and the sequence embedding as the bag gradient).
//
// The contract -- the fp32 operation order of a logit, an element, glog, demb and every sum -- is include/krs.h's (K29);
// nothing here may be contracted into an fma:
#pragma clang fp contract(off)
//
// Split: a token lives in a group of G = 8 / 16 / 32 / 64 lanes of one wave (8 G >= d), a lane owns 8 adjacent columns
// and keeps its slice of the token's embedding in fp32 registers for all 1 + N items.  Up to four item rows of a token
// are requested before the first dot product; the ids and the weight of the group's next token are requested a token
// ahead.  The partial dot of a lane goes through an xor butterfly, after which every lane of the group holds the same
// logit and does the same BCE arithmetic: no broadcast.  demb's slice is accumulated from the rows while they are
// still in registers and stored once.  Sums follow K24's scheme (regression.hip): a group adds its tokens in token
// order, the workgroup runs a fixed halving tree in LDS, one partial per workgroup is added in workgroup order (by a
// finish launch when there is more than one), and sum w comes from a pass of its own.  No float atomics, no host wait.
#include "krs_common.h"
#include "sampled_bce_plan.h"

namespace krs {
namespace {

constexpr int kThreads = KRS_SAMPLED_BCE_THREADS;
constexpr int kCols = sbce::kCols;
constexpr int kChunk = sbce::kChunk;

struct Args {
  const void* emb;
  const void* table;
  const void* pos;
  const void* neg;
  const float* w;
  float* loss;
  float* glog;
  void* demb;
  int* err;
  const float* w_partials;   // the W pass's w_blocks partials (with weights)
  float* partials;           // [gridDim.x], used when gridDim.x > 1
  int64_t lde, ldt, ldd, tokens, vocab;
  int d, n, is64, w_blocks;
  float count;               // S without weights: float(tokens)
};

// one correctly rounded fp32 division (v_div_scale / v_div_fmas / v_div_fixup): the contract counts on it
__device__ __forceinline__ float div_rn(float x, float y) { return x / y; }

__device__ __forceinline__ void zero8(float (&v)[kCols]) {
#pragma unroll
  for (int c = 0; c < kCols; ++c) v[c] = 0.0f;
}

// a lane's 8 columns from c0 of one row, as fp32; columns >= d are 0
template <typename T, bool VEC>
__device__ __forceinline__ void load_slice(const T* row, int c0, int d, float (&v)[kCols]) {
  if constexpr (VEC) {          // d % 8 == 0: the slice is whole or empty
    if (c0 >= d) {
      zero8(v);
    } else if constexpr (sizeof(T) == 2) {
      const uint4 raw = *reinterpret_cast<const uint4*>(row + c0);
      const uint32_t u[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[2 * i] = __uint_as_float(u[i] << 16);
        v[2 * i + 1] = __uint_as_float(u[i] & 0xffff0000u);
      }
    } else {
      const float4 lo = *reinterpret_cast<const float4*>(row + c0);
      const float4 hi = *reinterpret_cast<const float4*>(row + c0 + 4);
      v[0] = lo.x, v[1] = lo.y, v[2] = lo.z, v[3] = lo.w, v[4] = hi.x, v[5] = hi.y, v[6] = hi.z, v[7] = hi.w;
    }
  } else {
#pragma unroll
    for (int c = 0; c < kCols; ++c) v[c] = c0 + c < d ? load1(row + c0 + c) : 0.0f;
  }
}

template <typename T, bool VEC>
__device__ __forceinline__ void store_slice(T* row, int c0, int d, const float (&v)[kCols]) {
  if constexpr (VEC) {
    if (c0 >= d) return;
    if constexpr (sizeof(T) == 2) {
      *reinterpret_cast<uint4*>(row + c0) =
          make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
    } else {
      *reinterpret_cast<float4*>(row + c0) = make_float4(v[0], v[1], v[2], v[3]);
      *reinterpret_cast<float4*>(row + c0 + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
  } else {
#pragma unroll
    for (int c = 0; c < kCols; ++c)
      if (c0 + c < d) store1(row + c0 + c, v[c]);
  }
}

// id of item j of token t: j == 0 the positive, else negative j - 1
__device__ __forceinline__ int64_t item_id(const Args& a, int64_t t, int j) {
  return j == 0 ? ld_index(a.pos, a.is64, t) : ld_index(a.neg, a.is64, t * a.n + (j - 1));
}

// the first chunk's ids and the weight of a token
__device__ __forceinline__ void fetch_token(const Args& a, int64_t t, int items, int64_t (&id)[kChunk], float& w) {
#pragma unroll
  for (int k = 0; k < kChunk; ++k) id[k] = k < items ? item_id(a, t, k) : 0;
  w = a.w ? a.w[t] : 1.0f;
}

// the W pass's partials in workgroup order
__device__ __forceinline__ float w_sum(const Args& a) {
  float s = 0.0f;
  for (int j = 0; j < a.w_blocks; ++j) s += a.w_partials[j];
  return s;
}

__device__ __forceinline__ void finalize(const Args& a, float W, float total) {
  a.loss[0] = W != 0.0f ? div_rn(total, W) : 0.0f;
}

template <int G, bool VEC, typename TE, typename TT>
__global__ __launch_bounds__(kThreads) void sampled_bce_kernel(const Args a) {
  constexpr int kTokens = kThreads / G;           // tokens of a workgroup per sweep
  __shared__ float part[kThreads];
  __shared__ float s_shared;
  float S = a.count;
  if (a.w) {
    if (threadIdx.x == 0) s_shared = w_sum(a);
    __syncthreads();
    S = s_shared;
  }
  const int items = 1 + a.n;
  const float W = (float)items * S;
  const int l = threadIdx.x % G, q = threadIdx.x / G;
  const int c0 = l * kCols;
  const TE* emb = reinterpret_cast<const TE*>(a.emb);
  const TT* table = reinterpret_cast<const TT*>(a.table);
  const int64_t stride = (int64_t)gridDim.x * kTokens;
  int64_t t = (int64_t)blockIdx.x * kTokens + q;

  float acc = 0.0f;          // this group's tokens, in token order (the same value in all of its lanes)
  bool bad = false;
  int64_t next_id[kChunk];
  float next_w = 0.0f;
  if (t < a.tokens) fetch_token(a, t, items, next_id, next_w);
  for (; t < a.tokens; t += stride) {
    int64_t id[kChunk];
#pragma unroll
    for (int k = 0; k < kChunk; ++k) id[k] = next_id[k];
    const float w = next_w;
    if (t + stride < a.tokens) fetch_token(a, t + stride, items, next_id, next_w);

    float* gl = a.glog + t * items;
    TE* de = a.demb ? reinterpret_cast<TE*>(a.demb) + t * a.ldd : nullptr;
    float da[kCols];
    zero8(da);
    if (w == 0.0f || W == 0.0f) {      // a padded token: no row is requested, zeros go out
      for (int j = l; j < items; j += G) gl[j] = 0.0f;
      if (de) store_slice<TE, VEC>(de, c0, a.d, da);
      continue;
    }
    float e[kCols];
    load_slice<TE, VEC>(emb + t * a.lde, c0, a.d, e);
    float tok = 0.0f;
    for (int j0 = 0; j0 < items; j0 += kChunk) {
      if (j0 > 0) {
#pragma unroll
        for (int k = 0; k < kChunk; ++k) id[k] = j0 + k < items ? item_id(a, t, j0 + k) : 0;
      }
      float r[kChunk][kCols];
      bool ok[kChunk];
#pragma unroll
      for (int k = 0; k < kChunk; ++k) {           // every row of the chunk is requested before the first dot
        const bool in = j0 + k < items;
        ok[k] = in && id[k] >= 0 && id[k] < a.vocab;
        bad |= in && !ok[k];
        if (ok[k]) load_slice<TT, VEC>(table + id[k] * a.ldt, c0, a.d, r[k]);
        else zero8(r[k]);
      }
#pragma unroll
      for (int k = 0; k < kChunk; ++k) {
        if (j0 + k < items) {                      // (uniform over the kernel)
          float p = 0.0f;
#pragma unroll
          for (int c = 0; c < kCols; ++c) p = p + e[c] * r[k][c];
#pragma unroll
          for (int o = G / 2; o > 0; o >>= 1) p = p + __shfl_xor(p, o);
          float g = 0.0f;
          if (ok[k]) {
            const float x = p, y = j0 + k == 0 ? 1.0f : 0.0f;
            const float u = expf(-fabsf(x));
            const float s = 1.0f + u;
            const float lv = (fmaxf(x, 0.0f) - x * y) + log1pf(u);
            const float sg = x >= 0.0f ? div_rn(1.0f, s) : div_rn(u, s);
            tok = tok + lv;
            g = div_rn(w * (sg - y), W);
          }
          if (l == k) gl[j0 + k] = g;              // (kChunk <= G: lane k of the group)
#pragma unroll
          for (int c = 0; c < kCols; ++c) da[c] = da[c] + g * r[k][c];
        }
      }
    }
    acc = acc + w * tok;
    if (de) store_slice<TE, VEC>(de, c0, a.d, da);
  }
  if (bad && a.err && l == 0) atomicOr(a.err, KRS_FLAG_ID_OUT_OF_RANGE);

  part[threadIdx.x] = l == 0 ? acc : 0.0f;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (gridDim.x > 1) a.partials[blockIdx.x] = part[0];
    else finalize(a, W, part[0]);
  }
}

// the partials of `blocks` > 1 workgroups added in workgroup order
__global__ __launch_bounds__(KRS_SAMPLED_BCE_MAX_BLOCKS) void sampled_bce_finish_kernel(const Args a, int blocks) {
  __shared__ float part[KRS_SAMPLED_BCE_MAX_BLOCKS];
  const int t = threadIdx.x;
  part[t] = t < blocks ? a.partials[t] : 0.0f;
  __syncthreads();
  if (t == 0) {
    float s = 0.0f;
    for (int j = 0; j < blocks; ++j) s += part[j];
    const float S = a.w ? w_sum(a) : a.count;
    finalize(a, (float)(1 + a.n) * S, s);
  }
}

// W pass: a grid-strided sum per thread, the halving tree, one partial per workgroup
__global__ __launch_bounds__(KRS_SAMPLED_BCE_W_THREADS) void sampled_bce_wsum_kernel(const float* __restrict__ w,
                                                                                     int64_t tokens,
                                                                                     float* __restrict__ partials) {
  constexpr int kW = KRS_SAMPLED_BCE_W_THREADS;
  __shared__ float part[kW];
  float acc = 0.0f;
  for (int64_t i = (int64_t)blockIdx.x * kW + threadIdx.x; i < tokens; i += (int64_t)gridDim.x * kW) acc += w[i];
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int o = kW / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = part[0];
}

template <int G, bool VEC>
void launch_typed(const Args& a, int blocks, int emb_dtype, int table_dtype, hipStream_t st) {
  const dim3 grid(blocks), block(kThreads);
  const bool eb = emb_dtype == KRS_BF16, tb = table_dtype == KRS_BF16;
  if (eb && tb) hipLaunchKernelGGL((sampled_bce_kernel<G, VEC, uint16_t, uint16_t>), grid, block, 0, st, a);
  else if (eb) hipLaunchKernelGGL((sampled_bce_kernel<G, VEC, uint16_t, float>), grid, block, 0, st, a);
  else if (tb) hipLaunchKernelGGL((sampled_bce_kernel<G, VEC, float, uint16_t>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((sampled_bce_kernel<G, VEC, float, float>), grid, block, 0, st, a);
}

template <bool VEC>
void launch_group(const Args& a, const krs_sampled_bce_route& rt, int emb_dtype, int table_dtype, hipStream_t st) {
  switch (rt.g) {
    case 8: return launch_typed<8, VEC>(a, rt.blocks, emb_dtype, table_dtype, st);
    case 16: return launch_typed<16, VEC>(a, rt.blocks, emb_dtype, table_dtype, st);
    case 32: return launch_typed<32, VEC>(a, rt.blocks, emb_dtype, table_dtype, st);
    default: return launch_typed<64, VEC>(a, rt.blocks, emb_dtype, table_dtype, st);
  }
}

thread_local krs_sampled_bce_route g_route = {};

sbce::Call call_of(const void* emb, int64_t ld_emb, int emb_dtype, const void* table, int64_t ld_table, int table_dtype,
                   int64_t vocab, const void* pos, const void* neg, int itype, const float* weight, int64_t t, int64_t d,
                   int64_t n, const float* glog, const void* demb, int64_t ld_demb) {
  sbce::Call c;
  c.emb = emb, c.ld_emb = ld_emb, c.emb_dtype = emb_dtype;
  c.table = table, c.ld_table = ld_table, c.table_dtype = table_dtype, c.vocab = vocab;
  c.pos = pos, c.neg = neg, c.itype = itype, c.weight = weight;
  c.t = t, c.d = d, c.n = n;
  c.glog = glog, c.demb = demb, c.ld_demb = ld_demb;
  return c;
}

int refuse(const sbce::Plan& pl, const sbce::Call& c) {
  return fail(pl.status,
              "krs_sampled_bce_fwd_bwd: bad %s (t %lld, d %lld, n %lld, vocab %lld, emb dtype %d, table dtype %d, itype %d, "
              "ld_emb %lld, ld_table %lld, ld_demb %lld, emb %p, table %p, pos %p, neg %p, glog %p)",
              pl.why, (long long)c.t, (long long)c.d, (long long)c.n, (long long)c.vocab, c.emb_dtype, c.table_dtype,
              c.itype, (long long)c.ld_emb, (long long)c.ld_table, (long long)c.ld_demb, c.emb, c.table, c.pos, c.neg,
              c.glog);
}

}  // namespace
}  // namespace krs

extern "C" size_t krs_sampled_bce_workspace_bytes(int64_t t) { return krs::sbce::workspace_bytes(t); }

extern "C" int krs_sampled_bce_last_route(krs_sampled_bce_route* route) {
  if (route) *route = krs::g_route;
  return krs::g_route.kernel;
}

extern "C" int krs_sampled_bce_plan_route(const void* emb, int64_t ld_emb, int emb_dtype, const void* table,
                                          int64_t ld_table, int table_dtype, int64_t vocab, const void* pos,
                                          const void* neg, int itype, const float* weight, int64_t t, int64_t d,
                                          int64_t n, const float* glog, const void* demb, int64_t ld_demb,
                                          krs_sampled_bce_route* route) {
  using namespace krs;
  const sbce::Call call = call_of(emb, ld_emb, emb_dtype, table, ld_table, table_dtype, vocab, pos, neg, itype, weight,
                                  t, d, n, glog, demb, ld_demb);
  const sbce::Plan pl = sbce::plan(call);
  if (route) *route = pl.route;
  return pl.status == KRS_OK ? KRS_OK : refuse(pl, call);
}

extern "C" int krs_sampled_bce_fwd_bwd(const void* emb, int64_t ld_emb, int emb_dtype, const void* table,
                                       int64_t ld_table, int table_dtype, int64_t vocab, const void* pos,
                                       const void* neg, int itype, const float* weight, int64_t t, int64_t d, int64_t n,
                                       float* loss, float* glog, void* demb, int64_t ld_demb, int* err_flag,
                                       void* workspace, size_t workspace_bytes, void* stream) {
  using namespace krs;
  const char* what = "krs_sampled_bce_fwd_bwd";
  g_route = {};
  const sbce::Call call = call_of(emb, ld_emb, emb_dtype, table, ld_table, table_dtype, vocab, pos, neg, itype, weight,
                                  t, d, n, glog, demb, ld_demb);
  const sbce::Plan pl = sbce::plan(call);
  if (pl.status != KRS_OK) return refuse(pl, call);
  if (t == 0) return KRS_OK;
  KRS_REQUIRE(loss != nullptr, "%s: null loss", what);
  const size_t need = sbce::workspace_bytes(t);
  if (!workspace || workspace_bytes < need)
    return fail(KRS_ERR_WORKSPACE, "%s: workspace of %zu bytes at %p, %zu needed", what, workspace_bytes, workspace,
                need);
  float* ws = reinterpret_cast<float*>(workspace);
  Args a = {};
  a.emb = emb, a.table = table, a.pos = pos, a.neg = neg, a.w = weight;
  a.loss = loss, a.glog = glog, a.demb = demb, a.err = err_flag;
  a.w_partials = weight ? ws : nullptr;
  a.partials = ws + KRS_SAMPLED_BCE_W_BLOCKS;
  a.lde = ld_emb, a.ldt = ld_table, a.ldd = ld_demb, a.tokens = t, a.vocab = vocab;
  a.d = (int)d, a.n = (int)n, a.is64 = itype == KRS_I64, a.w_blocks = pl.w_blocks;
  a.count = (float)t;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (weight)
    hipLaunchKernelGGL(sampled_bce_wsum_kernel, dim3(pl.w_blocks), dim3(KRS_SAMPLED_BCE_W_THREADS), 0, st, weight, t,
                       ws);
  if (pl.route.kernel == KRS_SAMPLED_BCE_VEC) launch_group<true>(a, pl.route, emb_dtype, table_dtype, st);
  else launch_group<false>(a, pl.route, emb_dtype, table_dtype, st);
  if (pl.route.blocks > 1)
    hipLaunchKernelGGL(sampled_bce_finish_kernel, dim3(1), dim3(KRS_SAMPLED_BCE_MAX_BLOCKS), 0, st, a, pl.route.blocks);
  KRS_CHECK_LAUNCH(what);
  g_route = pl.route;
  return KRS_OK;
}
