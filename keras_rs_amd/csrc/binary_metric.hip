// K12 -- binary metrics: keras.metrics.BinaryAccuracy and keras.metrics.AUC, the two metrics the ml_perf step
// compiles (examples/ml_perf/main.py:201-210 of the reference), from one pass over the predictions.
//
// Replaces, per AUC update, keras' chain of clip, multiply, ceil, relu, two segment sums, two flips, two cumsums
// and the subtractions (metrics_utils.update_confusion_matrix_variables), and per accuracy update a compare, a
// cast, an equal and two sums.
//
//   * binary_hist_kernel   one launch per AUC spec (the accuracy rides in the first).  Samples are cut into chunks
//                          of kChunk.  A workgroup stages a chunk in LDS as (bin, wpos, wneg) -- bin = bucket + 1,
//                          bin 0 = "exceeds no threshold", padding = -1 -- and thread t, the owner of bin t (and
//                          t + threads, .. for a long threshold list), walks the staged samples in index order with
//                          broadcast LDS reads and adds the weights of its own.  Workgroup g of G takes the chunks
//                          g, g + G, .. in that order and writes one partial histogram [2, T + 1] to the workspace.
//                          The accuracy's w * match and w are staged beside them; the first 256 threads add them
//                          (sample t, t + 256, .. , a butterfly over the wave, the four waves in order), whatever
//                          the workgroup's size, so the accuracy has the same bits with or without an AUC beside it.
//   * binary_final_kernel  one workgroup per AUC spec and one for the accuracy: adds the G partials in the order of
//                          g, takes the sums over the bins >= i (tp, fp) and over the bins <= i (fn, tn) with
//                          two Hillis-Steele scans in LDS (fixed shape), and adds the four to the state with plain
//                          vector stores.
//
// G = min(chunks, kGroups) depends on n alone, never on the device: fixed summation order, no float atomics,
// bit-identical from call to call and from box to box.  Nothing waits for the host.
#include "krs_common.h"

namespace krs {
namespace {

constexpr int kChunk = KRS_BINARY_METRIC_CHUNK;
constexpr int kGroups = KRS_BINARY_METRIC_GROUPS;
constexpr int kMaxAucs = KRS_BINARY_METRIC_MAX_AUCS;
constexpr int kMaxT = KRS_BINARY_METRIC_MAX_THRESHOLDS;
constexpr int kMaxBins = kMaxT + 1;
constexpr int kAccThreads = 256;   // the threads that add the accuracy's terms, in every launch shape
static_assert(kChunk % kAccThreads == 0 && kChunk % 4 == 0, "the chunk is walked four samples at a time");

// p of one sample: the sigmoid for logits, then the clamp to [0, 1] (NaN -> 0)
__device__ __forceinline__ float probability(float x, int from_logits) {
  float p = from_logits ? 1.0f / (1.0f + expf(-x)) : x;
  p = p > 0.0f ? p : 0.0f;
  return p < 1.0f ? p : 1.0f;
}

// bin = bucket + 1 in [0, T]
__device__ __forceinline__ int bin_of(float p, int T, const float* __restrict__ th, bool explicit_thresholds) {
  if (!explicit_thresholds) {
    const int b = (int)ceilf(p * (float)(T - 1)) - 1;
    return (b > 0 ? b : 0) + 1;
  }
  int lo = 0, hi = T;   // the number of thresholds below p
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (th[mid] < p) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

template <typename P, int BPT>
__global__ __launch_bounds__(1024) void binary_hist_kernel(const P* __restrict__ pred, const float* __restrict__ labels,
                                                           const float* __restrict__ weights, float weight, int64_t n,
                                                           int do_acc, float acc_threshold, float* __restrict__ acc_part,
                                                           int T, const float* __restrict__ thresholds, int from_logits,
                                                           float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) int s_bin[kChunk];
  __shared__ __attribute__((aligned(16))) float s_wp[kChunk];
  __shared__ __attribute__((aligned(16))) float s_wn[kChunk];
  __shared__ float s_am[kChunk];   // w * match
  __shared__ float s_aw[kChunk];   // w
  __shared__ float s_th[kMaxT];
  __shared__ float s_red[2][kAccThreads / 64];
  const int tid = threadIdx.x, nthreads = blockDim.x;
  const int NB = T + 1;
  if (thresholds)
    for (int i = tid; i < T; i += nthreads) s_th[i] = thresholds[i];
  float ap[BPT], an[BPT];
#pragma unroll
  for (int k = 0; k < BPT; ++k) ap[k] = an[k] = 0.0f;
  float total = 0.0f, count = 0.0f;
  const int64_t n_chunks = ceil_div(n, (int64_t)kChunk);
  __syncthreads();

  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int64_t base = c * kChunk;
    const int m = (int)(n - base < kChunk ? n - base : kChunk);
    for (int i = tid; i < kChunk; i += nthreads) {
      int bin = -1;
      float wp = 0.0f, wn = 0.0f, am = 0.0f, aw = 0.0f;
      if (i < m) {
        const float x = load1(&pred[base + i]);
        const float y = labels[base + i];
        const float w = weights ? weights[base + i] : weight;
        if (T) {
          bin = bin_of(probability(x, from_logits), T, s_th, thresholds != nullptr);
          wp = y != 0.0f ? w : 0.0f;
          wn = y != 0.0f ? 0.0f : w;
        }
        am = (x > acc_threshold ? 1.0f : 0.0f) == y ? w : 0.0f;
        aw = w;
      }
      s_bin[i] = bin;
      s_wp[i] = wp;
      s_wn[i] = wn;
      s_am[i] = am;
      s_aw[i] = aw;
    }
    __syncthreads();
    if (T) {
      const int m4 = (m + 3) >> 2;
      for (int s = 0; s < m4; ++s) {
        const int4 b4 = reinterpret_cast<const int4*>(s_bin)[s];
        const float4 p4 = reinterpret_cast<const float4*>(s_wp)[s];
        const float4 n4 = reinterpret_cast<const float4*>(s_wn)[s];
#pragma unroll
        for (int k = 0; k < BPT; ++k) {
          const int mine = tid + k * nthreads;
          if (b4.x == mine) { ap[k] += p4.x; an[k] += n4.x; }
          if (b4.y == mine) { ap[k] += p4.y; an[k] += n4.y; }
          if (b4.z == mine) { ap[k] += p4.z; an[k] += n4.z; }
          if (b4.w == mine) { ap[k] += p4.w; an[k] += n4.w; }
        }
      }
    }
    if (do_acc && tid < kAccThreads) {
      float a = 0.0f, b = 0.0f;
#pragma unroll
      for (int i = tid; i < kChunk; i += kAccThreads) {
        a += s_am[i];
        b += s_aw[i];
      }
      for (int o = 1; o < 64; o <<= 1) {
        a += __shfl_xor(a, o);
        b += __shfl_xor(b, o);
      }
      if ((tid & 63) == 0) {
        s_red[0][tid >> 6] = a;
        s_red[1][tid >> 6] = b;
      }
    }
    __syncthreads();   // (the staged chunk has been read; the wave sums are in place)
    if (do_acc && tid == 0) {
      float a = s_red[0][0], b = s_red[1][0];
#pragma unroll
      for (int w = 1; w < kAccThreads / 64; ++w) {
        a += s_red[0][w];
        b += s_red[1][w];
      }
      total += a;
      count += b;
    }
  }

  if (T) {
    float* mine_part = part + (size_t)blockIdx.x * 2 * NB;
#pragma unroll
    for (int k = 0; k < BPT; ++k) {
      const int mine = tid + k * nthreads;
      if (mine < NB) {
        mine_part[mine] = ap[k];
        mine_part[NB + mine] = an[k];
      }
    }
  }
  if (do_acc && tid == 0) {
    acc_part[2 * blockIdx.x] = total;
    acc_part[2 * blockIdx.x + 1] = count;
  }
}

struct FinalSpecs {
  int n;
  int T[kMaxAucs];
  float* state[kMaxAucs];
  size_t offset[kMaxAucs];   // of the spec's partials in the workspace, in floats
};

__global__ __launch_bounds__(1024) void binary_final_kernel(const float* __restrict__ ws, int groups, FinalSpecs f,
                                                            float* __restrict__ acc_state) {
  __shared__ float hist[2][kMaxBins];     // [pos, neg][bin]
  __shared__ float buf[2][2][kMaxBins];   // [ping-pong][pos, neg][bin]
  const int tid = threadIdx.x;
  int j = -1;
#pragma unroll
  for (int m = 0; m < kMaxAucs; ++m)
    if (m == (int)blockIdx.x && m < f.n) j = m;
  if (j < 0) {   // the accuracy's workgroup
    if (acc_state && tid < 2) {
      float a = 0.0f;
      for (int g = 0; g < groups; ++g) a += ws[2 * g + tid];
      acc_state[tid] += a;
    }
    return;
  }
  int T = 0;
  float* state = nullptr;
  size_t offset = 0;
#pragma unroll
  for (int m = 0; m < kMaxAucs; ++m)
    if (m == j) {
      T = f.T[m];
      state = f.state[m];
      offset = f.offset[m];
    }
  const int NB = T + 1;
  const float* part = ws + offset;
  for (int col = tid; col < 2 * NB; col += 1024) {
    float a = 0.0f;
#pragma unroll 8
    for (int g = 0; g < groups; ++g) a += part[(size_t)g * 2 * NB + col];
    hist[col >= NB][col >= NB ? col - NB : col] = a;
  }
  // Two scans of the same histogram: over the bins >= i (tp, fp), then over the bins <= i (fn, tn).  Each of the four
  // is a sum of the weights it counts and of nothing else, so its relative error does not depend on how large the
  // other three are, and a count that no sample feeds is an exact zero (all - tp would leave the scans' rounding).
  for (int dir = 0; dir < 2; ++dir) {
    __syncthreads();   // (hist is complete; the last scan's sums have been read)
    for (int i = tid; i < NB; i += 1024) {
      buf[0][0][i] = hist[0][i];
      buf[0][1][i] = hist[1][i];
    }
    __syncthreads();
    int cur = 0;
    for (int o = 1; o < NB; o <<= 1) {   // buf[cur][h][i] = the sum of 2 o bins from i on (dir 0) or up to i (dir 1)
      for (int i = tid; i < NB; i += 1024) {
        const int other = dir == 0 ? i + o : i - o;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          float v = buf[cur][h][i];
          if (other >= 0 && other < NB) v += buf[cur][h][other];
          buf[cur ^ 1][h][i] = v;
        }
      }
      __syncthreads();
      cur ^= 1;
    }
    for (int i = tid; i < T; i += 1024) {
      if (dir == 0) {   // bucket >= i  <=>  bin >= i + 1
        state[i] += buf[cur][0][i + 1];
        state[T + i] += buf[cur][1][i + 1];
      } else {          // bucket < i  <=>  bin <= i
        state[2 * T + i] += buf[cur][1][i];
        state[3 * T + i] += buf[cur][0][i];
      }
    }
  }
}

int used_groups(int64_t n) {
  const int64_t chunks = ceil_div(n, (int64_t)kChunk);
  return (int)(chunks < kGroups ? chunks : kGroups);
}

template <typename P>
void launch_hist(int T, int groups, hipStream_t st, const P* pred, const float* labels, const float* weights,
                 float weight, int64_t n, int do_acc, float acc_threshold, float* acc_part, const float* thresholds,
                 int from_logits, float* part) {
  const int NB = T + 1;
  const int threads = NB <= 256 ? 256 : 1024;
#define KRS_LAUNCH_HIST(BPT)                                                                                       \
  hipLaunchKernelGGL((binary_hist_kernel<P, BPT>), dim3(groups), dim3(threads), 0, st, pred, labels, weights,      \
                     weight, n, do_acc, acc_threshold, acc_part, T, thresholds, from_logits, part)
  if (NB <= 1024) KRS_LAUNCH_HIST(1);
  else if (NB <= 2048) KRS_LAUNCH_HIST(2);
  else KRS_LAUNCH_HIST(3);
#undef KRS_LAUNCH_HIST
}

}  // namespace
}  // namespace krs

extern "C" size_t krs_binary_metrics_workspace_bytes(int64_t n, int n_aucs, const int* auc_T) {
  using namespace krs;
  if (n <= 0) return 0;
  size_t floats = 2 * (size_t)kGroups;
  for (int j = 0; j < n_aucs && j < kMaxAucs && auc_T; ++j)
    floats += (size_t)used_groups(n) * 2 * (size_t)((auc_T[j] > 0 ? auc_T[j] : 0) + 1);
  return floats * sizeof(float);
}

extern "C" int krs_binary_metrics(const void* pred, int dtype, const float* labels, const float* weights, float weight,
                                  int64_t n, float acc_threshold, float* acc_state, int n_aucs,
                                  const float* const* auc_thresholds, const int* auc_T, const int* auc_from_logits,
                                  float* const* auc_states, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace krs;
  const char* what = "krs_binary_metrics";
  KRS_REQUIRE(n >= 0, "%s: negative n", what);
  KRS_REQUIRE(dtype == KRS_F32 || dtype == KRS_BF16, "%s: bad dtype", what);
  KRS_REQUIRE(n_aucs >= 0 && n_aucs <= kMaxAucs, "%s: %d AUC specs outside the supported 0..%d "
              "(KRS_BINARY_METRIC_MAX_AUCS)", what, n_aucs, kMaxAucs);
  KRS_REQUIRE(acc_state || n_aucs > 0, "%s: neither an accuracy state nor an AUC spec", what);
  KRS_REQUIRE(n_aucs == 0 || (auc_T && auc_states), "%s: null spec arrays", what);
  FinalSpecs f;
  f.n = n_aucs;
  size_t offset = 2 * (size_t)kGroups;
  const int groups = n > 0 ? used_groups(n) : 0;
  for (int j = 0; j < kMaxAucs; ++j) {
    f.T[j] = 0;
    f.state[j] = nullptr;
    f.offset[j] = 0;
    if (j >= n_aucs) continue;
    const int T = auc_T[j];
    const bool explicit_thresholds = auc_thresholds && auc_thresholds[j];
    KRS_REQUIRE(T >= 2 && T <= kMaxT, "%s: %d thresholds outside the supported 2..%d "
                "(KRS_BINARY_METRIC_MAX_THRESHOLDS)", what, T, kMaxT);
    KRS_REQUIRE(explicit_thresholds || T >= 3, "%s: the even thresholds need T >= 3; pass both end points for T = 2",
                what);
    KRS_REQUIRE(auc_states[j], "%s: null state %d", what, j);
    f.T[j] = T;
    f.state[j] = auc_states[j];
    f.offset[j] = offset;
    offset += (size_t)groups * 2 * (size_t)(T + 1);
  }
  if (n == 0) return KRS_OK;
  KRS_REQUIRE(pred && labels, "%s: null argument", what);
  const size_t need = krs_binary_metrics_workspace_bytes(n, n_aucs, auc_T);
  if (!workspace || workspace_bytes < need)
    return fail(KRS_ERR_WORKSPACE, "%s: needs %zu workspace bytes, got %zu", what, need, workspace_bytes);
  float* ws = static_cast<float*>(workspace);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int launches = n_aucs > 0 ? n_aucs : 1;
  for (int j = 0; j < launches; ++j) {
    const int T = f.T[j];   // 0: the accuracy alone
    const int do_acc = acc_state && j == 0;
    const float* th = T && auc_thresholds ? auc_thresholds[j] : nullptr;
    const int from_logits = T && auc_from_logits ? auc_from_logits[j] != 0 : 0;
    if (dtype == KRS_BF16)
      launch_hist(T, groups, st, static_cast<const uint16_t*>(pred), labels, weights, weight, n, do_acc,
                  acc_threshold, ws, th, from_logits, ws + f.offset[j]);
    else
      launch_hist(T, groups, st, static_cast<const float*>(pred), labels, weights, weight, n, do_acc, acc_threshold,
                  ws, th, from_logits, ws + f.offset[j]);
    KRS_CHECK_LAUNCH(what);
  }
  hipLaunchKernelGGL(binary_final_kernel, dim3(n_aucs + (acc_state ? 1 : 0)), dim3(1024), 0, st, ws, groups, f,
                     acc_state);
  KRS_CHECK_LAUNCH(what);
  return KRS_OK;
}
