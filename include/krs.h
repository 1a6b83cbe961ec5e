/*
 * krs.h -- C ABI of libkrs_hip.so: the MI355X (gfx950) hot path behind the
 * keras-rs layer API (embedding gather+pool, its index-scatter gradient,
 * DotInteraction, FeatureCross).
 *
 * The reference (keras-team/keras-rs) has NO FFI of its own: its boundary for
 * this path is the Keras layer protocol plus the DistributedEmbedding backend
 * hook set (keras_rs/src/layers/embedding/base_distributed_embedding.py:990-1042).
 * Every entry point below therefore names the reference *Python* statement(s)
 * whose arithmetic it replaces; the Python layers in keras_rs_amd/layers call
 * these through ctypes from inside torch.autograd.Function objects.
 *
 * Conventions
 *   - plain C, no torch / HIP types: device pointers are `void*`, the stream is
 *     a `hipStream_t` passed as `void*` (NULL = the null stream);
 *   - every function returns 0 on success or a negative krs_status; the text of
 *     the last failure on the calling thread is krs_last_error();
 *   - no allocation, no ownership transfer, no hidden state: the caller owns
 *     inputs, outputs and workspaces (sizes from *_workspace_bytes()); calls are
 *     asynchronous and ordered by `stream`; safe from any host thread;
 *   - all matrices are row-major; `ld*` are row strides in ELEMENTS;
 *   - index work is bit-exact; floating point accumulates in fp32.
 */
#ifndef KRS_H_
#define KRS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KRS_VERSION 100 /* 0.1.0 */

typedef enum krs_status {
  KRS_OK = 0,
  KRS_ERR_INVALID = -1,     /* bad argument (null pointer, negative size, bad enum) */
  KRS_ERR_UNSUPPORTED = -2, /* valid but not implemented for this shape/dtype */
  KRS_ERR_LAUNCH = -3,      /* HIP launch / runtime failure */
  KRS_ERR_WORKSPACE = -4    /* workspace too small */
} krs_status;

/* KRS_I8: int8 rows with one fp32 step per row (krs_quantize_rows_q8, krs_embed_bag_fwd_q8); every other entry takes
 * KRS_F32 / KRS_BF16 only and refuses it. */
typedef enum krs_dtype { KRS_F32 = 0, KRS_BF16 = 1, KRS_I8 = 2 } krs_dtype;
typedef enum krs_itype { KRS_I32 = 0, KRS_I64 = 1 } krs_itype;

/* EmbedReduce combiners, embed_reduce.py:10 (SUPPORTED_COMBINERS). */
typedef enum krs_combiner { KRS_SUM = 0, KRS_MEAN = 1, KRS_SQRTN = 2 } krs_combiner;

/* keras activations FeatureCross(pre_activation=...) that are fused into the
 * GEMM epilogue; anything else is composed by the host layer. */
typedef enum krs_activation {
  KRS_ACT_NONE = 0,
  KRS_ACT_RELU = 1,
  KRS_ACT_SIGMOID = 2,
  KRS_ACT_TANH = 3
} krs_activation;

/* Bits OR'ed into the optional device-side error word of the embedding calls.
 * Out-of-range ids are never clamped: the row contributes nothing and the bit
 * is raised (SURVEY.md section 8c decision on keras ops.take out-of-range). */
#define KRS_FLAG_ID_OUT_OF_RANGE 1
#define KRS_FLAG_BAD_OFFSETS 2
#define KRS_FLAG_CAPACITY_OVERFLOW 4   /* krs_shard_route_static: lookups beyond the static capacity were dropped */
#define KRS_FLAG_NONFINITE_ROW 8       /* krs_quantize_rows_q8, krs_retrieval_topk_q8 (a query row): a row held a NaN or an infinity (stored as q = 0, step = 0) */

/* One embedding table ([vocab, dim] row-major).  Lives in DEVICE memory as an
 * array indexed by krs_feature.table.  Replaces the `embeddings` variable of
 * one EmbedReduce sublayer (base_distributed_embedding.py:836-852). */
typedef struct krs_table {
  void* weights;    /* [vocab, dim] fp32 or bf16 (table dtype of the call); krs_embed_bag_fwd_q8: [vocab, dim] int8 rows */
  float* slot;      /* optimizer slot: Adagrad accumulator [vocab, dim] fp32, or NULL;
                       krs_embed_bag_fwd_q8 (a quantized table has no optimizer): the [vocab] fp32 step of every row */
  int64_t row_base; /* global row id of row 0: tables of one call get disjoint
                       [row_base, row_base+vocab) ranges (sort keys of the backward),
                       in any order: row_base need not ascend with the table index */
  int32_t vocab;
  float lr;         /* learning rate of this table's fused optimizer */
} krs_table;

/* One feature = one (ids, table) pair; several features may name one table
 * (distributed_embedding_test.py:601-652).  DEVICE memory array.
 * Bags are numbered feature-major: bag = feature * batch + sample. */
typedef struct krs_feature {
  int64_t ids_base; /* dense mode (offsets == NULL): index of this feature's first
                       id in `ids`; bag (f, b) owns ids[ids_base + b*hot .. +hot) */
  int32_t table;    /* index into the krs_table array */
  int32_t hot;      /* dense mode: ids per bag (the L of a [batch, L] input) */
  int32_t combiner; /* krs_combiner */
  int32_t out_col;  /* first column of this feature's dim-wide slot in an output row */
} krs_feature;

int krs_version(void);
const char* krs_last_error(void);

/* ------------------------------------------------------------------------- *
 * K1  fused multi-table gather + weighted segment pool (forward)
 *
 * Replaces, for ALL features of a DistributedEmbedding in one launch, the
 * per-feature chain of the reference:
 *   keras.layers.Embedding.call -> ops.take(table, ids, axis=0)   embed_reduce.py:178
 *   x * w (w = ones when weights is None)                         embed_reduce.py:224-253
 *   ops.sum(axis=-2), divide_no_nan by sum(w) / sqrt(sum(w^2))     embed_reduce.py:255-274
 *   python loop over features                                     base_distributed_embedding.py:910-928
 *
 *   out[b*out_ld + feats[f].out_col + c] =
 *        scale(f,b) * sum_{p in bag(f,b)} w[p] * table_f[ids[p], c]
 *   scale = 1 (sum) | 1/sum w (mean) | 1/sqrt(sum w^2) (sqrtn); 0 where the
 *   divisor is 0 (divide_no_nan).  Accumulation is fp32 in ascending p.
 *
 * ids      [nnz] int32/int64, feature-major concatenation of all features' ids
 * offsets  CSR mode: [n_feats*batch + 1] (int32/int64) bag boundaries into ids;
 *          NULL = dense mode (krs_feature.ids_base / hot describe the bags)
 * weights  [nnz] fp32 per-id weights or NULL (= all ones)
 * nnz      number of ids (CSR: offsets[last]); also sizes the work split
 * bag_scale optional [n_feats*batch] fp32: receives scale(f,b) for the backward
 * err_flag optional device int, OR'ed with KRS_FLAG_* bits
 * ------------------------------------------------------------------------- */
int krs_embed_bag_fwd(const krs_table* tables, const krs_feature* feats, int n_feats,
                      const void* ids, int id_type,
                      const void* offsets, int off_type,
                      const float* weights, int64_t nnz,
                      int batch, int dim, int table_dtype,
                      void* out, int out_dtype, int64_t out_ld,
                      float* bag_scale, int* err_flag, void* stream);

/* Diagnostic, host only: where the CALLING THREAD's last krs_embed_bag_fwd ran.  Every field is 0 when there was no call
 * yet, the call was refused (any return other than KRS_OK) or had nothing to do (n_feats == 0 or batch == 0).
 *   kernel       KRS_EMBED_FWD_*: embed_bag_fwd_vec (pooled), embed_gather_hot1 (pure gather, feature-major),
 *                embed_gather_hot1_rows (pure gather, sample-major), embed_bag_fwd_generic
 *   lpr          lanes per row: 8 / 16 / 32 / 64 on the vector kernels, 1 .. 64 on the generic one
 *   has_w        per-id weights are read (pooled: the HAS_W build; generic: weights != NULL); 0 on the gather kernels
 *   stream       pooled kernel only: the STREAM build (nnz < 2 * bags)
 *   hot_rows     pooled kernel only: rows staged in LDS (the HR build: 0, 64 or 128; KRS_EMBED_OPT_HOTROWS)
 *   bpg          pooled kernel only: bags per group, 1 .. 16
 *   table_dtype, out_dtype  the krs_dtype pair of the instantiation
 *   blocks       workgroups launched
 * Returns `kernel`; `route` may be NULL.  Lets tests prove which kernel they ran. */
enum { KRS_EMBED_FWD_NONE = 0, KRS_EMBED_FWD_VEC, KRS_EMBED_FWD_HOT1, KRS_EMBED_FWD_HOT1_ROWS, KRS_EMBED_FWD_GENERIC };
typedef struct krs_embed_fwd_route {
  int32_t kernel, lpr, has_w, stream, hot_rows, bpg, table_dtype, out_dtype;
  int64_t blocks;
} krs_embed_fwd_route;
int krs_embed_bag_fwd_last_route(krs_embed_fwd_route* route);
/* Diagnostic, host only, no GPU needed: where a krs_embed_bag_fwd with these arguments WOULD run under the
 * KRS_EMBED_OPT_HOTROWS value in force (csrc/embed_fwd_plan.h, the planner the entry itself runs).  offsets, weights and
 * out are read as pointer VALUES only (nullness; the 16-byte alignment of out); nothing is dereferenced, no HIP call is
 * made and the last-route record is untouched.  Fills *route (all zero when nothing would be launched) and returns what
 * the entry returns before its first launch: KRS_OK, KRS_ERR_INVALID (null out, a negative size, dim <= 0, a bad dtype)
 * or KRS_ERR_UNSUPPORTED (batch > INT_MAX - 128, whose bag arithmetic the kernels do in int; a grid beyond 2^31 - 1
 * workgroups). */
int krs_embed_bag_fwd_plan_route(int n_feats, const void* offsets, const float* weights, int64_t nnz, int batch, int dim,
                                 int table_dtype, const void* out, int out_dtype, int64_t out_ld,
                                 krs_embed_fwd_route* route);

/* ------------------------------------------------------------------------- *
 * K16  int8 row-quantized tables for inference: the quantizer and the lookup
 *
 * The stored form of keras.layers.Embedding.quantize("int8") -- int8 rows plus one fp32 scale per row, abs-max --
 * except that the stored scale is the DEQUANTIZATION step (Keras stores its reciprocal), so that a gather is one
 * correctly rounded multiply.  For a row x[0..dim) (bf16 widened exactly), all in fp32 with IEEE operations:
 *   a    = max_c |x[c]|
 *   inv  = 127.0f / (a + 1e-7f)                      (correctly rounded division)
 *   q[c] = clip(rint(x[c] * inv), -127, 127)         (rint = round half to even)
 *   step = (a + 1e-7f) / 127.0f                      (correctly rounded division)
 * A row holding a NaN or an infinity gets q = 0, step = 0 and raises KRS_FLAG_NONFINITE_ROW in err_flag.
 *
 * table [vocab, dim] fp32 / bf16 (table_dtype), q [vocab, dim] int8, step [vocab] fp32; any dim >= 1, vocab up to
 * INT32_MAX.  One pass: a row of up to 1024 elements is read once and kept in registers between the abs-max and the
 * rounding, a longer one is read twice.  No allocation, no host wait.
 * ------------------------------------------------------------------------- */
int krs_quantize_rows_q8(const void* table, int table_dtype, int64_t vocab, int dim, int8_t* q, float* step,
                         int* err_flag, void* stream);

/* The K1 lookup on quantized tables: krs_table.weights = the int8 rows, krs_table.slot = the [vocab] steps.
 *   out[b*out_ld + feats[f].out_col + c] = scale(f,b) * sum_{p in bag(f,b)} w[p] * step[ids[p]] * q[ids[p], c]
 * Combiners, divide_no_nan and the out-of-range rule are krs_embed_bag_fwd's (an out-of-range id contributes nothing,
 * raises KRS_FLAG_ID_OUT_OF_RANGE and still counts in the denominator).  Accumulation is fp32: the factor w * step is
 * formed once per lookup, every element is then one fused multiply-add, in ascending p.  Every int8 value is
 * dequantized, -128 included.  Every table needs vocab >= 1: row 0 and step[0] are read (and masked) as the stand-in of
 * an invalid or padding slot, as krs_embed_bag_fwd reads row 0.  Arguments as krs_embed_bag_fwd without table_dtype and bag_scale (forward only).  No
 * allocation and no host wait: a lookup can be captured in a HIP graph. */
int krs_embed_bag_fwd_q8(const krs_table* tables, const krs_feature* feats, int n_feats,
                         const void* ids, int id_type,
                         const void* offsets, int off_type,
                         const float* weights, int64_t nnz,
                         int batch, int dim,
                         void* out, int out_dtype, int64_t out_ld,
                         int* err_flag, void* stream);
/* As krs_embed_bag_fwd_last_route / _plan_route, for krs_embed_bag_fwd_q8 (csrc/embed_fwd_q8_plan.h).  The record has
 * table_dtype = KRS_I8; kernel is KRS_EMBED_FWD_VEC (dim a multiple of 16, at most 1024: one 16-byte piece of 16
 * elements per lane, lpr 8 / 16 / 32 / 64) or KRS_EMBED_FWD_GENERIC; stream and hot_rows stay 0.  Refusals as K1's. */
int krs_embed_bag_fwd_q8_last_route(krs_embed_fwd_route* route);
int krs_embed_bag_fwd_q8_plan_route(int n_feats, const void* offsets, const float* weights, int64_t nnz, int batch, int dim,
                                    const void* out, int out_dtype, int64_t out_ld, krs_embed_fwd_route* route);

/* ------------------------------------------------------------------------- *
 * K2  index-scatter gradient of K1
 *
 * Replaces the autodiff of ops.take/multiply/sum (restated by the reference at
 * keras_rs/src/layers/embedding/jax/test_utils.py:395-417, accumulated per
 * table over features :450-468) and, in the fused forms, the per-table
 * optimizer step of jax/test_utils.py:474-497 (SGD: t -= lr*g;
 * Adagrad: acc += g*g; t -= lr*g/sqrt(acc), no epsilon).
 *
 *   dE_table[r, :] = sum over {p : ids[p] == r, feature(p) uses table}
 *                       w[p] * scale(bag(p)) * grad[b(p)*grad_ld + out_col + :]
 *
 * Step 1 (plan): stable sort of the nnz lookups by global row id
 * (tables[t].row_base + id).  Within one row the contributions are then
 * summed in ascending p: the result is deterministic (run-to-run bit-exact).
 * Step 2 (apply): one pass over the sorted segments that either writes the
 * dense gradient rows, or applies SGD / Adagrad to the touched rows in place.
 * ------------------------------------------------------------------------- */
size_t krs_embed_bag_bwd_workspace_bytes(int64_t nnz);

/* total_rows = max over tables of row_base+vocab (bounds the sort key bits). */
int krs_embed_bag_bwd_plan(const krs_table* tables, const krs_feature* feats, int n_feats,
                           const void* ids, int id_type,
                           const void* offsets, int off_type,
                           int batch, int64_t nnz, int64_t total_rows,
                           void* workspace, size_t workspace_bytes,
                           int* err_flag, void* stream);

/* The same plan for DENSE bags (no offsets) when the caller also holds the descriptors on the HOST
 * (tables_host / feats_host: host copies of the device arrays).  When the features of every table are
 * neighbours and tables (and their row bases) ascend with the features, each table's lookups are one
 * contiguous run and the sort runs per table on the id alone (fewer passes, 8-byte intermediate pairs);
 * any other layout takes the global sort of krs_embed_bag_bwd_plan.  The workspace it leaves is
 * consumed by the same apply calls, with one difference: out-of-range ids end their TABLE'S run
 * instead of the whole array -- which krs_embed_bag_bwd_dense and the fused forms skip wherever they
 * are; krs_embed_bag_bwd_sparse (output indexed by segment) needs the plan of krs_embed_bag_bwd_plan. */
int krs_embed_bag_bwd_plan_tables(const krs_table* tables, const krs_table* tables_host, int n_tables,
                                  const krs_feature* feats, const krs_feature* feats_host, int n_feats,
                                  const void* ids, int id_type, int batch, int64_t nnz, int64_t total_rows,
                                  void* workspace, size_t workspace_bytes, int* err_flag, void* stream);

/* Dense parity form: grad_tables[t].weights is the [vocab, dim] fp32 gradient
 * buffer of table t (krs_table array in device memory, same indexing and
 * row_base as `tables`).  Rows that are touched are OVERWRITTEN with their sum;
 * untouched rows are not written (caller zero-fills once). */
int krs_embed_bag_bwd_dense(const krs_table* grad_tables, int n_tables,
                            const krs_feature* feats, int n_feats,
                            const float* weights, const float* bag_scale,
                            const void* grad, int grad_dtype, int64_t grad_ld,
                            int batch, int dim, int64_t nnz,
                            const void* workspace, void* stream);

/* Fused SGD on the touched rows of tables[t].weights (dtype table_dtype). */
int krs_embed_bag_bwd_fused_sgd(const krs_table* tables, int n_tables,
                                const krs_feature* feats, int n_feats,
                                const float* weights, const float* bag_scale,
                                const void* grad, int grad_dtype, int64_t grad_ld,
                                int batch, int dim, int table_dtype, int64_t nnz,
                                const void* workspace, void* stream);

/* Fused Adagrad on the touched rows (tables[t].slot = fp32 accumulator). */
int krs_embed_bag_bwd_fused_adagrad(const krs_table* tables, int n_tables,
                                    const krs_feature* feats, int n_feats,
                                    const float* weights, const float* bag_scale,
                                    const void* grad, int grad_dtype, int64_t grad_ld,
                                    int batch, int dim, int table_dtype, int64_t nnz,
                                    const void* workspace, void* stream);

/* Row-wise Adagrad on the touched rows -- an OPT-IN variant, not the reference's rule (the FBGEMM / TorchRec
 * "rowwise_adagrad" form, no epsilon): acc[row] += mean_j g[row, j]^2;  w[row, j] -= lr * g[row, j] / sqrt(acc[row]).
 * tables[t].slot = fp32 [vocab]: ONE accumulator per row (the exact form keeps [vocab, dim], which is two
 * thirds of K2's HBM traffic at C3: 2 x dim x 4 bytes per touched row against 8 here). */
int krs_embed_bag_bwd_fused_adagrad_rowwise(const krs_table* tables, int n_tables,
                                            const krs_feature* feats, int n_feats,
                                            const float* weights, const float* bag_scale,
                                            const void* grad, int grad_dtype, int64_t grad_ld,
                                            int batch, int dim, int table_dtype, int64_t nnz,
                                            const void* workspace, void* stream);

/* Fused Adam on the touched rows ("lazy": a row that is not looked up keeps its moments and its
 * value).  The reference names keras.optimizers.Adam for 'sparsecore' tables and hands
 * (learning_rate, beta_1, beta_2, epsilon) to the SparseCore library
 * (embedding/jax/config_conversion.py:256-265; amsgrad unsupported); the arithmetic restated here
 * is Keras' Adam.update_step:
 *   m += (g - m)(1 - beta_1);  v += (g*g - v)(1 - beta_2);
 *   w -= lr * bias_correction * m / (sqrt(v) + epsilon),
 *   bias_correction = sqrt(1 - beta_2^t) / (1 - beta_1^t), t = 1-based step count (host side).
 * tables[t].slot = fp32 [2][vocab][dim]: m then v.  tables[t].lr = learning rate. */
int krs_embed_bag_bwd_fused_adam(const krs_table* tables, int n_tables,
                                 const krs_feature* feats, int n_feats,
                                 const float* weights, const float* bag_scale,
                                 const void* grad, int grad_dtype, int64_t grad_ld,
                                 int batch, int dim, int table_dtype, int64_t nnz,
                                 float beta_1, float beta_2, float epsilon, float bias_correction,
                                 const void* workspace, void* stream);

/* Fused FTRL on the touched rows: keras.optimizers.Ftrl.update_step with the options the
 * reference supports (embedding/jax/config_conversion.py:266-283: learning_rate_power, l1, l2,
 * beta, initial_accumulator_value; no l2 shrinkage):
 *   n' = n + g*g;  z += g - (n'^-p - n^-p) / lr * w;
 *   w = (clip(z, -l1, l1) - z) / (n'^-p / lr + 2*(l2 + beta / (2 lr)));  n = n'.
 * tables[t].slot = fp32 [2][vocab][dim]: accumulator n then linear z. */
int krs_embed_bag_bwd_fused_ftrl(const krs_table* tables, int n_tables,
                                 const krs_feature* feats, int n_feats,
                                 const float* weights, const float* bag_scale,
                                 const void* grad, int grad_dtype, int64_t grad_ld,
                                 int batch, int dim, int table_dtype, int64_t nnz,
                                 float learning_rate_power, float l1, float l2, float beta,
                                 const void* workspace, void* stream);

/* krs_embed_bag_bwd_fused_adam with the bias-correction factor read from DEVICE memory when the kernel runs
 * (*bias_correction_dev, one float): the form a step replayed from a HIP graph needs -- a by-value argument is frozen
 * into the captured launch, the device float is rewritten before every replay (krs_store_f32).  The layers use this
 * entry for eager steps as well, so both kinds of step run one code path. */
int krs_embed_bag_bwd_fused_adam_dyn(const krs_table* tables, int n_tables,
                                     const krs_feature* feats, int n_feats,
                                     const float* weights, const float* bag_scale,
                                     const void* grad, int grad_dtype, int64_t grad_ld,
                                     int batch, int dim, int table_dtype, int64_t nnz,
                                     float beta_1, float beta_2, float epsilon, const float* bias_correction_dev,
                                     const void* workspace, void* stream);

/* Step-dependent optimizer constants (scheduled learning rates, Adam's bias correction) -> device memory without a copy
 * from the host: values_host[0..count) are read NOW (on the calling thread) and travel as kernel arguments; the kernel
 * stores value i at (char*)dst + i * stride_bytes.  stride_bytes = sizeof(krs_table) with dst = &tables[0].lr rewrites the
 * learning rates of a descriptor array in place; stride 4 fills a float array.  No page-locked buffer the host could
 * overwrite too early, no wait: ordered on `stream` like any launch, so an eager call placed before a graph replay on the
 * same stream is seen by that replay and not by the one before it.  The reference evaluates schedules on the host every
 * step too (jax/config_conversion.py:136-176: callable learning rates). */
int krs_store_f32(void* dst, int64_t stride_bytes, const float* values_host, int count, void* stream);

/* Sparse form: unique global rows and their summed gradients.
 *   unique_rows [nnz] int64 (first *n_unique valid), row_grads [nnz, dim] fp32,
 *   n_unique device int64.
 * Needs the plan of krs_embed_bag_bwd_plan (global sort).  A workspace holding the plan of
 * krs_embed_bag_bwd_plan_tables yields *n_unique = -1 (unique_rows / row_grads are then meaningless; the
 * workspace itself records which sort filled it, so the answer follows a plan copied to another address). */
int krs_embed_bag_bwd_sparse(const krs_feature* feats, int n_feats,
                             const float* weights, const float* bag_scale,
                             const void* grad, int grad_dtype, int64_t grad_ld,
                             int batch, int dim, int64_t nnz,
                             const void* workspace,
                             int64_t* unique_rows, float* row_grads, int64_t* n_unique,
                             void* stream);

/* ------------------------------------------------------------------------- *
 * K3  FeatureCross (DCN-v2 cross layer)
 *
 * Replaces FeatureCross.call, feature_cross.py:182-194:
 *   u = act(h @ kernel + bias)            keras Dense inside the layer (:134-151)
 *   u = cast(u, compute dtype); u += diag_scale * x   (:189-192)
 *   y = x0 * u + x                         (:194)
 * with h = x (full rank) or h = x @ down_kernel (low rank, :185-187).
 *
 * krs_gemm: C[M,N] = epilogue(A[M,K] @ B), the MFMA kernel that owns the dense
 * projection.  B is given K-contiguous ("B transposed", Bt[N,K]) when
 * b_is_nk != 0, else as the keras kernel layout B[K,N].  Likewise a_is_km != 0
 * means A is given as At[K,M] (the weight-gradient contractions over the
 * batch).  Epilogue, applied on the fp32 accumulator v of element (m,n):
 *      v += bias[n]                (bias != NULL)
 *      v  = act(v)
 *      v  = x0[m,n] * (v + diag_scale * x[m,n]) + x[m,n]   (x0 != NULL: cross)
 *      v += beta * R[m,n]          (R != NULL: residual / gradient accumulate)
 *   u_out (optional, cross form only) receives v = act(A@B + bias), the
 *   activation output the backward needs (dx0 = g*(v + diag_scale*x), act'(v)).
 * ------------------------------------------------------------------------- */
typedef struct krs_gemm_epilogue {
  const float* bias;  /* [N] fp32 or NULL */
  int32_t act;        /* krs_activation */
  float diag_scale;
  const void* x0;     /* [M,N] (dtype of C) or NULL */
  const void* x;      /* [M,N] (dtype of C), required when x0 != NULL */
  int64_t ldx;        /* row stride of x0 and x */
  void* u_out;        /* [M,N] (dtype of C) or NULL */
  int64_t ldu;
  const void* r;      /* [M,N] (dtype of C) or NULL */
  int64_t ldr;
  float beta;
} krs_gemm_epilogue;

int krs_gemm(const void* a, int64_t lda, int a_is_km,
             const void* b, int64_t ldb, int b_is_nk,
             void* c, int64_t ldc,
             int64_t m, int64_t n, int64_t k,
             int in_dtype, int out_dtype,
             const krs_gemm_epilogue* epilogue,
             void* workspace, size_t workspace_bytes, void* stream);
/* Bytes of `workspace` a krs_gemm call of this shape needs (0 = none): split-K products keep one fp32 [M, N] slab per
 * split and reduce them in a fixed order (deterministic, no atomics) -- the weight-gradient contractions over the batch
 * (a_is_km), and since round 5 K-contiguous products whose output is too small for 256 x 256 tiles to fill the chip but
 * whose K is long (M = 8192 against N = 512, K = 3456: the per-rank products of a strongly-scaled job).  The figure is the
 * largest need over the input dtypes and B layouts (which the query does not see): enough for every call of this shape.  A
 * split call with less workspace than ITS need returns KRS_ERR_WORKSPACE. */
size_t krs_gemm_workspace_bytes(int64_t m, int64_t n, int64_t k, int a_is_km);

/* Data-gradient product of a cross layer FUSED with the elementwise backward of the cross layer below it in a stack
 * on one x0 (`xl = layer(x0, xl)` repeated, examples/ml_perf/model.py:332-336; gradients of feature_cross.py:182-194):
 *      G   = A[M,K] @ Bt[N,K]^T [+ beta * R]          dL/dx of the upper layer = dL/dy of the lower one (stored;
 *                                                      R == NULL: no residual -- the layer above is a Dense layer)
 *      dz  = G * x0 * act'(u)                          d(pre-activation) of the lower layer   (act' from its saved output u)
 *      dx0 = [dx0 +] G * u [+ G]                       its term of dL/dx0 (dx0_accumulate != 0: added to what dx0 holds;
 *                                                      fold_direct != 0: the lower layer's x IS x0, so the direct term
 *                                                      joins, the `dxd == dx0` rule of krs_cross_epilogue_bwd)
 *                                                      u_upper != NULL (needs R, beta = 1, dx0_accumulate = 0): the term of
 *                                                      the layer ABOVE joins here, dx0 = R * u_upper + G * u [+ G] -- R is its
 *                                                      dL/dy, u_upper its saved activation output; that layer then writes
 *                                                      no dL/dx0 of its own and this sum is rounded once, not twice)
 *                                                      dx0 == NULL (R == NULL form only): nothing is written -- the caller
 *                                                      passes u as the u_upper of the NEXT launch, whose R is this G
 *      dbias[n] = sum_m dz[m,n]                        fp32, fixed summation order (NULL: not wanted)
 * i.e. exactly krs_gemm(A, Bt, epilogue{r = R, beta}) followed by krs_cross_epilogue_bwd(g = G, u, x0, diag_scale = 0),
 * with G, dz and dx0 BIT-IDENTICAL to those two calls (dz and dx0 are computed from G as it is stored, after its one
 * rounding) -- without the second pass reading G, x0 and u back and with the streams written by the product's epilogue.
 * Row stride `ld` for x0, u, dz and dx0; workspace: krs_gemm_cross_bwd_workspace_bytes(m, n) when dbias is wanted.
 * bf16 tiles the 256x256 ring kernel covers run fused; every other shape / dtype runs the two calls (needs ldg == ld).
 * x0, u, dz and g_out are required (krs_gemm_dense_bwd is the form for a Dense layer below). */
size_t krs_gemm_cross_bwd_workspace_bytes(int64_t m, int64_t n);
int krs_gemm_cross_bwd(const void* a, int64_t lda, const void* bt, int64_t ldb,
                       const void* r, int64_t ldr, float beta,
                       void* g_out, int64_t ldg,
                       const void* x0, const void* u, void* dz, void* dx0, int64_t ld, int dx0_accumulate,
                       const void* u_upper, int fold_direct, float* dbias, int64_t m, int64_t n, int64_t k, int act, int dtype,
                       void* workspace, size_t workspace_bytes, void* stream);
/* The same fusion when the layer below is a Dense layer (examples/ml_perf/model.py:214-262) with saved output y:
 *      G   = A[M,K] @ Bt[N,K]^T,  dz = G * act'(y),  dbias[n] = sum_m dz[m,n]  (fp32, fixed order; NULL: not wanted)
 * g_out != NULL: G is stored there by every route (it is the true dL/dy of the lower layer's output, what autograd must
 * hand to anyone who observes that output); g_out == NULL: G is not stored by the fused route, and the two-call route
 * lands it in dz's buffer and applies the derivative in place -- the launch then streams y in and dz out where krs_gemm +
 * krs_dense_act_bwd write G, read G and y and write dz.  G and dz are bit-identical to those two calls (one rounding of
 * G, then the derivative).  Row stride `ld` for y and dz; same routes, gate and workspace
 * (krs_gemm_cross_bwd_workspace_bytes) as krs_gemm_cross_bwd. */
int krs_gemm_dense_bwd(const void* a, int64_t lda, const void* bt, int64_t ldb, void* g_out, int64_t ldg,
                       const void* y, void* dz, int64_t ld, float* dbias, int64_t m, int64_t n, int64_t k, int act,
                       int dtype, void* workspace, size_t workspace_bytes, void* stream);
/* Diagnostic, host only: the route the CALLING THREAD's last krs_gemm_cross_bwd / krs_gemm_dense_bwd took --
 * KRS_CROSS_BWD_NONE (no call yet, a refused call, or m == 0 / n == 0), KRS_CROSS_BWD_TWO_CALL (krs_gemm + the elementwise
 * pass), KRS_CROSS_BWD_PP64 / KRS_CROSS_BWD_PP256 (fused, on gemm_pp64_kernel / gemm_pp256_kernel).  *epilogue (if not
 * NULL) receives the fused epilogue number (3 .. 10: 9 = the dense form without G, 10 = with G), 0 for the other routes.
 * Lets tests prove which path they exercised. */
enum { KRS_CROSS_BWD_NONE = 0, KRS_CROSS_BWD_TWO_CALL = 1, KRS_CROSS_BWD_PP64 = 2, KRS_CROSS_BWD_PP256 = 3 };
int krs_gemm_cross_bwd_last_route(int* epilogue);
/* Diagnostic, host only, no GPU needed: the route krs_gemm_cross_bwd WOULD take for these arguments (those of
 * krs_gemm_cross_bwd up to `dtype`, without fold_direct, dbias and act, which no route depends on) under the pipeline option
 * in force; x0 == NULL asks for the dense form, krs_gemm_dense_bwd with y = u.  Pointer values are read for their alignment
 * only; nothing is dereferenced or launched and the last-route record is untouched.  Returns KRS_CROSS_BWD_* (or a negative
 * krs_status for arguments the entry refuses); *epilogue (if not NULL) receives the fused epilogue number, else 0. */
int krs_gemm_cross_bwd_plan_route(const void* a, int64_t lda, const void* bt, int64_t ldb, const void* r, int64_t ldr,
                                  float beta, void* g_out, int64_t ldg, const void* x0, const void* u, void* dz, void* dx0,
                                  int64_t ld, int dx0_accumulate, const void* u_upper, int64_t m, int64_t n, int64_t k,
                                  int dtype, int* epilogue);

/* Diagnostic, host only: where the CALLING THREAD's last krs_gemm ran.  Every field is 0 when there was no call yet, the
 * call was refused (any return other than KRS_OK) or had nothing to do (m == 0 or n == 0).
 *   kernel      KRS_GEMM_KERNEL_*: the kernel family that formed the products (gemm_generic_kernel, gemm_mfma_kernel,
 *               gemm_glds_kernel, gemm_tn_glds_kernel, gemm_pp256_kernel on K-contiguous / on K-strided operands,
 *               gemm_pp64_kernel, gemm_thin_kernel, gemm_rowdot_kernel, gemm_smallk_kernel)
 *   splits      workgroups along K per output tile (1 = no split-K)
 *   reduce      KRS_GEMM_REDUCE_*: the slab-reduce kernel that followed a split product (gemm_slab_reduce_kernel,
 *               gemm_slab_reduce_vec4_kernel, gemm_slab_reduce_vec8_kernel)
 *   epilogue    epilogue build of the tile kernel: 0 = general, 1 = cross, 2 = residual (bf16 output, unsplit)
 *   ep_vec      1 when every epilogue operand allowed 8-wide vector access
 *   thin_width  gemm_thin_kernel only: its width build (1, 4, 8, 16), else 0
 *   thin_is_a   gemm_thin_kernel only: 1 when A was the thin operand (m <= n), 0 when B was
 *   schedule    gemm_pp64_kernel with epilogue build 1 or 2 only, else 0: KRS_GEMM_SCHED_* bits of the epilogue schedule
 *               the launch took under KRS_GEMM_OPT_EPI_SCHEDULE -- LDS_LANDING (cross build: chunk 2 of x0 / x lands in the
 *               dead ring LDS), X_IS_X0 (cross build with x == x0: the operand is loaded once, all four chunks under the
 *               main loop's tail), STAGGER (rotated tile order of odd M panels and a half-period start offset of every
 *               other first-round workgroup).  `epilogue` stays 1 for every cross build: the arithmetic is one.
 * The two-call form of krs_gemm_cross_bwd / krs_gemm_dense_bwd runs krs_gemm's body and therefore leaves a record too;
 * their fused form does not touch it.  Returns `kernel`; `route` may be NULL.  Lets tests prove which kernel they ran. */
enum {
  KRS_GEMM_KERNEL_NONE = 0, KRS_GEMM_KERNEL_GENERIC = 1, KRS_GEMM_KERNEL_MFMA = 2, KRS_GEMM_KERNEL_GLDS = 3,
  KRS_GEMM_KERNEL_TN_GLDS = 4, KRS_GEMM_KERNEL_PP256 = 5, KRS_GEMM_KERNEL_PP256_KSTRIDED = 6, KRS_GEMM_KERNEL_PP64 = 7,
  KRS_GEMM_KERNEL_THIN = 8, KRS_GEMM_KERNEL_ROWDOT = 9, KRS_GEMM_KERNEL_SMALLK = 10
};
enum { KRS_GEMM_REDUCE_NONE = 0, KRS_GEMM_REDUCE_SCALAR = 1, KRS_GEMM_REDUCE_VEC4 = 2, KRS_GEMM_REDUCE_VEC8 = 3 };
typedef struct krs_gemm_route {
  int32_t kernel;
  int32_t splits;
  int32_t reduce;
  int32_t epilogue;
  int32_t ep_vec;
  int32_t thin_width;
  int32_t thin_is_a;
  int32_t schedule;
} krs_gemm_route;
enum { KRS_GEMM_SCHED_LDS_LANDING = 1, KRS_GEMM_SCHED_STAGGER = 2, KRS_GEMM_SCHED_X_IS_X0 = 4 };
int krs_gemm_last_route(krs_gemm_route* route);
/* Diagnostic, host only, no GPU needed: where a krs_gemm with these arguments (krs_gemm's, without the workspace pointer
 * and the stream) WOULD run under the pipeline option in force.  The decision is a pure function of sizes, strides, dtypes,
 * the 16-byte alignment of the pointer VALUES and the epilogue struct (read from host memory); no operand is dereferenced,
 * no HIP call is made and the last-route record is untouched.  Fills *route (all zero when nothing would be launched) and
 * returns what krs_gemm returns before its first launch: KRS_OK, KRS_ERR_INVALID, KRS_ERR_WORKSPACE (a split product with
 * fewer than its slab bytes) or KRS_ERR_UNSUPPORTED (a grid beyond the launch limits). */
int krs_gemm_plan_route(const void* a, int64_t lda, int a_is_km, const void* b, int64_t ldb, int b_is_nk, const void* c,
                        int64_t ldc, int64_t m, int64_t n, int64_t k, int in_dtype, int out_dtype,
                        const krs_gemm_epilogue* epilogue, size_t workspace_bytes, krs_gemm_route* route);

/* Tuning / diagnostic switches of krs_gemm (process-wide; results never depend on them).
 *   KRS_GEMM_OPT_PIPELINE: 4 = the big bf16 shapes run the four-stage ping-pong ring on 256x256 tiles (default, or
 *   the environment variable KRS_GEMM_PIPE at first use); 0 = every shape runs the two-stage 128x128 kernels and
 *   krs_gemm_cross_bwd its two-call form -- the reference schedule of the bit-for-bit tests and A/B harnesses.
 *   5 = the 32-k ring (gemm_pp256_kernel) also for the K-contiguous products that take the 64-k ring (gemm_pp64_kernel) by
 *   default: the A/B switch of round 6.
 *   (Rounds 2-4 used 5 / 6 / 7 for a five-stage ring, a prefetch schedule and a deep ring on 128x128 tiles; measured no
 *   faster and deleted in round 5.)
 *   KRS_GEMM_OPT_EPI_SCHEDULE (or the environment variable KRS_GEMM_EPI_SCHEDULE at first use): how gemm_pp64_kernel's
 *   streaming epilogues (cross, residual, fused cross backward) request their operands and order their tiles --
 *   0 = two chunks of x0 / x ahead, every workgroup starts at once, tiles in panel order: the reference schedule;
 *   1 = (default) the cross build keeps its bias in registers, lands chunk 2 of x0 / x in the dead ring LDS and asks for
 *       chunk 3 one chunk earlier, and a call with x == x0 takes a build that loads the operand once;
 *   2 = stagger: odd M panels start half way round their N tiles and every other workgroup of the first round starts
 *       half a tile period late, so that epilogues of some CUs meet main loops of others;
 *   3 = both; -1 = back to the default (the environment variable, else the built-in value).  Which tile a workgroup
 *   computes and when an operand is requested change speed only, never a bit. */
enum { KRS_GEMM_OPT_PIPELINE = 0, KRS_GEMM_OPT_EPI_SCHEDULE = 1 };
int krs_gemm_set_option(int key, int value);

/* Tuning switches of krs_embed_bag_fwd / krs_embed_bag_bwd_* (process-wide; results never depend on them).
 *   KRS_EMBED_OPT_PLAN: krs_embed_bag_bwd_plan_tables -- 0 = table-segmented sort where the layout allows it
 *   (default), 1 = always the global sort (A/B).
 *   KRS_EMBED_OPT_RANK: how the plan's scatter passes rank the keys of a round of 64 -- 0 = from the wave's LDS digit
 *   counters (a no-return add between two reads), one ballot per collided group, and one ballot per digit bit only
 *   for a round with more possible groups than bits (default); 1 = always one ballot per digit bit (A/B); 2 = always
 *   from the counters.  The three give the same plan, bit for bit.
 *   KRS_EMBED_OPT_HOTROWS: LDS staging of hot embedding rows in the pooled gather -- 0 = off (default), 64 / 128 =
 *   rows 0 .. n-1 of a workgroup's table are copied to LDS and lookups of them are served from there (one flat
 *   16-byte load per lookup, routed to LDS or memory by its address); pays only when ids are relabelled
 *   hot-first and those rows are NOT already cache hits (profiles/r3_k1_hot_rows_lds.txt: they are).
 *   KRS_EMBED_OPT_APPLY_DEPTH: how krs_embed_bag_bwd_* fetch the rest of a table row's segment beyond its first two
 *   lookups -- 0 = four gradient rows per trip, each trip a load of the lookups' values and then the gathers (A/B, and
 *   the reference of the bit-for-bit test); 4 (default) / 8 / 16 = the deep front: sixteen values in one coalesced
 *   load requested with the row, that many gradient rows requested together, the next values requested before these
 *   rows are summed.  Same bytes, same order of additions: the four give the same bits; 4 is the fastest at the
 *   benchmark's shape (profiles/k2_apply_depth_ab.txt).
 *   (Keys 0 and 1 -- the one-hot gather variants and the round-1 per-segment backward kernel -- were retired in
 *   round 5 with the kernels they selected; they are refused.) */
enum { KRS_EMBED_OPT_PLAN = 2, KRS_EMBED_OPT_HOTROWS = 3, KRS_EMBED_OPT_RANK = 4, KRS_EMBED_OPT_APPLY_DEPTH = 5 };
int krs_embed_set_option(int key, int value);

/* Elementwise halves of FeatureCross for the host-composed path (arbitrary
 * pre_activation callables) and for the backward:
 *   fwd: y = x0 * (u + diag_scale*x) + x                     feature_cross.py:191-194
 *   bwd: given g = dL/dy and u = act(z) (z = h@K+b):
 *        dx0 (+)= g * (u + diag_scale*x)
 *        dxd = g + diag_scale * g*x0      (the non-GEMM part of dL/dx)
 *              dxd == dx0 (same pointer) is the case "x is x0": dx0 then
 *              receives the sum of both lines and nothing else is written
 *        du  = dz = g*x0 * act'(z), act' written through u (relu: u>0,
 *              sigmoid: u(1-u), tanh: 1-u^2)
 *        dbias[n] = sum_m dz[m,n]         (optional)
 * Bias gradients (here, krs_dense_act_bwd, krs_colsum) are column sums over all m rows.  With a workspace of
 * krs_colsum_workspace_bytes(m, n) bytes they are formed in two stages -- per row group, then over the groups in
 * order -- and come out with the same bits on every run; with workspace == NULL the groups are added with fp32
 * atomics, whose order (and so the last bits) varies from run to run. */
size_t krs_colsum_workspace_bytes(int64_t m, int64_t n);
int krs_cross_epilogue_fwd(const void* u, const void* x0, const void* x, void* y,
                           int64_t m, int64_t n, int64_t ld, float diag_scale,
                           int dtype, void* stream);
int krs_cross_epilogue_bwd(const void* g, const void* u, const void* x0, const void* x,
                           void* du, void* dx0, int dx0_accumulate, void* dxd,
                           float* dbias,
                           int64_t m, int64_t n, int64_t ld, float diag_scale, int act,
                           int dtype, void* workspace, size_t workspace_bytes, void* stream);

/* Weight preparation for the two GEMM layouts of a Dense / FeatureCross step: dst [rows, cols] = cast(src) and
 * dst_t [cols, rows] = cast(src)^T, either may be NULL.  What `ops.cast(kernel, compute_dtype)` +
 * a transposed copy do on the host side of feature_cross.py:182-194 under a mixed-precision policy, in one
 * launch (bf16 rounding: round-to-nearest-even, as everywhere in this library). */
int krs_cast_transpose(const void* src, int64_t rows, int64_t cols, int64_t ld_src, int src_dtype,
                       void* dst, int64_t ld_dst, void* dst_t, int64_t ld_dst_t, int dst_dtype,
                       void* stream);
/* The same for several contiguous weights in ONE launch (the bf16 copies of every dense kernel of a model, refreshed
 * behind the optimizer step): srcs[i] is [rows[i], cols[i]] row-major, dsts[i] (same shape) and / or dst_ts[i]
 * ([cols[i], rows[i]]) receive the cast copy / its transpose; either output pointer of a tensor may be NULL. */
int krs_cast_transpose_many(int count, const void* const* srcs, const int64_t* rows, const int64_t* cols,
                            int src_dtype, void* const* dsts, void* const* dst_ts, int dst_dtype, void* stream);

/* Backward of the bias + activation epilogue of a Dense layer (keras.layers.Dense inside the DLRM MLP blocks,
 * examples/ml_perf/model.py:214-262): dz [m,n] = g * act'(y) with the derivative taken from the saved output y
 * (relu: y > 0; sigmoid: y(1-y); tanh: 1-y^2; none: 1, y may be NULL) and dbias [n] = column sums of dz (fp32).
 * dz or dbias may be NULL. */
int krs_dense_act_bwd(const void* g, int64_t ld_g, const void* y, int64_t ld_y, void* dz, int64_t ld_dz,
                      float* dbias, int64_t m, int64_t n, int act, int dtype, void* workspace,
                      size_t workspace_bytes, void* stream);

/* Adagrad step on a list of dense fp32 weights (the FeatureCross / Dense kernels and biases of one training step) in
 * one launch: acc += g*g; p -= lr * g / (sqrt(acc) + eps).  params / grads / accs / sizes: HOST arrays of `count`
 * device pointers and element counts.  The optimizer the ml_perf example attaches to the dense part
 * (examples/ml_perf/main.py: keras.optimizers.Adagrad, learning rate of configs/v6e_8.py); the fused table
 * optimizers are K2's. */
int krs_dense_adagrad(float* const* params, const float* const* grads, float* const* accs,
                      const int64_t* sizes, int count, float lr, float eps, void* stream);

/* Column sum: out[n] = sum_m a[m,n] (fp32 out).  Dense bias gradient. */
int krs_colsum(const void* a, int64_t lda, int64_t m, int64_t n, int dtype,
               float* out, void* workspace, size_t workspace_bytes, void* stream);

/* Diagnostic, host only: how the CALLING THREAD's last krs_cross_epilogue_fwd / _bwd, krs_dense_act_bwd or krs_colsum
 * walked its operand (csrc/dense_walk_plan.h, the one planner of the four entries and of krs_colsum_workspace_bytes).
 * Every field is 0 when there was no call yet, the call was refused (any return other than KRS_OK) or had nothing to do
 * (m == 0 or n == 0).
 *   kernel          KRS_DENSE_WALK_VEC: a thread owns v adjacent columns and moves them in 16 bytes (n and every leading
 *                   dimension a multiple of v, every non-null operand on 16 bytes); KRS_DENSE_WALK_SCALAR otherwise
 *   v               columns a thread owns: 4 (fp32) or 8 (bf16) on the vector kernels, 1 on the scalar ones
 *   acc             krs_cross_epilogue_bwd, vector kernel: the ACC build (dx0 given with dx0_accumulate)
 *   two_stage       the column sums went through the workspace and colsum_finish_kernel (run-to-run identical bits);
 *                   0: fp32 atomics, or no column sums were asked for
 *   rows_per_block  consecutive rows one wave (vector) / one workgroup (scalar) walks: a chunk
 *   strips          grid.x: strips of 64 threads (64 * v columns)
 *   chunks          row chunks: rows_per_block * chunks >= m > rows_per_block * (chunks - 1)
 *   grid_y          grid.y, and the rows of partial sums in the workspace: ceil(chunks / 4) on the vector kernels (one
 *                   chunk per wave), chunks on the scalar ones
 * krs_cross_epilogue_fwd has no row walk: it records kernel and v alone.
 * Returns `kernel`; `route` may be NULL.  Lets tests prove which kernel they ran. */
enum { KRS_DENSE_WALK_NONE = 0, KRS_DENSE_WALK_VEC, KRS_DENSE_WALK_SCALAR };
enum { KRS_DENSE_WALK_CROSS_FWD = 0, KRS_DENSE_WALK_CROSS_BWD, KRS_DENSE_WALK_DENSE_ACT_BWD, KRS_DENSE_WALK_COLSUM };
typedef struct krs_dense_walk_route {
  int32_t kernel, v, acc, two_stage, rows_per_block, reserved;
  int64_t strips, chunks, grid_y;
} krs_dense_walk_route;
int krs_dense_walk_last_route(krs_dense_walk_route* route);
/* Diagnostic, host only, no GPU needed: how entry `entry` (KRS_DENSE_WALK_CROSS_FWD ...) WOULD walk an [m, n] operand
 * of `dtype`.  ld: host array of the n_ld leading dimensions of the call's non-null matrices (krs_colsum: none, its lda
 * takes no part); ptrs: host array of its n_ptrs matrix operands, read as VALUES only (alignment; NULL entries are
 * skipped).  want_dbias / has_workspace: whether column sums are asked for (always, on krs_colsum) and a workspace is
 * given; dx0_accumulate: krs_cross_epilogue_bwd with dx0 != NULL and the flag set.  No HIP call is made and the
 * last-route record is untouched.  Fills *route (all zero when nothing would be launched) and returns what the entry
 * returns for these sizes before its first launch: KRS_OK, KRS_ERR_INVALID (a negative size, a leading dimension below
 * n, a bad dtype or entry) or KRS_ERR_UNSUPPORTED (m above 2^31 - 1). */
int krs_dense_walk_plan_route(int entry, int64_t m, int64_t n, int dtype, const int64_t* ld, int n_ld,
                              const void* const* ptrs, int n_ptrs, int want_dbias, int has_workspace,
                              int dx0_accumulate, krs_dense_walk_route* route);

/* ------------------------------------------------------------------------- *
 * K4  DotInteraction
 *
 * Replaces DotInteraction.call, dot_interaction.py:170-203: stack F features
 * [B,D] -> X[B,F,D]; P = X X^T; then either the row-major strictly/inclusive
 * lower triangle gather (indices of :118-132) or the masked flatten (:96-116).
 * feats: HOST array of F device pointers, feature f is [batch, dim] with row
 * stride ld[f] (views into one concat buffer are fine).
 *   out [batch, out_cols], out_cols = F*F (skip_gather) | F(F+1)/2 | F(F-1)/2
 * Backward: dX[b,i,:] = sum_j (G[b,i,j] + G[b,j,i]) X[b,j,:], G = the gradient
 * scattered back to [F,F] (zero above / on the masked part).
 * Any F (the reference has no limit): the MFMA path covers F <= 32 with 16-B aligned rows, one plain launch
 * F <= 64, beyond that one launch per (32 features i, 128 features j) block pair.  accumulate_mask addresses the
 * first 64 features.
 * ------------------------------------------------------------------------- */
int krs_dot_interaction_fwd(const void* const* feats, const int64_t* ld, int n_feats,
                            int64_t batch, int dim, int dtype,
                            int self_interaction, int skip_gather,
                            void* out, int64_t out_ld, void* stream);
int krs_dot_interaction_bwd(const void* const* feats, const int64_t* ld, int n_feats,
                            int64_t batch, int dim, int dtype,
                            int self_interaction, int skip_gather,
                            const void* grad_out, int64_t grad_ld,
                            void* const* grad_feats, const int64_t* grad_feat_ld,
                            void* stream);
/* The same with gradients that are already there: feature f with bit f of accumulate_mask set receives
 * grad_feats[f] + dX[f] (fp32 sum of the stored value and the new term, one rounding); the others are
 * overwritten.  Lets the gradient of the interaction join a gradient buffer the features' other consumer has
 * already written (the concat of the same features: examples/ml_perf/model.py:204-207) without a separate add. */
int krs_dot_interaction_bwd_accumulate(const void* const* feats, const int64_t* ld, int n_feats,
                                       int64_t batch, int dim, int dtype,
                                       int self_interaction, int skip_gather,
                                       const void* grad_out, int64_t grad_ld,
                                       void* const* grad_feats, const int64_t* grad_feat_ld,
                                       uint64_t accumulate_mask, void* stream);

/* Diagnostic, host only: where the CALLING THREAD's last krs_dot_interaction_fwd / _bwd / _bwd_accumulate ran.  Every
 * field is 0 when there was no call yet, the call was refused (any return other than KRS_OK) or had nothing to do
 * (batch == 0).
 *   kernel     KRS_DOT_*: dot_fwd_mfma_kernel, dot_fwd_generic_kernel, dot_fwd_block_kernel, dot_bwd_mfma_kernel,
 *              dot_bwd_valu_kernel, dot_bwd_generic_kernel, dot_bwd_block_kernel
 *   dtype      the krs_dtype of the features
 *   ks         forward MFMA only: k steps known at compile time, 8 (bf16, dim 128), 4 (bf16, dim 64) or 0 (run-time loop)
 *   fr         feature rows the build provides for: 32 on the MFMA kernels, 28 or 32 on the vector-ALU backward, 64 on
 *              the generic kernels, 0 (no limit) on the block kernels
 *   self       backward MFMA / vector ALU: the SELF build (self_interaction); 0 where the kernel reads the flag at run time
 *   multi      vector-ALU backward: the MULTI build (several samples per wave, or an [F, F] gradient of more columns
 *              than the one-sample build loads)
 *   acc        backward MFMA / vector ALU: the ACC build (accumulate_mask has a bit below n_feats)
 *   ng         backward MFMA / vector ALU: gradient elements each lane loads per sample group (64 * ng columns)
 *   lps_log2   vector-ALU backward: log2 of the lanes per sample (a lane owns two adjacent columns)
 *   spw        vector-ALU backward: samples per wave, 1 .. 16
 *   launches   kernel launches of the call: 1, or one per (32 features i, 128 features j) pair on the block kernels
 *   lds_bytes  dynamic LDS of the launch (the backward MFMA and vector-ALU kernels; never above 64 KiB)
 *   blocks     workgroups launched, summed over the launches
 * Returns `kernel`; `route` may be NULL.  Lets tests prove which kernel they ran. */
enum { KRS_DOT_NONE = 0, KRS_DOT_FWD_MFMA, KRS_DOT_FWD_GENERIC, KRS_DOT_FWD_BLOCK, KRS_DOT_BWD_MFMA, KRS_DOT_BWD_VALU,
       KRS_DOT_BWD_GENERIC, KRS_DOT_BWD_BLOCK };
typedef struct krs_dot_route {
  int32_t kernel, dtype, ks, fr, self, multi, acc, ng, lps_log2, spw, launches, lds_bytes;
  int64_t blocks;
} krs_dot_route;
int krs_dot_interaction_last_route(krs_dot_route* route);
/* Diagnostic, host only, no GPU needed: where a krs_dot_interaction_fwd (backward == 0: grad_out / grad_ld stand for out /
 * out_ld; grad_feats, grad_feat_ld and accumulate_mask are ignored) or a krs_dot_interaction_bwd_accumulate (backward != 0)
 * with these arguments WOULD run (csrc/dot_plan.h, the planner the entries themselves run; KRS_DOT_BWD_VALU in the
 * environment is honoured as they honour it).  The host tables feats, ld, grad_feats and grad_feat_ld are read; every
 * device pointer is read as a VALUE only (nullness, alignment): nothing is dereferenced on the device side, no HIP call
 * is made and the last-route record is untouched.  Fills *route (all zero when nothing would be launched) and returns
 * what the entry returns before its first launch: KRS_OK or KRS_ERR_INVALID (a null table or pointer, n_feats <= 0,
 * batch < 0, dim <= 0, a bad dtype). */
int krs_dot_interaction_plan_route(int backward, const void* const* feats, const int64_t* ld, int n_feats,
                                   int64_t batch, int dim, int dtype,
                                   int self_interaction, int skip_gather,
                                   const void* grad_out, int64_t grad_ld,
                                   void* const* grad_feats, const int64_t* grad_feat_ld,
                                   uint64_t accumulate_mask, krs_dot_route* route);

/* ------------------------------------------------------------------------- *
 * K5  MOD bucketise for row-sharded tables
 *
 * The reference shards rows MOD-N (sharding_strategy="MOD",
 * jax/embedding_utils.py:194; layout tensorflow/distributed_embedding.py:316-328):
 * global row r lives on shard r % n_shards at local row r / n_shards.
 * Stable counting sort of the nnz ids by destination shard:
 *   bucket_counts [n_shards] int64: ids per shard
 *   local_ids     [nnz] int32/int64 (id_type): ids[perm[i]] / n_shards, grouped by shard
 *   perm          [nnz] int32: source position of each bucketed id
 * ------------------------------------------------------------------------- */
size_t krs_mod_bucketize_workspace_bytes(int64_t nnz, int n_shards);
int krs_mod_bucketize(const void* ids, int id_type, int64_t nnz, int n_shards,
                      void* local_ids, int32_t* perm, int64_t* bucket_counts,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * K7  Binary cross-entropy of the DLRM head, forward + backward in one pass
 *
 * keras.losses.BinaryCrossentropy() as examples/ml_perf/main.py:201-210 compiles it (from_logits=False,
 * mean reduction) on the sigmoid output of the top MLP (examples/ml_perf/model.py:105-163):
 *   p = clip(pred, epsilon, 1 - epsilon);  loss = mean_i -(y_i log p_i + (1 - y_i) log(1 - p_i))
 *   dpred_i = grad_scale / n * ((1 - y_i) / (1 - p_i) - y_i / p_i), 0 where the clip is active
 * pred [n] fp32 / bf16 (contiguous), labels [n] fp32, loss = device scalar, dpred [n] in pred's dtype
 * (may be NULL: forward only).  partials: KRS_BCE_MAX_BLOCKS floats of scratch (device), or NULL = one workgroup
 * does all of it.  fp32 arithmetic, fixed summation order either way (deterministic for a given scratch choice).
 * ------------------------------------------------------------------------- */
#define KRS_BCE_MAX_BLOCKS 64
int krs_bce_fwd_bwd(const void* pred, int pred_dtype, const float* labels, int64_t n, float epsilon,
                    float grad_scale, float* loss, void* dpred, float* partials, void* stream);

/* ------------------------------------------------------------------------- *
 * K6  Row-sharded lookup: route / unpack / combine (the id side of the exchange)
 *
 * The reference's accelerated path hands per-partition id lists to the SparseCore library
 * (embedding.preprocess_sparse_dense_matmul_input, sharding_strategy="MOD":
 * jax/embedding_utils.py:144-217) and looks them up with tpu_sparse_dense_matmul
 * (jax/embedding_lookup.py:134-147).  Here the ranks exchange one PARTIALLY POOLED vector per
 * (bag, owner) pair (keras_rs_amd/sharded.py); these three calls are everything around the two
 * all-to-alls, each a fixed sequence of kernels on `stream` (no allocation, no host sync).
 *
 * krs_shard_route (home rank).  Lookups are given as for krs_embed_bag_fwd: ONE flat id buffer,
 * feature-major, dense bags (feats[f].hot ids per bag, feats[f].ids_base = first id of the feature)
 * or CSR (offsets[n_feats*batch + 1]).  Per lookup: id outside [0, feats[f].vocab) -> dropped,
 * KRS_FLAG_ID_OUT_OF_RANGE raised (never clamped); composite c = comp_off + id, owner = c % n_shards,
 * stacked local row = c / n_shards; stable grouping by owner; a SEGMENT = a run of one bag inside an
 * owner's bucket.  Outputs:
 *   packed   [<= nnz*(1 + emit_weights) + nnz] int32: per owner d, contiguously,
 *            [rows(lookups_d) | weights as fp32 bit patterns (lookups_d, only with emit_weights) |
 *             segment lengths (segments_d)]; weight = user weight x combiner scale of the bag
 *            (mean 1/sum w, sqrtn 1/sqrt(sum w^2), 0 where the divisor is 0: embed_reduce.py:255-274)
 *   seg_bag  [nnz] bag of every segment (first n_seg valid; segments are numbered in bucket order)
 *   seg_grow [nnz] row of the [batch*n_feats, dim] view of the output gradient the segment's partial
 *            takes in the backward: (bag % batch)*n_feats + bag / batch
 *   bag_seg  [n_feats*batch, n_shards] segment of (bag, owner), -1 where the bag has no lookup there
 *   counts   [3*n_shards] int64: lookups, segments, packed words per owner
 * emit_weights must be set when weights != NULL or any combiner is not KRS_SUM.
 * feats is the DEVICE copy of the descriptors, feats_host the same array on the host.
 *
 * krs_shard_unpack (owner rank): the packed blocks received from n_sources ranks (their `lookups` /
 * `segments` counts are HOST arrays), concatenated in source order -> rows[sum lookups],
 * w[sum lookups] (weighted != 0), offsets[sum segments + 1] (exclusive scan of the lengths): the CSR
 * form krs_embed_bag_fwd and the fused backward take.
 *
 * krs_shard_combine (home rank): out[b, f*dim + j] = sum over owners d of
 * partials[bag_seg[(f*batch + b)*n_shards + d]][j] (skipping -1), fp32 accumulation in ascending d,
 * one rounding to `dtype` (the dtype of partials and out).
 *
 * krs_publish_i64: copies src[0..n) to page-locked host memory (host_dst, device-visible) and then
 * writes `seq` to host_dst[n]; the host polls host_dst[n] instead of synchronising the stream.
 *
 * STATIC-CAPACITY form (krs_shard_route_static / krs_shard_unpack_static).  The reference makes every
 * buffer of the SparseCore exchange static with TableConfig.max_ids_per_partition /
 * max_unique_ids_per_partition (distributed_embedding_config.py:54-61), drops what does not fit
 * (allow_id_dropping=True, jax/embedding_utils.py:187-197) and learns better limits from running statistics
 * (update_stats, jax/distributed_embedding.py:657-664).  Same contract here: every (home, owner) pair
 * exchanges a block of fixed size, so the all-to-alls have equal splits and the host needs no count:
 *   block = [lookups kept, segments kept, need_l, need_s | rows[cap_lookups] |
 *            weights[cap_lookups] (only with emit_weights) | segment lengths[cap_segments]]   (int32 words;
 *            krs_shard_static_block_words() of them; unused slots are 0)
 * krs_shard_route_static writes n_shards such blocks into `packed`: owner d keeps the first cap_segments
 * segments of its bucket and of those the first cap_lookups lookups (a segment cut by the limit keeps its
 * head); anything dropped raises KRS_FLAG_CAPACITY_OVERFLOW in err_flag.  need_l / need_s = the largest
 * per-owner lookup / segment count of THIS call, repeated in every header (each rank learns every rank's
 * needs from the blocks it receives).  seg_grow is [n_shards*cap_segments] (gradient row of every segment
 * SLOT d*cap_segments + j; 0 for unused slots), bag_seg holds slots (-1 for no / dropped segment),
 * counts as in the exact form (before dropping).  Capacities must be multiples of 4.  When nothing
 * overflows, the kept lookups, their order and the segments are those of krs_shard_route.
 * krs_shard_unpack_static (owner): n_sources received blocks -> rows / w [n_sources*cap_lookups] (compact,
 * source order; the unused tail is row -1 / weight 0: outside every segment, and an invalid id for the
 * backward plan), offsets[n_sources*cap_segments + 1] (CSR over the segment SLOTS; unused slots are empty),
 * stats[4] (optional) = max need_l, max need_s over the sources, lookups, segments received.
 * ------------------------------------------------------------------------- */
typedef struct krs_shard_feature {
  int64_t ids_base;   /* dense bags: position of the feature's first id in `ids` */
  int64_t comp_off;   /* stacked local row offset of the feature's table, times n_shards */
  int32_t hot;        /* dense bags: ids per bag; ignored with CSR offsets */
  int32_t combiner;   /* krs_combiner */
  int32_t vocab;      /* valid ids are [0, vocab) */
  int32_t reserved;
} krs_shard_feature;

size_t krs_shard_route_workspace_bytes(int64_t nnz, int64_t n_bags, int n_shards);
int krs_shard_route(const krs_shard_feature* feats, const krs_shard_feature* feats_host, int n_feats,
                    const void* ids, int id_type, const void* offsets, int offset_type,
                    const float* weights, int64_t nnz, int batch, int n_shards, int emit_weights,
                    int32_t* packed, int32_t* seg_bag, int32_t* seg_grow, int32_t* bag_seg,
                    int64_t* counts, int32_t* err_flag,
                    void* workspace, size_t workspace_bytes, void* stream);
size_t krs_shard_unpack_workspace_bytes(int64_t total_segments);
int krs_shard_unpack(const int32_t* packed, int n_sources, const int64_t* lookups, const int64_t* segments,
                     int weighted, int32_t* rows, float* w, int32_t* offsets,
                     void* workspace, size_t workspace_bytes, void* stream);
int krs_shard_combine(const void* partials, const int32_t* bag_seg, int batch, int n_feats, int n_shards,
                      int dim, int dtype, void* out, int64_t out_ld, void* stream);
int64_t krs_shard_static_block_words(int64_t cap_lookups, int64_t cap_segments, int emit_weights);
int krs_shard_route_static(const krs_shard_feature* feats, const krs_shard_feature* feats_host, int n_feats,
                           const void* ids, int id_type, const void* offsets, int offset_type,
                           const float* weights, int64_t nnz, int batch, int n_shards, int emit_weights,
                           int64_t cap_lookups, int64_t cap_segments,
                           int32_t* packed, int32_t* seg_bag, int32_t* seg_grow, int32_t* bag_seg,
                           int64_t* counts, int32_t* err_flag,
                           void* workspace, size_t workspace_bytes, void* stream);
int krs_shard_unpack_static(const int32_t* packed, int n_sources, int64_t cap_lookups, int64_t cap_segments,
                            int weighted, int32_t* rows, float* w, int32_t* offsets, int64_t* stats,
                            void* workspace, size_t workspace_bytes, void* stream);
int krs_publish_i64(const int64_t* src, int n, int64_t* host_dst, int64_t seq, void* stream);

/* ---------------------------------------------------------------------------
 * K8 retrieval: exact row top-k and the fused score + top-k of
 * BruteForceRetrieval (brute_force_retrieval.py:126-148,
 * `top_k(matmul(query, candidates.T), k)`) and HardNegativeMining
 * (hard_negative_mining.py:43-94, `top_k(logits + labels * MAX_FLOAT)`).
 * Selection order, one total order: the fp32 key descending, then the index
 * ascending; -0.0 ranks as +0.0, NaN above +inf (torch.topk).  Rows come back
 * sorted in that order; results are bit-identical from call to call; no host
 * synchronisation (graph-capturable).  Returned keys / scores are the fp32
 * value (a NaN as the canonical quiet NaN, -0.0 as +0.0) rounded once to the
 * output dtype.  Indices and ids are int32.
 * ------------------------------------------------------------------------- */
/* Row top-k of X[rows, cols] (fp32 or bf16, row stride ld) on the key
 * x + boost_scale * boost, computed in fp32 (boost: same shape, dtype and
 * stride as X, or NULL).  out_idx [rows, k] int32 column indices; out_keys
 * [rows, k] fp32 keys or NULL.  1 <= k <= cols.  Workspace:
 * krs_topk_rows_workspace_bytes (0 for cols <= 2048). */
size_t krs_topk_rows_workspace_bytes(int64_t rows, int64_t cols, int k);
int krs_topk_rows(const void* x, const void* boost, float boost_scale, int64_t ld, int dtype,
                  int64_t rows, int64_t cols, int k, int32_t* out_idx, float* out_keys,
                  void* workspace, size_t workspace_bytes, void* stream);
/* Top-k of the scores Q[b, d] . C[n, d]^T per query row (both `dtype`, row
 * strides ldq / ldc in elements): out_scores [b, k] in `dtype` (or NULL),
 * out_ids [b, k] int32 = ids[index] when ids != NULL (int32 [n]), else the
 * candidate index.  bf16 multiplies on v_mfma_f32_32x32x16_bf16, fp32 on
 * v_mfma_f32_32x32x2_f32; the products accumulate in fp32.  k <= 128 and
 * d <= 512 run fused (the scores never leave the chip); other shapes run
 * krs_gemm into a query-chunked fp32 slab (<= about 1 GiB) and the
 * krs_topk_rows selection.  1 <= k <= n, d >= 1, b >= 0.  Workspace:
 * krs_retrieval_topk_workspace_bytes (always > 0 for b > 0). */
size_t krs_retrieval_topk_workspace_bytes(int64_t b, int64_t n, int64_t d, int k, int dtype);
int krs_retrieval_topk(const void* q, int64_t ldq, const void* c, int64_t ldc, const int32_t* ids,
                       int dtype, int64_t b, int64_t n, int64_t d, int k,
                       void* out_scores, int32_t* out_ids,
                       void* workspace, size_t workspace_bytes, void* stream);
/* KRS_RETRIEVAL_SLAB_BYTES in the environment, read on each call: a positive integer replaces the two-step path's slab
 * budget of 1 GiB (the fp32 score slab plus the selection lists of one query chunk) for krs_retrieval_topk and
 * krs_retrieval_topk_workspace_bytes; a chunk is never shorter than one query row.  A diagnostic: with a budget of a few
 * kilobytes a small call runs the chunk loop several times.  The size query and the call must see the same value.
 *
 * Diagnostic: where the calling thread's last krs_topk_rows, krs_retrieval_topk, krs_retrieval_topk_q8 or
 * krs_retrieval_mine ran, as planned by csrc/retrieval_plan.h (the planner the four entries themselves run).  All zero
 * after a refused call, a call with no query rows and before the first call.  (The probe of krs_retrieval_ivf is a
 * krs_retrieval_topk call and leaves its record; krs_retrieval_ivf plans its own scan and merge and records nothing.)
 *   kernel           KRS_RETR_FUSED   stage 1 (a 32-query tile against a candidate slice, row queues in LDS) and the merge
 *                                     of the S slice lists of each row
 *                    KRS_RETR_SLAB    krs_gemm into an fp32 slab of chunk_rows query rows, then the row selection, per chunk
 *                    KRS_RETR_ROWS    krs_topk_rows: the row selection alone
 *   variant          KRS_RETR_VARIANT_TOPK / _Q8 / _MINE / _ROWS: the entry
 *   es               bytes of an input element: 4, 2, or 1 (the int8 index)
 *   vec              FUSED: the VEC build of stage 1 (16-byte candidate loads: d * es and ldc * es multiples of 16, the
 *                    candidates on a 16-byte boundary); 0 = element loads
 *   S, qtiles, slice FUSED: candidate slices (a multiple of 8), query tiles of 32 rows, candidates per slice (a multiple
 *                    of 128); S * slice >= n
 *   row_bytes        FUSED: K extent of the LDS query tile, d * es rounded up to 32 bytes
 *   lds_bytes        FUSED: dynamic LDS of the stage-1 launch
 *   blocks           FUSED: workgroups of the stage-1 launch, S * qtiles
 *   select           the selection: KRS_SELECT_LDS (rows of at most 2048 pairs: one LDS sort per row), KRS_SELECT_RADIX
 *                    (radix select of the k best, one LDS sort of them) or KRS_SELECT_RADIX_MERGE (k > 2048: blocks of 2048
 *                    sorted in LDS, merged in global memory)
 *   select_len       pairs per selected row: S * k (FUSED), n (SLAB), cols (ROWS)
 *   select_p         slots sorted per row, a power of two: at or above select_len on KRS_SELECT_LDS, at or above k else
 *   select_launches  kernel launches of one selection (SLAB: per chunk)
 *   chunks           SLAB: query chunks, each one krs_gemm and one selection
 *   chunk_rows       SLAB: query rows of a full chunk (the last chunk has b - (chunks - 1) * chunk_rows)
 * Fields that do not apply are 0.  krs_retrieval_last_route returns `kernel`; `route` may be NULL. */
enum { KRS_RETR_NONE = 0, KRS_RETR_FUSED, KRS_RETR_SLAB, KRS_RETR_ROWS };
enum { KRS_RETR_VARIANT_NONE = 0, KRS_RETR_VARIANT_TOPK, KRS_RETR_VARIANT_Q8, KRS_RETR_VARIANT_MINE, KRS_RETR_VARIANT_ROWS };
enum { KRS_SELECT_NONE = 0, KRS_SELECT_LDS, KRS_SELECT_RADIX, KRS_SELECT_RADIX_MERGE };
typedef struct krs_retrieval_route {
  int32_t kernel, variant, es, vec, S, qtiles, row_bytes, lds_bytes, select, select_launches;
  int64_t slice, blocks, select_len, select_p, chunks, chunk_rows;
} krs_retrieval_route;
int krs_retrieval_last_route(krs_retrieval_route* route);
/* Diagnostic, host only, no GPU needed: where the entry `variant` names WOULD run with these arguments
 * (KRS_RETRIEVAL_SLAB_BYTES is honoured as the entry honours it).  KRS_RETR_VARIANT_ROWS reads b as rows, n as cols, ldc
 * as ld and c as x; d and ldq are ignored.  KRS_RETR_VARIANT_Q8 reads dtype as the query dtype and c as the int8 rows.
 * q and c are read as VALUES only (nullness, alignment); the operands the planner does not look at (outputs, steps,
 * ids, the workspace) are taken as given and large enough.  No HIP call is made and the last-route record is untouched.
 * Fills *route (all zero when nothing would be launched) and returns what the entry returns before its first launch:
 * KRS_OK, KRS_ERR_INVALID or KRS_ERR_UNSUPPORTED. */
int krs_retrieval_plan_route(int variant, const void* q, int64_t ldq, const void* c, int64_t ldc, int dtype, int64_t b,
                             int64_t n, int64_t d, int k, krs_retrieval_route* route);

/* ------------------------------------------------------------------------- *
 * K9  Ranking losses (keras_rs.losses): unreduced loss and logit gradient in one pass
 *
 * logits [batch, list] fp32 / bf16 with row stride ld (>= list; a column slice of a wider matrix needs no copy);
 * labels [batch, list] fp32, mask [batch, list] uint8 (NULL = all set), both contiguous.  An item is valid when
 * label >= 0 and its mask byte is non-zero.  x = (s_i - s_j) * inv_temperature (the reference divides by T).
 *
 * krs_pairwise_loss (pairwise_loss.py, pairwise_mean_squared_error.py): item_loss [batch, list] fp32 =
 *   sum_j w_ij phi(x_ij), w_ij = I(y_i > y_j) valid_i valid_j, with phi of `kind`:
 *     KRS_RANK_HINGE          relu(1 - x)
 *     KRS_RANK_LOGISTIC       relu(-x) + log(1 + exp(-|x|))
 *     KRS_RANK_SOFT_ZERO_ONE  where(x > 0, 1 - sigmoid(x), sigmoid(-x))
 *     KRS_RANK_MSE            ((y_i - y_j) - (s_i - s_j))^2 with w_ij = valid_i valid_j (i != j); no temperature
 * dlogits [batch, list] (logits' dtype, contiguous) = d(sum_i g_i item_loss_i) / ds, the gradient autodiff takes
 * of the reference's expression (relu'(0) = abs'(0) = 0), with g_i = g_scale * g[i] (g [batch, list] fp32, NULL =
 * g_scale).
 *
 * krs_listmle_loss (list_mle_loss.py:70-150): list_loss [batch] fp32 = sum over the valid items in the order label
 * descending, index ascending (exact: no offset breaks ties) of log(sum_{q >= r} exp(z_q - m) + 1e-10) - (z_r - m),
 * z = s * inv_temperature, m = the largest valid z; 0 for a list without a valid item.  dlogits = d(sum_b g_b
 * list_loss_b) / ds with g_b = g_scale * g[b] (g [batch] fp32 or NULL), the gradient through m included.
 *
 * Either output may be NULL, not both.  1 <= list <= KRS_RANK_MAX_LIST (a longer list is KRS_ERR_INVALID);
 * batch >= 0.  fp32 arithmetic in a fixed order: bit-identical from call to call; no host synchronisation.
 * ------------------------------------------------------------------------- */
#define KRS_RANK_MAX_LIST 4096
typedef enum krs_rank_loss {
  KRS_RANK_HINGE = 0,
  KRS_RANK_LOGISTIC = 1,
  KRS_RANK_SOFT_ZERO_ONE = 2,
  KRS_RANK_MSE = 3
} krs_rank_loss;
int krs_pairwise_loss(int kind, const void* logits, int64_t ld, int dtype, const float* labels,
                      const uint8_t* mask, const float* g, float g_scale, float inv_temperature,
                      int64_t batch, int64_t list, float* item_loss, void* dlogits, void* stream);
int krs_listmle_loss(const void* logits, int64_t ld, int dtype, const float* labels, const uint8_t* mask,
                     const float* g, float g_scale, float inv_temperature, int64_t batch, int64_t list,
                     float* list_loss, void* dlogits, void* stream);

/* ------------------------------------------------------------------------- *
 * K10  Ranking metrics (keras_rs.metrics): one sort of each list in LDS, up to KRS_METRIC_MAX_SPECS metrics from it
 *
 * scores [batch, list] fp32 / bf16 with row stride ld; labels, gain (NULL = 2^y - 1) [batch, list] fp32 and mask
 * [batch, list] uint8 (NULL = all set), contiguous.  The weight of item i of list b is
 * weights[b * weights_row_stride + i * weights_item_stride] (fp32; item stride 1 = a weight per item, 0 = one
 * weight per list, no [batch, list] copy needed), or the scalar `weight` for every item when weights is NULL (pass
 * 1 for an unweighted call).  An item is valid when label >= 0, its mask byte is non-zero and its weight is > 0; an invalid item counts with label 0 and weight 0 and ranks after every
 * valid item.  Order within a list: valid first, score descending (the total order of K8 / K9: -0 == +0, NaN above
 * +inf), then the tie key ascending in the index (shuffle_ties == 0) or descending in the 20-bit hash of (seed,
 * *draw, row, index) and then ascending in the index.
 *
 * krs_ranking_metrics (stage A).  Spec j is (kinds[j], ks[j]) -- host arrays; ks[j] <= 0 means the whole list;
 * k = min(ks[j], list) -- and gives values[j * batch + b], with rel = (label >= 1), r the 1-based rank:
 *     KRS_METRIC_DCG        sum_{r <= k} w_r (gain_r discount_r)              (not yet divided by the list weight)
 *     KRS_METRIC_NDCG       DCG / the same sum in the order w * gain descending, 0 when that is 0
 *     KRS_METRIC_MAP        sum_{r <= k} (cumsum(rel)_r / r) (w_r rel_r) / sum_all w rel, 0 when that is 0
 *     KRS_METRIC_MRR        max_{r <= k} rel_r / r
 *     KRS_METRIC_PRECISION  sum_{r <= k} rel_r / min(k, number of valid items), 0 when that is 0
 *     KRS_METRIC_RECALL     sum_{r <= k} rel_r / sum_all rel, 0 when that is 0
 * discount (NULL = 1 / log2(1 + r)): discount_len fp32 values for r = 1 .. discount_len, discount_len >= every k of
 * a DCG / NDCG spec.  sums [5, batch] fp32 receives per list: sum w gain, sum gain, sum w rel, sum rel, sum w.
 * order (NULL = not wanted) [batch, list] int32 receives the item index at each rank.  draw is a device int64
 * read by the launch (NULL = 0); it is not changed here.
 *
 * krs_ranking_metrics_accumulate (stage B).  Turns sums into the per-list weights of
 * get_list_weights (ranking_metrics_utils.py:132-224): with relevance = gain for DCG / NDCG and rel otherwise,
 *     0 when sum w == 0;  sum(w relevance) / sum(relevance) when sum relevance > 0;  otherwise the batch-wide
 *     sum of those quotients / #{lists with sum w > 0 and sum relevance > 0}, or 1 when there is no such list.
 * A DCG value is divided by its weight (0 when that is 0).  states[j] (host array of n_specs device pointers) is
 * spec j's {total, count}: total += sum_b value weight, count += sum_b weight.  out_values / out_weights (NULL =
 * not wanted) [n_specs, batch] receive the per-list values and weights.  draw (NULL = none) is advanced by one.
 * Up to 1024 lists run in one workgroup and one launch.  A larger batch is spread over up to 256 workgroups in three
 * launches (partial sums of the default weight; partial sums of the Mean update; the states) and needs
 * krs_ranking_metrics_accumulate_workspace_bytes(batch) bytes of device workspace (0 up to 1024 lists), which need not
 * be initialised; too little is KRS_ERR_WORKSPACE.
 *
 * Fixed summation orders and no float atomics: bit-identical from call to call.  No host synchronisation.
 * 1 <= list <= KRS_RANK_MAX_LIST and 1 <= n_specs <= KRS_METRIC_MAX_SPECS, otherwise KRS_ERR_INVALID.
 * ------------------------------------------------------------------------- */
#define KRS_METRIC_MAX_SPECS 8
typedef enum krs_metric_kind {
  KRS_METRIC_DCG = 0,
  KRS_METRIC_NDCG = 1,
  KRS_METRIC_MAP = 2,
  KRS_METRIC_MRR = 3,
  KRS_METRIC_PRECISION = 4,
  KRS_METRIC_RECALL = 5
} krs_metric_kind;
int krs_ranking_metrics(const void* scores, int64_t ld, int dtype, const float* labels, const uint8_t* mask,
                        const float* weights, int64_t weights_row_stride, int64_t weights_item_stride, float weight,
                        const float* gain, const float* discount, int64_t discount_len, int shuffle_ties,
                        uint64_t seed, const int64_t* draw, const int* kinds, const int* ks, int n_specs,
                        int64_t batch, int64_t list, float* values, float* sums, int32_t* order, void* stream);
size_t krs_ranking_metrics_accumulate_workspace_bytes(int64_t batch);
int krs_ranking_metrics_accumulate(const float* values, const float* sums, const int* kinds, int n_specs,
                                   int64_t batch, float* const* states, float* out_values, float* out_weights,
                                   int64_t* draw, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * K11  Retrieval training head: row softmax cross-entropy with its gradient, and the two logit corrections
 *
 * In all three, logits [rows, cols] is fp32 / bf16 with row stride ld (>= cols) and is computed on in fp32; outputs in
 * the logits' dtype have their own row stride.  rows >= 0 (0 is a successful no-op), 1 <= cols <= 2^30, otherwise
 * KRS_ERR_INVALID.  Fixed summation orders and no atomics: bit-identical from call to call.  No host synchronisation,
 * no workspace.
 *
 * krs_softmax_xent (keras.losses.CategoricalCrossentropy / SparseCategoricalCrossentropy with from_logits=True).
 * Labels are either dense, labels [rows, cols] fp32 with row stride ld_labels, or sparse, label_index [rows] int32
 * (y = one-hot of the index): exactly one of the two is non-NULL.  With y' = y (1 - label_smoothing) +
 * label_smoothing / cols (0 <= label_smoothing < 1), m = max_j x_j, Z = sum_j exp(x_j - m), S = sum_j y'_j:
 *     row_loss[r]   = sum_j y'_j ((m - x_j) + log Z)                 (fp32; labels are not renormalised)
 *     dlogits[r, j] = g_r (S exp(x_j - m) / Z - y'_j),  g_r = g_scale * g[r]  (g [rows] fp32, NULL = g_scale)
 * Either output may be NULL, not both.  A label_index outside [0, cols) is never used as an address: it makes that
 * row's loss and gradient NaN.  Logits must be finite.  Rows of up to 9216 columns are read from memory once; longer
 * rows twice.
 *
 * krs_sampling_correction (sampling_probability_correction.py:56-58): out = logits - log(min(max(p, epsilon), 1)).
 * probs [p_rows, cols] fp32, contiguous; logits row r reads probs row r mod p_rows (p_rows = 1 broadcasts one row).
 *
 * krs_remove_accidental_hits (remove_accidental_hits.py:84-97), in fp32 with every operation rounded on its own:
 *     pos = the first index of the row's largest label (0 for an all-zero row; -0 == +0, NaN above +inf)
 *     out[r, j] = logits[r, j] + ((ids[j] == ids[pos] ? 1 : 0) - labels[r, j]) * value
 * labels [rows, cols] fp32 with row stride ld_labels; ids [id_rows, cols] int32 / int64 (id_dtype: krs_itype),
 * contiguous, logits row r reads ids row r mod id_rows.
 * ------------------------------------------------------------------------- */
int krs_softmax_xent(const void* logits, int64_t ld, int dtype, const float* labels, int64_t ld_labels,
                     const int32_t* label_index, float label_smoothing, const float* g, float g_scale,
                     int64_t rows, int64_t cols, float* row_loss, void* dlogits, int64_t ld_dlogits, void* stream);
int krs_sampling_correction(const void* logits, int64_t ld, int dtype, const float* probs, int64_t p_rows,
                            float epsilon, int64_t rows, int64_t cols, void* out, int64_t ld_out, void* stream);
int krs_remove_accidental_hits(const void* logits, int64_t ld, int dtype, const float* labels, int64_t ld_labels,
                               const void* ids, int id_dtype, int64_t id_rows, float value, int64_t rows,
                               int64_t cols, void* out, int64_t ld_out, void* stream);

/* ------------------------------------------------------------------------- *
 * K12  Binary metrics (keras.metrics.BinaryAccuracy and keras.metrics.AUC, the metrics the ml_perf step compiles):
 *      one pass over the predictions, every requested state updated from it
 *
 * pred [n] fp32 / bf16 (computed on in fp32) and labels [n] fp32, contiguous.  Sample i weighs weights[i] (fp32), or
 * the scalar `weight` when weights is NULL (pass 1 for an unweighted call).
 *
 * Accuracy (acc_state != NULL): acc_state is {total, count}, keras.metrics.Mean:
 *     total += sum_i w_i (float(pred_i > acc_threshold) == label_i),   count += sum_i w_i
 * (a label that is neither 0 nor 1 matches nothing).
 *
 * AUC spec j of n_aucs (host arrays of n_aucs entries each): auc_states[j] is [4, T] fp32 with T = auc_T[j], the
 * rows true_positives, false_positives, true_negatives, false_negatives.  p = pred, or 1 / (1 + exp(-pred)) when
 * auc_from_logits[j]; then p = min(max(p, 0), 1) with NaN -> 0.  A sample is positive iff label != 0:
 * wpos = w positive, wneg = w (1 - positive).  Its bucket is
 *     auc_thresholds[j] == NULL (T >= 3; the even set -1e-7, 1/(T-1), .., (T-2)/(T-1), 1+1e-7):
 *         b = max((int)ceilf(p * (float)(T - 1)) - 1, 0)                              (fp32, exactly this)
 *     auc_thresholds[j] = T ascending fp32 values on the device, end points included:
 *         b = #{i : t_i < p} - 1                            (b < 0: the sample exceeds no threshold)
 * and then  pos[b] += wpos, neg[b] += wneg;  tp[i] += sum_{b >= i} pos[b], fp[i] += sum_{b >= i} neg[b],
 * fn[i] += sum pos - tp[i], tn[i] += sum neg - fp[i].
 *
 * Summation order (fixed; no float atomics; the same bits on any device, from call to call, and for a spec alone
 * or beside others): samples are cut into chunks of KRS_BINARY_METRIC_CHUNK; within a chunk a bin adds its samples
 * in index order.  Workgroup g of G = min(number of chunks, KRS_BINARY_METRIC_GROUPS) adds the chunks g, g + G,
 * g + 2 G, .. in that order; the G partials are added in the order of g; the sums over b >= i are one scan of
 * fixed shape.  workspace: krs_binary_metrics_workspace_bytes bytes on the device, which need not be initialised;
 * too little is KRS_ERR_WORKSPACE.  n >= 0; 0 <= n_aucs <= KRS_BINARY_METRIC_MAX_AUCS and
 * 2 <= T <= KRS_BINARY_METRIC_MAX_THRESHOLDS, otherwise KRS_ERR_INVALID.  No host synchronisation.
 * ------------------------------------------------------------------------- */
#define KRS_BINARY_METRIC_MAX_AUCS 4
#define KRS_BINARY_METRIC_MAX_THRESHOLDS 2048
#define KRS_BINARY_METRIC_CHUNK 1024
#define KRS_BINARY_METRIC_GROUPS 256
size_t krs_binary_metrics_workspace_bytes(int64_t n, int n_aucs, const int* auc_T);
int krs_binary_metrics(const void* pred, int dtype, const float* labels, const float* weights, float weight,
                       int64_t n, float acc_threshold, float* acc_state, int n_aucs,
                       const float* const* auc_thresholds, const int* auc_T, const int* auc_from_logits,
                       float* const* auc_states, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * K13  Fused in-batch softmax retrieval loss: the scores are formed tile by tile on the matrix cores and never stored
 *
 * q [b, d] and c [n, d] are bf16 with row strides ldq, ldc (>= d; a column slice of a wider matrix needs no copy).
 * Per query row i and candidate j, in fp32:
 *     s_ij   = sum_k q_ik c_jk  (fp32 accumulate)  + bias_j  + hit_value * [ids_j == ids_{pos_i} and j != pos_i]
 *     y'_ij  = (1 - ls) [j == pos_i] + ls / n
 *     m_i = max_j s_ij,  Z_i = sum_j exp(s_ij - m_i),  lse_i = m_i + log Z_i
 *     loss_i = sum_j y'_ij ((m_i - s_ij) + log Z_i)     (K11's accumulation: non-negative terms, no lse - s
 *                                                         cancellation)
 *     P_ij   = g_i (exp(s_ij - lse_i) - y'_ij),   g_i = g_scale * g[i]  (g [b] fp32, NULL = g_scale)
 *     dq_i   = sum_j P_ij c_j,    dc_j = sum_i P_ij q_i   (P rounded to bf16, nearest even, for these two products;
 *                                                         fp32 accumulate; stored in bf16 with row strides lddq, lddc)
 * pos: int32 [b], or NULL for pos_i = i (labels = eye(b, n)).  cand_bias: fp32 [n] or NULL (the sampling correction
 * -log(clip(p, eps, 1)) of SamplingProbabilityCorrection).  cand_ids: int32 / int64 [n] (id_dtype: krs_itype) or
 * NULL; hit_value is added to the accidental hits of RemoveAccidentalHits (the reference's constant 1.1754944e-40
 * changes no ordinary logit; a large negative finite value removes them).  ls = label_smoothing, 0 <= ls < 1.
 * A pos_i outside [0, n) is never used as an address: that row's loss is NaN and its g_i counts as NaN, so its dq
 * row and every dc entry are NaN, as in the stored-matrix head.  Scores must be finite.
 *
 * Known divergence from the stored-matrix head: for bf16 inputs that head rounds the scores to bf16 before the
 * corrections and the softmax; here they stay in fp32 (as K8 ranks fp32 scores).
 *
 * krs_retrieval_xent_fwd writes row_loss [b] and row_lse [b] (fp32); krs_retrieval_xent_bwd recomputes the scores
 * from q, c and row_lse and writes dq [b, d] and / or dc [n, d] (either may be NULL, not both).  Memory is
 * O((b + n) d): when the owner side of a sweep gives too few workgroups the other side is cut into slices whose
 * partials live in `workspace` (krs_retrieval_xent_workspace_bytes, at most about 16 (b + n) d floats, possibly 0;
 * it need not be initialised) and are combined in slice order.  No float atomics: bit-identical from call to call.
 * No host synchronisation.  b == 0 is a successful no-op.  n < 1, d < 1, d > 256, a dtype other than KRS_BF16 and
 * more than 2^31 - 1 rows are KRS_ERR_INVALID (the Python wrapper routes such shapes to a slab path built from
 * krs_gemm and K11); too little workspace is KRS_ERR_WORKSPACE.
 * ------------------------------------------------------------------------- */
size_t krs_retrieval_xent_workspace_bytes(int64_t b, int64_t n, int64_t d, int dtype);
int krs_retrieval_xent_fwd(const void* q, int64_t ldq, const void* c, int64_t ldc, int dtype, int64_t b, int64_t n,
                           int64_t d, const int32_t* pos, const float* cand_bias, const void* cand_ids, int id_dtype,
                           float hit_value, float label_smoothing, float* row_loss, float* row_lse, void* workspace,
                           size_t workspace_bytes, void* stream);
int krs_retrieval_xent_bwd(const void* q, int64_t ldq, const void* c, int64_t ldc, int dtype, int64_t b, int64_t n,
                           int64_t d, const int32_t* pos, const float* cand_bias, const void* cand_ids, int id_dtype,
                           float hit_value, float label_smoothing, const float* row_lse, const float* g, float g_scale,
                           void* dq, int64_t lddq, void* dc, int64_t lddc, void* workspace, size_t workspace_bytes,
                           void* stream);

/* ------------------------------------------------------------------------- *
 * K14  Hard-negative mining for the in-batch softmax loss: the fused stage 1 of K8 on K13's corrected score
 *
 * Replaces keras_rs.layers.HardNegativeMining (hard_negative_mining.py:43-94) in front of
 * CategoricalCrossentropy(from_logits=True, label_smoothing=ls) without ever storing the [b, n] scores.  For query row
 * i, with k = min(num_hard_negatives, n - 1) chosen by the caller:
 *     s_ij   = sum_d q_id c_jd (fp32 accumulate) + bias_j + hit_value * [ids_j == ids_{pos_i} and j != pos_i]
 *              (K13's score; the two corrections are added in this order, each rounded to fp32)
 *     M_i    = the k candidates j != pos_i that come first in K8's total order: the fp32 key s_ij descending, then
 *              the index ascending; -0.0 ranks as +0.0
 *     loss_i = softmax cross-entropy over the k + 1 logits (s_{i,pos_i}, s_{i,M_i}) against
 *              y' = (1 - ls) [slot 0] + ls / (k + 1)
 * The reference's top_k(logits + labels * MAX_FLOAT, k + 1, sorted=False) leaves the choice among equal scores at
 * the k-th place open; the loss does not depend on it, the gradient does.  Here the tie goes to the LOWEST index.
 * Scores stay in fp32 (K13's known divergence from the stored-matrix head, which rounds bf16 scores first) and must
 * be finite.
 *
 * krs_retrieval_mine writes, per row, out_idx [b, k] int32 (M_i, sorted in the total order), out_scores [b, k] fp32
 * (the corrected s_ij of those candidates, -0.0 as +0.0) and pos_score [b] fp32 (s_{i,pos_i}).  The softmax over the
 * k + 1 logits is K11 (krs_softmax_xent); its gradient P [b, k+1] gives dq_i = sum_m P_im c[idx_im] (K1 with
 * weights = P) and dc_j = sum_{(i,m): idx_im = j} P_im q_i (K2's plan + dense form with grad = q), which is what
 * keras_rs_amd.retrieval_ops.retrieval_xent(num_hard_negatives=...) runs.
 *
 * pos: int32 [b], or NULL for pos_i = i.  A pos_i outside [0, n) is never used as an address: the row then has no
 * positive and no accidental hits, its k candidates are mined among all n, and pos_score[i] is NaN.  The host op
 * makes that row's loss and its P row NaN: its dq row is NaN, and in dc exactly the rows of the k candidates mined
 * for it are NaN (K13, which touches every candidate for every row, makes all of dc NaN; here the other rows stay
 * finite).
 *
 * q [b, d], c [n, d]: fp32 or bf16 (one dtype), row strides ldq, ldc >= d in elements.  cand_bias fp32 [n] or NULL;
 * cand_ids int32 / int64 [n] (id_dtype: krs_itype) or NULL.  1 <= k <= min(n - 1, 128) and d <= 512; anything else,
 * null q / c / outputs, a bad dtype and n > 2^31 - 1 are KRS_ERR_INVALID (the Python wrapper routes larger k or d
 * to a slab path built from krs_gemm, krs_topk_rows and K11).  b == 0 is a successful no-op.  Workspace:
 * krs_retrieval_mine_workspace_bytes = the slice lists, b * S * k pairs of 8 bytes with S = the number of candidate
 * slices of stage 1 (a multiple of 8, about max(8, min(2048 / ceil(b / 32), n / 8192))), plus b * pow2(k) pairs when
 * S * k > 2048; it need not be initialised; too little is KRS_ERR_WORKSPACE.  No float atomics, no host
 * synchronisation, bit-identical from call to call.
 * ------------------------------------------------------------------------- */
size_t krs_retrieval_mine_workspace_bytes(int64_t b, int64_t n, int64_t d, int k, int dtype);
int krs_retrieval_mine(const void* q, int64_t ldq, const void* c, int64_t ldc, int dtype, int64_t b, int64_t n,
                       int64_t d, int k, const int32_t* pos, const float* cand_bias, const void* cand_ids, int id_dtype,
                       float hit_value, int32_t* out_idx, float* out_scores, float* pos_score, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * K15  The positive's rank among all candidates, from the embeddings: the scores are formed tile by tile on the
 *      matrix cores (K13's sweep) and never stored
 *
 * The evaluation counterpart of K13 (the idea of tfrs.metrics.FactorizedTopK): one sweep answers "how many
 * candidates beat the positive?" for every query, which gives every top-k accuracy and the reciprocal rank at once.
 * q [b, d] and c [n, d] are bf16 with row strides ldq, ldc (>= d), 1 <= d <= 256, n >= 1, b >= 0.  Per query row i:
 *     s_ij    = sum_k q_ik c_jk   (fp32 accumulate; no bias, no smoothing)
 *     rank_i  = #{ j != pos_i : j precedes pos_i in K8's total order and not (ids_j == ids_{pos_i}) }
 * K8's order: the fp32 key s_ij descending, then the index ascending; -0.0 == +0.0, NaN above +inf (all NaN equal).
 * Without ids, rank_i is the column at which krs_retrieval_topk with k = n returns the positive.
 * pos: int32 [b], or NULL for pos_i = i.  cand_ids: int32 / int64 [n] (id_dtype: krs_itype) or NULL; with ids, a
 * candidate other than the positive that carries the positive's id is not counted (K13's accidental hits, removed).
 * A pos_i outside [0, n) is never used as an address: that row gets rank -1 and pos_score NaN.
 *
 * out_rank [b] int32; out_pos_score [b] fp32 (s_{i,pos_i}) may be NULL.  s_{i,pos_i} leaves the same MFMA chain as
 * the streamed scores (a short first launch streams each workgroup's own positives, gathered through pos, and
 * keeps the diagonal), so a candidate row byte-identical to the positive's ties with it exactly and the index decides.
 *
 * Memory is O((b + n) d).  The candidate side is cut into K13's slices (from (b, n) alone); the slices' int32 counts
 * live in `workspace` and are added by a second small launch.  krs_retrieval_rank_workspace_bytes is the positives'
 * scores, 4 b bytes, plus 4 S b bytes when S > 1 slices are used, each rounded up to 256:
 *     at most 4 b + 32 (b + n) + 512 bytes                                     (S b <= 8 (b + n)).
 * It need not be initialised.  Integer counts only: exact, order-independent, bit-identical from call to call.  No
 * host synchronisation, no allocation, no scratch; graph-capturable.  b == 0 is a successful no-op.
 * A dtype other than KRS_BF16 and d > 256 are KRS_ERR_UNSUPPORTED (the Python wrapper routes them to a slab path built
 * from krs_gemm); null q, c or out_rank, d < 1, n < 1, more than 2^31 - 1 rows, a row stride below d and a bad id
 * dtype are KRS_ERR_INVALID; too little workspace is KRS_ERR_WORKSPACE.
 * ------------------------------------------------------------------------- */
size_t krs_retrieval_rank_workspace_bytes(int64_t b, int64_t n, int64_t d, int dtype);
int krs_retrieval_rank(const void* q, int64_t ldq, const void* c, int64_t ldc, int dtype, int64_t b, int64_t n,
                       int64_t d, const int32_t* pos, const void* cand_ids, int id_dtype, int32_t* out_rank,
                       float* out_pos_score, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * K17  BruteForceRetrieval over an int8 candidate index: K8's fused score + top-k on v_mfma_i32_32x32x32_i8
 *
 * The serving form of a two-tower model: the candidate index is stored as K16 stores a table, and the queries are
 * quantized on the way in (Keras' dynamic activation quantization).  The arithmetic, all of it pinned:
 *   Candidates  cq [n, d] int8 with row stride ldc (elements) and cstep [n] fp32: what krs_quantize_rows_q8 writes.
 *               Every int8 value counts, -128 included (the quantizer never emits it; a caller may).
 *   Queries     q [b, d] fp32 / bf16 (q_dtype) with row stride ldq.  Each row is quantized into the workspace by the
 *               rule of krs_quantize_rows_q8, bit for bit: qq [b, d] int8 and qstep [b] fp32.
 *   Non-finite  A query row holding a NaN or an infinity gets qq = 0, qstep = 0 and raises KRS_FLAG_NONFINITE_ROW in
 *               err_flag (which may be NULL): every score of that row is +0.0 and it returns candidates 0 .. k-1.
 *               Other rows are unaffected.
 *   Score       s_ij = fmul_rn(fmul_rn((float) idot_ij, cstep_j), qstep_i),  idot_ij = sum_e qq[i,e] * cq[j,e] in int32:
 *               two separately rounded fp32 multiplies in that order, nothing contracted.  |idot| <= 512 * 128 * 127
 *               < 2^24, so the conversion is exact; steps are 0 or >= 7.8e-10, so no score is subnormal.
 *   Order       K8's total order on s: fp32 descending, index ascending, -0.0 as +0.0.  Rows come back sorted.
 *               out_scores [b, k] is s rounded once to out_dtype (KRS_F32 / KRS_BF16), or NULL; out_ids [b, k] int32 is
 *               ids[index], or the index when ids is NULL.
 *   Shapes      1 <= k <= min(n, 128), 1 <= d <= 512, n <= INT32_MAX, b >= 0, ldq >= d, ldc >= d.  k > 128 (with
 *               k <= n) and d > 512 are KRS_ERR_UNSUPPORTED with a message naming the limit: there is no slab path.
 *               Other bad shapes, a bad dtype and a null q, cq, cstep or out_ids (b > 0) are KRS_ERR_INVALID, the shape
 *               checks first; too little workspace is KRS_ERR_WORKSPACE; b == 0 is a successful no-op.
 *   Execution   Three stages on `stream`: the query quantizer, K8's stage 1 (a 32-query tile against a candidate slice,
 *               one MFMA per 32 bytes of K, the scaling in the epilogue, then K8's threshold test and row queues) and
 *               K8's slice merge.  16-byte candidate loads when d % 16 == 0, ldc % 16 == 0 and cq is 16-byte aligned,
 *               byte loads otherwise.  Integer dot products are exact, so ids, order and score bits are a function of
 *               the inputs alone: bit-identical from call to call.  No allocation, no host wait; graph-capturable.
 * krs_retrieval_topk_q8_workspace_bytes: K8's slice lists plus the quantized queries (b rows of d rounded up to 32
 * bytes, and 4 b bytes), each rounded up to 256; > 0 for b > 0 on a supported shape, 0 otherwise.  It need not be
 * initialised.
 * ------------------------------------------------------------------------- */
size_t krs_retrieval_topk_q8_workspace_bytes(int64_t b, int64_t n, int64_t d, int k);
int krs_retrieval_topk_q8(const void* q, int64_t ldq, int q_dtype, const int8_t* cq, int64_t ldc, const float* cstep,
                          const int32_t* ids, int64_t b, int64_t n, int64_t d, int k, void* out_scores, int out_dtype,
                          int32_t* out_ids, int* err_flag, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * K18  Dense and FeatureCross in int8: C = epilogue(scale(Aq . Wq^T)) on v_mfma_i32_32x32x32_i8
 *
 * The serving form of keras.layers.Dense.quantize("int8"): int8 weights with one step per output channel, activations
 * quantized per row on the way in, an exact int32 product, two fp32 scalings, then krs_gemm's epilogue.  All pinned:
 *   Weights      A Keras kernel W [K, N] is stored TRANSPOSED: wq [N, K] int8, K-contiguous with row stride ldw
 *                (elements), plus wstep [N] fp32 -- exactly what krs_quantize_rows_q8 writes for the rows of W^T (Keras'
 *                abs_max_quantize(kernel, axis=0), with the stored dequantization step).
 *   Activations  aq [M, K] int8 with row stride lda and astep [M] fp32: what krs_quantize_rows_q8 writes for the rows of
 *                A [M, K] fp32 / bf16 (Keras' dynamic per-row input quantization, as K17 does for queries).  Operands are
 *                pre-quantized at this level; the Python op runs the quantizer in front.
 *   Product      idot_ij = sum_e aq[i,e] * wq[j,e] in int32: exact, every int8 value counts, -128 included.
 *                k <= 131072, so the sum cannot overflow; a larger k is KRS_ERR_UNSUPPORTED.
 *                z_ij = fmul_rn(fmul_rn((float) idot_ij, wstep_j), astep_i): the conversion rounds to nearest even
 *                (|idot| may exceed 2^24 here, unlike K17), then two separately rounded multiplies in that order, nothing
 *                contracted.  idot is exact, so z is a function of the inputs alone -- not of tile shape or route.
 *   Epilogue     krs_gemm's on v = z, the same krs_gemm_epilogue and operand rules (x0, x, u_out, r in the dtype of C):
 *                + bias, act, x0 * (v + diag_scale * x) + x, + beta * R, one rounding to out_dtype (KRS_F32 / KRS_BF16).
 *   Non-finite   The quantizer gives a row with a NaN or an infinity q = 0, step = 0 (KRS_FLAG_NONFINITE_ROW); a finite
 *                row has step >= 1e-7 / 127.  Where astep_i == 0 every element of row i of C (and of u_out) is the
 *                canonical quiet NaN (0x7fc00000, rounded to out_dtype), whatever the epilogue: a poisoned input stays
 *                visible without a host read.  Other rows are unaffected.
 *   Shapes       m, n, k >= 0; m == 0 or n == 0 is a successful no-op; k == 0 gives z = 0.  Null aq, astep, wq, wstep, c,
 *                a negative size, a bad out_dtype, x0 without x: KRS_ERR_INVALID, the shape checks first.  k > 131072,
 *                m or n > 2^31 - 1, a grid beyond the launch limits: KRS_ERR_UNSUPPORTED with a message naming the limit.
 *   Execution    One launch, no workspace, no split-K, no allocation, no host wait: graph-capturable.  Kernels
 *                (csrc/gemm_q8_plan.h decides, a pure host function): KRS_GEMM_Q8_KERNEL_RING -- 256 x 256 tiles, 128-k
 *                pieces by LDS-DMA on gemm_pp64_kernel's five-slot ping-pong ring -- where aq and wq are on 16 bytes, lda
 *                and ldw are multiples of 16, k is whole 128-k pieces and at least three, m, n >= 256 and the 256-tiles
 *                number at least 192; KRS_GEMM_Q8_KERNEL_TILE128 -- 128 x 128 tiles, a K tail zero-filled in LDS -- for
 *                every other shape with k % 16 == 0 and operands aligned like that (m = 1 and n = 1 included);
 *                KRS_GEMM_Q8_KERNEL_GENERIC -- byte loads, one output per thread -- for the rest (k = 13, any k that is
 *                not a multiple of 16, unaligned strides or bases).
 * krs_gemm_q8_last_route / krs_gemm_q8_plan_route: as krs_gemm_last_route / krs_gemm_plan_route.  The record: kernel
 * (KRS_GEMM_Q8_KERNEL_*), ep_vec (1 when every epilogue operand allowed 8-wide vector access), k_tail (TILE128 only: 1
 * when k is not whole 128-byte tile rows and the tail is zero-filled), epilogue (RING only: 1 = the cross build -- bf16
 * output, x0 without R, ep_vec -- whose x0 / x loads are issued ahead, as krs_gemm's build 1; else 0, the general
 * epilogue).  All zero after a refused call or a no-op.
 * ------------------------------------------------------------------------- */
enum {
  KRS_GEMM_Q8_KERNEL_NONE = 0, KRS_GEMM_Q8_KERNEL_GENERIC = 1, KRS_GEMM_Q8_KERNEL_TILE128 = 2, KRS_GEMM_Q8_KERNEL_RING = 3
};
typedef struct krs_gemm_q8_route {
  int32_t kernel;
  int32_t ep_vec;
  int32_t k_tail;
  int32_t epilogue;
} krs_gemm_q8_route;
int krs_gemm_q8(const int8_t* aq, int64_t lda, const float* astep, const int8_t* wq, int64_t ldw, const float* wstep,
                void* c, int64_t ldc, int64_t m, int64_t n, int64_t k, int out_dtype, const krs_gemm_epilogue* epilogue,
                void* stream);
int krs_gemm_q8_last_route(krs_gemm_q8_route* route);
int krs_gemm_q8_plan_route(const int8_t* aq, int64_t lda, const float* astep, const int8_t* wq, int64_t ldw,
                           const float* wstep, const void* c, int64_t ldc, int64_t m, int64_t n, int64_t k, int out_dtype,
                           const krs_gemm_epilogue* epilogue, krs_gemm_q8_route* route);

/* ------------------------------------------------------------------------- *
 * K19  Fused multi-head self-attention over [b, l] token sequences: the score matrix, the probabilities and the
 *      dropout mask are never stored
 *
 * q, k, v hold one row per token: token (bi, i) is row bi * l + i, head hi starts at column hi * dh, rows are ldq / ldk /
 * ldv elements apart (>= h * dh; the three may be column slices of one packed [b * l, 3 h dh] projection output).  out,
 * dout, dq, dk, dv have the same layout with strides of their own.  dtype (KRS_F32 / KRS_BF16) is the type of all of
 * them; lse is fp32 [b, h, l].  Per (bi, hi), query i and key j, in fp32:
 *     s_ij      = scale * sum_d q_id k_jd                                         (fp32 accumulate)
 *     allowed   = (!causal || j <= i) && (key_valid == NULL || key_valid[bi, j])   (key_valid: uint8 [b, l], 1 = token)
 *     m_i = max_allowed s_ij,  Z_i = sum_allowed exp(s_ij - m_i),  lse_i = m_i + log Z_i
 *     P_ij      = exp(s_ij - lse_i) for allowed j, else 0
 *     P~_ij     = keep_ij * P_ij / (1 - p)                                         (p = dropout_p, 0 <= p < 1)
 *     o_i       = sum_j P~_ij v_j
 *     delta_i   = sum_d dO_id o_id,   dP~_ij = dO_i . v_j,   dS_ij = P_ij (keep_ij / (1 - p) * dP~_ij - delta_i)
 *     dV_j      = sum_i P~_ij dO_i,   dQ_i = scale sum_j dS_ij k_j,   dK_j = scale sum_i dS_ij q_i
 * A decision: a row with no allowed key (left padding, an all-padding sequence) has o_i = 0 and lse_i = -inf and
 * contributes exactly zero to dq, dk and dv; no NaN appears.  (Keras adds -1e9 to masked scores, which gives such a
 * row the uniform average over all keys, future ones included.)  Inputs must be finite.
 *
 * The dropout mask is a pure function of (seed, *draw, bi, hi, i, j), 32-bit unsigned arithmetic throughout:
 *     mix(x)    : x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 *     base      = mix(mix(mix(mix(mix(seed_lo ^ 0x9e3779b9) ^ seed_hi) ^ draw_lo) ^ draw_hi) ^ (bi * h + hi))
 *     keep_ij   <=> mix(base + ((i << 12) | j)) >= floor(p * 2^32)
 * The forward and both backward sweeps recompute it.  draw is a device int64 the call only READS (the caller advances
 * it with a device-side add after the forward, so a step can be captured in a graph); NULL when dropout_p == 0.
 *
 * Routes (csrc/seq_attn_plan.h decides, a pure host function):
 *   KRS_SEQ_ATTN_FAST     bf16, dh <= 128 (dpad 32 / 64 / 128).  Scores on v_mfma_f32_32x32x16_bf16 with an online
 *                         softmax over key tiles; P~ and dS are rounded to bf16 (nearest even) for the second products;
 *                         fp32 accumulate; outputs rounded once to bf16.  Rows that are not whole 16-byte chunks on
 *                         16-byte boundaries (dh = 50, odd strides) load element-wise.
 *   KRS_SEQ_ATTN_GENERIC  fp32 at any dh <= 256, bf16 at 128 < dh <= 256: fp32 FMA throughout, outputs rounded once.
 * One owner per output element and no float atomics on either route: bit-identical from call to call.
 * Known divergence: Keras' MultiHeadAttention multiplies q by 1 / sqrt(key_dim) in the compute dtype before the
 * product; here the fp32 score is scaled.
 *
 * krs_seq_attn_fwd writes out and lse.  krs_seq_attn_bwd takes them back with dout and writes dq, dk, dv (any may be
 * NULL to skip it, not all); it needs krs_seq_attn_workspace_bytes of workspace (delta, fp32 [b, h, l]; it need not be
 * initialised; too little is KRS_ERR_WORKSPACE); the forward uses none.  No host synchronisation.
 * b == 0 or l == 0 is a successful no-op.  b < 0, h < 1, l < 0, dh < 1, a bad dtype, dropout_p outside [0, 1), a stride
 * below h * dh, a null operand or output, and dropout without draw are KRS_ERR_INVALID.  l > 4096, dh > 256 and
 * b * h * l > 2^31 - 1 (the launch grid) are KRS_ERR_UNSUPPORTED with a message naming the limit.
 * krs_seq_attn_last_route: the route of the process's last krs_seq_attn_fwd / _bwd call, whichever thread made it (an
 * autograd engine runs the backward on a thread of its own): kernel, and dpad on the fast route, else 0; both zero
 * after a refused call or a no-op.  Returns kernel.
 * ------------------------------------------------------------------------- */
enum { KRS_SEQ_ATTN_NONE = 0, KRS_SEQ_ATTN_FAST = 1, KRS_SEQ_ATTN_GENERIC = 2 };
size_t krs_seq_attn_workspace_bytes(int64_t b, int64_t h, int64_t l, int64_t dh, int dtype);
int krs_seq_attn_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, int dtype,
                     int64_t b, int64_t h, int64_t l, int64_t dh, const uint8_t* key_valid, int causal, float scale,
                     float dropout_p, uint64_t seed, const int64_t* draw, void* out, int64_t ldo, float* lse,
                     void* workspace, size_t workspace_bytes, void* stream);
int krs_seq_attn_bwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, int dtype,
                     int64_t b, int64_t h, int64_t l, int64_t dh, const uint8_t* key_valid, int causal, float scale,
                     float dropout_p, uint64_t seed, const int64_t* draw, const void* out, int64_t ldo, const void* dout,
                     int64_t lddo, const float* lse, void* dq, int64_t lddq, void* dk, int64_t lddk, void* dv,
                     int64_t lddv, void* workspace, size_t workspace_bytes, void* stream);
int krs_seq_attn_last_route(int* kernel, int* dpad);

/* ------------------------------------------------------------------------- *
 * K20  The recurrence of a GRU layer (keras.layers.GRU: reset_after=True, tanh, sigmoid), all l steps in one launch
 *
 * Weights in Keras' shapes and gate order z, r, h: kernel [d, 3u], recurrent_kernel [u, 3u], bias [2, 3u] (row 0 the
 * input bias, row 1 the recurrent bias rb).  The input projection runs OUTSIDE these entries, as a Dense product:
 * xz = x . kernel + bias[0], one row of 3u per token, token (bi, t) at row bi * l + t, rows ldxz elements apart
 * (>= 3u: a view of a wider buffer qualifies).  At a valid step, with h the carried state, in fp32:
 *     a  = h . recurrent_kernel                          (slices a_z, a_r, a_h; fp32 accumulate)
 *     z  = sigmoid(xz_z + a_z + rb_z)      r = sigmoid(xz_r + a_r + rb_r)
 *     q  = a_h + rb_h                      c = tanh(xz_h + r * q)
 *     h' = z * h + (1 - z) * c
 * At a masked step (valid[bi, t] == 0; valid: uint8 [b, l] or NULL = every step valid) the state is carried unchanged
 * and the step's sequence output is the previous step's output: zeros before the first valid step, even when h0 is
 * not zero (the rule of Keras' backend rnn); from the first valid step on the output equals the state.
 * Backward, with g the gradient arriving at h' (this step's output gradient plus the carried one):
 *     dh  = g * z              dc_pre = g * (1 - z) * (1 - c^2)          dz_pre = g * (h - c) * z * (1 - z)
 *     dq  = dc_pre * r         dr_pre = dc_pre * q * r * (1 - r)
 *     dxz = (dz_pre, dr_pre, dc_pre)      da = (dz_pre, dr_pre, dq)      dh += da . recurrent_kernel^T
 * A masked step passes g through and contributes zeros to dxz and da; the gradient of an output before the first
 * valid step goes nowhere.
 *
 * dtype (KRS_F32 / KRS_BF16) is the type of xz, recurrent_kernel, h0, hs, h_last, the reserve and every gradient;
 * recurrent_bias is fp32 [3u] or NULL.  hs [b, l, u] is the sequence output, h_last [b, u] the final STATE (an
 * all-padding sequence: h0); either may be NULL, not both.  reserve [b, l, 4u] (krs_gru_reserve_bytes) receives
 * z, r, c, q of every step for the backward and needs hs; with reserve NULL (inference) only the outputs are written,
 * and they are bit for bit those of the training forward.
 * krs_gru_bwd reads recurrent_kernel, valid, h0, hs and the reserve back with dhs [b, l, u] and dh_last [b, u] (either
 * may be NULL = zeros) and writes dxz [b, l, 3u], da [b, l, 3u], h_prev [b, l, u] (NULL to skip: the h_{t-1} each step
 * used, the left operand of d recurrent_kernel = h_prev^T . da) and dh0 [b, u] (NULL to skip).  The weight gradients
 * are products and column sums of these, outside: d recurrent_kernel as one krs_gemm, d bias[1] = krs_colsum(da).
 *
 * Routes (csrc/gru_plan.h decides, a pure host function):
 *   KRS_GRU_FAST     bf16, u <= 128 (upad 32 / 64 / 128).  A workgroup owns 32 batch rows and walks every step alone;
 *                    the recurrent kernel is staged once into LDS as bf16; h . U and da . U^T run on
 *                    v_mfma_f32_32x32x16_bf16.  Rounded to bf16 (nearest even): recurrent_kernel and xz as given, the
 *                    A-operand copy of h, da, the reserve, the outputs.  The carried state, the carried dh and the
 *                    accumulators stay fp32.  The backward reads h_{t-1} from hs (bf16).
 *   KRS_GRU_GENERIC  fp32 at any u <= 1024, bf16 at 128 < u <= 1024: fp32 FMA, the carried state in LDS (never
 *                    rounded), the recurrent kernel read through L2 each step; 4 batch rows per workgroup.
 * One owner per output element and no atomics on either route: bit-identical from call to call.  No workgroup waits
 * on another: no grid barrier, no cooperative launch, no flags.  No host synchronisation.
 * b == 0 or l == 0 is a successful no-op.  b < 0, l < 0, u < 1, a bad dtype, a null operand, ldxz < 3u and a call that
 * wants no output are KRS_ERR_INVALID; u > 1024 is KRS_ERR_UNSUPPORTED with a message naming the limit.
 * krs_gru_last_route: the route of the process's last krs_gru_fwd / _bwd call, whichever thread made it: kernel, and
 * upad on the fast route, else 0; both zero after a refused call or a no-op.  Returns kernel.
 * ------------------------------------------------------------------------- */
enum { KRS_GRU_NONE = 0, KRS_GRU_FAST = 1, KRS_GRU_GENERIC = 2 };
size_t krs_gru_reserve_bytes(int64_t b, int64_t l, int64_t u, int dtype);
int krs_gru_fwd(const void* xz, int64_t ldxz, const void* recurrent_kernel, const float* recurrent_bias,
                const uint8_t* valid, const void* h0, int dtype, int64_t b, int64_t l, int64_t u, void* hs,
                void* h_last, void* reserve, void* stream);
int krs_gru_bwd(const void* recurrent_kernel, const uint8_t* valid, const void* h0, const void* hs,
                const void* reserve, const void* dhs, const void* dh_last, int dtype, int64_t b, int64_t l, int64_t u,
                void* dxz, void* da, void* h_prev, void* dh0, void* stream);
int krs_gru_last_route(int* kernel, int* upad);

/* ------------------------------------------------------------------------- *
 * K21  Partitioned (IVF) retrieval: K8's score + top-k over the candidates of the best few leaves only
 *
 * The partitioning stage of ScaNN on float rows (the serving side of keras_rs_amd.layers.PartitionedRetrieval).
 *   Index       centroids [leaves, d] with row stride ldm; the candidate rows c [n, d] (row stride ldc) REGROUPED so that
 *               leaf l owns the stored rows [leaf_offsets[l], leaf_offsets[l+1]) (leaf_offsets int32 [leaves + 1],
 *               ascending, from 0 to n; trusted); row_index int32 [n], the original candidate index of each stored
 *               row, ASCENDING INSIDE EVERY LEAF; ids int32 [n] INDEXED BY ORIGINAL INDEX, or NULL.
 *   Probe       The probed leaves of query row i are the krs_retrieval_topk result for q_i against the centroids with
 *               k = probes: K8's order, score descending, leaf index ascending, NaN above +inf.  out_leaves
 *               [b, probes] int32 receives them when not NULL.
 *   Select      The result is K8's top-k over the candidates of the probed leaves only, in K8's total order: the fp32
 *               score descending, then the ORIGINAL candidate index ascending, -0.0 as +0.0.  out_ids [b, k] is
 *               ids[original index], or the original index when ids is NULL; out_scores [b, k] (or NULL) is the fp32
 *               score rounded once to dtype.
 *   Short       If the probed leaves of a query hold m < k candidates, slots m .. k-1 hold id -1 (also with ids) and
 *               score -inf.
 *   Bits        A (query, candidate) score leaves the MFMA chain of krs_retrieval_topk (same K steps, same
 *               instructions, same zeroed K tail), whatever tile the query lands in.  So with probes == leaves the ids and
 *               score bits are those of krs_retrieval_topk on the same candidates in their original order, and with
 *               fewer probes those of krs_retrieval_topk on the rows of the probed leaves gathered in ascending
 *               original index with ids = those indices.
 *   Shapes      q, centroids and c share dtype (KRS_F32 / KRS_BF16).  1 <= probes <= min(leaves, 128), 1 <= k <=
 *               min(n, 128), 1 <= d <= 512, n <= INT32_MAX, b >= 0, b * probes <= INT32_MAX, row strides >= d.
 *               probes > 128 (with probes <= leaves), k > 128 (with k <= n), d > 512 and b * probes > 2^31 - 1 are
 *               KRS_ERR_UNSUPPORTED with a message naming the limit: there is no slab path.  Other bad shapes, a bad
 *               dtype, a row stride below d and a null q, centroids, c, leaf_offsets, row_index or out_ids (b > 0) are
 *               KRS_ERR_INVALID, the shape checks first; too little workspace is KRS_ERR_WORKSPACE; every refusal comes
 *               before the first launch.  b == 0 is a successful no-op.
 *   Execution   On `stream`: (a) the probe, krs_retrieval_topk on the centroids; (b) the inversion of the b * probes
 *               (query, slot) pairs into per-leaf pair lists: an integer histogram, an exclusive scan of the counts and
 *               one of the tile counts ceil(count / 32), then each pair into its leaf's segment; (c) the scan, K8's
 *               stage 1 per (leaf, tile of <= 32 pairs): the query tile gathered through the list, the candidate loop
 *               over the leaf's stored rows, the queued pair carrying row_index, k pairs written per (query, slot); the
 *               grid is the static bound ceil(b * probes / 32) + min(leaves, b * probes) and a workgroup finds its leaf
 *               by binary search in the tile scan; (d) K8's merge of the probes lists of each query.  Integer atomics
 *               place a pair inside its leaf's list; no result depends on that place.  Bit-identical from call to call,
 *               no allocation, no host wait: graph-capturable.
 * krs_retrieval_ivf_workspace_bytes: the probe's K8 workspace and its [b, probes] result, five int32 arrays of
 * leaves + 1 and the scan's partial sums, the b * probes pair list, the b * probes * k (score, index) pairs of 8 bytes,
 * and b * pow2(k) pairs for the merge when probes * k > 2048; each rounded up to 256.  The pairs dominate: this is more
 * than K8's b * S * k as soon as probes > S.  > 0 for b > 0 on a supported shape, 0 otherwise.  It need not be
 * initialised.
 * ------------------------------------------------------------------------- */
size_t krs_retrieval_ivf_workspace_bytes(int64_t b, int64_t n, int64_t d, int64_t leaves, int probes, int k, int dtype);
int krs_retrieval_ivf(const void* q, int64_t ldq, const void* centroids, int64_t ldm, const void* c, int64_t ldc,
                      const int32_t* leaf_offsets, const int32_t* row_index, const int32_t* ids, int dtype, int64_t b,
                      int64_t n, int64_t d, int64_t leaves, int probes, int k, void* out_scores, int32_t* out_ids,
                      int32_t* out_leaves, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * K22  Fused residual add + dropout + layer norm over the rows of [n, d], forward and backward
 *
 * x, residual, y, sum (and s, dy, dsum, dx, dres of the backward) are [n, d] matrices of one dtype (KRS_F32 /
 * KRS_BF16), each with a row stride of its own (>= d); gamma, beta, mean, rstd, dgamma, dbeta are fp32.  Per row i, in
 * fp32, with round() the rounding to dtype (nearest even; nothing in fp32):
 *     s_ij   = round( residual_ij + x_ij * keep_ij / (1 - p) )        residual NULL = 0; p = 0: keep = 1
 *              (1 / (1 - p) is the fp32 quotient 1.0f / (1.0f - p); the sum is ONE fused multiply-add, so s is the
 *               exactly rounded value of the line above however residual and x cancel)
 *     mean_i = (1/d) sum_j s_ij        var_i = (1/d) sum_j (s_ij - mean_i)^2        rstd_i = 1 / sqrt(var_i + eps)
 *     y_ij   = round( gamma_j * (s_ij - mean_i) * rstd_i + beta_j )   gamma NULL = 1, beta NULL = 0
 * The statistics are taken from the ROUNDED s (what an unfused composition does, and what the backward reloads), in two
 * passes over the row held in registers.  With residual NULL and p == 0, s is x itself.
 * Forms of krs_ln_fwd, by its pointers: norm (y only), add-norm (y and sum: s is written to sum, the next residual and
 * what the backward needs), add (sum only, y NULL: no statistics; gamma, beta, mean, rstd must be NULL).  mean and rstd
 * [n] may be NULL when no backward follows.
 * Dropout keeps element (i, j) by K19's hash (mix and base as written there, the row index in place of bi * h + hi):
 *     keep_ij <=> mix(base(seed, *draw, (uint32) i) + j) >= floor(p * 2^32)
 * The forward and the backward recompute it; no mask is stored.  draw is a device int64 the call only READS; NULL
 * when dropout_p == 0.
 *
 * krs_ln_bwd, with xh = (s - mean) * rstd and g = dy * gamma, all fp32:
 *     ds_ij    = rstd_i * ( g_ij - mean_j(g_i.) - xh_ij * mean_j(g_i. xh_i.) ) + dsum_ij     dy NULL: first term 0;
 *     dres     = round(ds)      dx = round(ds * keep / (1 - p))                              dsum NULL: 0
 *     dgamma_j = sum_i dy_ij xh_ij        dbeta_j = sum_i dy_ij
 * s is the forward's sum (x in the norm form).  Every output may be NULL to skip it, not all; with p == 0, dx and dres
 * are equal: ask for one.  dgamma / dbeta need dy and krs_ln_workspace_bytes(n, d) of workspace (it need not be
 * initialised; too little is KRS_ERR_WORKSPACE): every workgroup adds the rows it owns, in a fixed order, into one fp32
 * partial row per vector, and a second kernel adds the partial rows in workgroup order.  No atomics anywhere:
 * bit-identical from call to call.  No host synchronisation.
 *
 * Routes (csrc/ln_plan.h decides, a pure host function).  lanes_per_row = 8 (d <= 64), 16 (<= 128), 32 (<= 256) or 64
 * lanes of one wave own a row, 8 registers a lane up to d = 512, then 16, 32, 64; a workgroup of 4 waves has
 * 256 / lanes_per_row rows in flight and owns a contiguous block of rows.
 *   KRS_LN_VEC    every base on 16 bytes, every stride and d a whole number of 16-byte chunks (8 bf16, 4 fp32): a lane
 *                 moves 16 bytes per access.
 *   KRS_LN_ELEM   anything else (d = 50, odd strides): element accesses, consecutive lanes on consecutive columns.
 * The two routes add a row's elements in different orders; each is bit-identical to itself.
 * n == 0 is a successful no-op.  n < 0, d < 1, a bad dtype, dropout_p outside [0, 1), eps < 0, a stride below d, a
 * null x, a call that wants no output, dropout without draw, dy without s / mean / rstd, dgamma or dbeta without dy, and
 * a backward with neither dy nor dsum are KRS_ERR_INVALID.  d > 4096 (the row lives in a wave's registers) and
 * n > 2^31 - 1 are KRS_ERR_UNSUPPORTED with a message naming the limit.
 * krs_ln_last_route: the route of the process's last krs_ln_fwd / _bwd call, whichever thread made it: kernel,
 * lanes_per_row and vec; all zero after a refused call or a no-op.  Returns kernel.
 * ------------------------------------------------------------------------- */
enum { KRS_LN_NONE = 0, KRS_LN_VEC = 1, KRS_LN_ELEM = 2 };
size_t krs_ln_workspace_bytes(int64_t n, int64_t d);
int krs_ln_fwd(const void* x, int64_t ldx, const void* residual, int64_t ldr, const float* gamma, const float* beta,
               int dtype, int64_t n, int64_t d, float eps, float dropout_p, uint64_t seed, const int64_t* draw, void* y,
               int64_t ldy, void* sum, int64_t lds, float* mean, float* rstd, void* stream);
int krs_ln_bwd(const void* s, int64_t lds, const void* dy, int64_t lddy, const void* dsum, int64_t lddsum,
               const float* gamma, const float* mean, const float* rstd, int dtype, int64_t n, int64_t d, float dropout_p,
               uint64_t seed, const int64_t* draw, void* dx, int64_t lddx, void* dres, int64_t lddres, float* dgamma,
               float* dbeta, void* workspace, size_t workspace_bytes, void* stream);
int krs_ln_last_route(int* kernel, int* lanes_per_row, int* vec);

/* ------------------------------------------------------------------------- *
 * K23  Asymmetric hashing over K21's partition, and the reorder stage (ScaNN's score_ah(...) and reorder(...); the
 *      serving side of keras_rs_amd.layers.AsymmetricHashingRetrieval)
 *
 *   Index       K21's centroids [leaves, d], leaf_offsets [leaves + 1], row_index [n] and ids [n], unchanged, and in
 *               place of K21's regrouped float rows:
 *                 codebooks  bf16 [blocks][16][m], blocks = ceil(d / m), m = dimensions per block in {2, 4, 8}: 16 centres
 *                            per block, contiguous.  Columns at or beyond d of the last block are zero (the kernels read
 *                            them as zero whatever they hold).
 *                 codes      uint8 [n, ldcode], STORED (leaf) order like K21's rows, on a 4-byte boundary.  A row holds one
 *                            4-bit code per block: block j is nibble j, nibble j sits in byte j / 2, the even j in the low
 *                            four bits.  A row is krs_ah_code_bytes(d, m) = 4 * ceil(blocks / 8) bytes, the nibbles from
 *                            `blocks` on being zero; ldcode (bytes) is at least that and a multiple of 4.
 *                 rows       the float rows [n, d] in ORIGINAL order with row stride ldr, only for reordering.
 *   Residual    What a code quantizes is e = x - centroid[leaf(x)].  decode(code row) is the d-vector whose block j is
 *               codebooks[j][nibble j].
 *
 * krs_ah_encode: codes of n stored rows.  Stored row s is x[row_index[s]] (x[s] when row_index is NULL; x is [n, d] with
 * row stride ldx, KRS_F32 / KRS_BF16, centroids of the same dtype) and belongs to leaf row_leaf[s].  Per element
 * e = fsub(float(x), float(centroid)); per block and centre dist = 0, then for t = 0 .. m-1 in order u = fsub(e_t,
 * float(c_t)), dist = fadd(dist, fmul(u, u)), every operation rounded to fp32 on its own, nothing contracted; columns
 * at or beyond d count as e = 0, c = 0.  The code is the centre with the least dist, the LOWEST code on a tie: numpy
 * float32 reproduces the codes bit for bit.  A row_index outside [0, n) reads as a zero row and a row_leaf outside
 * [0, leaves) as a zero centroid.  One pass: a thread owns 8 columns of a row (16-byte loads when x, centroids, their
 * strides and d allow, element loads otherwise), the codebooks sit in LDS, m lanes OR their bits into one 4-byte store.
 * n == 0 is a successful no-op; d > 512 is KRS_ERR_UNSUPPORTED; a bad shape, dtype, m, stride, alignment or a null
 * operand is KRS_ERR_INVALID.
 *
 * krs_retrieval_rescore: the k best of each query's r listed candidates by their EXACT scores.  idx int32 [b, r] (row
 * stride ldi) holds original candidate indices; an entry outside [0, n), -1 by convention, is padding.  The result is
 * BruteForceRetrieval's order over the listed candidates: the fp32 score descending, then the index ascending, out_ids
 * = ids[index] (the index when ids is NULL), out_scores (or NULL) rounded once to dtype; id -1 and score -inf where
 * fewer than k entries are real.  Indices listed twice come back twice.
 *   Bits        A rescored score leaves K8's MFMA chain: one wave takes (query, 32 candidates), the query row is the A
 *               fragment of all 32 tile rows, the gathered rows are the B fragment, the instruction, the K-step order and
 *               the zeroed K tail are krs_retrieval_topk's for both dtypes.  So the score of (query, candidate) has the
 *               bits krs_retrieval_topk gives it.
 *   Shapes      q [b, d] and rows [n, d] share dtype; 1 <= k <= r <= 128, d <= 512 (beyond: KRS_ERR_UNSUPPORTED).
 *               Workspace: b * r pairs of 8 bytes, rounded up to 256 (0 for an unsupported shape).  The selection is
 *               K8's LDS route.  No host wait, no allocation: graph-capturable.  b == 0 is a successful no-op.
 *
 * krs_retrieval_ivf_ah: krs_retrieval_ivf with the scan over the codes.  On `stream`: (a) K21's probe, keeping its fp32
 * scores; (b) K21's inversion; (c) the scan, K21's work item (leaf, tile of <= 32 pairs) on K8's stage 1 with the B
 * fragment decoded from the codebooks in LDS, r pairs written per (query, slot); (d) K8's merge to r pairs per query;
 * (e) rows == NULL: r must equal k and the merged pairs are the result; rows != NULL: k <= r <= 128 and the merged
 * indices go through krs_retrieval_rescore's launches.
 *   AH score    of query i and a candidate of probed leaf l:
 *                   fadd( chain(bf16(q_i), decode(code)), probe_score(i, l) )
 *               chain is K8's bf16 MFMA chain (v_mfma_f32_32x32x16_bf16, K8's K steps, zeroed K tail); probe_score is
 *               the fp32 score step (a) has for (q_i, centroid_l), not rounded to dtype; fp32 queries are rounded to
 *               bf16 (nearest even) for the scan only -- probe and reorder run in `dtype`, as K21 does.
 *   Result      Without rows: K21's outputs with AH scores (order: AH score descending, original index ascending).  With
 *               rows: exact scores in krs_retrieval_rescore's order.  Short results end in id -1, score -inf.
 *   Shapes      K21's limits and refusals under this entry's name, and: m not in {2, 4, 8}, r < k, r != k without rows,
 *               a code stride below krs_ah_code_bytes or not a multiple of 4, codes off a 4-byte boundary are
 *               KRS_ERR_INVALID; r > 128 is KRS_ERR_UNSUPPORTED.  Required pointers (b > 0): q, centroids, codebooks,
 *               codes, leaf_offsets, row_index, out_ids.  b == 0 is a successful no-op.  Bit-identical from call to
 *               call, graph-capturable.
 * krs_retrieval_ivf_ah_workspace_bytes: krs_retrieval_ivf_workspace_bytes with k = r, plus b * probes fp32 probe scores,
 * plus, with reorder != 0, b * r int32 indices and b * r pairs; each rounded up to 256.  0 for b <= 0 or a refused shape.
 * ------------------------------------------------------------------------- */
int64_t krs_ah_code_bytes(int64_t d, int m);
int krs_ah_encode(const void* x, int64_t ldx, const int32_t* row_index, const int32_t* row_leaf, const void* centroids,
                  int64_t ldm, int dtype, const void* codebooks, int64_t n, int64_t d, int64_t leaves, int m,
                  uint8_t* codes, int64_t ldcode, void* stream);
size_t krs_retrieval_rescore_workspace_bytes(int64_t b, int r, int k);
int krs_retrieval_rescore(const void* q, int64_t ldq, const void* rows, int64_t ldr, const int32_t* idx, int64_t ldi,
                          const int32_t* ids, int dtype, int64_t b, int64_t n, int64_t d, int r, int k, void* out_scores,
                          int32_t* out_ids, void* workspace, size_t workspace_bytes, void* stream);
size_t krs_retrieval_ivf_ah_workspace_bytes(int64_t b, int64_t n, int64_t d, int64_t leaves, int probes, int k, int r,
                                            int m, int reorder, int dtype);
int krs_retrieval_ivf_ah(const void* q, int64_t ldq, const void* centroids, int64_t ldm, const void* codebooks, int m,
                         const uint8_t* codes, int64_t ldcode, const int32_t* leaf_offsets, const int32_t* row_index,
                         const void* rows, int64_t ldr, const int32_t* ids, int dtype, int64_t b, int64_t n, int64_t d,
                         int64_t leaves, int probes, int k, int r, void* out_scores, int32_t* out_ids, int32_t* out_leaves,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * K24  Regression head: MSE / MAE / Huber loss, its gradient and the batch sums of the regression metrics from ONE
 *      read of the predictions (keras.losses.MeanSquaredError / MeanAbsoluteError / Huber,
 *      keras.metrics.RootMeanSquaredError / MeanSquaredError / MeanAbsoluteError)
 *
 * Operands  pred [b, c] fp32 / bf16 (dtype) with row stride ld_pred >= c; target [b, c] fp32 with row stride
 *           ld_target >= c; sample_weight [b] fp32 or NULL (every w_b = 1).  b >= 0, 1 <= c <= 2^31 - 1,
 *           b <= 2^31 - 1.  b == 0 launches nothing and returns KRS_OK: no output is written (the scalar loss of no
 *           rows is 0 under every reduction, which is the caller's to store).
 * Kinds     with e = fsub(float(pred), target) per element:
 *               KRS_REGRESSION_MSE    f = e * e                         f' = e + e
 *               KRS_REGRESSION_MAE    f = |e|                           f' = sign(e)
 *               KRS_REGRESSION_HUBER  a = |e|;  a <= delta ? f = 0.5 * (e * e),          f' = e
 *                                                          : f = delta * a - 0.5 * (delta * delta), f' = delta * sign(e)
 *           sign(e) = float(e > 0) - float(e < 0) for an ordered e and e itself for a NaN: sign(+-0) = 0, and a NaN
 *           error gives a NaN gradient under every kind.  delta > 0 (read for HUBER only).
 * Row       r_b = f(e_b0) + f(e_b1) + .. in column order, from 0;  v_b = r_b / float(c);  t_b = w_b * v_b (v_b
 *           without sample_weight).
 * Reduction (krs_regression_reduction; the meanings of keras_rs_amd.losses.REDUCTIONS as K11's callers give them)
 *               NONE                     loss[b] = t_b                            s_b = w_b
 *               SUM                      loss[0] = T                              s_b = w_b
 *               SUM_OVER_BATCH_SIZE      loss[0] = T * phi, phi = 1 / float(b)    s_b = w_b * phi
 *               MEAN_WITH_SAMPLE_WEIGHT  with sample_weight: loss[0] = W != 0 ? T / W : 0,  s_b = W != 0 ? w_b / W : 0;
 *                                        without: SUM_OVER_BATCH_SIZE
 *           T = sum_b t_b and W = sum_b w_b in the summation order below (s_b = 1 or phi without sample_weight).
 * Gradient  dpred [b, c] in pred's dtype with row stride ld_dpred, or NULL (forward only):
 *               k_b = (g_b * s_b) / float(c);    dpred[b, j] = round_to_dtype(k_b * f'(e_bj))
 *           g_b = g[b] when g (device, [b] fp32) is given -- the upstream gradient of reduction NONE -- else g_scale.
 *           Every operation above is one fp32 operation rounded on its own (the kernels are compiled with
 *           fp contract off; divisions are correctly rounded), so dpred is a pure function of the inputs, bit for
 *           bit -- under MEAN_WITH_SAMPLE_WEIGHT together with the order of W.
 * Sums      sums [3] fp32 (device) or NULL, WRITTEN by the call from the same pass:
 *               with sample_weight     { sum_b w_b * (q_b / float(c)),  sum_b w_b * (a_b / float(c)),  sum_b w_b }
 *               without                { sum_b q_b,                     sum_b a_b,                     float(b * c) }
 *           q_b / a_b: the row's sum of e * e / |e| in column order.  They are keras' {total, count} updates of
 *           MeanSquaredError / RootMeanSquaredError (entries 0, 2) and MeanAbsoluteError (entries 1, 2).
 * Order     (fixed; no float atomics; the same bits from call to call)  Work is cut into items: one row on the
 *           element route, V = 4 (fp32) / 8 (bf16) consecutive rows on the vector route, whose last b % V rows are
 *           items of one row appended to workgroup 0.  G = min(KRS_REGRESSION_MAX_BLOCKS, max(1, ceil(items /
 *           KRS_REGRESSION_THREADS))) workgroups of KRS_REGRESSION_THREADS threads; thread t of workgroup j adds
 *           the items j * THREADS + t, + G * THREADS, .. in that order (rows of an item in row order), the
 *           workgroup adds its threads' sums in a halving tree (x[t] += x[t + o], o = THREADS / 2 .. 1), and the G
 *           partials are added in workgroup order.  W of MEAN_WITH_SAMPLE_WEIGHT comes from a pass of its own over
 *           the b weights BEFORE the main pass, in the element route's order over [b, 1] whatever the main route is.
 * Access    KRS_REGRESSION_VEC: c == 1, every row stride 1 and pred, target, sample_weight, g, loss (NONE) and dpred
 *           on 16 bytes: 16-byte loads of pred and stores of dpred.  KRS_REGRESSION_ELEM: everything else.  The choice
 *           is csrc/regression_plan.h's.
 * Launches  [W pass] + main + [finish, when G > 1].  No host wait, no allocation: a call captures into a HIP graph.
 * workspace krs_regression_workspace_bytes(b, c) bytes on the device (5 * KRS_REGRESSION_MAX_BLOCKS floats for b > 0,
 *           0 otherwise); it need not be initialised.  Too little is KRS_ERR_WORKSPACE.
 * Refusals  (KRS_ERR_INVALID, the value named in krs_last_error) a kind, reduction or dtype outside its enum,
 *           delta <= 0 or NaN for HUBER, b < 0, c < 1, a size above 2^31 - 1, a row stride below c, and for b > 0 a
 *           NULL pred or target, or all of loss, dpred and sums NULL.
 *
 * krs_regression_last_route: how the calling thread's last krs_regression_fwd_bwd ran (all 0 before the first call,
 * after a refusal or for b == 0): kernel, v (rows of an item), blocks (G), launches.  Returns `kernel`; route may be
 * NULL.  krs_regression_plan_route: the same answer without a GPU and without touching the record; pointers are read as
 * VALUES (nullness, alignment).  Returns what the entry returns before its first launch.
 * ------------------------------------------------------------------------- */
#define KRS_REGRESSION_MAX_BLOCKS 256
#define KRS_REGRESSION_THREADS 1024
typedef enum krs_regression_kind { KRS_REGRESSION_MSE = 0, KRS_REGRESSION_MAE = 1, KRS_REGRESSION_HUBER = 2 } krs_regression_kind;
typedef enum krs_regression_reduction {
  KRS_REGRESSION_NONE = 0,
  KRS_REGRESSION_SUM = 1,
  KRS_REGRESSION_SUM_OVER_BATCH_SIZE = 2,
  KRS_REGRESSION_MEAN_WITH_SAMPLE_WEIGHT = 3
} krs_regression_reduction;
enum { KRS_REGRESSION_ROUTE_NONE = 0, KRS_REGRESSION_VEC = 1, KRS_REGRESSION_ELEM = 2 };
typedef struct krs_regression_route {
  int32_t kernel, v, blocks, launches;
} krs_regression_route;
size_t krs_regression_workspace_bytes(int64_t b, int64_t c);
int krs_regression_fwd_bwd(int kind, float delta, int reduction, const void* pred, int64_t ld_pred, int dtype,
                           const float* target, int64_t ld_target, const float* sample_weight, int64_t b, int64_t c,
                           const float* g, float g_scale, float* loss, void* dpred, int64_t ld_dpred, float* sums,
                           void* workspace, size_t workspace_bytes, void* stream);
int krs_regression_last_route(krs_regression_route* route);
int krs_regression_plan_route(int reduction, const void* pred, int64_t ld_pred, int dtype, const float* target,
                              int64_t ld_target, const float* sample_weight, int64_t b, int64_t c, const float* g,
                              const float* loss, const void* dpred, int64_t ld_dpred, krs_regression_route* route);

#ifdef __cplusplus
}
#endif
#endif /* KRS_H_ */
