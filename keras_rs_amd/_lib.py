"""ctypes binding of libkrs_hip.so (the C ABI of include/krs.h).

The HIP library is the product: there is no CPU fallback.  Importing this
module works anywhere (so `-m "not gpu"` tests can check the symbols), but any
compute call without the library or without a GPU raises.
"""

from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KRS_LIB", os.path.join(_HERE, "libkrs_hip.so"))

F32, BF16, I8 = 0, 1, 2
I32, I64 = 0, 1
SUM, MEAN, SQRTN = 0, 1, 2
COMBINERS = {"sum": SUM, "mean": MEAN, "sqrtn": SQRTN}
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH = 0, 1, 2, 3
FLAG_ID_OUT_OF_RANGE = 1
FLAG_BAD_OFFSETS = 2
FLAG_CAPACITY_OVERFLOW = 4
FLAG_NONFINITE_ROW = 8
MAX_LIST = 4096   # KRS_RANK_MAX_LIST

# struct layouts of include/krs.h
TABLE_DT = np.dtype(
    [("weights", "<u8"), ("slot", "<u8"), ("row_base", "<i8"), ("vocab", "<i4"), ("lr", "<f4")]
)
FEATURE_DT = np.dtype(
    [("ids_base", "<i8"), ("table", "<i4"), ("hot", "<i4"), ("combiner", "<i4"), ("out_col", "<i4")]
)
SHARD_FEATURE_DT = np.dtype(
    [("ids_base", "<i8"), ("comp_off", "<i8"), ("hot", "<i4"), ("combiner", "<i4"), ("vocab", "<i4"),
     ("reserved", "<i4")]
)


class GemmEpilogue(C.Structure):
    _fields_ = [
        ("bias", C.c_void_p),
        ("act", C.c_int32),
        ("diag_scale", C.c_float),
        ("x0", C.c_void_p),
        ("x", C.c_void_p),
        ("ldx", C.c_int64),
        ("u_out", C.c_void_p),
        ("ldu", C.c_int64),
        ("r", C.c_void_p),
        ("ldr", C.c_int64),
        ("beta", C.c_float),
    ]


class GemmRoute(C.Structure):
    _fields_ = [(name, C.c_int32) for name in
                ("kernel", "splits", "reduce", "epilogue", "ep_vec", "thin_width", "thin_is_a", "schedule")]


# krs_gemm_set_option keys, and the bits of GemmRoute.schedule (include/krs.h)
GEMM_OPT_PIPELINE, GEMM_OPT_EPI_SCHEDULE = 0, 1
GEMM_SCHED_LDS_LANDING, GEMM_SCHED_STAGGER, GEMM_SCHED_X_IS_X0 = 1, 2, 4


class GemmQ8Route(C.Structure):
    _fields_ = [(name, C.c_int32) for name in ("kernel", "ep_vec", "k_tail", "epilogue")]


class EmbedFwdRoute(C.Structure):
    _fields_ = [(name, C.c_int32) for name in
                ("kernel", "lpr", "has_w", "stream", "hot_rows", "bpg", "table_dtype", "out_dtype")] + [("blocks", C.c_int64)]


class DotRoute(C.Structure):
    _fields_ = [(name, C.c_int32) for name in
                ("kernel", "dtype", "ks", "fr", "self", "multi", "acc", "ng", "lps_log2", "spw", "launches",
                 "lds_bytes")] + [("blocks", C.c_int64)]


class DenseWalkRoute(C.Structure):
    _fields_ = [(name, C.c_int32) for name in ("kernel", "v", "acc", "two_stage", "rows_per_block", "reserved")] + \
               [(name, C.c_int64) for name in ("strips", "chunks", "grid_y")]


# krs_dense_walk_route.kernel and the `entry` of krs_dense_walk_plan_route (include/krs.h)
WALK_NONE, WALK_VEC, WALK_SCALAR = 0, 1, 2
WALK_CROSS_FWD, WALK_CROSS_BWD, WALK_DENSE_ACT_BWD, WALK_COLSUM = 0, 1, 2, 3


class RetrievalRoute(C.Structure):
    _fields_ = [(name, C.c_int32) for name in
                ("kernel", "variant", "es", "vec", "S", "qtiles", "row_bytes", "lds_bytes", "select",
                 "select_launches")] + [(name, C.c_int64) for name in
                                        ("slice", "blocks", "select_len", "select_p", "chunks", "chunk_rows")]


class RegressionRoute(C.Structure):
    _fields_ = [(name, C.c_int32) for name in ("kernel", "v", "blocks", "launches")]


# krs_regression_kind, krs_regression_reduction and krs_regression_route.kernel (include/krs.h)
REG_MSE, REG_MAE, REG_HUBER = 0, 1, 2
REG_NONE, REG_SUM, REG_SUM_OVER_BATCH_SIZE, REG_MEAN_WITH_SAMPLE_WEIGHT = 0, 1, 2, 3
REG_ROUTE_NONE, REG_VEC, REG_ELEM = 0, 1, 2
REG_MAX_BLOCKS, REG_THREADS = 256, 1024


# Prototype of every entry point include/krs.h declares, in its order: name -> (restype, argtypes).  Any pointer is a
# void* (pass L.ptr(t), an int or None; ctypes arrays and C.byref(struct) where the C side takes an array or a struct).
# tests/test_capi_symbols.py parses the header and checks this table against it row by row.
_P, _I, _I64, _U64, _SZ, _F = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_size_t, C.c_float
_EMBED_BWD = [_P, _I, _P, _I, _P, _P, _P, _I, _I64, _I, _I, _I, _I64]   # tables .. nnz of the fused K2 optimizers
PROTOTYPES = {
    "krs_version": (_I, []),
    "krs_last_error": (C.c_char_p, []),
    "krs_embed_bag_fwd": (_I, [_P, _P, _I, _P, _I, _P, _I, _P, _I64, _I, _I, _I, _P, _I, _I64, _P, _P, _P]),
    "krs_embed_bag_fwd_last_route": (_I, [_P]),
    "krs_embed_bag_fwd_plan_route": (_I, [_I, _P, _P, _I64, _I, _I, _I, _P, _I, _I64, _P]),
    "krs_quantize_rows_q8": (_I, [_P, _I, _I64, _I, _P, _P, _P, _P]),
    "krs_embed_bag_fwd_q8": (_I, [_P, _P, _I, _P, _I, _P, _I, _P, _I64, _I, _I, _P, _I, _I64, _P, _P]),
    "krs_embed_bag_fwd_q8_last_route": (_I, [_P]),
    "krs_embed_bag_fwd_q8_plan_route": (_I, [_I, _P, _P, _I64, _I, _I, _P, _I, _I64, _P]),
    "krs_embed_bag_bwd_workspace_bytes": (_SZ, [_I64]),
    "krs_embed_bag_bwd_plan": (_I, [_P, _P, _I, _P, _I, _P, _I, _I, _I64, _I64, _P, _SZ, _P, _P]),
    "krs_embed_bag_bwd_plan_tables": (_I, [_P, _P, _I, _P, _P, _I, _P, _I, _I, _I64, _I64, _P, _SZ, _P, _P]),
    "krs_embed_bag_bwd_dense": (_I, [_P, _I, _P, _I, _P, _P, _P, _I, _I64, _I, _I, _I64, _P, _P]),
    "krs_embed_bag_bwd_fused_sgd": (_I, _EMBED_BWD + [_P, _P]),
    "krs_embed_bag_bwd_fused_adagrad": (_I, _EMBED_BWD + [_P, _P]),
    "krs_embed_bag_bwd_fused_adagrad_rowwise": (_I, _EMBED_BWD + [_P, _P]),
    "krs_embed_bag_bwd_fused_adam": (_I, _EMBED_BWD + [_F, _F, _F, _F, _P, _P]),
    "krs_embed_bag_bwd_fused_ftrl": (_I, _EMBED_BWD + [_F, _F, _F, _F, _P, _P]),
    "krs_embed_bag_bwd_fused_adam_dyn": (_I, _EMBED_BWD + [_F, _F, _F, _P, _P, _P]),
    "krs_store_f32": (_I, [_P, _I64, _P, _I, _P]),
    "krs_embed_bag_bwd_sparse": (_I, [_P, _I, _P, _P, _P, _I, _I64, _I, _I, _I64, _P, _P, _P, _P, _P]),
    "krs_gemm": (_I, [_P, _I64, _I, _P, _I64, _I, _P, _I64, _I64, _I64, _I64, _I, _I, _P, _P, _SZ, _P]),
    "krs_gemm_workspace_bytes": (_SZ, [_I64, _I64, _I64, _I]),
    "krs_gemm_cross_bwd_workspace_bytes": (_SZ, [_I64, _I64]),
    "krs_gemm_cross_bwd": (_I, [_P, _I64, _P, _I64, _P, _I64, _F, _P, _I64, _P, _P, _P, _P, _I64, _I, _P, _I, _P,
                                _I64, _I64, _I64, _I, _I, _P, _SZ, _P]),
    "krs_gemm_dense_bwd": (_I, [_P, _I64, _P, _I64, _P, _I64, _P, _P, _I64, _P, _I64, _I64, _I64, _I, _I, _P, _SZ, _P]),
    "krs_gemm_cross_bwd_last_route": (_I, [_P]),
    "krs_gemm_cross_bwd_plan_route": (_I, [_P, _I64, _P, _I64, _P, _I64, _F, _P, _I64, _P, _P, _P, _P, _I64, _I, _P, _I64,
                                           _I64, _I64, _I, _P]),
    "krs_gemm_last_route": (_I, [_P]),
    "krs_gemm_plan_route": (_I, [_P, _I64, _I, _P, _I64, _I, _P, _I64, _I64, _I64, _I64, _I, _I, _P, _SZ, _P]),
    "krs_gemm_set_option": (_I, [_I, _I]),
    "krs_embed_set_option": (_I, [_I, _I]),
    "krs_colsum_workspace_bytes": (_SZ, [_I64, _I64]),
    "krs_cross_epilogue_fwd": (_I, [_P, _P, _P, _P, _I64, _I64, _I64, _F, _I, _P]),
    "krs_cross_epilogue_bwd": (_I, [_P, _P, _P, _P, _P, _P, _I, _P, _P, _I64, _I64, _I64, _F, _I, _I, _P, _SZ, _P]),
    "krs_cast_transpose": (_I, [_P, _I64, _I64, _I64, _I, _P, _I64, _P, _I64, _I, _P]),
    "krs_cast_transpose_many": (_I, [_I, _P, _P, _P, _I, _P, _P, _I, _P]),
    "krs_dense_act_bwd": (_I, [_P, _I64, _P, _I64, _P, _I64, _P, _I64, _I64, _I, _I, _P, _SZ, _P]),
    "krs_dense_adagrad": (_I, [_P, _P, _P, _P, _I, _F, _F, _P]),
    "krs_colsum": (_I, [_P, _I64, _I64, _I64, _I, _P, _P, _SZ, _P]),
    "krs_dense_walk_last_route": (_I, [_P]),
    "krs_dense_walk_plan_route": (_I, [_I, _I64, _I64, _I, _P, _I, _P, _I, _I, _I, _I, _P]),
    "krs_dot_interaction_fwd": (_I, [_P, _P, _I, _I64, _I, _I, _I, _I, _P, _I64, _P]),
    "krs_dot_interaction_bwd": (_I, [_P, _P, _I, _I64, _I, _I, _I, _I, _P, _I64, _P, _P, _P]),
    "krs_dot_interaction_bwd_accumulate": (_I, [_P, _P, _I, _I64, _I, _I, _I, _I, _P, _I64, _P, _P, _U64, _P]),
    "krs_dot_interaction_last_route": (_I, [_P]),
    "krs_dot_interaction_plan_route": (_I, [_I, _P, _P, _I, _I64, _I, _I, _I, _I, _P, _I64, _P, _P, _U64, _P]),
    "krs_mod_bucketize_workspace_bytes": (_SZ, [_I64, _I]),
    "krs_mod_bucketize": (_I, [_P, _I, _I64, _I, _P, _P, _P, _P, _SZ, _P]),
    "krs_bce_fwd_bwd": (_I, [_P, _I, _P, _I64, _F, _F, _P, _P, _P, _P]),
    "krs_shard_route_workspace_bytes": (_SZ, [_I64, _I64, _I]),
    "krs_shard_route": (_I, [_P, _P, _I, _P, _I, _P, _I, _P, _I64, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "krs_shard_unpack_workspace_bytes": (_SZ, [_I64]),
    "krs_shard_unpack": (_I, [_P, _I, _P, _P, _I, _P, _P, _P, _P, _SZ, _P]),
    "krs_shard_combine": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _I64, _P]),
    "krs_shard_static_block_words": (_I64, [_I64, _I64, _I]),
    "krs_shard_route_static": (_I, [_P, _P, _I, _P, _I, _P, _I, _P, _I64, _I, _I, _I, _I64, _I64, _P, _P, _P, _P, _P,
                                    _P, _P, _SZ, _P]),
    "krs_shard_unpack_static": (_I, [_P, _I, _I64, _I64, _I, _P, _P, _P, _P, _P, _SZ, _P]),
    "krs_publish_i64": (_I, [_P, _I, _P, _I64, _P]),
    "krs_topk_rows_workspace_bytes": (_SZ, [_I64, _I64, _I]),
    "krs_topk_rows": (_I, [_P, _P, _F, _I64, _I, _I64, _I64, _I, _P, _P, _P, _SZ, _P]),
    "krs_retrieval_topk_workspace_bytes": (_SZ, [_I64, _I64, _I64, _I, _I]),
    "krs_retrieval_topk": (_I, [_P, _I64, _P, _I64, _P, _I, _I64, _I64, _I64, _I, _P, _P, _P, _SZ, _P]),
    "krs_retrieval_last_route": (_I, [_P]),
    "krs_retrieval_plan_route": (_I, [_I, _P, _I64, _P, _I64, _I, _I64, _I64, _I64, _I, _P]),
    "krs_pairwise_loss": (_I, [_I, _P, _I64, _I, _P, _P, _P, _F, _F, _I64, _I64, _P, _P, _P]),
    "krs_listmle_loss": (_I, [_P, _I64, _I, _P, _P, _P, _F, _F, _I64, _I64, _P, _P, _P]),
    "krs_ranking_metrics": (_I, [_P, _I64, _I, _P, _P, _P, _I64, _I64, _F, _P, _P, _I64, _I, _U64, _P, _P, _P, _I, _I64,
                                 _I64, _P, _P, _P, _P]),
    "krs_ranking_metrics_accumulate_workspace_bytes": (_SZ, [_I64]),
    "krs_ranking_metrics_accumulate": (_I, [_P, _P, _P, _I, _I64, _P, _P, _P, _P, _P, _SZ, _P]),
    "krs_softmax_xent": (_I, [_P, _I64, _I, _P, _I64, _P, _F, _P, _F, _I64, _I64, _P, _P, _I64, _P]),
    "krs_sampling_correction": (_I, [_P, _I64, _I, _P, _I64, _F, _I64, _I64, _P, _I64, _P]),
    "krs_remove_accidental_hits": (_I, [_P, _I64, _I, _P, _I64, _P, _I, _I64, _F, _I64, _I64, _P, _I64, _P]),
    "krs_binary_metrics_workspace_bytes": (_SZ, [_I64, _I, _P]),
    "krs_binary_metrics": (_I, [_P, _I, _P, _P, _F, _I64, _F, _P, _I, _P, _P, _P, _P, _P, _SZ, _P]),
    "krs_retrieval_xent_workspace_bytes": (_SZ, [_I64, _I64, _I64, _I]),
    "krs_retrieval_xent_fwd": (_I, [_P, _I64, _P, _I64, _I, _I64, _I64, _I64, _P, _P, _P, _I, _F, _F, _P, _P, _P, _SZ,
                                    _P]),
    "krs_retrieval_xent_bwd": (_I, [_P, _I64, _P, _I64, _I, _I64, _I64, _I64, _P, _P, _P, _I, _F, _F, _P, _P, _F, _P,
                                    _I64, _P, _I64, _P, _SZ, _P]),
    "krs_retrieval_mine_workspace_bytes": (_SZ, [_I64, _I64, _I64, _I, _I]),
    "krs_retrieval_mine": (_I, [_P, _I64, _P, _I64, _I, _I64, _I64, _I64, _I, _P, _P, _P, _I, _F, _P, _P, _P, _P, _SZ,
                                _P]),
    "krs_retrieval_rank_workspace_bytes": (_SZ, [_I64, _I64, _I64, _I]),
    "krs_retrieval_rank": (_I, [_P, _I64, _P, _I64, _I, _I64, _I64, _I64, _P, _P, _I, _P, _P, _P, _SZ, _P]),
    "krs_retrieval_topk_q8_workspace_bytes": (_SZ, [_I64, _I64, _I64, _I]),
    "krs_retrieval_topk_q8": (_I, [_P, _I64, _I, _P, _I64, _P, _P, _I64, _I64, _I64, _I, _P, _I, _P, _P, _P, _SZ, _P]),
    "krs_gemm_q8": (_I, [_P, _I64, _P, _P, _I64, _P, _P, _I64, _I64, _I64, _I64, _I, _P, _P]),
    "krs_gemm_q8_last_route": (_I, [_P]),
    "krs_gemm_q8_plan_route": (_I, [_P, _I64, _P, _P, _I64, _P, _P, _I64, _I64, _I64, _I64, _I, _P, _P]),
    "krs_seq_attn_workspace_bytes": (_SZ, [_I64, _I64, _I64, _I64, _I]),
    "krs_seq_attn_fwd": (_I, [_P, _I64, _P, _I64, _P, _I64, _I, _I64, _I64, _I64, _I64, _P, _I, _F, _F, _U64, _P, _P,
                              _I64, _P, _P, _SZ, _P]),
    "krs_seq_attn_bwd": (_I, [_P, _I64, _P, _I64, _P, _I64, _I, _I64, _I64, _I64, _I64, _P, _I, _F, _F, _U64, _P, _P,
                              _I64, _P, _I64, _P, _P, _I64, _P, _I64, _P, _I64, _P, _SZ, _P]),
    "krs_seq_attn_last_route": (_I, [_P, _P]),
    "krs_gru_reserve_bytes": (_SZ, [_I64, _I64, _I64, _I]),
    "krs_gru_fwd": (_I, [_P, _I64, _P, _P, _P, _P, _I, _I64, _I64, _I64, _P, _P, _P, _P]),
    "krs_gru_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I64, _I64, _I64, _P, _P, _P, _P, _P]),
    "krs_gru_last_route": (_I, [_P, _P]),
    "krs_retrieval_ivf_workspace_bytes": (_SZ, [_I64, _I64, _I64, _I64, _I, _I, _I]),
    "krs_retrieval_ivf": (_I, [_P, _I64, _P, _I64, _P, _I64, _P, _P, _P, _I, _I64, _I64, _I64, _I64, _I, _I, _P, _P, _P,
                               _P, _SZ, _P]),
    "krs_ln_workspace_bytes": (_SZ, [_I64, _I64]),
    "krs_ln_fwd": (_I, [_P, _I64, _P, _I64, _P, _P, _I, _I64, _I64, _F, _F, _U64, _P, _P, _I64, _P, _I64, _P, _P, _P]),
    "krs_ln_bwd": (_I, [_P, _I64, _P, _I64, _P, _I64, _P, _P, _P, _I, _I64, _I64, _F, _U64, _P, _P, _I64, _P, _I64, _P,
                        _P, _P, _SZ, _P]),
    "krs_ln_last_route": (_I, [_P, _P, _P]),
    "krs_ah_code_bytes": (_I64, [_I64, _I]),
    "krs_ah_encode": (_I, [_P, _I64, _P, _P, _P, _I64, _I, _P, _I64, _I64, _I64, _I, _P, _I64, _P]),
    "krs_retrieval_rescore_workspace_bytes": (_SZ, [_I64, _I, _I]),
    "krs_retrieval_rescore": (_I, [_P, _I64, _P, _I64, _P, _I64, _P, _I, _I64, _I64, _I64, _I, _I, _P, _P, _P, _SZ, _P]),
    "krs_retrieval_ivf_ah_workspace_bytes": (_SZ, [_I64, _I64, _I64, _I64, _I, _I, _I, _I, _I, _I]),
    "krs_retrieval_ivf_ah": (_I, [_P, _I64, _P, _I64, _P, _I, _P, _I64, _P, _P, _P, _I64, _P, _I, _I64, _I64, _I64, _I64,
                                  _I, _I, _I, _P, _P, _P, _P, _SZ, _P]),
    "krs_regression_workspace_bytes": (_SZ, [_I64, _I64]),
    "krs_regression_fwd_bwd": (_I, [_I, _F, _I, _P, _I64, _I, _P, _I64, _P, _I64, _I64, _P, _F, _P, _P, _I64, _P, _P, _SZ,
                                    _P]),
    "krs_regression_last_route": (_I, [_P]),
    "krs_regression_plan_route": (_I, [_I, _P, _I64, _I, _P, _I64, _P, _I64, _I64, _P, _P, _P, _I64, _P]),
}
SYMBOLS = list(PROTOTYPES)

_lib = None


class KrsError(RuntimeError):
    pass


def lib() -> C.CDLL:
    """Loads libkrs_hip.so; loud failure when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise KrsError(
                f"{LIB_PATH} is missing: build it with `python -m keras_rs_amd.build` "
                "(hipcc --offload-arch=gfx950).  keras_rs_amd has no CPU fallback."
            )
        handle = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in PROTOTYPES.items():
            fn = getattr(handle, name, None)   # (an older build loaded through KRS_LIB may lack newer entries)
            if fn is not None:
                fn.restype, fn.argtypes = restype, argtypes
        _lib = handle
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise KrsError(f"{what} failed ({rc}): {lib().krs_last_error().decode()}")


def require_device(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise KrsError(
            f"{what}: tensor is on {t.device}; keras_rs_amd runs on MI355X HIP kernels only "
            "(no CPU fallback)"
        )


def rowmajor(t: torch.Tensor, what: str, expected: str = "a matrix") -> torch.Tensor:
    """t itself when a kernel can walk it as rows with a leading dimension (read ld = t.stride(0), or the width when
    there is one row at most), else a contiguous copy."""
    require_device(t, what)
    if t.dim() != 2:
        raise KrsError(f"{what}: expected {expected}, got shape {tuple(t.shape)}")
    # a row-broadcast view (strides (0, 1), e.g. the gradient of y.sum(0)) has no leading dimension a kernel can walk
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        return t.contiguous()
    return t


def ptr(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def fdtype(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise KrsError(f"unsupported float dtype {t.dtype} (float32 / bfloat16 only)")


def itype(t: torch.Tensor) -> int:
    if t.dtype == torch.int32:
        return I32
    if t.dtype == torch.int64:
        return I64
    raise KrsError(f"unsupported index dtype {t.dtype} (int32 / int64 only)")


# page-locked staging blocks set aside for descriptor uploads issued while a stream is CAPTURING (hipHostMalloc is not
# allowed then, and the memcpy node of the graph reads its source at every replay: a block handed out there is never
# reused)
_CAPTURE_PIN_BYTES = 4096
_capture_pins: list = []
_capture_pins_held: list = []


def _reserve_capture_pins(count: int = 64) -> None:
    if not _capture_pins and not _capture_pins_held:
        block = torch.empty(count * _CAPTURE_PIN_BYTES, dtype=torch.uint8).pin_memory()
        _capture_pins.extend(block[i * _CAPTURE_PIN_BYTES:(i + 1) * _CAPTURE_PIN_BYTES] for i in range(count))


def struct_to_device(arr: np.ndarray, device) -> torch.Tensor:
    """Uploads a numpy structured array (krs_table / krs_feature) as raw bytes."""
    host = torch.from_numpy(arr.view(np.uint8).reshape(-1).copy())
    if torch.device(device).type == "cuda":
        if torch.cuda.is_current_stream_capturing():
            n = host.numel()
            if n > _CAPTURE_PIN_BYTES or not _capture_pins:
                raise KrsError("descriptor upload during graph capture: run the step eagerly first (descriptors are "
                               "cached; the few that change per step use a reserved page-locked block of 4 KB)")
            pin = _capture_pins.pop()
            _capture_pins_held.append(pin)
            pin[:n].copy_(host)
            dev = torch.empty(n, dtype=torch.uint8, device=device)
            dev.copy_(pin[:n], non_blocking=True)
            return dev
        _reserve_capture_pins()
        # page-locked staging + asynchronous copy: a pageable upload makes the host wait for everything
        # queued on the stream (a pipeline drain per descriptor; the host allocator keeps the staging
        # block alive until the copy has run)
        return host.pin_memory().to(device, non_blocking=True)
    return host.to(device)
