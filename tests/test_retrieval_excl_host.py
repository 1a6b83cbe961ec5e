"""K27 without a GPU: what the planner reports for the exclusion variants, and what the two entries refuse before their
first launch (operands are addresses that are never read)."""

import pytest
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import retrieval_ops as ops

Q, C, X, OUT, WS = 0x7F0000100000, 0x7E0000100000, 0x7D0000100000, 0x7C0000100000, 0x7B0000100000


@pytest.mark.parametrize("variant,parent", [("topk_excl", "topk"), ("q8_excl", "q8")])
def test_plan_is_the_parents_plus_the_mask(variant, parent):
    for b, n, d, k in [(33, 2100, 8, 10), (64, 1 << 20, 128, 100), (8192, 1 << 20, 128, 100)]:
        rc, route = ops.plan_route(variant, b, n, d, k, torch.bfloat16)
        rc0, route0 = ops.plan_route(parent, b, n, d, k, torch.bfloat16)
        assert rc == rc0 == 0 and route["variant"] == variant and route["kernel"] == "fused"
        assert route["lds_bytes"] == route0["lds_bytes"] + 4 * (32 * 4 + 4)
        for name in ("S", "slice", "qtiles", "vec", "es", "row_bytes", "blocks", "select", "select_len"):
            assert route[name] == route0[name], name
    rc, route = ops.plan_route("topk_excl", 33, 2100, 8, 129, torch.float32)
    assert rc == 0 and route["kernel"] == "slab" and route["variant"] == "topk_excl"
    assert ops.plan_route("q8_excl", 33, 2100, 8, 129, torch.float32)[0] == -2       # no slab path over int8


def _call(q8, e, excl=X, ws_bytes=None, b=33, n=2100, d=8, k=10):
    lib = L.lib()
    if q8:
        need = lib.krs_retrieval_topk_q8_excl_workspace_bytes(b, n, d, k, e)
        rc = lib.krs_retrieval_topk_q8_excl(Q, d, L.F32, C, d, C, None, b, n, d, k, None, L.F32, OUT, None, WS,
                                            need if ws_bytes is None else ws_bytes, None, excl, e, e)
    else:
        need = lib.krs_retrieval_topk_excl_workspace_bytes(b, n, d, k, L.F32, e)
        rc = lib.krs_retrieval_topk_excl(Q, d, C, d, None, L.F32, b, n, d, k, None, OUT, WS,
                                         need if ws_bytes is None else ws_bytes, None, excl, e, e)
    return rc, need, lib.krs_last_error().decode()


@pytest.mark.parametrize("q8", [False, True])
def test_entries_refuse_before_the_first_launch(q8):
    rc, need, msg = _call(q8, 2049)
    assert rc == -2 and need == 0 and "2048" in msg                  # KRS_ERR_UNSUPPORTED naming the limit
    assert _call(q8, 5, excl=None)[0] == -1                          # KRS_ERR_INVALID: a null list with e > 0
    assert _call(q8, -1)[0] == -1
    rc, need, msg = _call(q8, 5, ws_bytes=256)
    assert rc == -4 and need > 256                                   # KRS_ERR_WORKSPACE
    parent = (L.lib().krs_retrieval_topk_q8_workspace_bytes(33, 2100, 8, 10) if q8
              else L.lib().krs_retrieval_topk_workspace_bytes(33, 2100, 8, 10, L.F32))
    assert _call(q8, 5, ws_bytes=256)[1] >= parent + 4 * 33 * 5 and _call(q8, 0, ws_bytes=0)[1] == parent
    assert ops.last_route()["kernel"] is None                        # nothing ran
