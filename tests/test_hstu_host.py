"""K31 without a GPU: the planner's record for the case table of tests/test_hstu_attention_gpu.py, every documented
limit and invalid argument, the workspace of the partial dpos tables, and HSTUBlock's host logic."""

import ctypes as C

import pytest
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import layers
from keras_rs_amd import sequence_ops as S
from keras_rs_amd.build import build
from tests.test_hstu_attention_gpu import CASES, FAST

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -4


@pytest.fixture(scope="module", autouse=True)
def _library():
    build()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c[:9]))
def test_the_planner_gives_the_stated_record(case):
    dtype, b, h, l, dh, bias, _, _, packed, route, dpad = case
    td = torch.bfloat16 if dtype == "bf16" else torch.float32
    hb = {"none": 0, "shared": 1, "per_head": h}[bias]
    for backward in (False, True):
        rc, rec = S.hstu_plan_route(b, h, l, dh, td, ld=4 * h * dh if packed else None, hb=hb, backward=backward)
        assert rc == OK and (rec.kernel, rec.dpad) == (route, dpad)
        assert rec.vec == int(route == FAST and dh % 8 == 0)
        if route == FAST:                       # tiles, validity, window; with dpos the exchange tiles and the bins
            lds = 256 * dpad + 256 + 1280
            bins = -(-l // 32) * 32 + 128
            assert rec.lds_bytes == lds + (4 * (4096 + bins) if backward and hb else 0)
        # the workspace holds one table per workgroup of the key sweep (fast) or per (b, h) (generic)
        tables = b * h * -(-l // 128) * bins if route == FAST else b * h * (2 * l - 1)
        assert S.hstu_workspace_bytes(b, h, l, dh, td, hb) == (-(-4 * tables // 256) * 256 if hb else 0)


def _plan(b=2, h=3, l=40, dh=16, dtype=L.BF16, ld=None, hb=0, pos=None):
    rec = L.HstuAttnRoute(7, 7, 7, 7)
    ld = h * dh if ld is None else ld
    rc = L.lib().krs_hstu_attn_plan_route(256, ld, 256, ld, 256, ld, dtype, b, h, l, dh, pos, hb, None, ld, None,
                                          C.addressof(rec))
    return rc, (rec.kernel, rec.dpad, rec.vec, rec.lds_bytes)


@pytest.mark.parametrize("kwargs, code, names", [
    (dict(l=4097), UNSUPPORTED, "l <= 4096"), (dict(dh=257), UNSUPPORTED, "dh <= 256"),
    (dict(b=2 ** 20, h=2 ** 4, l=2 ** 8), UNSUPPORTED, "2^31"), (dict(b=-1), INVALID, "b >= 0"),
    (dict(h=0), INVALID, "h >= 1"), (dict(dh=0), INVALID, "dh >= 1"), (dict(dtype=7), INVALID, "dtype"),
    (dict(hb=2, pos=256), INVALID, "hb"), (dict(ld=47), INVALID, "stride"),
])
def test_limits_and_invalid_arguments_return_their_codes(kwargs, code, names):
    rc, rec = _plan(**kwargs)
    assert rc == code and rec == (0, 0, 0, 0)
    assert names in L.lib().krs_last_error().decode()


def test_no_ops_workspace_refusals_and_null_gradients():
    assert _plan(b=0) == (OK, (0, 0, 0, 0)) and _plan(l=0) == (OK, (0, 0, 0, 0))
    assert _plan(dh=50)[1][:3] == (FAST, 64, 0) and _plan(ld=50, dh=16)[1][:3] == (FAST, 32, 0)
    lib = L.lib()
    head = (256, 48, 256, 48, 256, 48, L.BF16, 2, 3, 40, 16)
    tail = (None, 1, 1.0, 1.0, 256, 48)                      # valid, causal, alpha, inv_n, dout, lddo
    grads = (256, 48, 256, 48, 256, 48)
    need = S.hstu_workspace_bytes(2, 3, 40, 16, torch.bfloat16, 1)
    assert need >= 2 * 3 * (64 + 128) * 4
    assert lib.krs_hstu_attn_bwd(*head, 256, 1, *tail, *grads, 256, 256, need - 1, None) == WORKSPACE
    assert lib.krs_hstu_attn_bwd(*head, None, 0, *tail, *grads, 256, None, 0, None) == INVALID       # dpos without pos
    assert lib.krs_hstu_attn_bwd(*head, None, 0, *tail, None, 48, None, 48, None, 48, None, None, 0, None) == INVALID
    assert "no gradient" in lib.krs_last_error().decode()
    assert lib.krs_hstu_attn_fwd(*head, None, 0, None, 1, 1.0, 1.0, None, 48, None) == INVALID       # null output
    assert lib.krs_hstu_attn_last_route(None) == 0


def test_hstu_block_weights_config_and_refusals():
    blk = layers.HSTUBlock(2, 4, 10, position_bias="per_head", dropout=0.1, seed=3, device="cpu")
    blk.build((2, 7, 12))
    assert [tuple(w.shape) for w in blk.weights] == [(12,), (12,), (12, 32), (32,), (2, 19), (8,), (8,), (8, 12), (12,)]
    shared = layers.HSTUBlock(2, 4, 10, device="cpu")
    shared.build((2, 7, 12))
    assert tuple(shared.position_table.shape) == (1, 19)
    none = layers.HSTUBlock(2, 4, 10, position_bias=None, device="cpu")
    none.build((2, 7, 12))
    assert none.position_table is None and len(none.weights) == 8
    cfg = blk.get_config()
    assert layers.HSTUBlock.from_config(cfg).get_config() == cfg
    assert (cfg["num_heads"], cfg["key_dim"], cfg["max_length"], cfg["position_bias"], cfg["seed"]) == (2, 4, 10, "per_head", 3)
    for kwargs, name in ((dict(num_heads=0), "num_heads"), (dict(key_dim=0), "key_dim"), (dict(max_length=0), "max_length"),
                         (dict(position_bias="relative"), "position_bias"), (dict(dropout=1.0), "dropout"),
                         (dict(max_length=5000), "max_length")):
        with pytest.raises(ValueError, match=name):
            layers.HSTUBlock(**{**dict(num_heads=2, key_dim=4, max_length=10), **kwargs})
    with pytest.raises(ValueError, match="max_length"):
        blk(torch.zeros(2, 11, 12))
    with pytest.raises(ValueError, match=r"\[B, L, d\]"):
        blk(torch.zeros(11, 12))
    assert "HSTUBlock" in layers.__all__
