"""K26 without a GPU: the planner of krs_vocab_lookup, the home slot against the mixer krs.h writes down, the refusals
that return before a launch, and the host rules of IntegerLookup / StringLookup."""

import ctypes as C

import pytest

from keras_rs_amd import _lib as L
from keras_rs_amd import layers as kl
from keras_rs_amd.build import build
from keras_rs_amd.layers import lookup

LDS_MAX_TOKENS = 5120      # 160 KB of LDS / 16-byte slots / 2 (load 0.5)
MIN_IDS = 4096             # vocab_plan.h kLdsMinIds
FAKE = 0x10000             # pointers are read as values: any aligned non-NULL number


@pytest.fixture(scope="module")
def lib():
    build()
    return L.lib()


def plan(lib, n_tokens, n, ids=FAKE, out=FAKE, in_type=L.I64, out_type=L.I64, hint=L.VOCAB_AUTO, ipl=0, slots=None):
    route = L.VocabRoute()
    slots = (lib.krs_vocab_table_bytes(n_tokens) - 128) // 16 if slots is None else slots
    rc = lib.krs_vocab_plan_route(FAKE, slots, ids, in_type, n, 1, out, out_type, hint, ipl, C.byref(route))
    return rc, route


@pytest.mark.parametrize("n_tokens,n,hint,route,slots,ipl,blocks", [
    (0, 1, L.VOCAB_AUTO, L.VOCAB_GLOBAL, 8, 1, 1),
    (1, 1024, L.VOCAB_AUTO, L.VOCAB_GLOBAL, 8, 1, 4),
    (1024, 1 << 22, L.VOCAB_AUTO, L.VOCAB_GLOBAL, 2048, 1, 1 << 14),      # (measured: AUTO never takes the LDS route)
    (3, MIN_IDS, L.VOCAB_LDS, L.VOCAB_LDS, 8, 4, 1),
    (1024, MIN_IDS - 1, L.VOCAB_LDS, L.VOCAB_LDS, 2048, 4, 1),
    (1024, 1 << 22, L.VOCAB_LDS, L.VOCAB_LDS, 2048, 4, 256),
    (LDS_MAX_TOKENS, 1 << 16, L.VOCAB_LDS, L.VOCAB_LDS, 10240, 4, 16),
    (LDS_MAX_TOKENS, 1 << 16, L.VOCAB_AUTO, L.VOCAB_GLOBAL, 10240, 1, 256),
    (LDS_MAX_TOKENS + 1, 1 << 16, L.VOCAB_LDS, None, 10248, 0, 0),           # one token more does not fit: refused
    (LDS_MAX_TOKENS + 1, 1 << 16, L.VOCAB_GLOBAL, L.VOCAB_GLOBAL, 10248, 1, 256),
    (1 << 20, 1025, L.VOCAB_AUTO, L.VOCAB_GLOBAL, 1 << 21, 1, 5),
])
def test_planner_route_slots_and_bytes(lib, n_tokens, n, hint, route, slots, ipl, blocks):
    assert lib.krs_vocab_table_bytes(n_tokens) == 128 + 16 * slots and slots % 8 == 0 and slots >= 2 * n_tokens
    rc, r = plan(lib, n_tokens, n, hint=hint)
    if route is None:
        assert rc == -1 and (r.route, r.blocks) == (0, 0)
        return
    assert rc == 0
    assert (r.route, r.slots, r.ids_per_lane, r.blocks, r.vec) == (route, slots, ipl, blocks, int(ipl > 1))
    assert r.lds_bytes == (16 * slots if route == L.VOCAB_LDS else 0)


def test_planner_access_and_hints(lib):
    assert plan(lib, 100, 100, ipl=4)[1].vec == 1
    assert plan(lib, 100, 100, ipl=4, ids=FAKE + 8)[1].vec == 0                # ids 8 bytes off a 16-byte boundary
    assert plan(lib, 100, 100, ipl=4, out=FAKE + 8)[1].vec == 0
    assert plan(lib, 100, 100, ipl=2, in_type=L.I32)[1].vec == 0               # 2 int32 ids are 8 bytes a lane
    assert plan(lib, 100, 100, ipl=2)[1].vec == 1 and plan(lib, 100, 100, ipl=1)[1].vec == 0
    assert plan(lib, 100, 1 << 20, hint=L.VOCAB_GLOBAL, ipl=8)[1].ids_per_lane == 8
    assert plan(lib, 100, 1 << 20, hint=L.VOCAB_LDS, ipl=8)[1].ids_per_lane == 4
    rc, r = plan(lib, 100, 0)
    assert (rc, r.route, r.blocks) == (0, 0, 0)


@pytest.mark.parametrize("key", [0, 1, -1, 2 ** 32 + 1, -2 ** 63, 2 ** 63 - 1, 123456789012345])
@pytest.mark.parametrize("slots", [8, 16, 10240, (1 << 21) + 8])
def test_home_slot_is_the_mixer_of_the_header(lib, key, slots):
    m = (1 << 64) - 1
    x = key & m; x ^= x >> 30; x = x * 0xbf58476d1ce4e5b9 & m; x ^= x >> 27; x = x * 0x94d049bb133111eb & m  # noqa: E702
    x ^= x >> 31
    assert lib.krs_vocab_home_slot(key, slots) == (x * slots) >> 64


def test_refusals_before_any_launch(lib):
    bad = [plan(lib, 4, 4, slots=12)[0], plan(lib, 4, 4, slots=0)[0], plan(lib, 4, 4, in_type=2)[0],
           plan(lib, 4, 4, out_type=-1)[0], plan(lib, 4, 4, ids=None)[0], plan(lib, 4, 4, out=None)[0],
           plan(lib, 4, -1)[0], plan(lib, 4, 4, ipl=3)[0], plan(lib, 4, 4, hint=3)[0],
           plan(lib, 4, 4, ids=FAKE, out=FAKE, slots=-8)[0]]
    assert bad == [-1] * len(bad)
    # the entries themselves: every refusal returns before the first launch, so none of this needs a GPU
    assert lib.krs_vocab_lookup(None, 8, FAKE, L.I64, 4, 0, 0, 1, FAKE, L.I64, None, 0, 0, None) == -1
    assert lib.krs_vocab_lookup(FAKE, 12, FAKE, L.I64, 4, 0, 0, 1, FAKE, L.I64, None, 0, 0, None) == -1
    assert lib.krs_vocab_lookup(FAKE, 8, None, L.I64, 4, 0, 0, 1, FAKE, L.I64, None, 0, 0, None) == -1
    assert lib.krs_vocab_lookup(FAKE, 8, FAKE, 5, 4, 0, 0, 1, FAKE, L.I64, None, 0, 0, None) == -1
    assert b"slots" in lib.krs_last_error() or b"ids_itype" in lib.krs_last_error()
    assert lib.krs_vocab_upsert(None, 8, FAKE, L.I64, None, 4, L.VOCAB_SET, 1, None, None) == -1
    assert lib.krs_vocab_upsert(FAKE, 9, FAKE, L.I64, None, 4, L.VOCAB_SET, 1, None, None) == -1
    assert lib.krs_vocab_upsert(FAKE, 8, None, L.I64, None, 4, L.VOCAB_ADD, 0, None, None) == -1
    assert lib.krs_vocab_upsert(FAKE, 8, FAKE, 7, None, 4, L.VOCAB_ADD, 0, None, None) == -1
    assert lib.krs_vocab_upsert(FAKE, 8, FAKE, L.I64, None, 4, 2, 0, None, None) == -1
    assert lib.krs_vocab_export(None, 8, FAKE, FAKE, 4, FAKE, FAKE, 8, None) == -1
    assert lib.krs_vocab_export(FAKE, 8, None, FAKE, 4, FAKE, FAKE, 8, None) == -1
    assert lib.krs_vocab_export(FAKE, 20, FAKE, FAKE, 4, FAKE, FAKE, 8, None) == -1
    assert lib.krs_vocab_export(FAKE, 8, FAKE, FAKE, 4, FAKE, FAKE, 4, None) == -4
    assert lib.krs_vocab_table_bytes(-1) == 0 and lib.krs_vocab_export_workspace_bytes(12) == 0


@pytest.mark.parametrize("mask_token", [None, 0])
@pytest.mark.parametrize("num_oov", [0, 1, 3])
def test_vocabulary_rules(mask_token, num_oov):
    special = ([] if mask_token is None else [mask_token]) + [-1] * num_oov
    layer = kl.IntegerLookup(vocabulary=[12, 36, 1138], mask_token=mask_token, num_oov_indices=num_oov, device="cpu")
    assert layer.vocabulary_size() == 3 + len(special)
    assert layer.get_vocabulary() == special + [12, 36, 1138]
    assert layer.get_vocabulary(include_special_tokens=False) == [12, 36, 1138]
    strings = kl.StringLookup(vocabulary=["a", "b"], mask_token=None if mask_token is None else "", device="cpu",
                              num_oov_indices=num_oov)
    assert strings.get_vocabulary() == ([] if mask_token is None else [""]) + ["[UNK]"] * num_oov + ["a", "b"]
    assert strings.vocabulary_size() == 2 + len(special)
    # a vocabulary given WITH its special entries is the same vocabulary; the config round trip keeps everything
    again = kl.IntegerLookup.from_config(layer.get_config() | {"vocabulary": layer.get_vocabulary(), "device": "cpu"})
    assert again.get_vocabulary() == layer.get_vocabulary() and again.get_config() == layer.get_config() | \
        {"name": again.name}
    assert kl.StringLookup.from_config(strings.get_config() | {"device": "cpu"}).get_vocabulary() == \
        strings.get_vocabulary()


def test_layer_refusals(monkeypatch):
    for kwargs in ({"output_mode": "one_hot"}, {"invert": True}, {"sparse": True}, {"idf_weights": [1.0]},
                   {"vocabulary": "vocab.txt"}):
        for cls in (kl.IntegerLookup, kl.StringLookup):
            with pytest.raises(NotImplementedError, match=next(iter(kwargs))):
                cls(device="cpu", **kwargs)
    with pytest.raises(ValueError, match="repeated"):
        kl.IntegerLookup(vocabulary=[1, 2, 1], device="cpu")
    with pytest.raises(ValueError, match="reserved OOV"):
        kl.IntegerLookup(vocabulary=[1, -1], device="cpu")
    with pytest.raises(ValueError, match="max_tokens"):
        kl.IntegerLookup(vocabulary=[1, 2, 3], max_tokens=3, device="cpu")
    with pytest.raises(L.KrsError, match="no CPU fallback"):
        kl.IntegerLookup(vocabulary=[1, 2], device="cpu")([1, 2])
    monkeypatch.setattr(lookup, "fingerprint", lambda data: 7)
    with pytest.raises(ValueError, match="fingerprint"):
        kl.StringLookup(vocabulary=["a", "b"], device="cpu")


def test_state_dict_carries_the_vocabulary():
    src = kl.StringLookup(vocabulary=["x", "yy", "z"], device="cpu")
    dst = kl.StringLookup(device="cpu")
    dst.load_state_dict(src.state_dict())
    assert dst.get_vocabulary() == src.get_vocabulary() and dst.vocabulary.equal(src.vocabulary)
