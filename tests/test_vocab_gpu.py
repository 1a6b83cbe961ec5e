"""K26 on the GPU: krs_vocab_lookup / _upsert / _export and the lookup layers against a plain Python dict (and
collections.Counter).  Results are integers: every comparison is exact."""

import ctypes as C
from collections import Counter

import numpy as np
import pytest
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import layers as kl
from keras_rs_amd import vocab_ops as V

pytestmark = pytest.mark.gpu
DEV = "cuda"
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
LDS_MAX_TOKENS = 5120


def dev(values, dtype=torch.int64):
    return torch.tensor(list(values), dtype=dtype, device=DEV)


def expect(vocab, ids, mask_token=None, num_oov=1):
    """Keras' index layout from a dict"""
    where = {int(t): i for i, t in enumerate(vocab)}
    start = num_oov + (mask_token is not None)
    oov = {0: lambda t: -1, 1: lambda t: start - 1}.get(num_oov, lambda t: start - num_oov + t % num_oov)
    return [0 if t == mask_token else start + where[t] if t in where else oov(t) for t in ids]


def check(vocab, ids, table=None, ids_dtype=torch.int64, **kw):
    table = V.build_table(dev(vocab)) if table is None else table
    got = V.lookup(table, dev(ids, ids_dtype), **kw)
    want = expect(vocab, ids, kw.get("mask_token"), kw.get("num_oov_indices", 1))
    assert got.dtype == kw.get("out_dtype", torch.int64) and got.cpu().tolist() == want


@pytest.mark.parametrize("home", [15, 6])      # the chain wraps past the end / crosses the 128-byte line (slots 7 | 8)
@pytest.mark.parametrize("hint", [L.VOCAB_GLOBAL, L.VOCAB_LDS])
def test_probe_chains(home, hint):
    same = [k for k in range(4096) if V.home_slot(k, 16) == home]
    vocab, absent_same = same[:5], same[5:9]
    table = V.build_table(dev(vocab), slots=16)
    occupied = {(home + i) % 16 for i in range(5)}
    absent_empty = [k for k in range(4096, 8192) if V.home_slot(k, 16) not in occupied][:4]
    check(vocab, vocab + absent_same + absent_empty + vocab[::-1], table=table, route_hint=hint)
    keys, places = V.export(table)
    assert sorted(zip(keys.cpu().tolist(), places.cpu().tolist())) == sorted(zip(vocab, range(5)))
    slot_of = {k: (table.buf[16:].view(-1, 2)[:, 0] == k).nonzero().item() for k in vocab}
    assert set(slot_of.values()) == occupied


@pytest.mark.parametrize("ids_dtype,out_dtype", [(torch.int64, torch.int64), (torch.int32, torch.int32),
                                                 (torch.int32, torch.int64), (torch.int64, torch.int32)])
@pytest.mark.parametrize("ipl", [0, 2, 4, 8])
def test_keys_and_dtypes(ids_dtype, out_dtype, ipl):
    vocab = [0, -1, I64_MIN, I64_MAX, 2 ** 32, 2 ** 32 + 1, 7]
    ids = [0, -1, 7, 1, -7, 2 ** 31 - 1, -2 ** 31] * 5 if ids_dtype == torch.int32 else \
        vocab + [1, I64_MIN + 1, I64_MAX - 1, 2 ** 32 - 1, 2 ** 32 + 2] * 6
    check(vocab, ids[:33], ids_dtype=ids_dtype, out_dtype=out_dtype, ids_per_lane=ipl)     # 33: no multiple of 2, 4, 8
    check([t for t in vocab if t != I64_MIN], [I64_MIN, 0], ids_per_lane=ipl)              # an absent side-slot token
    check([5], [5, 6, 5], ids_dtype=ids_dtype, out_dtype=out_dtype, ids_per_lane=ipl)      # a vocabulary of one token
    check(vocab, [], ids_dtype=ids_dtype, out_dtype=out_dtype, ids_per_lane=ipl)           # n = 0


@pytest.mark.parametrize("hint", [L.VOCAB_GLOBAL, L.VOCAB_LDS])
def test_ids_off_the_16_byte_boundary(hint):
    vocab = list(range(100, 140))
    ids = list(range(90, 150)) * 3 + [1]
    buf = dev([0] + ids)
    view = buf[1:]
    assert view.data_ptr() % 16 == 8
    got = V.lookup(V.build_table(dev(vocab)), view, route_hint=hint, ids_per_lane=4)
    assert V.last_route().vec == 0 and got.cpu().tolist() == expect(vocab, ids)
    check(vocab, ids, route_hint=hint, ids_per_lane=4)
    assert V.last_route().vec == 1


@pytest.mark.parametrize("mask_token", [None, 0])
@pytest.mark.parametrize("num_oov", [0, 1, 3])
def test_index_layout(mask_token, num_oov):
    vocab = [12, 36, 1138, -5, I64_MAX]
    ids = [36, 0, -7, -1, -3, 4, 5, 1138, I64_MIN, -5, 12, 7]
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    check(vocab, ids, mask_token=mask_token, num_oov_indices=num_oov, err_flag=err)
    assert err.item() == (L.FLAG_OOV_TOKEN if num_oov == 0 else 0)
    err.zero_()
    check(vocab, vocab + ([0] if mask_token == 0 else []), mask_token=mask_token, num_oov_indices=num_oov, err_flag=err)
    assert err.item() == 0
    layer = kl.IntegerLookup(vocabulary=vocab, mask_token=mask_token, num_oov_indices=max(num_oov, 1), device=DEV)
    shaped = dev(ids).reshape(3, 4)
    assert layer(shaped).tolist() == np.reshape(expect(vocab, ids, mask_token, max(num_oov, 1)), (3, 4)).tolist()
    if num_oov == 0:
        with pytest.raises(ValueError, match="num_oov_indices=0"):
            kl.IntegerLookup(vocabulary=vocab, mask_token=mask_token, num_oov_indices=0, device=DEV)(shaped)


@pytest.mark.parametrize("n_tokens,hint,route", [(LDS_MAX_TOKENS, L.VOCAB_LDS, L.VOCAB_LDS),
                                                 (LDS_MAX_TOKENS, L.VOCAB_AUTO, L.VOCAB_GLOBAL),
                                                 (LDS_MAX_TOKENS + 1, L.VOCAB_AUTO, L.VOCAB_GLOBAL)])
def test_routes(n_tokens, hint, route):
    rng = np.random.default_rng(n_tokens)
    vocab = rng.permutation(np.unique(rng.integers(0, 1 << 40, 2 * n_tokens))[:n_tokens]).tolist()
    ids = rng.choice(vocab, 4096 + 3).tolist() + rng.integers(1 << 40, 1 << 41, 300).tolist()
    table = V.build_table(dev(vocab))
    ids_t, want = dev(ids), expect(vocab, ids, num_oov=3)
    got = V.lookup(table, ids_t, num_oov_indices=3, route_hint=hint)
    ran, planned = V.last_route(), L.VocabRoute()
    L.lib().krs_vocab_plan_route(L.ptr(table.buf), table.slots, L.ptr(ids_t), L.I64, len(ids), 3, L.ptr(got), L.I64, hint,
                                 0, C.byref(planned))
    fields = [name for name, _ in L.VocabRoute._fields_]
    assert ran.route == route and [getattr(ran, f) for f in fields] == [getattr(planned, f) for f in fields]
    assert got.cpu().tolist() == want
    if n_tokens > LDS_MAX_TOKENS:
        with pytest.raises(L.KrsError, match="does not fit in LDS"):
            V.lookup(table, ids_t, route_hint=L.VOCAB_LDS)


def test_set_mode_flags_a_repeated_key():
    assert V.build_table(dev([3, 1, 2])).n_items() == 3
    with pytest.raises(ValueError, match="repeated"):
        V.build_table(dev([3, 1, 3]))
    with pytest.raises(ValueError, match="repeated"):
        V.build_table(dev([I64_MIN, 1, I64_MIN]))


@pytest.mark.parametrize("batch", [[42] * 4096, list(range(-2000, 2096)), [I64_MIN, 5, I64_MIN, I64_MAX, 5, 5]])
def test_add_mode_counts(batch):
    table = V.count_into(V.new_table(0, DEV), dev(batch))
    keys, counts = V.export(table)
    assert dict(zip(keys.cpu().tolist(), counts.cpu().tolist())) == dict(Counter(batch)) and \
        table.n_items() == len(set(batch)) <= table.capacity


def test_adapt_rehashes_and_orders_like_keras():
    first, second = [7] * 3 + [9] * 3 + [1, 2], list(range(100, 400)) + [9, 5, 5, 5, 0]
    layer = kl.IntegerLookup(mask_token=0, device=DEV)
    layer.adapt([dev(first), dev(second)])      # 8 ids fit the first table; 305 more force a rehash
    counts = Counter(first + second)
    del counts[0]
    order = sorted(counts, key=lambda t: (counts[t], t), reverse=True)
    assert layer.get_vocabulary() == [0, -1] + order and order[:4] == [9, 7, 5, 399]
    cut = kl.IntegerLookup(max_tokens=7, mask_token=0, device=DEV)      # 5 learned tokens: cuts through the tie of ones
    cut.adapt(dev(first + second))
    assert cut.get_vocabulary() == [0, -1, 9, 7, 5, 399, 398] and cut.vocabulary_size() == 7
    assert cut(dev([399, 7, 397, 0])).tolist() == [5, 3, 1, 0]
    strings = kl.StringLookup(max_tokens=4, device=DEV)
    strings.adapt([["b", "a", "c"], ["c", "a", "d"]])
    assert strings.get_vocabulary() == ["[UNK]", "c", "a", "d"]
    assert strings([["a", "zz"], ["d", "c"]]).tolist() == [[2, 0], [3, 1]]


def test_ragged_and_state():
    layer = kl.IntegerLookup(vocabulary=[10, 20, 30], device=DEV)
    offsets = dev([0, 2, 2, 5], torch.int32)
    out = layer(kl.Ragged(dev([20, 11, 30, 10, 20]), offsets))
    assert out.values.tolist() == [2, 0, 3, 1, 2] and out.row_offsets is offsets
    other = kl.IntegerLookup(device=DEV)
    other.load_state_dict(layer.state_dict())
    assert other.get_vocabulary() == layer.get_vocabulary() and other(dev([30, 31])).tolist() == [3, 0]


@pytest.mark.parametrize("n_ids,hint", [(37, L.VOCAB_AUTO), (4096 + 5, L.VOCAB_LDS)])
def test_graph_capture_replays_on_new_ids(n_ids, hint):
    vocab = list(range(1000, 1300))
    table = V.build_table(dev(vocab))
    rng = np.random.default_rng(n_ids)
    ids = dev(rng.integers(900, 1400, n_ids).tolist())
    eager = V.lookup(table, ids, num_oov_indices=2, route_hint=hint)      # (a first run outside the capture)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = V.lookup(table, ids, num_oov_indices=2, route_hint=hint)
    for seed in range(3):
        fresh = np.random.default_rng(seed).integers(900, 1400, n_ids).tolist()
        ids.copy_(dev(fresh))
        graph.replay()
        assert out.cpu().tolist() == expect(vocab, fresh, num_oov=2)
    assert eager.shape == out.shape
