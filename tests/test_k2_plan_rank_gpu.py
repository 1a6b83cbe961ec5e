"""K2 plan: the ranking of a scatter pass (KRS_EMBED_OPT_RANK: 0 = LDS counts with a ballot fallback per round, 1 = always
ballots, 2 = always LDS counts) must not change one byte of the plan.

The sorted (key, value) arrays are read out of the plan workspace and compared with a stable numpy sort -- comparing
only the updates they lead to would miss two swapped lookups of one row whenever the row has two of them (a two-term
sum commutes).  The offsets mirror plan_layout() of keras_rs_amd/csrc/krs_bag_plan.h: with A = align256(4 * nnz),
keys_sorted starts at byte A and vals_sorted at byte 2 * A + align256(8 * nnz + 8).

Shapes: 2-3 tiles of 4096 lookups with a partial last tile (one shape of 11 / 12 tiles for the way workgroups pick their
tile), two neighbouring features on table 0.  Inside a tile, position q is wave q // 512, round (q % 512) // 64, lane
q % 64 of the scatter kernels."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KRS_EMBED_OPT_PLAN, KRS_EMBED_OPT_RANK = 2, 4
TILE, WAVE_KEYS = 4096, 512
MODES = (1, 2, 0)                       # ballots (the reference ranking), counts, automatic
FORMS = ("segmented", "global", "csr")
BATCH = {"vocab3": 1700, "crafted1023": 1500, "crafted1024": 1500, "two_pass_bad": 1031, "three_pass": 1031,
         "eleven_tiles": 5003}


def _crafted_ids(nnz, vocab, rng):
    """Ids by position for ONE table sorted in one 10-bit pass (vocab 1023: ids 0 .. 1022 and the invalid pattern fill
    10 bits), so that positions are (wave, round, lane) of the pass that ranks them."""
    ids = rng.integers(0, vocab, nnz)
    lane = np.arange(64)
    # tile 0: one id everywhere -- every wave's counter reaches 512 in one half-word (id 7: the HIGH half of word 3)
    ids[:TILE] = 7
    t1 = TILE
    # tile 1, wave 0: lanes l and 63 - l equal (32 collided pairs per round), other ids every round
    for r in range(8):
        ids[t1 + r * 64: t1 + (r + 1) * 64] = 40 * r + np.minimum(lane, 63 - lane)
    # wave 1: ids 2k and 2k + 1 in neighbouring lanes = both halves of one counter word in one instruction; even rounds
    # all lanes distinct, odd rounds lanes 2j and 2j + 1 equal (pairs whose ids 2k, 2k + 1 still share words)
    for r in range(8):
        w = t1 + WAVE_KEYS + r * 64
        ids[w: w + 64] = (lane + 64 * (r // 2)) if r % 2 == 0 else (lane >> 1) + 32 * (r // 2)
    # wave 2: as many collided lanes as the fallback threshold of a 10-bit digit allows (popc / 2 > 10 <=> 22 lanes):
    # 21 = nine pairs and a triple (count-and-fix in mode 0), then 22 = eleven pairs (ballots in mode 0); the collided
    # lanes lie anywhere in the round
    for r in range(8):
        w = t1 + 2 * WAVE_KEYS + r * 64
        perm = rng.permutation(64)
        row = 100 + lane                 # distinct
        groups = [2] * 9 + [3] if r % 2 == 0 else [2] * 11
        at = 0
        for g, n in enumerate(groups):
            row[perm[at: at + n]] = 500 + 7 * g + r
            at += n
        assert at == (21 if r % 2 == 0 else 22)
        ids[w: w + 64] = row
    # waves 3 .. 7 of tile 1 and the partial tile 2: uniform random (already there)
    assert ids.max() < vocab and nnz > 2 * TILE and nnz % TILE != 0
    return ids


@functools.lru_cache(maxsize=None)
def _shape(name):
    """(vocabs, table of every feature, hots, batch, ids, has out-of-range ids); computed once, never modified."""
    rng = np.random.default_rng(41)
    batch = BATCH[name]
    if name == "vocab3":                 # 2 key bits: every round collides in <= 3 groups of ~21 lanes
        vocabs, tix, hots = [3], [0, 0], [5, 1]
    elif name in ("crafted1023", "crafted1024"):
        # 1023 rows: ONE 10-bit pass in every form (1024 rows need an 11th bit for the invalid pattern: 6 + 5 bits, kept
        # as a second case on the same ids)
        vocabs, tix, hots = [int(name[7:])], [0, 0], [5, 2]
    elif name == "eleven_tiles":
        # 7 + 5 tiles table-segmented, 11 global: more than eight tiles and no multiple of eight -- the tiles are dealt to
        # a grid of 16 workgroups (tile = (b & 7) * 2 + (b >> 3)), those past the last tile exit
        vocabs, tix, hots = [3000, 50_000], [0, 0, 1], [4, 1, 4]
    elif name == "two_pass_bad":         # 17 bits: two passes; second table tiny
        vocabs, tix, hots = [70_000, 37], [0, 0, 1], [3, 1, 7]
    else:                                # 21 bits: three passes
        vocabs, tix, hots = [1_200_000], [0, 0], [7, 1]
    nnz = batch * sum(hots)
    if name.startswith("crafted"):
        ids = _crafted_ids(nnz, 1023, rng)
    else:
        ids = np.concatenate([rng.integers(0, vocabs[tix[f]], batch * hots[f]) for f in range(len(tix))])
    bad = name == "two_pass_bad"
    if bad:
        where = rng.permutation(nnz)[:300]
        ids[where] = np.where(where % 2 == 0, -5, 2_000_000_000)
    ids = ids.astype(np.int32)
    ids.setflags(write=False)
    return vocabs, tix, hots, batch, ids, bad


@functools.lru_cache(maxsize=None)
def _expected(name):
    """{form: (keys_sorted u32, vals_sorted u64)} by stable numpy sorts."""
    vocabs, tix, hots, batch, ids, _ = _shape(name)
    nnz = len(ids)
    row_base = np.concatenate([[0], np.cumsum(vocabs)]).astype(np.int64)
    pos = np.arange(nnz, dtype=np.int64)
    feat = np.repeat(np.arange(len(tix)), [batch * h for h in hots])
    base = np.concatenate([[0], np.cumsum([batch * h for h in hots])])[feat]
    table = np.asarray(tix)[feat]
    bag = feat * batch + (pos - base) // np.asarray(hots)[feat]
    vals = ((bag.astype(np.uint64) << np.uint64(32)) | pos.astype(np.uint64))
    id64 = ids.astype(np.int64)
    valid = (id64 >= 0) & (id64 < np.asarray(vocabs)[table])
    key = np.where(valid, row_base[table] + id64, 0xFFFFFFFF).astype(np.uint32)
    glob = np.argsort(key, kind="stable")
    # per table run: stable by id, out-of-range ids (+inf) last; the runs follow each other in table order
    seg = np.argsort(table.astype(np.int64) * (1 << 40) + np.where(valid, id64, 1 << 39), kind="stable")
    out = {"segmented": (key[seg], vals[seg]), "global": (key[glob], vals[glob])}
    out["csr"] = out["global"]
    for k, v in out.values():
        k.setflags(write=False)
        v.setflags(write=False)
    return out


def _align256(n):
    return (n + 255) // 256 * 256


def _sorted_arrays(ws, nnz):
    """keys_sorted / vals_sorted of a plan workspace (layout: see the module docstring)."""
    a = _align256(4 * nnz)
    k_off, v_off = a, 2 * a + _align256(8 * nnz + 8)
    keys = ws[k_off: k_off + 4 * nnz].view(torch.int32).cpu().numpy().view(np.uint32)
    vals = ws[v_off: v_off + 8 * nnz].view(torch.int64).cpu().numpy().view(np.uint64)
    return keys, vals


class _Problem:
    """The bags of a shape on the device; plan(form) under whatever rank mode is set."""

    def __init__(self, name, dim=8, seed=9):
        from keras_rs_amd.embedding_ops import FusedBags

        self.vocabs, self.tix, self.hots, self.batch, ids, self.bad = _shape(name)
        self.dev = torch.device("cuda:0")
        self.ids = torch.from_numpy(np.array(ids)).to(self.dev)
        self.nnz = len(ids)
        g = torch.Generator(device=self.dev).manual_seed(seed)
        self.tables = [torch.rand(v, dim, device=self.dev, generator=g) * 2 - 1 for v in self.vocabs]
        self.slots = [torch.full((v, dim), 0.1, device=self.dev) for v in self.vocabs]
        self.dim = dim
        self.fb = FusedBags(self.tables, [(self.tix[f], "sum", f * dim) for f in range(len(self.tix))], slots=self.slots,
                            lrs=[0.01 * (t + 1) for t in range(len(self.vocabs))])
        offs = np.concatenate([[0], np.cumsum(np.repeat(self.hots, self.batch))]).astype(np.int32)
        self.offsets = torch.from_numpy(offs).to(self.dev)

    def plan(self, form):
        from keras_rs_amd import _lib as L

        L.check(L.lib().krs_embed_set_option(KRS_EMBED_OPT_PLAN, 1 if form == "global" else 0), "krs_embed_set_option")
        err = torch.zeros(1, dtype=torch.int32, device=self.dev)
        if form == "csr":
            ws = self.fb.plan_backward(self.ids, self.batch, offsets=self.offsets, err_flag=err)
        else:
            ws = self.fb.plan_backward(self.ids, self.batch, hots=self.hots, err_flag=err, global_order=False)
        torch.cuda.synchronize()
        assert bool(int(err.item()) & 1) == self.bad
        return ws

    def apply_form(self, form):
        return {} if form == "csr" else {"hots": self.hots}


def _set(key, value):
    from keras_rs_amd import _lib as L

    L.check(L.lib().krs_embed_set_option(key, value), "krs_embed_set_option")


def _reset():
    from keras_rs_amd import _lib as L

    L.lib().krs_embed_set_option(KRS_EMBED_OPT_RANK, 0)
    L.lib().krs_embed_set_option(KRS_EMBED_OPT_PLAN, 0)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(BATCH))
def test_plan_arrays_equal_a_stable_sort(name, mode):
    """keys_sorted and vals_sorted, entry by entry, in the table-segmented, the global and the CSR form."""
    exp = _expected(name)
    try:
        pr = _Problem(name)
        _set(KRS_EMBED_OPT_RANK, mode)
        for form in FORMS:
            keys, vals = _sorted_arrays(pr.plan(form), pr.nnz)
            np.testing.assert_array_equal(keys, exp[form][0], err_msg=f"{name} mode {mode} {form}: keys_sorted")
            np.testing.assert_array_equal(vals, exp[form][1], err_msg=f"{name} mode {mode} {form}: vals_sorted")
    finally:
        _reset()


def test_rank_mode_is_validated():
    from keras_rs_amd import _lib as L

    try:
        assert L.lib().krs_embed_set_option(KRS_EMBED_OPT_RANK, 3) != 0
        assert L.lib().krs_embed_set_option(KRS_EMBED_OPT_RANK, -1) != 0
        assert L.lib().krs_embed_set_option(KRS_EMBED_OPT_RANK, 2) == 0
    finally:
        _reset()


@pytest.mark.parametrize("name", ["two_pass_bad", "three_pass"])
def test_updates_equal_under_every_rank_mode(name):
    """The fused Adagrad tables and slots and the fp32 dense gradient of rank modes 0 and 2 against mode 1, bit for bit."""
    res = {}
    try:
        for mode in MODES:
            _set(KRS_EMBED_OPT_RANK, mode)
            for form in FORMS:
                pr = _Problem(name)
                g = torch.Generator(device=pr.dev).manual_seed(3)
                grad = torch.rand(pr.batch, len(pr.tix) * pr.dim, device=pr.dev, generator=g) * 2 - 1
                w = torch.rand(pr.nnz, device=pr.dev, generator=g) * 0.9 + 0.1
                start = [t.clone() for t in pr.tables]
                ws = pr.plan(form)
                dense = pr.fb.backward_dense(ws, grad, pr.batch, pr.nnz, weights=w, **pr.apply_form(form))
                pr.fb.backward_fused("adagrad", ws, grad, pr.batch, pr.nnz, weights=w, **pr.apply_form(form))
                torch.cuda.synchronize()
                assert not torch.equal(start[0], pr.tables[0])
                res[mode, form] = (pr.tables, pr.slots, list(dense))
    finally:
        _reset()
    for form in FORMS:
        for mode in (0, 2):
            for part in range(3):
                for a, b in zip(res[1, form][part], res[mode, form][part]):
                    assert torch.equal(a, b), (name, mode, form, part)


def test_count_ranking_is_deterministic():
    """Two plans of the crafted shape in mode 2: the two sorted arrays byte for byte."""
    try:
        pr = _Problem("crafted1023")
        _set(KRS_EMBED_OPT_RANK, 2)
        for form in FORMS:
            a = [x.tobytes() for x in _sorted_arrays(pr.plan(form), pr.nnz)]
            b = [x.tobytes() for x in _sorted_arrays(pr.plan(form), pr.nnz)]
            assert a == b, form
    finally:
        _reset()
