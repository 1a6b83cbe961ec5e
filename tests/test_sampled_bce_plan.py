"""K29's host planner without a GPU: krs_sampled_bce_plan_route against the rule include/krs.h states (K29: Logit,
Order, Access, Launches, Refusals)."""

import ctypes as C

import pytest

from keras_rs_amd import _lib as L

A = 1 << 20        # an address on 16 bytes; A + 4 is not


def plan(d, edt=L.F32, tdt=L.F32, emb=A, lde=None, table=A, ldt=None, t=300, n=1, weight=A, demb=A, ldd=None):
    route = L.SampledBceRoute()
    rc = L.lib().krs_sampled_bce_plan_route(emb, d if lde is None else lde, edt, table, d if ldt is None else ldt, tdt,
                                            1000, A, A if n else None, L.I32, weight, t, d, n, A, demb,
                                            d if ldd is None else ldd, C.byref(route))
    return rc, route


# d, emb dtype, table dtype, overrides, vector route expected
CASES = [
    (1, L.F32, L.F32, {}, False),
    (50, L.BF16, L.BF16, {}, False),
    (64, L.F32, L.BF16, {}, True),
    (64, L.BF16, L.F32, {"emb": A + 4}, False),              # a misaligned base
    (64, L.BF16, L.BF16, {"table": A + 2}, False),
    (64, L.F32, L.F32, {"demb": A + 8}, False),
    (64, L.F32, L.F32, {"demb": None, "ldd": 0}, True),       # forward only: demb's alignment is not asked for
    (72, L.BF16, L.BF16, {"lde": 80, "t": 37}, True),         # a strided view, strides on 16 bytes
    (72, L.BF16, L.BF16, {"lde": 76}, False),                 # 152-byte rows
    (72, L.F32, L.F32, {"ldt": 76}, True),                    # 304-byte rows
    (128, L.BF16, L.F32, {"t": 1, "n": 0, "weight": None}, True),
    (136, L.F32, L.BF16, {"t": 100000, "n": 64}, True),
    (512, L.BF16, L.BF16, {"t": 5000}, True),
    (512, L.F32, L.F32, {"ldt": 513}, False),
]


@pytest.mark.parametrize("d,edt,tdt,over,vec", CASES)
def test_plan_follows_the_stated_rule(d, edt, tdt, over, vec):
    rc, route = plan(d, edt, tdt, **over)
    t, weighted = over.get("t", 300), over.get("weight", A) is not None
    g = next(g for g in (8, 16, 32, 64) if 8 * g >= d)
    blocks = min(L.SBCE_MAX_BLOCKS, -(-t // (L.SBCE_THREADS // g)))
    assert rc == 0
    assert (route.kernel, route.g, route.blocks) == (L.SBCE_VEC if vec else L.SBCE_ELEM, g, blocks)
    assert route.launches == int(weighted) + 1 + int(blocks > 1)


@pytest.mark.parametrize("over", [{"d": 0}, {"d": 513}, {"d": 64, "n": 65}, {"d": 64, "lde": 63}, {"d": 64, "ldt": 63},
                                  {"d": 64, "ldd": 63}, {"d": 64, "edt": 2}, {"d": 64, "emb": None}])
def test_plan_refusals(over):
    rc, route = plan(**over)
    assert rc == -1 and (route.kernel, route.g, route.blocks, route.launches) == (0, 0, 0, 0)
    assert b"krs_sampled_bce_fwd_bwd: bad" in L.lib().krs_last_error()

