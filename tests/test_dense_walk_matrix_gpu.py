"""Every case of tests/dense_walk_cases.py through the entry it names (the C ABI directly: the Python wrappers only pass
ld = n and aligned bases), against the float64 restatement (tests/dense_walk_restatement.py) at the bounds whose count
of roundings the case module's docstring writes out:

  * krs_dense_walk_last_route is the route the case claims -- kernel, v, the ACC build, two-stage, rows_per_block, strips,
    chunks, grid_y -- so no "vector" case passes on the scalar kernel;
  * every elementwise output is within C u M (+ 2^-8 |ref| for a bf16 output), every column sum within
    (depth + 4) u M with the depth of ITS route, the BCE loss within (chain + 9) u M;
  * pad columns (n .. ld - 1) of every input hold NaN; the pad columns of every output, a guard row behind row m - 1 and
    the live elements of outputs that are not accumulated into start as a NaN bit pattern: outside the live elements
    that pattern is unchanged afterwards, inside it nothing of it is left (so dx0's initial values are not read on the
    plain build);
  * the two-stage column sums are the same bits over two calls; the atomics form is held to the bound alone.

Each case prints its largest error as a fraction of its bound (`ratio ...`), the last test the largest per entry, dtype
and output: measured values, recorded in DESIGN.md, not used to set a bound."""

import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import dense_ops
from tests import dense_walk_cases as T
from tests.test_dense_walk_host import FIELDS, route_tuple

pytestmark = pytest.mark.gpu

IDS = [c.name for c in T.CASES]
NAN = {"fp32": 0x7FC00000, "bf16": 0x7FC0}            # the pads of the inputs
SENTINEL = {"fp32": 0x7FC12345, "bf16": 0x7FC1}       # outputs before the call: a NaN no arithmetic produces
BITS = {"fp32": np.uint32, "bf16": np.uint16}
WORST = {}


def to_bits(values, dtype):
    b = np.ascontiguousarray(values, dtype=np.float64).astype(np.float32).view(np.uint32)
    return b if dtype == "fp32" else (b >> 16).astype(np.uint16)


def from_bits(bits, dtype):
    b = bits.astype(np.uint32) if dtype == "fp32" else bits.astype(np.uint32) << 16
    return b.view(np.float32).astype(np.float64)


class Matrix:
    """An [m, n] operand with leading dimension ld, `off` elements into a flat device buffer that also holds a guard row."""

    def __init__(self, dtype, m, n, ld, off, values=None, fill=None):
        self.dtype, self.m, self.n, self.ld, self.off = dtype, m, n, ld, off
        host = np.full(off + (m + 1) * ld + 8, NAN[dtype] if fill is None else fill, dtype=BITS[dtype])
        self.rows = host[off:off + m * ld].reshape(m, ld)[:, :n]        # (a view of host)
        if values is not None:
            self.rows[...] = to_bits(values, dtype)
        self.live = np.zeros(host.shape, dtype=bool)
        self.live[off:off + m * ld].reshape(m, ld)[:, :n] = True
        self.before = host
        signed = host.view(np.int32 if dtype == "fp32" else np.int16)
        self.dev = torch.from_numpy(signed).cuda()
        self.ptr = self.dev.data_ptr() + off * host.itemsize
        assert self.dev.data_ptr() % 16 == 0

    def read(self):
        """(the live elements as float64, whether everything else kept its bits)"""
        after = self.dev.cpu().numpy().view(BITS[self.dtype])
        kept = np.array_equal(after[~self.live], self.before[~self.live])
        got = after[self.off:self.off + self.m * self.ld].reshape(self.m, self.ld)[:, :self.n]
        return from_bits(got, self.dtype), kept


def vector_out(n):
    return Matrix("fp32", 1, n, n, 0, fill=SENTINEL["fp32"])


def last_route():
    rt = L.DenseWalkRoute()
    L.lib().krs_dense_walk_last_route(C.byref(rt))
    return route_tuple(rt)


def workspace(case):
    if case.ws != "two_stage":
        return None, None, 0
    nbytes = int(L.lib().krs_colsum_workspace_bytes(case.m, case.n))
    ws = torch.full((nbytes,), 0x7F, dtype=torch.uint8, device="cuda")
    return ws, ws.data_ptr(), nbytes


def launch(case, t, ins):
    """One call of the case's entry on fresh outputs -> {name: Matrix} of its outputs."""
    lib, dt, st = L.lib(), (L.BF16 if case.dtype == "bf16" else L.F32), L.stream_ptr()
    m, n, off = case.m, case.n, case.off
    new = lambda ld, values=None: Matrix(case.dtype, m, n, ld, off, values, fill=SENTINEL[case.dtype])
    ws, ws_ptr, ws_bytes = workspace(case)
    outs = {}
    if case.entry == "cross_fwd":
        outs["y"] = new(case.lds[0])
        rc = lib.krs_cross_epilogue_fwd(ins["u"].ptr, ins["x0"].ptr, ins["x"].ptr, outs["y"].ptr, m, n, case.lds[0], case.diag, dt, st)
    elif case.entry == "cross_bwd":
        ld = case.lds[0]
        for name in case.outs:
            outs[name] = vector_out(n) if name == "dbias" else new(ld, t["init"] if name == "dx0" and case.acc else None)
        ptr = lambda name: outs[name].ptr if name in outs else None
        rc = lib.krs_cross_epilogue_bwd(ins["g"].ptr, None if case.u_null else ins["u"].ptr, ins["x0"].ptr, ins["x"].ptr, ptr("dz"),
                                        ptr("dx0"), int(case.acc), ptr("dx0") if case.fold else ptr("dxd"), ptr("dbias"), m, n, ld,
                                        case.diag, case.act, dt, ws_ptr, ws_bytes, st)
    elif case.entry == "dense_act_bwd":
        ldg, ldy, ldz = case.lds
        if "dz" in case.outs:
            outs["dz"] = new(ldz)
        if "dbias" in case.outs:
            outs["dbias"] = vector_out(n)
        ptr = lambda name: outs[name].ptr if name in outs else None
        rc = lib.krs_dense_act_bwd(ins["g"].ptr, ldg, ins["y"].ptr if case.act else None, ldy, ptr("dz"), ldz, ptr("dbias"), m, n,
                                   case.act, dt, ws_ptr, ws_bytes, st)
    else:
        outs["colsum"] = vector_out(n)
        rc = lib.krs_colsum(ins["a"].ptr, case.lds[0], m, n, dt, outs["colsum"].ptr, ws_ptr, ws_bytes, st)
    L.check(rc, case.entry)
    torch.cuda.synchronize()
    return outs


def record(case, name, ratio):
    key = (case.entry, case.dtype, name)
    WORST[key] = max(WORST.get(key, 0.0), ratio)


@pytest.mark.parametrize("index", [i for i, c in enumerate(T.CASES) if c.entry != "bce"], ids=[n for n in IDS if not n.startswith("bce")])
def test_case_runs_on_its_route_within_its_bound_and_touches_nothing_else(index):
    case = T.CASES[index]
    t, ref, mag, bound = T.reference_of(index)
    lds = dict(zip(("g", "y", "dz"), case.lds)) if case.entry == "dense_act_bwd" else {}
    ins = {k: Matrix(case.dtype, case.m, case.n, lds.get(k, case.lds[0]), case.off, v) for k, v in t.items() if k != "init"}
    outs = launch(case, t, ins)
    route = last_route()
    assert route == T.claim(case), dict(zip(FIELDS, route))
    got = {}
    for name, buf in outs.items():
        values, kept = buf.read()
        assert kept, f"{name}: an element outside the [m, n] output changed"
        got[name] = values[0] if name in ("dbias", "colsum") else values
    assert set(got) == set(ref)
    for name in ref:
        ratio, where = T.worst_ratio({name: got[name]}, {name: ref[name]}, bound)
        print(f"ratio {case.name} {name} {ratio:.4f}")
        record(case, name, ratio)
        assert ratio <= 1.0, f"{name} leaves its bound at {where}: {ratio:.3f} of it"
    for k, buf in ins.items():
        assert buf.read()[1] and np.array_equal(buf.dev.cpu().numpy().view(BITS[case.dtype]), buf.before), f"input {k} was written"
    if case.ws == "two_stage":
        name = "colsum" if case.entry == "colsum" else "dbias"
        again = launch(case, t, ins)[name]
        assert torch.equal(again.dev, outs[name].dev), "the two-stage column sums differ between two calls"
        assert last_route() == route


@pytest.mark.parametrize("index", [i for i, c in enumerate(T.CASES) if c.entry == "bce"], ids=[n for n in IDS if n.startswith("bce")])
def test_bce_with_partials_and_as_one_workgroup(index):
    case = T.CASES[index]
    t, ref, mag, _ = T.reference_of(index)
    n = case.n
    pred = Matrix(case.dtype, 1, n, n, 0, t["pred"])
    labels = Matrix("fp32", 1, n, n, 0, t["labels"])
    scratch = torch.full((T.BCE_MAX_BLOCKS,), float("nan"), device="cuda")
    for partials in (True, False):
        loss, dpred = vector_out(1), Matrix(case.dtype, 1, n, n, 0, fill=SENTINEL[case.dtype])
        rc = L.lib().krs_bce_fwd_bwd(pred.ptr, L.BF16 if case.dtype == "bf16" else L.F32, labels.ptr, n, T.BCE_EPS, T.BCE_SCALE,
                                     loss.ptr, dpred.ptr, scratch.data_ptr() if partials else None, L.stream_ptr())
        L.check(rc, "krs_bce_fwd_bwd")
        torch.cuda.synchronize()
        bound = T.bounds(case, ref, mag, partials=partials)
        got = {}
        for name, buf in (("loss", loss), ("dpred", dpred)):
            values, kept = buf.read()
            assert kept, name
            got[name] = values[0, 0] if name == "loss" else values[0]
        for name in ("loss", "dpred"):
            ratio, where = T.worst_ratio({name: got[name]}, {name: ref[name]}, bound)
            print(f"ratio {case.name} {'partials' if partials else 'one_workgroup'} {name} {ratio:.4f}")
            record(case, name, ratio)
            assert ratio <= 1.0, f"{name} leaves its bound at {where}: {ratio:.3f} of it (partials: {partials})"
        assert pred.read()[1] and labels.read()[1]


def test_the_wrapper_hands_back_the_buffers_it_was_given():
    """dxd == dx0: the returned dxd IS dx0, and with dx0_into that is the tensor passed (form "b": tanh, accumulate, fold)."""
    index = next(i for i, c in enumerate(T.CASES) if c.form == "b" and c.dtype == "fp32" and T.claim(c)[0] == T.VEC)
    case = T.CASES[index]
    t, ref, mag, bound = T.reference_of(index)
    dev = {k: torch.from_numpy(v.astype(np.float32)).cuda() for k, v in t.items()}
    into = dev["init"].clone()
    du, dx0, dxd, dbias = dense_ops.cross_epilogue_bwd(dev["g"], dev["u"], dev["x0"], dev["x"], case.diag, act=case.act, dx0_into=into,
                                                       fold_direct=True)
    two_stage = dataclasses.replace(case, ws="two_stage")             # (the wrapper always brings the workspace)
    assert dx0 is into and dxd is dx0 and last_route() == T.claim(two_stage)
    got = {"dz": du, "dx0": dx0, "dbias": dbias}
    assert T.worst_ratio({k: v.double().cpu().numpy() for k, v in got.items()}, ref, T.bounds(two_stage, ref, mag))[0] <= 1.0
    du, dx0, dxd, dbias = dense_ops.cross_epilogue_bwd(dev["g"], dev["u"], dev["x0"], dev["x"], case.diag, act=case.act, fold_direct=True)
    assert dxd is dx0 and dx0 is not into and last_route()[2] == 0
    plain = (dx0.double() + dev["init"].double()).cpu().numpy()       # (the initial value added here, in float64)
    assert T.worst_ratio({"dx0": plain}, {"dx0": ref["dx0"]}, bound)[0] <= 1.0


def test_zz_the_largest_error_of_every_entry_as_a_fraction_of_its_bound():
    """(reads what the cases above recorded; prints nothing when run alone)"""
    for (entry, dtype, name), ratio in sorted(WORST.items()):
        print(f"worst {entry} {dtype} {name} {ratio:.4f}")
    assert all(r <= 1.0 for r in WORST.values())
