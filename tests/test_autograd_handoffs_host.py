"""The backward hand-offs of keras_rs_amd.autograd (Dx0Relay, DenseActRelay: when the data-gradient product of one layer
may run the elementwise backward of the layer below it) without a GPU.  The decisions are host logic -- graph task ids,
tensor identity, dtypes -- so the six dense_ops entry points the Functions call are replaced by plain-torch stand-ins that
compute in float64, round where the kernels store a matrix, and log every call.  Checked per case, in bf16 (the fusions
engage) and fp32 (only the dL/dx0 relay does), with every FUSE_* switch on and off:
  (a) the call log, entry for entry, against the literal recorded below;
  (b) every gradient and captured value against a float64 torch composition of the same model;
  (c) switches on against switches off on the same stand-ins;
  (d) nothing is left on a relay or counted on a weight after the pass, nor after the graph is dropped without one."""

import contextlib
import gc
from typing import NamedTuple

import pytest
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import autograd as A
from keras_rs_amd import dense_ops as D

B, WIDTH, RANK = 64, 32, 16
DENSE = ((8, L.ACT_TANH), (4, L.ACT_SIGMOID))       # (units, activation) of the Dense layers, bottom first
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}


# ---- the stand-ins ------------------------------------------------------------------------------------------------------

def _act64(z, act):
    return {L.ACT_NONE: lambda t: t, L.ACT_RELU: torch.relu, L.ACT_SIGMOID: torch.sigmoid, L.ACT_TANH: torch.tanh}[act](z)


def _dact64(y, act):
    """act' written through the saved output (include/krs.h: relu y > 0, sigmoid y(1-y), tanh 1-y^2)."""
    if act == L.ACT_RELU:
        return (y > 0).double()
    if act == L.ACT_SIGMOID:
        return y * (1.0 - y)
    if act == L.ACT_TANH:
        return 1.0 - y * y
    return torch.ones_like(y)


def _entry(name, **flags):
    return name + "[" + ",".join(k if v is True else f"{k}={v}" for k, v in flags.items() if v) + "]"


class StandIns:
    """dense_ops.gemm, cross_epilogue_bwd, gemm_cross_bwd, gemm_dense_bwd, dense_act_bwd and cast_transpose with the real
    signatures: float64 arithmetic, ONE rounding to the output dtype per stored matrix (G of the two fused products first;
    dz and dx0 then from G as stored), fp32 bias gradients.  `log` gets one entry per call: the name and what selects
    its form."""

    def __init__(self):
        self.log = []

    def gemm(self, a, b, *, a_is_km=False, b_is_nk=False, out_dtype=None, bias=None, act=L.ACT_NONE, diag_scale=0.0,
             x0=None, x=None, want_u=False, r=None, beta=1.0, out=None):
        self.log.append(_entry("gemm", a_is_km=a_is_km, b_is_nk=b_is_nk, f32=out_dtype == torch.float32, bias=bias is not None,
                               act=act, cross=x0 is not None, want_u=want_u, r=r is not None, out=out is not None))
        assert a.dtype == b.dtype and a.dim() == b.dim() == 2
        z = (a.double().t() if a_is_km else a.double()) @ (b.double().t() if b_is_nk else b.double())
        if bias is not None:
            z = z + bias.double()
        z = _act64(z, act)
        odt = out_dtype or a.dtype
        u = z.to(odt) if want_u else None
        if x0 is not None:
            assert x0.dtype == odt and x.dtype == odt
            z = x0.double() * (z + float(diag_scale or 0.0) * x.double()) + x.double()
        if r is not None:
            assert r.dtype == odt
            z = z + float(beta) * r.double()
        if out is None:
            return z.to(odt), u
        out.copy_(z)
        return out, u

    def cross_epilogue_bwd(self, g, u, x0, x, diag_scale=0.0, *, act=L.ACT_NONE, dx0_into=None, want_du=True, want_dxd=True,
                           want_dbias=True, fold_direct=False, want_dx0=True):
        self.log.append(_entry("cross_epilogue_bwd", act=act, u=u is not None, dx0_into=dx0_into is not None, want_du=want_du,
                               want_dxd=want_dxd, want_dbias=want_dbias, fold_direct=fold_direct, want_dx0=want_dx0))
        assert u is not None or not (want_dx0 or act != L.ACT_NONE)
        diag = float(diag_scale or 0.0)
        g64, x064, x64 = g.double(), x0.double(), x.double()
        dz = g64 * x064 * (_dact64(u.double(), act) if act != L.ACT_NONE else 1.0)
        direct = g64 + diag * g64 * x064
        dx0 = None
        if want_dx0:
            t = g64 * (u.double() + diag * x64)
            if dx0_into is not None:
                assert dx0_into.is_contiguous()
                t = t + dx0_into.double()
            if fold_direct:
                t = t + direct
            dx0 = dx0_into.copy_(t) if dx0_into is not None else t.to(x.dtype)
        dxd = dx0 if fold_direct else (direct.to(x.dtype) if want_dxd else None)
        return (dz.to(x.dtype) if want_du else None), dx0, dxd, (dz.sum(0).float() if want_dbias else None)

    def gemm_cross_bwd(self, a, bt, r, x0, u, *, act=L.ACT_NONE, dx0_into=None, want_dbias=True, fold_direct=False,
                       beta=1.0, u_upper=None, want_dx0=True):
        self.log.append(_entry("gemm_cross_bwd", r=r is not None, act=act, dx0_into=dx0_into is not None, want_dbias=want_dbias,
                               fold_direct=fold_direct, u_upper=u_upper is not None, want_dx0=want_dx0))
        assert a.dtype == bt.dtype == x0.dtype == u.dtype and (r is None or r.dtype == a.dtype)
        assert want_dx0 or (r is None and dx0_into is None and u_upper is None and not fold_direct)
        assert u_upper is None or (dx0_into is None and r is not None and beta == 1.0 and u_upper.dtype == a.dtype)
        z = a.double() @ bt.double().t()
        if r is not None:
            z = z + float(beta) * r.double()
        G = z.to(a.dtype)
        G64, u64 = G.double(), u.double()
        dz = G64 * x0.double() * _dact64(u64, act)
        dx0 = None
        if want_dx0:
            t = G64 * u64
            if u_upper is not None:
                t = t + r.double() * u_upper.double()
            if dx0_into is not None:
                assert dx0_into.is_contiguous() and dx0_into.dtype == a.dtype and dx0_into.shape == G.shape
                t = t + dx0_into.double()
            if fold_direct:
                t = t + G64
            dx0 = dx0_into.copy_(t) if dx0_into is not None else t.to(a.dtype)
        return G, dz.to(a.dtype), dx0, (dz.sum(0).float() if want_dbias else None)

    def gemm_dense_bwd(self, a, bt, y, act, want_dbias=True, want_g=False):
        self.log.append(_entry("gemm_dense_bwd", act=act, want_dbias=want_dbias, want_g=want_g))
        assert a.dtype == bt.dtype == y.dtype
        G = (a.double() @ bt.double().t()).to(a.dtype)
        dz = G.double() * _dact64(y.double(), act)
        return dz.to(a.dtype), (dz.sum(0).float() if want_dbias else None), (G if want_g else None)

    def dense_act_bwd(self, g, y, act, want_dbias=True):
        self.log.append(_entry("dense_act_bwd", act=act, y=y is not None, want_dbias=want_dbias))
        dz = g.double() * (_dact64(y.double(), act) if act != L.ACT_NONE else 1.0)
        return (dz.to(g.dtype) if act != L.ACT_NONE else g), (dz.sum(0).float() if want_dbias else None)

    def cast_transpose(self, w, dtype, want_plain=True, want_t=True):
        self.log.append(_entry("cast_transpose", no_plain=not want_plain, no_t=not want_t))
        w = w.detach()
        plain = (w if w.dtype == dtype else w.to(dtype)) if want_plain else None
        return plain, (w.to(dtype).t().contiguous() if want_t else None)

    NAMES = ("gemm", "cross_epilogue_bwd", "gemm_cross_bwd", "gemm_dense_bwd", "dense_act_bwd", "cast_transpose")


@contextlib.contextmanager
def _patched(fuse):
    """The stand-ins on dense_ops and every FUSE_* switch of keras_rs_amd.autograd set to `fuse`; both restored afterwards."""
    s = StandIns()
    switches = [n for n in dir(A) if n.startswith("FUSE_")]
    old = {n: getattr(A, n) for n in switches}
    real = {n: getattr(D, n) for n in StandIns.NAMES}
    try:
        for n in switches:
            setattr(A, n, fuse)
        for n in StandIns.NAMES:
            setattr(D, n, getattr(s, n))
        yield s
    finally:
        for n, v in real.items():
            setattr(D, n, v)
        for n, v in old.items():
            setattr(A, n, v)


# ---- the layers as the package wires them -----------------------------------------------------------------------------------

def _wire_cross(x0, x, down, kernel, bias, diag, act, cd):
    """What layers.FeatureCross.call and the Keras adapter do past their device check."""
    return A.cross_layer(x0, x, down, kernel, bias, diag, act, cd)


def _wire_dense(x, kernel, bias, act, cd):
    """What layers.Dense.call does past its device check."""
    return A.dense_layer(x, kernel, bias, act, cd)


# ---- models: a stack of cross layers on one x0, Dense layers over it ------------------------------------------------------

class Spec(NamedTuple):
    cross: int = 0
    dense: int = 0
    full_rank: bool = False
    diag: float = 0.0
    act: int = L.ACT_NONE          # pre-activation of the cross layers
    foreign: bool = False          # the bottom layer runs on a copy of x0: the next layer's relay_up does not match


class Net:
    """ref: the float64 torch composition (weights = the fp32 master weights in float64); otherwise the Functions of
    keras_rs_amd.autograd in compute dtype `dtype` over fp32 variables."""

    def __init__(self, spec, dtype, ref, seed=7):
        gen = torch.Generator().manual_seed(seed)
        leaf = (lambda t: t.double().requires_grad_()) if ref else (lambda t: torch.nn.Parameter(t))
        rnd = lambda *s: torch.randn(*s, generator=gen)                                              # noqa: E731
        self.spec, self.dtype, self.ref = spec, dtype, ref
        self.named, self.cross_w, self.dense_w, self.relays = [], [], [], []
        for i in range(spec.cross):
            k_in = WIDTH if spec.full_rank else RANK
            w = (None if spec.full_rank else leaf(rnd(WIDTH, RANK) / WIDTH ** 0.5), leaf(rnd(k_in, WIDTH) / k_in ** 0.5),
                 leaf(rnd(WIDTH) * 0.1))
            self.cross_w.append(w)
            self.named += [(f"c{i}.{n}", t) for n, t in zip(("down", "kernel", "bias"), w) if t is not None]
        d_in = WIDTH
        for j in range(spec.dense):
            w = (leaf(rnd(d_in, DENSE[j][0]) / d_in ** 0.5), leaf(rnd(DENSE[j][0]) * 0.1))
            self.dense_w.append(w)
            self.named += [(f"d{j}.{n}", t) for n, t in zip(("kernel", "bias"), w)]
            d_in = DENSE[j][0]

    def cross(self, i, x0, x):
        down, kernel, bias = self.cross_w[i]
        if self.ref:
            u = _act64((x if down is None else x @ down) @ kernel + bias, self.spec.act)
            return x0 * (u + self.spec.diag * x) + x
        y = _wire_cross(x0, x, down, kernel, bias, self.spec.diag, self.spec.act, self.dtype)
        self.relays.append(y._krs_dx0_relay)
        return y

    def dense(self, j, x):
        kernel, bias = self.dense_w[j]
        if self.ref:
            return _act64(x @ kernel + bias, DENSE[j][1])
        y = _wire_dense(x, kernel, bias, DENSE[j][1], self.dtype)
        self.relays.append(y._krs_dense_relay)
        return y

    def forward(self, x):
        """The output of every layer, bottom first."""
        outs, xl = [], x
        for i in range(self.spec.cross):
            if i == 0 and self.spec.foreign:
                other = x * 1.0
                xl = self.cross(i, other, other)
            else:
                xl = self.cross(i, x, xl)
            outs.append(xl)
        for j in range(self.spec.dense):
            xl = self.dense(j, xl)
            outs.append(xl)
        return outs

    def grads(self):
        return {n: t.grad.clone() for n, t in self.named if t.grad is not None}

    def zero_grads(self):
        for _, t in self.named:
            t.grad = None

    def settled(self, relays=True):
        """(d): nothing waits on a relay, no use of a weight is still counted."""
        return (all(r.fused is None and getattr(r, "buf", None) is None for r in self.relays if relays)
                and all(getattr(t, "_krs_pending_cross", 0) == 0 for _, t in self.named))


def _wide(t):
    return t if t.dtype == torch.float64 else t.float()


def _loss(out, w):
    return (_wide(out) * w[:, :out.shape[1]].to(_wide(out).dtype)).sum() / out.shape[0]


def _inputs(dtype, ref):
    gen = torch.Generator().manual_seed(101)
    x0 = (torch.randn(B, WIDTH, generator=gen) * 0.5).to(dtype)
    w = torch.randn(B, WIDTH, generator=gen)
    return (x0.double() if ref else x0), w


# ---- what a caller can observe (tests/test_dense_bwd_fusion_gpu.py::_observe, the observers that need no device) ------------

OBSERVERS = ["backward", "grad_y", "grad_y_x", "grad_y_kernel", "backward_inputs_y", "hook_read", "hook_scale", "node_prehook",
             "node_hook", "second_consumer", "layer_twice", "retain_graph_twice"]
# some layer's backward does not run under these: what the layer above left for it stays until the graph goes
CAPTURE_ONLY = ("grad_y", "grad_y_kernel", "backward_inputs_y")


def _observe(net, how, yi):
    """One step of `net`; `y` is the output of layer `yi`.  Returns every gradient the observer `how` can see, by name."""
    x0, w = _inputs(net.dtype, net.ref)
    x = x0.clone().requires_grad_()
    got = {}
    outs = net.forward(x)
    y, out = outs[yi], outs[-1]
    if how == "layer_twice":
        out = out + net.forward(x * 0.5)[-1]
    loss = _loss(out, w)
    if how == "second_consumer":
        loss = loss + 0.5 * (_wide(y) ** 2).mean()
    if how in ("backward", "second_consumer", "layer_twice"):
        loss.backward()
    elif how == "grad_y":
        (got["y"],) = torch.autograd.grad(loss, [y])
    elif how == "grad_y_x":
        got["y"], got["x"] = torch.autograd.grad(loss, [y, x])
    elif how == "grad_y_kernel":
        got["y"], got["lower.kernel"] = torch.autograd.grad(loss, [y, dict(net.named)[_layer_name(net.spec, yi) + ".kernel"]])
    elif how == "backward_inputs_y":
        loss.backward(inputs=[y])
        got["y"] = y.grad.clone()
    elif how in ("hook_read", "hook_scale", "node_prehook", "node_hook"):
        seen = []
        if how == "node_prehook":
            y.grad_fn.register_prehook(lambda gout: seen.append(gout[0].clone()))
        elif how == "node_hook":
            y.grad_fn.register_hook(lambda gin, gout: seen.append(gout[0].clone()))
        else:
            def hook(g):
                seen.append(g.clone())
                return g * 2.0 if how == "hook_scale" else None

            y.register_hook(hook)
        loss.backward()
        got["y"] = seen[0]
    elif how == "retain_graph_twice":
        loss.backward(retain_graph=True)
        loss.backward()
    else:
        raise AssertionError(how)
    if how not in ("grad_y", "grad_y_x", "grad_y_kernel", "backward_inputs_y"):
        got.update(net.grads())
        got["x"] = x.grad.clone()
    settled = net.ref or how in CAPTURE_ONLY or net.settled()
    del outs, y, out, loss
    gc.collect()
    # (this list keeps the relays of a dropped graph: only a pass that ran every backward has emptied them)
    return got, settled and (net.ref or net.settled(relays=how not in CAPTURE_ONLY))


def _layer_name(spec, i):
    return f"c{i}" if i < spec.cross else f"d{i - spec.cross}"


def _partial_passes(net, how, yi):
    """tests/test_layers_gpu.py::test_cross_stack_hands_dx0_down_the_layers: a partial pass (the gradient of the middle
    output only: the top layer leaves its term of dL/dx0 behind) and then the full pass on the same graph; a partial
    pass and then a pass that stops below the top layer, which must not pick that buffer up."""
    x0, w = _inputs(net.dtype, net.ref)
    x = x0.clone().requires_grad_()
    got = {}
    for tag, top in (("full", -1), ("lower", 1)):
        net.zero_grads()
        x.grad = None
        outs = net.forward(x)
        loss = _loss(outs[-1], w)
        torch.autograd.grad(loss, [outs[1]], retain_graph=True)
        net.zero_grads()
        x.grad = None
        if top == -1:
            loss.backward(retain_graph=True)
        else:
            _loss(outs[1], w).backward()
        got.update({f"{tag}.{n}": g for n, g in net.grads().items()})
        got[f"{tag}.x"] = x.grad.clone()
    settled = net.ref or net.settled()
    del outs, loss
    gc.collect()
    return got, settled and (net.ref or net.settled())


def _function_node(t):
    node = t.grad_fn
    while not isinstance(node, torch.autograd.function.BackwardCFunction):
        node = node.next_functions[0][0]
    return node


def _direct_calls(net, how, yi):
    """Every backward called by hand, top first, outside any backward pass (graph task -1): no hand-off of any kind."""
    x0, w = _inputs(net.dtype, net.ref)
    x = x0.clone().requires_grad_()
    outs = net.forward(x)
    if net.ref:
        _loss(outs[-1], w).backward()
        return dict(net.grads(), x=x.grad.clone()), True
    got = {}
    g = (w[:, :outs[-1].shape[1]] / B).to(net.dtype)
    gx0 = 0.0
    for i in reversed(range(len(outs))):
        node, name = _function_node(outs[i]), _layer_name(net.spec, i)
        with torch.no_grad():       # (as the engine runs a backward)
            if i >= net.spec.cross:
                g, got[name + ".kernel"], got[name + ".bias"] = A.DenseFn.backward(node, g)[:3]
            else:
                t0, tx, got[name + ".down"], got[name + ".kernel"], got[name + ".bias"] = A.CrossLayerFn.backward(node, g)[:5]
                gx0, g = gx0 + t0.double(), tx
    got["x"] = gx0.to(net.dtype)
    settled = net.settled()
    del outs, node
    gc.collect()
    return got, settled and net.settled()


# ---- the cases --------------------------------------------------------------------------------------------------------------

CASES = {}
for _n in (1, 2, 3):
    CASES[f"cross{_n}"] = (_observe, Spec(cross=_n), "backward", 0)
    CASES[f"cross{_n}_dense1"] = (_observe, Spec(cross=_n, dense=1), "backward", 0)
    CASES[f"cross{_n}_dense2"] = (_observe, Spec(cross=_n, dense=2), "backward", 0)
CASES["full_rank"] = (_observe, Spec(cross=2, dense=1, full_rank=True), "backward", 0)
CASES["diag_scale"] = (_observe, Spec(cross=3, dense=1, diag=0.2, act=L.ACT_TANH), "backward", 0)
CASES["foreign_x"] = (_observe, Spec(cross=3, dense=1, foreign=True), "backward", 0)
# one hand-off each, y = the lower layer's output: Dense -> Dense, cross -> cross, Dense over the top of a two-layer stack
# (whose own term of dL/dx0 is deferred to its data-gradient product: u_upper)
KINDS = {"dense_dense": (Spec(dense=2), 0), "cross_cross": (Spec(cross=2), 0), "dense_over_cross": (Spec(cross=2, dense=1), 1)}
for _kind, (_spec, _yi) in KINDS.items():
    for _how in OBSERVERS:
        CASES[f"{_kind}-{_how}"] = (_observe, _spec, _how, _yi)
CASES["middle_of_three-second_consumer"] = (_observe, Spec(cross=3, dense=2), "second_consumer", 1)
CASES["partial_passes"] = (_partial_passes, Spec(cross=3, diag=0.2, act=L.ACT_TANH), None, None)
CASES["partial_passes_fusable"] = (_partial_passes, Spec(cross=3), None, None)
CASES["direct_calls"] = (_direct_calls, Spec(cross=2, dense=2), None, None)


def run_case(name, dtype, fuse):
    """(gradients by name, call log, settled) of one case on the stand-ins."""
    fn, spec, how, yi = CASES[name]
    with _patched(fuse) as s:
        got, settled = fn(Net(spec, DTYPES[dtype], ref=False), how, yi)
    return got, s.log, settled


def run_reference(name, dtype):
    fn, spec, how, yi = CASES[name]
    return fn(Net(spec, DTYPES[dtype], ref=True), how, yi)[0]


def error_against(got, ref):
    """The largest error of any gradient, as a fraction of that gradient's largest magnitude."""
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    return max(float((got[n].detach().double() - ref[n].detach()).abs().max()) / float(ref[n].detach().abs().max())
               for n in ref)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", list(CASES))
def test_hand_offs_on_stand_ins(name, dtype):
    ref = run_reference(name, dtype)
    on, log_on, settled_on = run_case(name, dtype, True)
    off, log_off, settled_off = run_case(name, dtype, False)
    # (a) the calls, entry for entry
    assert not any(e.startswith(("gemm_cross_bwd", "gemm_dense_bwd")) for e in log_off)
    at = 1 + 2 * list(DTYPES).index(dtype)
    assert log_on == [ENTRIES[c] for c in LOGS[RECORDED[name][at]]], log_on
    assert log_off == [ENTRIES[c] for c in LOGS[RECORDED[name][at + 1]]], log_off
    # (b) against float64
    print(f"{name} {dtype}: off {error_against(off, ref):.3e} on {error_against(on, ref):.3e}")
    if dtype == "fp32":
        for n in ref:
            for got in (on, off):
                torch.testing.assert_close(got[n].double(), ref[n], rtol=5e-5, atol=5e-5, msg=lambda m: f"{name} / {n}: {m}")
    else:
        # the switches-off error recorded below + one further bf16 rounding of the largest entry: the two forms round G
        # at the same place and differ in the order of one sum
        bound = RECORDED[name][0] + 2.0 ** -8
        assert error_against(off, ref) <= bound and error_against(on, ref) <= bound
    # (c) on against off: the rule of tests/test_dense_bwd_fusion_gpu.py::_compare
    assert set(on) == set(off)
    for n in off:
        u, v = on[n], off[n]
        if (CASES[name][1].cross == 0 and not n.endswith("bias")) or n == "y":
            assert torch.equal(u, v), (n, float((u.float() - v.float()).abs().max()))
        else:
            torch.testing.assert_close(u.float(), v.float(), rtol=2.0 ** -6, atol=2.0 ** -7 * float(v.float().abs().max()),
                                       msg=lambda m: f"{name} / {n}: {m}")
    # (d)
    assert settled_on and settled_off


def test_a_graph_dropped_without_a_backward_pass_leaves_nothing_counted():
    with _patched(True):
        net = Net(Spec(cross=3, dense=2), torch.bfloat16, ref=False)
        x0, _ = _inputs(torch.bfloat16, False)
        outs = net.forward(x0.clone().requires_grad_())
        assert all(t._krs_pending_cross == 1 for n, t in net.named if n.startswith("c") and not n.endswith("bias"))
        del outs
        gc.collect()
        assert net.settled()


def test_the_fused_calls_of_the_whole_chain():
    """Three low-rank layers, Dense over Dense over them, bf16: what is not a plain product, with the switches on and off."""
    special = lambda log: [e for e in log if not e.startswith(("gemm[", "cast_transpose"))]      # noqa: E731
    _, log_on, _ = run_case("cross3_dense2", "bf16", True)
    _, log_off, _ = run_case("cross3_dense2", "bf16", False)
    assert special(log_on) == [
        "dense_act_bwd[act=2,y,want_dbias]",
        "gemm_dense_bwd[act=3,want_dbias,want_g]",
        "gemm_cross_bwd[want_dbias]",                                        # (no R, want_dx0=False: the term is deferred)
        "gemm_cross_bwd[r,want_dbias,u_upper,want_dx0]",
        "gemm_cross_bwd[r,dx0_into,want_dbias,fold_direct,want_dx0]"]
    assert len(log_on) - len(special(log_on)) - log_on.count("cast_transpose[]") == 20
    assert special(log_off) == [
        "dense_act_bwd[act=2,y,want_dbias]",
        "dense_act_bwd[act=3,y,want_dbias]",
        "cross_epilogue_bwd[u,want_du,want_dbias,want_dx0]",
        "cross_epilogue_bwd[u,dx0_into,want_du,want_dbias,want_dx0]",
        "cross_epilogue_bwd[u,dx0_into,want_du,want_dbias,fold_direct,want_dx0]"]
    assert len(log_off) - len(special(log_off)) - log_off.count("cast_transpose[]") == 24


# ---- recorded on the commit before the relays became records -------------------------------------------------------------

# one letter per distinct call
ENTRIES = {
    "a": "cast_transpose[]",
    "b": "cross_epilogue_bwd[act=3,u,dx0_into,want_du,want_dbias,fold_direct,want_dx0]",
    "c": "cross_epilogue_bwd[act=3,u,dx0_into,want_du,want_dxd,want_dbias,want_dx0]",
    "d": "cross_epilogue_bwd[act=3,u,want_du,want_dxd,want_dbias,want_dx0]",
    "e": "cross_epilogue_bwd[u,dx0_into,fold_direct,want_dx0]",
    "f": "cross_epilogue_bwd[u,dx0_into,want_du,want_dbias,fold_direct,want_dx0]",
    "g": "cross_epilogue_bwd[u,dx0_into,want_du,want_dbias,want_dx0]",
    "h": "cross_epilogue_bwd[u,dx0_into,want_dx0]",
    "i": "cross_epilogue_bwd[u,want_du,want_dbias,fold_direct,want_dx0]",
    "j": "cross_epilogue_bwd[u,want_du,want_dbias,want_dx0]",
    "k": "cross_epilogue_bwd[u,want_du,want_dbias]",
    "l": "cross_epilogue_bwd[want_du,want_dbias]",
    "m": "dense_act_bwd[act=2,y,want_dbias]",
    "n": "dense_act_bwd[act=3,y,want_dbias]",
    "o": "gemm[a_is_km,f32]",
    "p": "gemm[b_is_nk,bias,act=2]",
    "q": "gemm[b_is_nk,bias,act=3,cross,want_u]",
    "r": "gemm[b_is_nk,bias,act=3]",
    "s": "gemm[b_is_nk,bias,cross,want_u]",
    "t": "gemm[b_is_nk,r]",
    "u": "gemm[b_is_nk]",
    "v": "gemm_cross_bwd[r,dx0_into,want_dbias,fold_direct,want_dx0]",
    "w": "gemm_cross_bwd[r,want_dbias,fold_direct,u_upper,want_dx0]",
    "x": "gemm_cross_bwd[r,want_dbias,u_upper,want_dx0]",
    "y": "gemm_cross_bwd[want_dbias,fold_direct,want_dx0]",
    "z": "gemm_cross_bwd[want_dbias]",
    "A": "gemm_dense_bwd[act=3,want_dbias,want_g]",
}

# every distinct log, one letter per call, forward and backward
LOGS = [
    "aausiouot",   # 0
    "aausarnoyouot",   # 1
    "aausarnouiouot",   # 2
    "aausarapmoAoyouot",   # 3
    "aausarapmounouiouot",   # 4
    "aausarapmoAouiouot",   # 5
    "aausaauslouowouot",   # 6
    "aausaausjouotfouot",   # 7
    "aausaausarnozouowouot",   # 8
    "aausaausarnoujouotfouot",   # 9
    "aausaausarapmoAozouowouot",   # 10
    "aausaausarapmounoujouotfouot",   # 11
    "aausaausarapmoAoujouotfouot",   # 12
    "aausaausaauslouoxouovouot",   # 13
    "aausaausaausjouotgouotfouot",   # 14
    "aausaausaausarnozouoxouovouot",   # 15
    "aausaausaausarnoujouotgouotfouot",   # 16
    "aausaausaausarapmoAozouoxouovouot",   # 17
    "aausaausaausarapmounoujouotgouotfouot",   # 18
    "aausaausaausarapmoAoujouotgouotfouot",   # 19
    "asasarnoujotfot",   # 20
    "aauqaauqaauqarnoudouotcouotbouot",   # 21
    "aausaausaausarnozouoxouotiouot",   # 22
    "aausaausaausarnoujouotgouotiouot",   # 23
    "arapmoAou",   # 24
    "arapmounou",   # 25
    "arapmoA",   # 26
    "arapmou",   # 27
    "arapmoAnou",   # 28
    "araparapmoAoumoAou",   # 29
    "araparapmounoumounou",   # 30
    "arapmoAoumoAou",   # 31
    "arapmounoumounou",   # 32
    "aausaauslouow",   # 33
    "aausaausjouot",   # 34
    "aausaauslouowekouot",   # 35
    "aausaausaausaauslouowouotlouowouot",   # 36
    "aausaausaausaausjouotfouotjouotfouot",   # 37
    "aausaauslouowouotlouowouot",   # 38
    "aausaausjouotfouotjouotfouot",   # 39
    "aausaausarnoz",   # 40
    "aausaausarnou",   # 41
    "aausaausarnozouow",   # 42
    "aausaausarnoujouot",   # 43
    "aausaausarnozlouowouot",   # 44
    "aausaausaraausaausarnozouowouotnozouowouot",   # 45
    "aausaausaraausaausarnoujouotfouotnoujouotfouot",   # 46
    "aausaausarnozouowouotnozouowouot",   # 47
    "aausaausarnoujouotfouotnoujouotfouot",   # 48
    "aausaausaausarapmoAozouoxhkouovouot",   # 49
    "aauqaauqaauqdouotdouotcouotbouotaauqaauqaauqdouotdouotbouot",   # 50
    "aausaausaauslouoxlouoxouovouotaausaausaauslouoxlouowouot",   # 51
    "aausaausaausjouotjouotgouotfouotaausaausaausjouotjouotfouot",   # 52
    "aausaausarapmounoujouotiouot",   # 53
]

# case: (largest error of the switches-off bf16 run against float64, as a fraction of each gradient's largest magnitude,
#        rounded up to two digits; the index in LOGS of the bf16 on, bf16 off, fp32 on and fp32 off runs).
#        The switches-on errors were equal to them to four digits in every case but middle_of_three-second_consumer (9.3e-3).
RECORDED = {
    "cross1": (0.004, 0, 0, 0, 0),
    "cross1_dense1": (0.006, 1, 2, 2, 2),
    "cross1_dense2": (0.0059, 3, 4, 5, 4),
    "cross2": (0.0049, 6, 7, 7, 7),
    "cross2_dense1": (0.0082, 8, 9, 9, 9),
    "cross2_dense2": (0.01, 10, 11, 12, 11),
    "cross3": (0.0069, 13, 14, 14, 14),
    "cross3_dense1": (0.009, 15, 16, 16, 16),
    "cross3_dense2": (0.0096, 17, 18, 19, 18),
    "full_rank": (0.0067, 20, 20, 20, 20),
    "diag_scale": (0.011, 21, 21, 21, 21),
    "foreign_x": (0.009, 22, 23, 23, 23),
    "dense_dense-backward": (0.0061, 24, 25, 24, 25),
    "dense_dense-grad_y": (0.005, 26, 27, 26, 27),
    "dense_dense-grad_y_x": (0.0061, 24, 25, 24, 25),
    "dense_dense-grad_y_kernel": (0.005, 24, 25, 24, 25),
    "dense_dense-backward_inputs_y": (0.005, 27, 27, 27, 27),
    "dense_dense-hook_read": (0.0061, 24, 25, 24, 25),
    "dense_dense-hook_scale": (0.0061, 28, 25, 28, 25),
    "dense_dense-node_prehook": (0.0061, 24, 25, 24, 25),
    "dense_dense-node_hook": (0.0061, 24, 25, 24, 25),
    "dense_dense-second_consumer": (0.0053, 28, 25, 28, 25),
    "dense_dense-layer_twice": (0.0056, 29, 30, 29, 30),
    "dense_dense-retain_graph_twice": (0.0061, 31, 32, 31, 32),
    "cross_cross-backward": (0.0049, 6, 7, 7, 7),
    "cross_cross-grad_y": (0.0038, 33, 34, 34, 34),
    "cross_cross-grad_y_x": (0.0044, 6, 7, 7, 7),
    "cross_cross-grad_y_kernel": (0.0038, 6, 7, 7, 7),
    "cross_cross-backward_inputs_y": (0.0038, 33, 34, 34, 34),
    "cross_cross-hook_read": (0.0049, 6, 7, 7, 7),
    "cross_cross-hook_scale": (0.0049, 35, 7, 7, 7),
    "cross_cross-node_prehook": (0.0049, 6, 7, 7, 7),
    "cross_cross-node_hook": (0.0049, 6, 7, 7, 7),
    "cross_cross-second_consumer": (0.0049, 35, 7, 7, 7),
    "cross_cross-layer_twice": (0.0045, 36, 37, 37, 37),
    "cross_cross-retain_graph_twice": (0.0049, 38, 39, 39, 39),
    "dense_over_cross-backward": (0.0082, 8, 9, 9, 9),
    "dense_over_cross-grad_y": (0.0057, 40, 41, 41, 41),
    "dense_over_cross-grad_y_x": (0.0082, 8, 9, 9, 9),
    "dense_over_cross-grad_y_kernel": (0.0057, 42, 43, 43, 43),
    "dense_over_cross-backward_inputs_y": (0.0057, 40, 41, 41, 41),
    "dense_over_cross-hook_read": (0.0082, 8, 9, 9, 9),
    "dense_over_cross-hook_scale": (0.0082, 44, 9, 9, 9),
    "dense_over_cross-node_prehook": (0.0082, 8, 9, 9, 9),
    "dense_over_cross-node_hook": (0.0082, 8, 9, 9, 9),
    "dense_over_cross-second_consumer": (0.008, 44, 9, 9, 9),
    "dense_over_cross-layer_twice": (0.007, 45, 46, 46, 46),
    "dense_over_cross-retain_graph_twice": (0.0082, 47, 48, 48, 48),
    "middle_of_three-second_consumer": (0.0079, 49, 18, 19, 18),
    "partial_passes": (0.0075, 50, 50, 50, 50),
    "partial_passes_fusable": (0.0069, 51, 52, 52, 52),
    "direct_calls": (0.01, 53, 53, 53, 53),
}
