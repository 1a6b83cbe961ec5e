"""The case table of tests/test_retrieval_xent_matrix_gpu.py (K13, csrc/retrieval_xent.hip, on every instantiation of
xent_kernel<DPAD, MODE, VEC>) and of its check without a GPU, tests/test_retrieval_xent_cases_host.py.  Data and CPU
helpers only: nothing here touches a device.

A matrix case fixes a shape (b, n, d) of contiguous bf16 inputs and states what launch_sweep is meant to run for it:
DPAD (the first of 32, 64, 128, 256 that holds d), VEC (whole 16-byte chunks: d % 8 == 0), and for each of the two
sweeps -- forward / dq (owner = queries) and dc (owner = candidates) -- the number of owner workgroups and of slices.
The slice plans were worked out by hand from plan_sweep (csrc/retrieval_xent_plan.h); the host test asserts them
against the planner itself, so a change of the slice rule shows up as a failing case, not as lost coverage:

    (40, 161)   fwd/dq: 1 owner block, S = 3 slices of 64 (the last slice: one full tile and a tile of one row)
                dc:     2 owner blocks (the second: 33 rows -- a full wave and a wave with one row), S = 1,
                        tiles of 32 + 8
    (161, 40)   fwd/dq: 2 owner blocks, S = 1         dc: 1 owner block, S = 3

The builders give every test of a case the same inputs (the host test checks the float64 reference of exactly what the
GPU test runs)."""

from collections import namedtuple

import torch

Case = namedtuple("Case", "name b n d dpad vec fwd dc")      # fwd, dc: (owner blocks, slices)
Order = namedtuple("Order", "name b n d order extreme_bias")

WIDTHS = (5, 31, 32, 33, 40, 64, 65, 72, 129, 136, 255)
PLANS = {(40, 161): ((1, 3), (2, 1)), (161, 40): ((2, 1), (1, 3))}      # (b, n) -> (fwd/dq, dc)
SLICE_ROWS = 64                                                          # of every sliced sweep of the table
LS = 0.1
SCALE = 0.5


def dpad_of(d):
    return next(p for p in (32, 64, 128, 256) if d <= p)


def _case(b, n, d):
    fwd, dc = PLANS[(b, n)]
    return Case(f"{b}x{n}x{d}", b, n, d, dpad_of(d), d % 8 == 0, fwd, dc)


CASES = [_case(b, n, d) for d in WIDTHS for (b, n) in PLANS]

# what tests/test_retrieval_xent_gpu.py compares with float64 already (contiguous bf16, so VEC is d % 8 == 0 again)
TESTED_BEFORE = [(1, 1, 8), (3, 5, 8), (33, 65, 16), (129, 300, 100), (300, 1000, 128), (257, 513, 256), (512, 512, 128)]

ORDER_SHAPES = ((33, 300, 16), (40, 161, 48))
ORDERS = [Order(f"{o}-{b}x{n}x{d}", b, n, d, o, False) for (b, n, d) in ORDER_SHAPES
          for o in ("ascending", "descending", "last-outlier")]
ORDERS += [Order(f"ascending-extreme-bias-{b}x{n}x{d}", b, n, d, "ascending", True) for (b, n, d) in ORDER_SHAPES]


def bias_of(prob, eps=1e-6):
    """the sampling correction of SamplingProbabilityCorrection: -log(clip(p, eps, 1))"""
    return -torch.log(torch.clamp(prob.to(torch.float32), eps, 1.0))


def inputs(b, n, d, scale=SCALE, seed=0, dtype=torch.bfloat16):
    """q, c, pos (a permutation prefix when b <= n, else drawn with repeats, so queries share positives), sampling
    probabilities and row weights in [-0.5, 1.5): CPU tensors."""
    gen = torch.Generator().manual_seed(seed)
    q = (torch.randn(b, d, generator=gen) * scale).to(dtype)
    c = (torch.randn(n, d, generator=gen) * scale).to(dtype)
    pos = torch.randperm(n, generator=gen)[:b] if b <= n else torch.randint(0, n, (b,), generator=gen)
    prob = torch.rand(n, generator=gen) * 0.2 + 1e-4
    w = torch.rand(b, generator=gen) * 2.0 - 0.5
    return q, c, pos, prob, w


def matrix_inputs(case):
    """(q, c, pos, bias, w) of a matrix case"""
    q, c, pos, prob, w = inputs(case.b, case.n, case.d, seed=1000 + 7 * case.d + case.b)
    return q, c, pos, bias_of(prob), w


def order_inputs(case):
    """(q, c, pos, bias, w) of a structured-order case: q_i = a_i u + 0.05 eps, c_j = t_j u + 0.05 eps with u a random
    unit vector and a_i in [1, 2), so query i's scores follow a_i t_j along the candidates.  t ascends from -30 to 30
    (every tile lifts the running maximum), descends (the first tile holds it), or is -30 with one +30 in the last
    row: the dominant score arrives in the last, partial tile of the last slice.  extreme_bias alternates the sampling
    probability between 1e-9 and 1, so the bias alternates 13.8 and 0."""
    b, n, d = case.b, case.n, case.d
    gen = torch.Generator().manual_seed(2000 + n + d + len(case.order))
    u = torch.randn(d, generator=gen)
    u = u / u.norm()
    a = torch.rand(b, generator=gen) + 1.0
    t = torch.linspace(-30.0, 30.0, n)
    if case.order == "descending":
        t = t.flip(0)
    elif case.order == "last-outlier":
        t = torch.full((n,), -30.0)
        t[n - 1] = 30.0
    else:
        assert case.order == "ascending"
    q = (a[:, None] * u[None, :] + 0.05 * torch.randn(b, d, generator=gen)).to(torch.bfloat16)
    c = (t[:, None] * u[None, :] + 0.05 * torch.randn(n, d, generator=gen)).to(torch.bfloat16)
    pos = torch.randint(0, n, (b,), generator=gen)
    w = torch.rand(b, generator=gen) * 2.0 - 0.5
    if case.extreme_bias:
        prob = torch.where(torch.arange(n) % 2 == 0, torch.tensor(1e-9), torch.tensor(1.0))
    else:
        prob = torch.rand(n, generator=gen) * 0.2 + 1e-4
    return q, c, pos, bias_of(prob), w
