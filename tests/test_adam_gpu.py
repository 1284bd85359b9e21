"""The HIP kernels of the Adam / AdamW / RMSProp update and of clipping by the
global gradient norm (csrc/kernels/elementwise.hip: solver4_kernel, its
scalar twin solver1_kernel, sqnorm_partial_kernel, sqnorm_finish_kernel)
against the float64 oracle, cases and derived bounds of
tests/test_adam_ref.py, on every path that a size, an alignment or the
variant selector picks.

Gaps, the bf16 weight copy and the cleared gradients are compared exactly,
values against the bounds derived in test_adam_ref.py.  ``pytest -s`` prints
the worst |error| / bound; docs/OPS.md ("Updates") has the figures measured
on an MI355X.
"""
import pytest
import torch

import veles_amd.ops as ops
from test_adam_ref import (ALPHA, BETA1, BETA2, DECAY, EPS, GSCALE, L1, LR, N,
                           TABLES, ZERO_FROM, check_sqnorm,
                           check_zero_gradients, gradients, place, run_adam,
                           run_clip, sqnorm_input, start_state, table)
from test_step_tail_ref import BF, Ratios, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = Ratios()
NEW = ["adam", "adamw", "rmsprop"]


@pytest.fixture(autouse=True, scope="module")
def _report():
    yield
    print("\nworst |error| / bound: " + ", ".join(
        "%s %.3g" % kv for kv in sorted(WORST.items())))


class scalar_twin(object):
    """hvk_set_gemm_variant(67): every hvk_solver4 call runs solver1_kernel."""

    def __enter__(self):
        ops._lib.lib().hvk_set_gemm_variant(67)

    def __exit__(self, *exc):
        ops._lib.lib().hvk_set_gemm_variant(-1)


# ------------------------------------------------- the ref cases, per path
@pytest.mark.parametrize("zero", ZERO_FROM)
@pytest.mark.parametrize("name", TABLES)
def test_vector_kernel(name, zero):
    """n = 1032 from an aligned base: solver4_kernel, whole float4s and the
    element path at every segment end, gap and zero_from."""
    WORST.merge(run_adam(DEV, name, zero, n=N + 1)[0])


@pytest.mark.parametrize("route", ["odd_n", "slice"])
@pytest.mark.parametrize("name", TABLES)
def test_scalar_twin(name, route):
    """n = 1031, and buf[1:] of a longer buffer: solver1_kernel."""
    n, off = (N, 0) if route == "odd_n" else (N + 1, 1)
    for zero in ZERO_FROM:
        WORST.merge(run_adam(DEV, name, zero, n=n, offset=off)[0])


@pytest.mark.parametrize("name", TABLES)
def test_step_1000_and_zero_gradients(name):
    WORST.merge(run_adam(DEV, name, 514, steps=1, first_step=1000,
                         n=N + 1)[0])
    r, (w, s1, s2), _ = run_adam(DEV, name, 0, steps=3, zero_grads=True)
    WORST.merge(r)
    check_zero_gradients(name, start_state(N)[0], w, s1, s2)


def _three_steps(name, forced):
    n = N + 1
    segs = table(name)
    w0, gen = start_state(n)
    w, s1, s2 = (place(t, DEV) for t in (w0, torch.full((n,), 0.25),
                                         torch.full((n,), 0.5)))
    lp = torch.full((n,), 7.0, dtype=BF, device=DEV)
    for t in (1, 2, 3):
        g = gradients(n, gen).to(DEV)
        if forced:
            with scalar_twin():
                ops.solver_update(w, g, s1, s2, segs, w_lp=lp, gscale=GSCALE,
                                  zero_grad=514, step=t)
        else:
            ops.solver_update(w, g, s1, s2, segs, w_lp=lp, gscale=GSCALE,
                              zero_grad=514, step=t)
    return [x.cpu() for x in (w, s1, s2, lp, g)]


@pytest.mark.parametrize("name", TABLES)
def test_twin_bit_identical(name):
    """The scalar twin forced on the aligned case gives the bits of the
    vector kernel: w, s1, s2, w_lp and grad."""
    for a, b in zip(_three_steps(name, False), _three_steps(name, True)):
        assert same_bits(a, b)


# --------------------------------------------------------- grid-stride wrap
SWEEP = 2048 * 256 * 4
BIG = SWEEP + 1036


@pytest.mark.parametrize("name", NEW)
def test_grid_stride_wrap(name):
    """One sweep of the grid is 2048 x 256 float4s; a segment end off the
    4-grid, a gap and zero_from lie in the second sweep."""
    mode = ops.SOLVERS[name]
    rho = ALPHA if mode == 6 else BETA2
    bounds = [(3, 1000001), (1000001, SWEEP + 515), (SWEEP + 519, BIG - 2)]
    segs = [(b, e, LR[k], DECAY[k], L1[k], BETA1, mode, EPS[k], rho)
            for k, (b, e) in enumerate(bounds)]
    WORST.merge(run_adam(DEV, name, SWEEP + 770, steps=1, n=BIG,
                         segs=segs)[0])


# ------------------------------------------------------------------ sqnorm
@pytest.mark.parametrize("n", [1, 3, 4, 255, 1027, BIG])
def test_grad_sqnorm(n):
    x = sqnorm_input(n + 1)
    for off in (0, 1):
        xd = place(x[off:off + n], DEV, off)
        a = ops.grad_sqnorm(xd)
        b = ops.grad_sqnorm(xd, out=torch.full((1,), 7.0, device=DEV),
                            ws=torch.full((2048,), 7.0, device=DEV))
        assert same_bits(a, b), "two calls differ"
        WORST.merge(check_sqnorm(x[off:off + n], a, True))
    z = ops.grad_sqnorm(torch.zeros(n, device=DEV))
    assert float(z.cpu()[0]) == 0.0


def test_grad_sqnorm_small_workspace():
    """A workspace shorter than the grid caps the grid."""
    x = sqnorm_input(70001)
    ws = torch.full((5,), 7.0, device=DEV)
    got = ops.grad_sqnorm(x.to(DEV), ws=ws)
    want = float((x.double() ** 2).sum())
    assert abs(float(got.cpu()[0]) - want) <= 1e-4 * want


# -------------------------------------------------------------------- clip
@pytest.mark.parametrize("name", TABLES + ["momentum"])
def test_clip(name):
    WORST.merge(run_clip(DEV, name, n=N + 1))
    WORST.merge(run_clip(DEV, name, n=N))


# ------------------------------------------------------------------- graph
@pytest.mark.parametrize("name", ["adam", "mixed"])
def test_graph_replay(name):
    """grad_sqnorm and the update captured as one linear chain; the table is
    refreshed with step = t before each replay, outside the capture; five
    replays give the bits of five eager steps."""
    n, clip = N + 1, 8.0            # |g| ~ 0.3 * sqrt(1032) ~ 10: clips
    segs = table(name)
    w0, gen = start_state(n)
    grads = [gradients(n, gen) for _ in range(5)]

    def state():
        return [place(t, DEV) for t in (w0, torch.zeros(n), torch.zeros(n))] \
            + [torch.zeros(n, dtype=BF, device=DEV)]

    def update(w, s1, s2, lp, g, sq, ws, tab, t):
        ops.grad_sqnorm(g, out=sq, ws=ws)
        ops.solver_update(w, g, s1, s2, segs, w_lp=lp, gscale=GSCALE,
                          zero_grad=514, table=tab, step=t, sqnorm=sq,
                          clip_norm=clip)

    def scratch():
        return (torch.zeros(1, device=DEV), torch.zeros(2048, device=DEV),
                ops.SegmentTable(torch.device(DEV, 0)))

    eager = state()
    sq, ws, tab = scratch()
    norms = []
    for t, g in enumerate(grads, 1):
        update(*eager, g.to(DEV), sq, ws, tab, t)
        norms.append(GSCALE * float(sq.cpu()[0]) ** 0.5)
    assert min(norms) > clip, norms

    replay = state()
    sq, ws, tab = scratch()
    gbuf = torch.zeros(n, device=DEV)
    warm = [t.clone() for t in replay]
    update(*warm, gbuf.clone(), sq, ws, tab, 1)     # loads, allocates
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        update(*replay, gbuf, sq, ws, tab, 1)
    torch.cuda.synchronize()
    for t in replay[1:3]:
        assert not t.any(), "the capture itself ran the update"
    for t, g in enumerate(grads, 1):
        tab.update(ops._pack_solver_segs(segs, step=t))
        gbuf.copy_(g.to(DEV))
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, replay):
        assert same_bits(a, b)
    assert not gbuf[514:].any() and gbuf[:514].all()
