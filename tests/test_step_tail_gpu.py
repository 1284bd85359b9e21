"""The HIP kernels that end every training step (csrc/kernels/elementwise.hip:
softmax_ce_kernel<16> / <0>, mse_kernel, sgd4_kernel, sgd_kernel,
solver_kernel, dropout_kernel, dropout_bf16x8_kernel) against the float64
references, cases and derived bounds of tests/test_step_tail_ref.py, on every
path a shape, dtype, alignment or variant selects and at the edges of each.

Indices (argmax, confusion, error counts, masks, cleared gradients, untouched
gaps, the bf16 weight copy) are compared exactly; values against the bounds
derived in test_step_tail_ref.py.  Worst measured |error| / bound on an
MI355X (``pytest -s`` prints them again):

    softmax  p 0.025; err f32 0.82 (the label column: p - 1 and its product
             with scale round at ~1/B, against the 1e-7 / B term); err bf16
             1.00 (the half-ulp of the store itself); loss 0.012; against
             the older 1e-4 of the row maximum: p 0.002, err f32 0.003
    MSE      err f32 0.86, err bf16 1.00, mse_out 0.36, metrics 0.15
    SGD      w 0.29, mom 0.27
    solvers  w 0.58, s1 0.47, s2 0.30; Rprop edges s1 0.72, w 0.36, s2 exact
"""
import numpy as np
import pytest
import torch

import veles_amd.ops as ops
from test_step_tail_ref import (
    BF, DROPOUT_P, F32, M32, MSE_SHAPES, SGD_N, SGD_TABLES, SOFTMAX_SHAPES,
    SOLVER_TABLES, Ratios, check_dropout, dropout_boundary_cases,
    dropout_input, hash32_inv, run_mse, run_rprop_edges, run_sgd, run_softmax,
    run_solver, same_bits, sgd_state, softmax_inputs, softmax_range_rows,
    softmax_tie_rows)

pytestmark = pytest.mark.gpu
DEV = "cuda"
_DT = {"f32": F32, "bf16": BF}
WORST = Ratios()


@pytest.fixture(autouse=True, scope="module")
def _report():
    yield
    print("\nworst |error| / bound: " + ", ".join(
        "%s %.3f" % kv for kv in sorted(WORST.items())))


class variant(object):
    """The library's A/B selector (65: softmax re-reading form, 66: scalar
    dropout), restored on exit."""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        ops._lib.lib().hvk_set_gemm_variant(self.v)

    def __exit__(self, *exc):
        ops._lib.lib().hvk_set_gemm_variant(-1)


# --------------------------------------------------------------- softmax
@pytest.mark.parametrize("B,C", SOFTMAX_SHAPES)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_softmax_shapes(B, C, dt):
    """Register form up to C = 1024, re-reading form beyond, both grid-stride
    loops (4099 x 10, 1029 x 1025); metrics from non-zero values over two
    calls; every output together, singly, and without labels."""
    x, lab = softmax_inputs(B, C, _DT[dt])
    for edt in (F32, BF):
        WORST.merge(run_softmax(DEV, x, lab, err_dtype=edt, calls=2)[1])
    for one in ("probs", "max_idx", "confusion"):
        WORST.merge(run_softmax(DEV, x, lab, want=(one,))[1])
    WORST.merge(run_softmax(DEV, x, None, want=("probs", "max_idx"))[1])


@pytest.mark.parametrize("C", [130, 1030])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_softmax_ties_first_index(C, dt):
    x, lab, first = softmax_tie_rows(C, _DT[dt])
    out, r = run_softmax(DEV, x, lab)
    assert out["max_idx"].tolist() == first
    WORST.merge(r)
    with variant(65):
        out, _ = run_softmax(DEV, x, lab)
    assert out["max_idx"].tolist() == first


@pytest.mark.parametrize("C", [2, 130, 1030])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_softmax_range_finite(C, dt):
    """Spread 160, equal values, +-1e4: finite outputs, the loss on the 1e-30
    clamp (69.08 per row whose label holds no probability)."""
    x, lab = softmax_range_rows(C, _DT[dt])
    for edt in (F32, BF):
        out, _ = run_softmax(DEV, x, lab, err_dtype=edt, exact_only=True)
        assert torch.isfinite(out["err"].float()).all()
        assert torch.isfinite(out["probs"]).all()
        assert torch.isfinite(out["metrics"]).all()


@pytest.mark.parametrize("B,C", [(5, 10), (37, 1000), (9, 1031)])
def test_softmax_all_unlabelled(B, C):
    """Every label -1: err all zero, metrics and confusion bitwise as they
    were (run_softmax holds both to their start values)."""
    x, lab = softmax_inputs(B, C, BF, labels="none")
    out, _ = run_softmax(DEV, x, lab)
    assert not out["err"].any()
    assert same_bits(out["metrics"], torch.tensor([3.0, 1.5, 7.0]))
    assert out["confusion"].eq(1).all()


@pytest.mark.parametrize("C", [1000, 1024])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_softmax_forms_bit_identical(C, dt):
    """B = 4 is one block, so the metrics are bitwise equal as well."""
    x, lab = softmax_inputs(4, C, _DT[dt], labels="all")
    a, _ = run_softmax(DEV, x, lab, err_dtype=_DT[dt])
    with variant(65):
        b, _ = run_softmax(DEV, x, lab, err_dtype=_DT[dt])
    for k in ("err", "probs", "metrics"):
        assert same_bits(a[k], b[k]), k
    assert torch.equal(a["max_idx"], b["max_idx"])
    assert torch.equal(a["confusion"], b["confusion"])


# ------------------------------------------------------------------- MSE
@pytest.mark.parametrize("B,D", MSE_SHAPES)
def test_mse(B, D):
    """f32 / bf16 operands in every mix, err f32 / bf16, with and without
    mse_out, valid_rows 0 / 3 / B, metrics from non-zero values."""
    WORST.merge(run_mse(DEV, B, D))


# ------------------------------------------------------------------- SGD
def test_sgd_route_selection():
    """The buffers of run_sgd's vector routes are what hvk_sgd4 takes, the
    others what it declines."""
    fn = ops._lib.lib().hvk_sgd4
    seg = ops._segs_tensor(ops._pack_sgd_segs([(0, 8, 0.0, 0.0, 0.0, 0.0)]),
                           torch.device(DEV, 0))
    hold = torch.zeros(SGD_N + 1, device=DEV)
    g, m = torch.zeros(SGD_N, device=DEV), torch.zeros(SGD_N, device=DEV)
    s = torch.cuda.current_stream().cuda_stream

    def rc(w, n):
        return fn(w.data_ptr(), g.data_ptr(), m.data_ptr(), None,
                  seg.data_ptr(), 1, n, 1.0, n, s)
    assert SGD_N % 4 == 0 and SGD_N > 4 * 256 * 5
    assert rc(hold[:SGD_N], SGD_N) == 0
    assert rc(hold[1:], SGD_N) == -1
    assert rc(hold[:SGD_N - 1], SGD_N - 1) == -1


@pytest.mark.parametrize("table", sorted(SGD_TABLES))
@pytest.mark.parametrize("route", ["sgd4", "grid1", "grid3", "odd", "view",
                                   "nomom"])
def test_sgd(table, route):
    """Segment boundaries at every residue mod 4, length-1 segments, gaps,
    1 / 2 / 40 segments, zero_grad True / False / on and off the 4-grid,
    through hvk_sgd4, hvk_sgd4_grid (each thread loops) and the scalar
    kernel by each of its routes."""
    WORST.merge(run_sgd(DEV, SGD_TABLES[table], route))


def test_sgd_routes_agree_off_grid():
    """The vector kernel's element-by-element path and the scalar kernel see
    the same segments: the same elements change."""
    segs = SGD_TABLES["len1_gaps"]
    w0, g0, m0 = sgd_state(SGD_N)
    res = []
    for view in (False, True):
        hold = torch.zeros(SGD_N + 1, device=DEV)
        w = hold[1:] if view else hold[:SGD_N]
        w.copy_(w0)
        ops.sgd_update(w, g0.to(DEV), m0.to(DEV), segs, gscale=0.3)
        res.append(w.cpu() != w0)
    assert torch.equal(res[0], res[1])


# --------------------------------------------------------------- solvers
@pytest.mark.parametrize("table", sorted(SOLVER_TABLES))
def test_solver(table):
    """Four steps, each from the GPU's own previous state; w, s1 and s2 every
    step; zero_grad as an offset and as False; w_lp bitwise, gaps included."""
    WORST.merge(run_solver(DEV, SOLVER_TABLES[table], "solver"))


@pytest.mark.parametrize("mode", [1, 2])
def test_solver_large_state(mode):
    WORST.merge(run_solver(DEV, SOLVER_TABLES["mode%d" % mode], "solver",
                           steps=2, zero=(False,), s1_start=1e6))


def test_rprop_edges():
    """Both clamps, the start from lr (s1 = 0 and s1 < 0), g = 0, pg = 0,
    sign flips, and the +-1e-25 pairs whose product underflows."""
    WORST.merge(run_rprop_edges(DEV))


# ---------------------------------------------------------------- dropout
def _seed_dev(seed):
    s = seed & M32
    return torch.tensor([s - (1 << 32) if s >= (1 << 31) else s],
                        dtype=torch.int32, device=DEV)


def _dropout_x(path):
    """bf16x8: the vector kernel; the other three the scalar kernel."""
    if path == "bf16x8":
        return dropout_input(4096, BF).to(DEV)
    if path == "bf16_odd":
        return dropout_input(4099, BF).to(DEV)
    if path == "bf16_view":
        return dropout_input(4097, BF).to(DEV)[1:]
    return dropout_input(4099, F32).to(DEV)


@pytest.mark.parametrize("p", DROPOUT_P)
@pytest.mark.parametrize("path", ["bf16x8", "bf16_odd", "bf16_view", "f32"])
def test_dropout_exact(p, path):
    """The mask is hash >= dropout_thresh(p) on every element, the values the
    IEEE float32 product rounded once; p = 0 returns x, p = 1 zeros; the host
    seed and the device seed draw the same mask."""
    seed = 0x9ABCDEF1
    x = _dropout_x(path)
    y = ops.dropout(x, p, seed)
    check_dropout(x, y, p, seed)
    yd = ops.dropout(x, p, 0, seed_dev=_seed_dev(seed))
    assert same_bits(y, yd)


@pytest.mark.parametrize("p", DROPOUT_P)
def test_dropout_scalar_variant_bit_identical(p):
    x = _dropout_x("bf16x8")
    y = ops.dropout(x, p, 4321)
    with variant(66):
        ys = ops.dropout(x, p, 4321)
    assert same_bits(y, ys)
    check_dropout(x, ys, p, 4321)


@pytest.mark.parametrize("p", DROPOUT_P)
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_dropout_threshold_placement(p, dt):
    """The indices whose hashes are T - 1 and T (and, for p = 0.4, the ends
    of the window between the double and the float32 threshold), placed at
    elements 0 and 11 of a 16-element buffer through ``base``."""
    seed = 77
    x = dropout_input(16, _DT[dt]).to(DEV)
    sd = _seed_dev(seed)
    for h, kept in dropout_boundary_cases(p, seed):
        j = int(hash32_inv(np.array([h]), seed)[0])
        for k in (0, 11):
            base = (j - k) & M32
            y = ops.dropout(x, p, 0, seed_dev=sd, base=base)
            keep = check_dropout(x, y, p, seed, base)
            assert bool(keep[k]) == kept


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_dropout_base_wraps(dt):
    x = dropout_input(16, _DT[dt]).to(DEV)
    base = (1 << 32) - 5
    for p in (0.3, 0.5):
        y = ops.dropout(x, p, 0, seed_dev=_seed_dev(1234), base=base)
        check_dropout(x, y, p, 1234, base)
        y0 = ops.dropout(x[5:13], p, 0, seed_dev=_seed_dev(1234))
        assert same_bits(y[5:13], y0)
