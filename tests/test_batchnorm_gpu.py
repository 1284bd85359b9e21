"""The batch-normalisation kernels (csrc/kernels/batchnorm.hip) against the
float64 oracle of test_batchnorm_ref.py, fed with the GPU's own bf16 tensors.

float32 results (saved mean and invstd, running statistics, dgamma, dbeta)
are held to the bounds derived there for the ``shifted`` rule with the
reduction depth of the kernel's grid (``geom``); bf16 results (y, dx) to half
a bf16 ulp of the exact value plus the propagated float32 term.

Strict ReLU: the backward reads the y the forward wrote, and so does the
oracle (y itself is checked against the oracle on its own), so both take the
same side of the kink: no element is left out of the dx comparison, and
there is no exclusion cap to keep or seeds to choose for it.

P_wrap, the smallest P with more partials per channel than the 64 lanes of
the finishing kernel that share a channel: G = ceil(P / (4 RY)) > 64; for
C = 256 (32 channel groups, RY = 8) that is P = 64 * 32 + 1 = 2049.

The worst |error| / bound per quantity goes to
profiles/batchnorm/gpu_tests_figures.txt."""
import os

import numpy as np
import pytest
import torch

from veles_amd import ops
from veles_amd.ops import _lib
from test_batchnorm_ref import (check_case, geom, large_mean_case, make_case)
from test_step_tail_ref import BF, Ratios, same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIGURES = os.path.join(ROOT, "profiles", "batchnorm", "gpu_tests_figures.txt")
P_WRAP = 2049
ONE_WG = 32        # C = 256: the last P that one workgroup covers (4 RY)
WORST = Ratios()


@pytest.fixture(scope="module", autouse=True)
def figures():
    yield
    if not WORST:
        return
    os.makedirs(os.path.dirname(FIGURES), exist_ok=True)
    with open(FIGURES, "w") as f:
        f.write("# worst |error| / bound per quantity over "
                "tests/test_batchnorm_gpu.py\n")
        for k in sorted(WORST):
            f.write("%-8s %.4f\n" % (k, WORST[k]))


def to_gpu(case, misalign=False):
    x, err, aux, g, b, rm, rv = case
    dev = torch.device("cuda")
    out = [t.to(dev) for t in case]
    if misalign:
        buf = torch.empty(x.numel() + 4, dtype=x.dtype, device=dev)
        out[0] = buf[4:].view(x.shape)
        out[0].copy_(x)
        assert out[0].data_ptr() % 16 == 8
    return out


def run_gpu(dcase, act, aux_act, accumulate="overwrite", grads=None,
            training=True, save=None, ws=None, need_dx=True):
    x, err, aux, g, b, rm, rv = dcase
    rm, rv = rm.clone(), rv.clone()
    save = {} if save is None else save
    ws = {} if ws is None else ws
    y = ops.batchnorm_fwd(x, g, b, rm, rv, training=training, act=act,
                          save=save, ws=ws)
    out = {"y": y, "rm": rm, "rv": rv, "save": save}
    if training:
        C = x.shape[-1]
        dg, db = grads if grads is not None else (
            torch.full((C,), 9.0, device=x.device),
            torch.full((C,), -9.0, device=x.device))
        out["dx"] = ops.batchnorm_bwd(
            err, x, y, g, save, dg, db, act=act, accumulate=accumulate,
            aux=aux if aux_act else None, aux_act=aux_act, ws=ws,
            need_dx=need_dx)
        out["dg"], out["db"] = dg, db
    torch.cuda.synchronize()
    return out


def is_vec(x):
    return bool(_lib.lib().hvk_bn_vec(x.data_ptr(), x.shape[-1], x.shape[-1]))


def check(tag, case, dcase, got, act, aux_act, **kw):
    x = dcase[0]
    C = x.shape[-1]
    P = x.numel() // C
    ge = geom(P, C, is_vec(x))
    assert ops.bn_partials(P, C, is_vec(x)) == ge["G"]
    r = Ratios()
    res = check_case(r, "", got, *case, act, aux_act, "shifted", ge["depth"],
                     True, **kw)
    print(tag, tuple(x.shape), "act", act, "aux", aux_act, "G", ge["G"],
          {k: round(v, 4) for k, v in r.items()})
    WORST.merge(r)
    return res


CASES = [
    # vector path: 1, 3, 12, 32 and 65 channel groups (2 tiles of 33)
    ((65, 8), 0, 0), ((65, 24), 1, 3), ((65, 96), 3, 1), ((65, 256), 2, 4),
    ((65, 520), 4, 2),
    # element path
    ((65, 3), 3, 3), ((65, 20), 1, 0), ((65, 50), 0, 2),
    # rows: C = 256 has 8 row lanes per workgroup
    ((2, 256), 3, 0), ((7, 256), 0, 3), ((ONE_WG, 256), 1, 1),
    ((ONE_WG + 1, 256), 3, 3), ((63, 256), 4, 0), ((64, 256), 2, 2),
    ((P_WRAP, 256), 3, 3),
    # C = 8: 256 row lanes, one workgroup up to 1024 rows
    ((1024, 8), 3, 1), ((1025, 8), 1, 3),
    # past the caps of the grids (1024 row slices of a reduction, 2048 of an
    # elementwise pass): lanes take more than the 4 unrolled rows of a sum
    # and more than one row of an apply pass, through the loops' tails
    ((40000, 256), 3, 3), ((600000, 8), 1, 1), ((21000, 50), 3, 1),
    # layouts
    ((2, 5, 7, 16), 3, 3), ((100, 4096), 3, 0), ((4, 9, 24), 1, 4),
]


# shape -> whether the reduction's grid is at its cap too
CAPPED = {(40000, 256): True, (600000, 8): False, (21000, 50): True}


@pytest.mark.parametrize("shape,act,aux_act", CASES)
def test_kernels_against_the_oracle(shape, act, aux_act):
    case = make_case(shape, 11, dtype=BF)
    dcase = to_gpu(case)
    C = shape[-1]
    assert is_vec(dcase[0]) == (C % 8 == 0)
    got = run_gpu(dcase, act, aux_act)
    check("", case, dcase, got, act, aux_act)
    if shape in CAPPED:
        ge = geom(shape[0], C, C % 8 == 0)
        # rows per lane of an apply pass (2048 // NTX slices at most) and of
        # a reduction (4 are unrolled); whether the reduction's cap holds
        assert -(-shape[0] // (2048 // ge["NTX"] * ge["RY"])) >= 2
        assert (-(-shape[0] // (ge["G"] * ge["RY"])) > 4,
                ge["G"] == 1024 // ge["NTX"]) == (CAPPED[shape],) * 2
    if shape == (P_WRAP, 256):
        assert geom(P_WRAP, 256, True)["G"] == 65
        assert geom(P_WRAP - 1, 256, True)["G"] == 64
    if shape[0] in (ONE_WG, ONE_WG + 1) and C == 256:
        assert geom(shape[0], 256, True)["G"] == 1 + (shape[0] > ONE_WG)


@pytest.mark.parametrize("act", [0, 1, 2, 3, 4])
def test_every_activation_and_its_derivative(act):
    case = make_case((130, 40), 13, dtype=BF)
    dcase = to_gpu(case)
    check("", case, dcase, run_gpu(dcase, act, act), act, act)
    # own_derivative off: the layer's activation, a linear backward
    got = run_gpu(dcase, act, 0)
    x, err, aux, g = dcase[:4]
    dg, db = torch.zeros_like(g), torch.zeros_like(g)
    dx = ops.batchnorm_bwd(err, x, None, g, got["save"], dg, db, act=0)
    lin = run_gpu(dcase, 0, 0)
    assert same_bits(dx, lin["dx"])


def test_accumulate_adds_and_overwrite_replaces():
    case = make_case((70, 24), 17, dtype=BF)
    dcase = to_gpu(case)
    base = torch.full((24,), 3.0), torch.full((24,), -2.0)
    got = run_gpu(dcase, 1, 0, accumulate=True,
                  grads=tuple(t.cuda() for t in base))
    check("accumulate", case, dcase, got, 1, 0, dg0=base[0], db0=base[1])
    got = run_gpu(dcase, 1, 0, need_dx=False)
    assert got["dx"] is None
    check("no dx", case, dcase, got, 1, 0)


@pytest.mark.parametrize("shape", [(33, 64), (5, 50), (1, 8), (1, 3)])
def test_eval_mode_uses_and_keeps_the_running_statistics(shape):
    case = make_case(shape, 19, dtype=BF)
    dcase = to_gpu(case)
    for act in range(5):
        got = run_gpu(dcase, act, 0, training=False)
        check("eval", case, dcase, got, act, 0, training=False)
        assert torch.equal(got["rm"], dcase[5])
        assert torch.equal(got["rv"], dcase[6])


@pytest.mark.parametrize("P", [2000, 8192])
def test_large_mean(P):
    """mean 64, std 0.5 (test_batchnorm_ref shows that E[x^2] - mean^2 in
    float32 leaves these bounds)"""
    x = large_mean_case(P).to(BF)
    C = x.shape[1]
    gen = torch.Generator().manual_seed(1)
    case = (x, torch.randn(P, C, generator=gen).to(BF), None,
            torch.ones(C), torch.zeros(C), torch.zeros(C), torch.ones(C))
    dcase = [None if t is None else t.cuda() for t in case]
    got = run_gpu(dcase, 0, 0)
    check("large mean", case, dcase, got, 0, 0)


def test_large_mean_with_an_outlier_in_the_first_row():
    """A zero in row 0 of channels of mean 64, std 0.5 (what a ReLU leaves):
    the shift is the mean of the first 8 rows, 8 away from the channel's
    mean, and the results stay inside the bounds, which grow with (K -
    mean)^2 / var (printed)"""
    x = large_mean_case(4096).to(BF)
    x[0] = 0
    C = x.shape[1]
    gen = torch.Generator().manual_seed(2)
    case = (x, torch.randn(4096, C, generator=gen).to(BF), None,
            torch.ones(C), torch.zeros(C), torch.zeros(C), torch.ones(C))
    dcase = [None if t is None else t.cuda() for t in case]
    got = run_gpu(dcase, 0, 0)
    f, fe = check("outlier row", case, dcase, got, 0, 0)
    rel = (fe["var"] / f["var"]).max()
    err = (np.abs(got["save"]["invstd"].double().cpu().numpy() -
                  f["invstd"]) / f["invstd"]).max()
    print("bound on var: %.2e of var; invstd off by %.2e" % (rel, err))
    assert rel < 1e-2


def test_vector_and_element_paths_agree():
    case = make_case((77, 64), 23, dtype=BF)
    a, b = to_gpu(case), to_gpu(case, misalign=True)
    assert is_vec(a[0]) and not is_vec(b[0])
    ga, gb = run_gpu(a, 3, 3), run_gpu(b, 3, 3)
    _, fa = check("vector", case, a, ga, 3, 3)
    _, fb = check("element", case, b, gb, 3, 3)
    for k in ("mean", "invstd"):
        d = (ga["save"][k] - gb["save"][k]).abs().double().cpu().numpy()
        key = "mu" if k == "mean" else k
        assert (d <= fa[key] + fb[key]).all(), k
    # y: each path is within its bound of the oracle, so they are within the
    # sum of the two of each other, element by element
    from test_batchnorm_ref import bf_half_ulp, bn_ref, rows
    from test_step_tail_ref import f64
    f = bn_ref(rows(case[0]), *(f64(t) for t in case[3:7]), 3)
    bound = sum(e["y"] + bf_half_ulp(np.abs(f["y"]) + e["y"])
                for e in (fa, fb))
    d = np.abs(rows(ga["y"]) - rows(gb["y"]))
    assert (d <= bound).all()


def test_two_runs_are_bit_identical():
    for shape in ((P_WRAP, 256), (300, 50)):
        case = make_case(shape, 29, dtype=BF)
        dcase = to_gpu(case)
        a, b = run_gpu(dcase, 1, 3), run_gpu(dcase, 1, 3)
        for k in ("y", "rm", "rv", "dx", "dg", "db"):
            assert same_bits(a[k], b[k]), k
        for k in ("mean", "invstd", "table"):
            assert same_bits(a["save"][k], b["save"][k]), k


def test_graph_replays_move_the_running_statistics():
    """one captured training step replayed five times = five eager steps"""
    case = make_case((200, 48), 31, dtype=BF)
    x, err, aux, g, b, rm0, rv0 = to_gpu(case)
    C = 48

    def step(rm, rv, save, ws, out, dx, dg, db):
        ops.batchnorm_fwd(x, g, b, rm, rv, act=3, save=save, out=out, ws=ws)
        ops.batchnorm_bwd(err, x, out, g, save, dg, db, act=3, aux=aux,
                          aux_act=1, out=dx, ws=ws)

    def state():
        return (rm0.clone(), rv0.clone(), {}, {}, torch.empty_like(x),
                torch.empty_like(x), torch.zeros(C, device="cuda"),
                torch.zeros(C, device="cuda"))
    eager = state()
    for _ in range(5):
        step(*eager)
    torch.cuda.synchronize()
    st = state()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(*st)                      # allocates save / ws
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    kept = {k: v.data_ptr() for k, v in list(st[2].items()) +
            list(st[3].items())}
    st[0].copy_(rm0)
    st[1].copy_(rv0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(*st)
    assert kept == {k: v.data_ptr() for k, v in list(st[2].items()) +
                    list(st[3].items())}
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(st[0], rm0)
    for a, b_ in zip(eager[:2] + eager[4:], st[:2] + st[4:]):
        assert same_bits(a, b_)


def test_host_checks_on_the_gpu():
    case = make_case((6, 8), 37, dtype=BF)
    x, err, aux, g, b, rm, rv = to_gpu(case)
    with pytest.raises(TypeError):
        ops.batchnorm_fwd(x.float(), g, b, rm, rv)
    with pytest.raises(ValueError):
        ops.batchnorm_fwd(x, g.cpu(), b, rm, rv)
    with pytest.raises(ValueError):
        ops.batchnorm_fwd(x[:1], g, b, rm, rv)
    with pytest.raises(ValueError):
        ops.batchnorm_fwd(x.t(), g, b, rm, rv)
    save = {}
    y = ops.batchnorm_fwd(x, g, b, rm, rv, save=save)
    dg, db = torch.zeros_like(g), torch.zeros_like(g)
    with pytest.raises(TypeError):
        ops.batchnorm_bwd(err.float(), x, y, g, save, dg, db)
    with pytest.raises(ValueError):
        ops.batchnorm_bwd(err.cpu(), x, y, g, save, dg, db)
    # 2^31 elements: rejected before any launch
    big = torch.empty((2 ** 31 // 8, 8), dtype=BF, device="cuda")
    with pytest.raises(ValueError):
        ops.batchnorm_fwd(big, g, b, rm, rv)
    del big
    assert _lib.lib().hvk_bn_partials(2 ** 31 // 8, 8, 1) == -1
    # a row pitch: the left 8 columns of a [6][24] tensor
    wide = torch.randn(6, 24, device="cuda").to(BF)
    y1 = ops.batchnorm_fwd(wide[:, :8], g, b, rm.clone(), rv.clone())
    y2 = ops.batchnorm_fwd(wide[:, :8].contiguous(), g, b, rm.clone(),
                           rv.clone())
    assert same_bits(y1, y2)
    assert torch.isfinite(wide.float()).all()
