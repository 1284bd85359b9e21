"""The layer-normalisation kernels (csrc/kernels/layernorm.hip) against the
float64 oracle of test_layernorm_ref.py, fed with the GPU's own bf16 tensors.

float32 results (saved mean and invstd, dgamma, dbeta) are held to the bounds
derived there with the reduction depths of the kernel's path (``path`` /
``slices``); bf16 results (y, dx) to half a bf16 ulp of the exact value plus
the propagated float32 term.

Shapes: the smallest that reach every path and edge.  Row ownership changes
with C (``path``): the vector path (C % 8 = 0, 16-byte grid) switches at
C = 128, 256, 512, 1024, 2048 (the last wave-owned row), 4096 and 8192 (the
last row kept in registers); the element path at 16, 64, 256, 1024 and 8192.
Each edge is taken with the first C past it; an element-path C that is a
multiple of 8 gets there through a misaligned base.  Rows: a workgroup pass
takes RPB = 256 / L rows; the forward and the dx-only kernel stride when
P > 2048 RPB, the kernels with column sums when P > 4096 RPB (1024 slices of
4 RPB rows): C = 8 (RPB 16) and C = 257 (element path, RPB 1) pass both caps,
C = 8200 the forward's and the dx kernel's on the re-reading path (whose
column-sum kernel strides over rows from P = 5 on: G = ceil(P / 4)).
Element rows of 1025 .. 8192 columns are staged in LDS by the column-loop
kernels (C = 1025, 8192 misaligned, 8193 past it).

The worst |error| / bound per quantity goes to
profiles/layernorm/gpu_tests_figures.txt."""
import os

import numpy as np
import pytest
import torch

from veles_amd import ops
from veles_amd.ops import _lib
from test_layernorm_ref import (check_case, large_mean_case, make_case, path,
                                run, slices)
from test_step_tail_ref import BF, Ratios, same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIGURES = os.path.join(ROOT, "profiles", "layernorm", "gpu_tests_figures.txt")
WORST = Ratios()


@pytest.fixture(scope="module", autouse=True)
def figures():
    yield
    if not WORST:
        return
    os.makedirs(os.path.dirname(FIGURES), exist_ok=True)
    with open(FIGURES, "w") as f:
        f.write("# worst |error| / bound per quantity over "
                "tests/test_layernorm_gpu.py\n")
        for k in sorted(WORST):
            f.write("%-8s %.4f\n" % (k, WORST[k]))


def misaligned(t):
    """a copy of t that starts 8 bytes past the 16-byte grid"""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    out = buf[4:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 8
    return out


def pitched(t, k=3, at=1):
    """a 2-D column slice of a [P][k C] buffer (as attention's [B T][3E])"""
    P, C = t.shape
    wide = torch.zeros(P, k * C, dtype=t.dtype, device=t.device)
    v = wide[:, at * C:(at + 1) * C]
    v.copy_(t)
    assert not v.is_contiguous()
    return v


def to_gpu(case, layout=None):
    dev = torch.device("cuda")
    out = [None if t is None else t.to(dev) for t in case]
    for i in (0, 1, 2):
        if out[i] is not None and layout is not None:
            out[i] = layout(out[i])
    return out


def is_vec(*ts):
    fn = _lib.lib().hvk_ln_vec
    return all(t is None or bool(fn(
        t.data_ptr(), t.stride(0) if t.dim() == 2 else t.shape[-1],
        t.shape[-1])) for t in ts)


def check(tag, case, dcase, got, **kw):
    x = dcase[0]
    C = x.shape[-1]
    P = x.numel() // C
    vec = is_vec(*dcase[:3]) and C % 8 == 0
    p = path(C, vec)
    G, Dcol = slices(P, C, vec)
    assert ops.ln_partials(P, C, vec) == G
    r = Ratios()
    res = check_case(r, "", got, case, p["Drow"], Dcol, True, **kw)
    print(tag, tuple(x.shape), "residual" if case[1] is not None else "plain",
          "vec" if vec else "elem", p["kind"], "L", p["L"], "K", p["K"], "G",
          G, {k: round(v, 4) for k, v in r.items()})
    WORST.merge(r)
    return res


def go(shape, residual, layout=None, vec=None, seed=11, **kw):
    case = make_case(shape, seed, residual, dtype=BF)
    dcase = to_gpu(case, layout)
    if vec is not None:
        assert (is_vec(*dcase[:3]) and shape[-1] % 8 == 0) == vec
    got = run(dcase, **kw)
    torch.cuda.synchronize()
    return case, dcase, got


# C: the issue's list, then both sides of every switch of the vector path
C_VEC = [8, 64, 128, 136, 256, 264, 512, 520, 1000, 1024, 1032, 2048, 2056,
         4096, 4104, 8192, 8200]
# ... of the element path (not a multiple of 8: it is taken anyway)
C_ELEM = [1, 3, 17, 50, 65, 257, 1025, 8193]
# ... and its last Cs, multiples of 8, through a misaligned base
C_ELEM_MISALIGNED = [16, 64, 256, 1024, 8192]


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("C", C_VEC + C_ELEM)
def test_every_width_against_the_oracle(C, residual):
    case, dcase, got = go((5, C), residual, vec=C % 8 == 0)
    check("", case, dcase, got)


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("C", C_ELEM_MISALIGNED)
def test_a_misaligned_base_takes_the_element_path(C, residual):
    case, dcase, got = go((5, C), residual, layout=misaligned, vec=False)
    check("misaligned", case, dcase, got)


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("C", [8, 50, 64, 520, 1025, 2056, 8200])
@pytest.mark.parametrize("P", [1, 2, 5, 33, 257])
def test_rows_against_the_oracle(P, C, residual):
    case, dcase, got = go((P, C), residual)
    check("", case, dcase, got)


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("shape", [(32769, 8), (65537, 8), (2049, 257),
                                   (4097, 257), (2049, 1025)])
def test_rows_past_the_grid_caps(shape, residual):
    P, C = shape
    vec = C % 8 == 0
    p = path(C, vec)
    assert P > 2048 * p["RPB"]
    assert (slices(P, C, vec)[0] == 1024 and P > 4096 * p["RPB"]) == \
        (shape in ((65537, 8), (4097, 257)))
    case, dcase, got = go(shape, residual)
    check("capped", case, dcase, got)


@pytest.mark.parametrize("residual", [False, True])
def test_rows_past_the_grid_cap_of_the_rereading_kernels(residual):
    case, dcase, got = go((2049, 8200), residual)
    assert path(8200, True)["kind"] == "reread"
    check("capped", case, dcase, got)


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("shape", [(2, 5, 7, 16), (4, 9, 24), (3, 4, 6)])
def test_layouts(shape, residual):
    case, dcase, got = go(shape, residual)
    assert got["y"].shape == dcase[0].shape == got["dx"].shape
    check("", case, dcase, got)


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("C,vec", [(64, True), (520, True), (50, False),
                                   (12, False)])
def test_rows_with_a_pitch(C, vec, residual):
    """column slices of a [P][3 C] buffer, the output into one too"""
    case = make_case((33, C), 13, residual, dtype=BF)
    dcase = to_gpu(case, pitched)
    x, r, err, g, b = dcase
    assert (is_vec(x, r, err) and C % 8 == 0) == vec
    save = {}
    y = pitched(torch.zeros_like(x).contiguous())
    dx = pitched(torch.zeros_like(x).contiguous(), at=2)
    wide_y, wide_dx = y._base, dx._base
    ops.layernorm_fwd(x, g, b, residual=r, save=save, out=y)
    dg, db = torch.zeros_like(g), torch.zeros_like(g)
    ops.layernorm_bwd(err, x, g, save, dg, db, residual=r, out=dx)
    torch.cuda.synchronize()
    got = {"y": y, "save": save, "dx": dx, "dg": dg, "db": db}
    check("pitched", case, [x, r, err, dx, y], got)
    # nothing outside the slices was written
    assert (wide_y[:, :C] == 0).all() and (wide_y[:, 2 * C:] == 0).all()
    assert (wide_dx[:, :2 * C] == 0).all()
    # and the bits are those of the contiguous call (vector path: same path)
    if vec:
        c = run([t if t is None else t.contiguous() for t in dcase])
        for k in ("y", "dx", "dg", "db"):
            assert same_bits(got[k].contiguous(), c[k]), k


def test_one_column_gives_beta():
    case, dcase, got = go((9, 1), True)
    check("C = 1", case, dcase, got)
    assert same_bits(got["y"], dcase[4].to(BF).expand(9, 1).contiguous())
    assert (got["dx"] == 0).all()


def test_accumulate_adds_and_overwrite_replaces():
    base = torch.full((24,), 3.0), torch.full((24,), -2.0)
    case, dcase, got = go((70, 24), True, accumulate=True,
                          grads=tuple(t.cuda() for t in base))
    check("accumulate", case, dcase, got, dg0=base[0], db0=base[1])
    case, dcase, got = go((70, 24), True, need_dx=False)
    assert got["dx"] is None
    check("no dx", case, dcase, got)


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("C", [2000, 8192])
def test_large_mean(C, residual):
    """rows of mean 64, std 0.5 (test_layernorm_ref shows that E[s^2] -
    mean^2 in float32 and a residual rounded to bf16 leave these bounds)"""
    case = large_mean_case(16, C, residual=residual)
    case = tuple(t if t is None or t.dim() == 1 else t.to(BF) for t in case)
    dcase = to_gpu(case)
    got = run(dcase)
    torch.cuda.synchronize()
    check("large mean", case, dcase, got)


def test_both_column_sum_variants():
    """the A/B switch of tools/bench_layernorm.py: column sums inside the dx
    kernel or in a pass of their own, both within the bounds"""
    fn = _lib.lib().hvk_ln_colsum
    old = fn(-1)
    try:
        for mode in (0, 1):
            assert fn(mode) == (old if mode == 0 else 0)
            for C in (64, 1000, 4096, 257):
                case, dcase, got = go((37, C), True)
                check("colsum %d" % mode, case, dcase, got)
    finally:
        fn(old)
    assert fn(old) == old


def test_vector_and_element_paths_agree():
    for residual in (False, True):
        case = make_case((77, 64), 23, residual, dtype=BF)
        a, b = to_gpu(case), to_gpu(case, misaligned)
        assert is_vec(*a[:3]) and not is_vec(*b[:3])
        ga, gb = run(a), run(b)
        torch.cuda.synchronize()
        fa, ea, ra, ba = check("vector", case, a, ga)
        fb, eb, rb, bb = check("element", case, b, gb)
        from test_step_tail_ref import bf_half_ulp, f64
        for k, key in (("mean", "mu"), ("invstd", "invstd")):
            d = np.abs(f64(ga["save"][k]) - f64(gb["save"][k]))
            assert (d <= ea[key] + eb[key]).all(), k
        for k in ("dg", "db"):
            assert (np.abs(f64(ga[k]) - f64(gb[k])) <= ba[k] + bb[k]).all()
        # y, dx: each path is within its bound of the oracle, so they are
        # within the sum of the two of each other, element by element
        for k, want, e1, e2 in (("y", fa["y"], ea["y"], eb["y"]),
                                ("dx", ra["dx"], ba["dx"], bb["dx"])):
            bound = sum(e + bf_half_ulp(np.abs(want) + e) for e in (e1, e2))
            d = np.abs(f64(ga[k]) - f64(gb[k])).reshape(want.shape)
            assert (d <= bound).all(), k


def test_two_runs_are_bit_identical():
    for shape in ((2049, 256), (300, 50), (40, 4104), (9, 8200)):
        case = make_case(shape, 29, True, dtype=BF)
        dcase = to_gpu(case)
        a, b = run(dcase), run(dcase)
        torch.cuda.synchronize()
        for k in ("y", "dx", "dg", "db"):
            assert same_bits(a[k], b[k]), k
        for k in ("mean", "invstd"):
            assert same_bits(a["save"][k], b["save"][k]), k


def test_forward_and_backward_capture_in_one_graph():
    """one captured forward + backward replayed five times = the eager bits"""
    case = make_case((200, 48), 31, True, dtype=BF)
    x, r, err, g, b = to_gpu(case)
    C = 48

    def step(save, ws, out, dx, dg, db):
        ops.layernorm_fwd(x, g, b, residual=r, save=save, out=out)
        ops.layernorm_bwd(err, x, g, save, dg, db, residual=r, out=dx, ws=ws)

    def state():
        return ({}, {}, torch.empty_like(x), torch.empty_like(x),
                torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda"))
    eager = state()
    step(*eager)
    torch.cuda.synchronize()
    st = state()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(*st)                      # allocates save / ws
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    kept = {k: v.data_ptr() for k, v in list(st[0].items()) +
            list(st[1].items())}
    assert set(st[0]) == {"mean", "invstd"} and set(st[1]) == {"bwd"}
    for t in st[2:]:
        t.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(*st)
    assert kept == {k: v.data_ptr() for k, v in list(st[0].items()) +
                    list(st[1].items())}
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    for a, b_ in zip(eager[2:], st[2:]):
        assert same_bits(a, b_)
    for k in ("mean", "invstd"):
        assert same_bits(eager[0][k], st[0][k])


# ----------------------------------------------------------------- ops.add
# 3 10^6 elements pass the grid cap of the element path (2048 workgroups of
# 256 lanes, one element each), ADD_CAP_VEC that of the vector path (8 each)
ADD_CAP_VEC = 2048 * 256 * 8 + 8 * 5


@pytest.mark.parametrize("n", [1, 7, 8, 8 * 1024 + 3, 8 * 1024, 3 * 10 ** 6,
                               ADD_CAP_VEC])
def test_add_bit_for_bit(n):
    gen = torch.Generator().manual_seed(n)
    a = (3 * torch.randn(n, generator=gen)).to(BF).cuda()
    b = (3 * torch.randn(n, generator=gen)).to(BF).cuda()
    want = (a.float() + b.float()).bfloat16()
    assert same_bits(ops.add(a, b), want)
    if n > 4:        # the element path on the same values, and in place
        am = misaligned(a)
        assert same_bits(ops.add(am, b), want)
        ops.add(am, b, out=am)
        assert same_bits(am, want)


@pytest.mark.parametrize("shape", [(33, 64), (33, 50), (5, 8), (1100, 24),
                                   (3, 2304)])
def test_add_with_pitches(shape):
    gen = torch.Generator().manual_seed(5)
    a = torch.randn(shape, generator=gen).to(BF).cuda()
    b = torch.randn(shape, generator=gen).to(BF).cuda()
    want = (a.float() + b.float()).bfloat16()
    ap, bp = pitched(a), pitched(b, k=2, at=0)
    out = pitched(torch.zeros_like(a), k=4, at=2)
    assert ops.add(ap, bp, out=out) is out
    assert same_bits(out.contiguous(), want)
    C = shape[1]
    assert (out._base[:, :2 * C] == 0).all() and \
        (out._base[:, 3 * C:] == 0).all()
    assert same_bits(ops.add(ap, b), want)      # mixed: pitched + contiguous
    assert same_bits(ops.add(a.view(-1, 1, C), b.view(-1, 1, C)).view(shape),
                     want)


# -------------------------------------------------------------- host checks
def test_host_checks_on_the_gpu():
    case = make_case((6, 8), 37, True, dtype=BF)
    x, r, err, g, b = to_gpu(case)
    with pytest.raises(TypeError):
        ops.layernorm_fwd(x.float(), g, b)
    with pytest.raises(ValueError):
        ops.layernorm_fwd(x, g.cpu(), b)
    with pytest.raises(ValueError):
        ops.layernorm_fwd(x.t(), g, b)
    with pytest.raises(ValueError):
        ops.layernorm_fwd(x, g, b, residual=r[:5])
    with pytest.raises(ValueError):
        ops.layernorm_fwd(x, g, b, residual=r.cpu())
    with pytest.raises(TypeError):
        ops.layernorm_fwd(x, g, b, residual=r.float())
    save = {}
    ops.layernorm_fwd(x, g, b, residual=r, save=save)
    dg, db = torch.zeros_like(g), torch.zeros_like(g)
    with pytest.raises(TypeError):
        ops.layernorm_bwd(err.float(), x, g, save, dg, db)
    with pytest.raises(ValueError):
        ops.layernorm_bwd(err.cpu(), x, g, save, dg, db)
    with pytest.raises(ValueError):
        ops.layernorm_bwd(err, x, g, {k: v.cpu() for k, v in save.items()},
                          dg, db)
    with pytest.raises(TypeError):
        ops.add(x, r.float())
    with pytest.raises(ValueError):
        ops.add(x, r[:5])
    # 2^31 elements: rejected before any launch
    big = torch.empty((2 ** 31 // 8, 8), dtype=BF, device="cuda")
    with pytest.raises(ValueError, match=r"2\^31"):
        ops.layernorm_fwd(big, g, b)
    with pytest.raises(ValueError, match=r"2\^31"):
        ops.add(big, big)
    del big
    # the entry points themselves refuse what the host checks let through
    lib = _lib.lib()
    p = x.data_ptr()
    s = torch.cuda.current_stream().cuda_stream
    m, i = save["mean"].data_ptr(), save["invstd"].data_ptr()
    assert lib.hvk_ln_fwd(p, 8, None, 8, p, 8, 2 ** 28, 8, g.data_ptr(),
                          b.data_ptr(), 1e-5, m, i, s) == -1
    assert lib.hvk_ln_fwd(p, 7, None, 8, p, 8, 6, 8, g.data_ptr(),
                          b.data_ptr(), 1e-5, m, i, s) == -1
    assert lib.hvk_add(p, 8, p, 8, p, 8, 2 ** 28, 8, s) == -1
    assert lib.hvk_add(p, 8, p, 4, p, 8, 6, 8, s) == -1
    torch.cuda.synchronize()
