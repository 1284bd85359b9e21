"""The feed-forward activation kernels (csrc/kernels/ffn.hip) and
``ops.ffn_fwd`` / ``ops.ffn_bwd`` on the GPU against the float64 oracle and
the bounds of test_ffn_ref.py, fed with the GPU's own bf16 tensors.

Paths of the backward: tile (du^T wanted; P and F multiples of 64; a slab is
4 row tiles when P % 256 == 0, else 1), vector row (F % 8 == 0, 16-byte
grid), guarded element (everything else).

Grid-stride caps, each passed by one shape: the forward's grid is at most
2048 x 1024 workgroups of 256 lanes (a contiguous tensor is one long row:
more than 2048 * 256 groups of 8 = 4 194 304 elements wrap in x; more than
1024 pitched rows wrap in y); the row path has at most 256 slabs of 8 rows
(P > 2048 wraps); the tile path at most 512 grid rows (more than 512 slabs:
P = 64 * 513 with one tile per slab).

The worst |error| / bound per quantity goes to
profiles/ffn/gpu_tests_figures.txt."""
import os

import pytest
import torch

from veles_amd import ops
from test_ffn_ref import (ACTS, K, SHAPES, bf, check_stages, db1_bound,
                          du_bound, h_bound, make_case, oracle, sweep, worst)
from test_step_tail_ref import BF, same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIGURES = os.path.join(ROOT, "profiles", "ffn", "gpu_tests_figures.txt")
WORST = {}


def see(name, r):
    WORST[name] = max(WORST.get(name, 0.0), r)
    assert r <= 1.0, (name, r)


@pytest.fixture(scope="module", autouse=True)
def figures():
    yield
    if not WORST:
        return
    os.makedirs(os.path.dirname(FIGURES), exist_ok=True)
    with open(FIGURES, "w") as f:
        f.write("# worst |error| / bound per quantity over "
                "tests/test_ffn_gpu.py\n")
        for k in sorted(WORST):
            f.write("%-20s %.4f\n" % (k, WORST[k]))


def misaligned(t):
    """a copy of t that starts 8 bytes past the 16-byte grid"""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    out = buf[4:4 + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 8
    return out


def pitched(t, k=3, at=1):
    """a 2-D column slice of a [P][k F] buffer"""
    P, C = t.shape
    wide = torch.zeros(P, k * C, dtype=t.dtype, device=t.device)
    v = wide[:, at * C:(at + 1) * C]
    v.copy_(t)
    assert not v.is_contiguous() or P == 1
    return v


def rand_case(P, F_, seed=3):
    g = torch.Generator().manual_seed(seed * 1000 + P + F_)
    u = (2.0 * torch.randn(P, F_, generator=g)).clamp(-16, 16).to(BF)
    dh = torch.randn(P, F_, generator=g).to(BF)
    return u, dh


def slabs(P, F_, transposed):
    if transposed:
        return P // (64 * (4 if P % 256 == 0 else 1))
    return min(-(-P // 32), 256)


def run_act(u, dh, act, layout=None, transposed=False, alias=False,
            accumulate="overwrite", tag=""):
    """forward and backward of one case on the GPU, checked against float64;
    returns the GPU tensors (h, du, dut, db1)"""
    dev = torch.device("cuda")
    P, F_ = u.shape
    lay = layout or (lambda t: t)
    ud, dhd = lay(u.to(dev)), lay(dh.to(dev))
    h = lay(torch.zeros(P, F_, dtype=BF, device=dev))
    ops.ffn_act_fwd(ud, act, out=h)
    du = dhd if alias else lay(torch.zeros(P, F_, dtype=BF, device=dev))
    dut = torch.zeros(F_, P, dtype=BF, device=dev) if transposed else None
    db1 = torch.full((F_,), 2.0, device=dev)
    ws = {}
    assert ops.ffn_partials(P, F_, transposed) == slabs(P, F_, transposed)
    ops.ffn_act_bwd(dhd, ud, act, out=du, out_t=dut, db1=db1,
                    accumulate=accumulate, ws=ws)
    torch.cuda.synchronize()
    assert ws["act_bwd"].numel() == F_ * slabs(P, F_, transposed)
    if not alias:
        assert torch.equal(dhd.cpu(), dh)       # inputs untouched
    assert torch.equal(ud.cpu(), u)
    ref, d = oracle(u, act)
    hc, duc = h.cpu().double(), du.cpu().double()
    want = dh.double() * d
    if act == "str":
        assert torch.equal(hc, ref) and torch.equal(duc, want)
    rh = worst((hc - ref).abs(), h_bound(ref, u))
    rd = worst((duc - want).abs(), du_bound(dh, d, u))
    see(act + " h", rh)
    see(act + " du", rd)
    base = 2.0 if accumulate is True else 0.0
    # added to 2.0: one more float32 rounding, of the sum's size
    got = db1.cpu().double()
    rb = worst((got - base - duc.sum(0)).abs(),
               db1_bound(duc) + (2.0 ** -24 * got.abs() if base else 0.0))
    see(act + " db1", rb)
    if transposed:
        assert torch.equal(dut.cpu(), du.cpu().t())
    print(tag, (P, F_), act, "h %.3f du %.3f db1 %.3f" % (rh, rd, rb))
    return h, du, dut, db1


@pytest.mark.parametrize("act", ACTS)
def test_sweep_of_every_bf16_value(act):
    """[256][256] holding every normal bf16 u with 2^-100 <= |u| <= 16 and 0
    (repeated to fill), through the tile path and the row path"""
    s = sweep()
    n = 256 * 256
    u = s.repeat(-(-n // s.numel()))[:n].view(256, 256).to(BF)
    assert torch.equal(u.float().view(-1)[:s.numel()], s)
    g = torch.Generator().manual_seed(9)
    dh = (torch.randn(256, 256, generator=g) * 2).to(BF)
    a = run_act(u, dh, act, transposed=True, tag="sweep tile")
    b = run_act(u, dh, act, tag="sweep row")
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", ((64, 64), (128, 192), (256, 64),
                                   (320, 128)))
def test_tile_path(shape, act):
    """one tile; several column tiles; one slab of four tiles; five slabs
    (an odd count)"""
    u, dh = rand_case(*shape)
    run_act(u, dh, act, transposed=True, tag="tile")


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", ((1, 8), (63, 72), (257, 136)))
def test_vector_row_path(shape, act):
    u, dh = rand_case(*shape)
    run_act(u, dh, act, tag="vector")


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", ((5, 7), (65, 1)))
def test_element_path(shape, act):
    u, dh = rand_case(*shape)
    run_act(u, dh, act, tag="element")


@pytest.mark.parametrize("act", ("gelu", "str"))
def test_base_eight_bytes_off_the_grid_takes_the_element_path(act):
    u, dh = rand_case(33, 72)
    a = run_act(u, dh, act, layout=misaligned, tag="misaligned")
    b = run_act(u, dh, act, tag="aligned")
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])


@pytest.mark.parametrize("shape,transposed", (((63, 72), False),
                                              ((64, 64), True),
                                              ((5, 7), False)))
def test_rows_that_are_column_slices_of_a_wider_buffer(shape, transposed):
    u, dh = rand_case(*shape)
    run_act(u, dh, "gelu", layout=pitched, transposed=transposed,
            tag="pitched")


@pytest.mark.parametrize("shape,transposed", (((128, 192), True),
                                              ((63, 72), False),
                                              ((5, 7), False)))
def test_du_may_alias_dh_and_h_may_alias_u(shape, transposed):
    u, dh = rand_case(*shape)
    a = run_act(u, dh, "gelu_tanh", transposed=transposed, alias=True,
                tag="alias")
    b = run_act(u, dh, "gelu_tanh", transposed=transposed, tag="apart")
    assert same_bits(a[1], b[1]) and same_bits(a[3], b[3])
    ud = u.cuda()
    ops.ffn_act_fwd(ud, "gelu_tanh", out=ud)
    assert same_bits(ud, a[0])


def test_accumulate_adds_to_db1():
    u, dh = rand_case(128, 64)
    run_act(u, dh, "gelu", transposed=True, accumulate=True, tag="acc tile")
    run_act(u, dh, "gelu", accumulate=True, tag="acc row")


@pytest.mark.parametrize("shape,layout,transposed", (
    ((1025, 4104), None, False),      # forward: one long row past 2048 x 256
    ((1030, 16), pitched, False),     # forward: more than 1024 pitched rows
    ((2056, 8), None, False),         # vector row path: more than 256 slabs
    ((2051, 3), None, False),         # element path: the same
    ((64 * 513, 64), None, True)))    # tile path: 513 slabs on 512 grid rows
def test_past_the_grid_stride_wrap(shape, layout, transposed):
    u, dh = rand_case(*shape)
    run_act(u, dh, "gelu", layout=layout, transposed=transposed, tag="wrap")


def test_gpu_host_checks():
    dev = torch.device("cuda")
    u = torch.zeros(64, 72, dtype=BF, device=dev)
    with pytest.raises(ValueError, match="multiples of 64"):
        ops.ffn_act_bwd(u, u, out_t=torch.zeros(72, 64, dtype=BF, device=dev))
    with pytest.raises(TypeError):
        ops.ffn_act_fwd(u.float())
    with pytest.raises(ValueError):
        ops.ffn_act_bwd(u[:, :64], u)
    with pytest.raises(ValueError):
        ops.ffn_partials(63, 64, True)
    fn = ops._lib.lib().hvk_ffn_act_fwd
    p = u.data_ptr()
    assert fn(p, 72, p, 72, 1 << 25, 72, 0, None) == -1     # 2^31 elements
    assert fn(p, 64, p, 72, 64, 72, 0, None) == -1          # pitch below F
    assert fn(p, 72, p, 72, 64, 72, 3, None) == -1          # no such act


def _whole(case, act, save=None):
    x, w1, w2, bias, err = case
    P, I = x.shape
    F_, E = w1.shape[0], w2.shape[0]
    dev = x.device
    save = {} if save is None else save
    y = ops.ffn_fwd(x, w1, w2, bias, act, save=save)
    dw1 = torch.empty(F_, I, device=dev)
    dw2 = torch.empty(E, F_, device=dev)
    dbias = torch.empty(F_ + E, device=dev)
    ei = ops.ffn_bwd(err, x, w1, w2, save, dw1, dw2, dbias, act)
    torch.cuda.synchronize()
    return save, y, dw1, dw2, dbias, ei


@pytest.fixture
def deterministic():
    ops.set_deterministic(True)
    yield
    ops.set_deterministic(False)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_ffn_stage_by_stage_on_the_saved_tensors(shape, act, deterministic):
    """every stage against float64 on the GPU's own stored operands: each
    bound is one GEMM's, K |ref| + k 2^-24 sum |a| |b| (float32 outputs:
    2^-24 |ref|), or the element-wise one"""
    case = make_case(*shape, BF, "cuda")
    save, y, dw1, dw2, dbias, ei = _whole(case, act)
    nn = shape[0] % 64 == 0
    assert ("dut" in save) == nn and ("dyt" in save) == nn
    fig = {}
    out = check_stages(*case, act, save, y, dw1, dw2, dbias, ei, K, fig)
    for k, v in fig.items():
        WORST["ffn " + k] = max(WORST.get("ffn " + k, 0.0), v)
    print(shape, act, {k: "%.3f" % v for k, v in out.items()})
    if nn:
        assert torch.equal(save["dut"], save["dh"].t())


def test_both_default_switch_variants_and_two_runs_give_equal_bits(
        deterministic):
    case = make_case(128, 64, 256, 64, BF, "cuda")
    runs = []
    old = ops.set_ffn_tile(True)
    try:
        for tile in (True, True, False):
            ops.set_ffn_tile(tile)
            save, *rest = _whole(case, "gelu")
            assert ("dut_ws" in save) == (not tile)
            runs.append(rest + [save[k] for k in ("u", "h", "dh", "dut",
                                                  "dyt")])
    finally:
        ops.set_ffn_tile(old)
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert same_bits(a, b)


def test_forward_and_backward_capture_in_one_graph(deterministic):
    """ffn_fwd + ffn_bwd captured once and replayed five times = eager"""
    case = make_case(128, 64, 256, 64, BF, "cuda")
    eager = _whole(case, "gelu")
    x, w1, w2, bias, err = case
    save = {}
    outs = [torch.empty_like(t) for t in eager[1:]]
    y, dw1, dw2, dbias, ei = outs

    def step():
        ops.ffn_fwd(x, w1, w2, bias, "gelu", save=save, out=y)
        ops.ffn_bwd(err, x, w1, w2, save, dw1, dw2, dbias, "gelu",
                    err_input=ei)

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        step()                                  # the first call allocates
    torch.cuda.synchronize()
    kept = {k: v.data_ptr() for k, v in save.items()}
    for t in outs:
        t.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    assert kept == {k: v.data_ptr() for k, v in save.items()}
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager[1:], outs):
        assert same_bits(a, b)
    for k in ("u", "h", "dh", "dut", "dyt"):
        assert same_bits(eager[0][k], save[k]), k
