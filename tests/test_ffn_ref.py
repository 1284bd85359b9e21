"""Position-wise feed-forward (docs/OPS.md "Position-wise feed-forward"): the
float64 oracle, the bounds the GPU tests use, the CPU path of
``ops.ffn_act_fwd`` / ``ffn_act_bwd`` / ``ffn_fwd`` / ``ffn_bwd`` inside them,
and wrong rules outside them.

Bounds, with K = 2^-8 (1 + 2^-10), half a bf16 ulp, against float64 on the
bf16 inputs:

    h     |err| <= K |ref| + 4 2^-24 |u|
    du    |err| <= |dh| (K |a'(u)| + 4 2^-24 (1 + |u|))
    "str" bit-exact
    db1   against the float64 sum of the stored du: <= P 2^-24 sum |du|

The sweep is every normal bf16 u with 2^-100 <= |u| <= 16, and u = 0
(subnormal u stays out: the kernels flush them)."""
import math

import pytest
import torch

from veles_amd import ops

K = 2.0 ** -8 * (1 + 2.0 ** -10)
EPS = 2.0 ** -24
ERF_TERM = 4.0          # the factor of 2^-24 in the bounds
ACTS = ("gelu", "gelu_tanh", "str")


def sweep():
    """every normal bf16 with 2^-100 <= |u| <= 16, and 0, as float32"""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    u = bits.view(torch.bfloat16).float()
    a = u.abs()
    return u[torch.isfinite(u) & (((a >= 2.0 ** -100) & (a <= 16)) |
                                  (u == 0))]


def bf(t):
    """round to bf16, back in float64"""
    return t.float().to(torch.bfloat16).double()


def oracle(u, act):
    """(a(u), a'(u)) in float64 from torch's own GELU and autograd"""
    u = u.double().clone().requires_grad_()
    if act == "str":
        h = torch.relu(u)               # derivative 0 at u = 0
    else:
        h = torch.nn.functional.gelu(
            u, approximate="tanh" if act == "gelu_tanh" else "none")
    d, = torch.autograd.grad(h.sum(), u)
    return h.detach(), d


def h_bound(ref, u):
    return K * ref.abs() + ERF_TERM * EPS * u.double().abs()


def du_bound(dh, d, u):
    return dh.double().abs() * (K * d.abs() +
                                ERF_TERM * EPS * (1 + u.double().abs()))


def worst(err, bound):
    """max |err| / bound; a zero bound must meet a zero error"""
    z = bound == 0
    assert (err[z] == 0).all()
    return float((err[~z] / bound[~z]).max()) if (~z).any() else 0.0


DH = (1.0, 0.8125, -1.4375, 3.0, -0.005859375)     # bf16 values


def test_oracle_is_torchs_gelu_and_its_closed_forms():
    u = sweep()
    for act in ACTS:
        h, d = oracle(u, act)
        assert h.dtype == torch.float64 and d.dtype == torch.float64
        # the ops module's closed forms, in float64, are the same functions
        h2 = ops.ffn_act_ref(u.double(), act)
        d2 = ops.ffn_dact_ref(u.double(), act)
        assert float((h - h2).abs().max()) <= 1e-14 * 16
        assert float((d - d2).abs().max()) <= 1e-13
    h, d = oracle(torch.tensor([0.0, -0.75, 3.0]), "gelu")
    assert h[0] == 0 and d[0] == 0.5
    phi = math.exp(-0.5 * 9) / math.sqrt(2 * math.pi)
    Phi = 0.5 * math.erfc(-3 / math.sqrt(2))
    assert abs(float(d[2]) - (Phi + 3 * phi)) < 1e-15


@pytest.mark.parametrize("act", ACTS)
def test_cpu_path_inside_the_bounds_on_the_full_sweep(act):
    u = sweep()
    ref, d = oracle(u, act)
    h = ops.ffn_act_fwd(u, act)
    assert h.dtype == torch.float32
    r = worst((bf(h) - ref).abs(), h_bound(ref, u))
    print(act, "h worst |err| / bound %.3f" % r)
    assert r <= 1.0
    if act == "str":
        assert torch.equal(h, torch.clamp_min(u, 0))
    for dhv in DH:
        dh = torch.full_like(u, dhv)
        du = ops.ffn_act_bwd(dh, u, act)
        want = dh.double() * d
        r = worst((bf(du) - want).abs(), du_bound(dh, d, u))
        print(act, "du (dh = %g) worst |err| / bound %.3f" % (dhv, r))
        assert r <= 1.0
        if act == "str":
            assert torch.equal(du.double(), want)


def _sigmoid_gelu(u):
    return u * torch.sigmoid(1.702 * u)


def test_wrong_rules_leave_the_bounds_by_ten_times():
    u = sweep()
    dh = torch.ones_like(u)
    for act, other in (("gelu", "gelu_tanh"), ("gelu_tanh", "gelu")):
        ref, d = oracle(u, act)
        # 1: the other GELU mode, forward
        r = worst((bf(ops.ffn_act_ref(u, other)) - ref).abs(),
                  h_bound(ref, u))
        print(act, "forward by the other mode: %.0f x" % r)
        assert r >= 10
        # 2: the other mode's derivative
        r = worst((bf(ops.ffn_dact_ref(u, other)) - d).abs(),
                  du_bound(dh, d, u))
        print(act, "derivative by the other mode: %.0f x" % r)
        assert r >= 10
        # 3: x sigmoid(1.702 x)
        r = worst((bf(_sigmoid_gelu(u)) - ref).abs(), h_bound(ref, u))
        print(act, "x sigmoid(1.702 x): %.0f x" % r)
        assert r >= 10
        # 4: a derivative without the u phi(u) term (Phi alone)
        Phi = torch.where(u == 0, torch.full_like(u, 0.5),
                          ops.ffn_act_ref(u, act) /
                          torch.where(u == 0, torch.ones_like(u), u))
        r = worst((bf(Phi) - d).abs(), du_bound(dh, d, u))
        print(act, "derivative without u phi(u): %.0f x" % r)
        assert r >= 10


def db1_bound(du):
    return du.shape[0] * EPS * du.double().abs().sum(0)


def test_db1_is_the_sum_of_the_stored_du_and_sees_a_dropped_row():
    g = torch.Generator().manual_seed(5)
    P, F_ = 130, 24
    u = torch.randn(P, F_, generator=g).to(torch.bfloat16).float()
    dh = torch.randn(P, F_, generator=g).to(torch.bfloat16).float()
    db1 = torch.empty(F_)
    du = ops.ffn_act_bwd(dh, u, "gelu", db1=db1)
    want = du.double().sum(0)
    bound = db1_bound(du)
    assert ((db1.double() - want).abs() <= bound).all()
    dropped = du[:-1].double().sum(0)
    r = float(((dropped - want).abs() / bound).max())
    print("db1 without the last row: %.0f x" % r)
    assert r >= 10


def gemm_bound(a, b, ref, k, half_ulp):
    """one GEMM's bound: half_ulp |ref| + k 2^-24 sum |a| |b| over its k
    products (a [M][k], b [k][N] float64)"""
    return half_ulp * ref.abs() + k * EPS * (a.abs() @ b.abs())


SHAPES = ((130, 8, 64, 16), (128, 64, 256, 64), (9, 40, 24, 40))


def make_case(P, I, F_, E, dtype, device="cpu", seed=0):
    g = torch.Generator().manual_seed(seed + P)
    r = lambda *s: torch.randn(*s, generator=g)     # noqa: E731
    x = r(P, I).to(dtype).to(device)
    w1 = (r(F_, I) / I ** 0.5).to(dtype).to(device)
    w2 = (r(E, F_) / F_ ** 0.5).to(dtype).to(device)
    bias = (0.5 * r(F_ + E)).to(device)
    err = r(P, E).to(dtype).to(device)
    return x, w1, w2, bias, err


def check_stages(x, w1, w2, bias, err, act, save, y, dw1, dw2, dbias, ei,
                 half_ulp, figures=None):
    """every stage of ffn_fwd / ffn_bwd against float64 on that stage's own
    stored inputs: each bound is one GEMM's, or the element-wise one"""
    d = lambda t: t.detach().double().cpu()     # noqa: E731
    x, w1, w2, bias, err, y, ei = map(d, (x, w1, w2, bias, err, y, ei))
    u, h, du = d(save["u"]), d(save["h"]), d(save["dh"])
    P, I = x.shape
    F_, E = w1.shape[0], w2.shape[0]
    b1, b2 = bias[:F_], bias[F_:]
    out = {}

    def stage(name, got, ref, bound):
        r = worst((got - ref).abs(), bound)
        out[name] = r
        if figures is not None:
            figures[name] = max(figures.get(name, 0.0), r)
        assert r <= 1.0, (name, r)

    ref = x @ w1.t() + b1
    stage("u", u, ref, gemm_bound(x, w1.t(), ref, I, half_ulp) +
          EPS * b1.abs())
    hr, dr = oracle(u, act)
    stage("h", h, hr, (K if half_ulp else 2 * EPS) * hr.abs() +
          ERF_TERM * EPS * u.abs())
    ref = h @ w2.t() + b2
    stage("y", y.view(P, E), ref,
          gemm_bound(h, w2.t(), ref, F_, half_ulp) + EPS * b2.abs())
    g = err.view(P, E)
    stage("db2", d(dbias)[F_:], g.sum(0), P * EPS * g.abs().sum(0))
    ref = g.t() @ h
    stage("dw2", d(dw2), ref, gemm_bound(g.t(), h, ref, P, EPS))
    # dh was overwritten by du: du against float64 dh of the stored operands
    # carries the dh GEMM's bound through |a'|, plus the element-wise one
    dhr = g @ w2
    dhb = gemm_bound(g, w2, dhr, E, half_ulp)
    ref = dhr * dr
    stage("du", du, ref, dhb * dr.abs() + (dhr.abs() + dhb) * (
        (K if half_ulp else 2 * EPS) * dr.abs() +
        ERF_TERM * EPS * (1 + u.abs())))
    stage("db1", d(dbias)[:F_], du.sum(0), db1_bound(du))
    ref = du.t() @ x
    stage("dw1", d(dw1), ref, gemm_bound(du.t(), x, ref, P, EPS))
    ref = du @ w1
    stage("err_input", ei.view(P, I), ref,
          gemm_bound(du, w1, ref, F_, half_ulp))
    return out


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_cpu_ffn_stage_by_stage_against_float64(shape, act):
    P, I, F_, E = shape
    x, w1, w2, bias, err = make_case(P, I, F_, E, torch.float32)
    save = {}
    y = ops.ffn_fwd(x, w1, w2, bias, act, save=save)
    dw1, dw2 = torch.empty(F_, I), torch.empty(E, F_)
    dbias = torch.empty(F_ + E)
    ei = ops.ffn_bwd(err, x, w1, w2, save, dw1, dw2, dbias, act)
    out = check_stages(x, w1, w2, bias, err, act, save, y, dw1, dw2, dbias,
                       ei, 0.0)
    print(shape, act, {k: "%.3f" % v for k, v in out.items()})
    # evaluation: no save, h over u, same y
    y2 = ops.ffn_fwd(x, w1, w2, bias, act)
    assert torch.equal(y, y2)
    # 3-D input, no bias, no err_input
    x3 = x.view(1, P, I)
    y3 = ops.ffn_fwd(x3, w1, w2, None, act, save=save)
    assert tuple(y3.shape) == (1, P, E)
    assert ops.ffn_bwd(err.view(1, P, E), x3, w1, w2, save, dw1, dw2, None,
                       act, need_err_input=False) is None


def test_whole_layer_matches_float64_autograd():
    P, I, F_, E = 9, 40, 24, 40
    x, w1, w2, bias, err = make_case(P, I, F_, E, torch.float32)
    for act, approx in (("gelu", "none"), ("gelu_tanh", "tanh")):
        net = torch.nn.Sequential(
            torch.nn.Linear(I, F_), torch.nn.GELU(approximate=approx),
            torch.nn.Linear(F_, E)).double()
        with torch.no_grad():
            net[0].weight.copy_(w1)
            net[0].bias.copy_(bias[:F_])
            net[2].weight.copy_(w2)
            net[2].bias.copy_(bias[F_:])
        xd = x.double().requires_grad_()
        yd = net(xd)
        yd.backward(err.double())
        save = {}
        y = ops.ffn_fwd(x, w1, w2, bias, act, save=save)
        dw1, dw2 = torch.empty(F_, I), torch.empty(E, F_)
        dbias = torch.empty(F_ + E)
        ei = ops.ffn_bwd(err, x, w1, w2, save, dw1, dw2, dbias, act)
        for got, want in ((y, yd), (ei, xd.grad), (dw1, net[0].weight.grad),
                          (dw2, net[2].weight.grad),
                          (dbias[:F_], net[0].bias.grad),
                          (dbias[F_:], net[2].bias.grad)):
            assert float((got.double() - want.detach()).abs().max()) <= \
                1e-5 * float(want.detach().abs().max())


def test_aux_act_multiplies_err_input_by_the_derivative_below():
    P, I, F_, E = 9, 40, 24, 40
    x, w1, w2, bias, err = make_case(P, I, F_, E, torch.float32)
    save = {}
    ops.ffn_fwd(x, w1, w2, bias, "gelu", save=save)
    dw1, dw2 = torch.empty(F_, I), torch.empty(E, F_)
    plain = ops.ffn_bwd(err, x, w1, w2, save, dw1, dw2, None, "gelu").clone()
    aux = torch.rand(P, I)
    fused = ops.ffn_bwd(err, x, w1, w2, save, dw1, dw2, None, "gelu",
                        aux=aux, aux_act="sigmoid")
    assert torch.allclose(fused, plain * aux * (1 - aux), rtol=1e-6,
                          atol=1e-7)


def test_accumulate_adds_and_overwrite_replaces():
    P, I, F_, E = 9, 40, 24, 40
    x, w1, w2, bias, err = make_case(P, I, F_, E, torch.float32)
    save = {}
    ops.ffn_fwd(x, w1, w2, bias, "gelu", save=save)
    g = [torch.full((F_, I), 7.0), torch.full((E, F_), 7.0),
         torch.full((F_ + E,), 7.0)]
    ops.ffn_bwd(err, x, w1, w2, save, *g, "gelu")
    first = [t.clone() for t in g]
    assert all((t != 7.0).all() for t in first)
    ops.ffn_bwd(err, x, w1, w2, save, *g, "gelu", accumulate="overwrite")
    assert all(torch.equal(a, b) for a, b in zip(g, first))
    ops.ffn_bwd(err, x, w1, w2, save, *g, "gelu", accumulate=True)
    for a, b in zip(g, first):
        assert torch.allclose(a, 2 * b, rtol=1e-6, atol=1e-7)
    db1 = torch.full((F_,), 3.0)
    ops.ffn_act_bwd(err[:, :F_].contiguous(), save["u"], "gelu", db1=db1,
                    accumulate=True)
    db0 = torch.empty(F_)
    ops.ffn_act_bwd(err[:, :F_].contiguous(), save["u"], "gelu", db1=db0)
    assert torch.allclose(db1, db0 + 3.0, rtol=1e-6, atol=1e-6)


def test_host_checks():
    P, I, F_, E = 9, 40, 24, 40
    x, w1, w2, bias, err = make_case(P, I, F_, E, torch.float32)
    save = {}
    ops.ffn_fwd(x, w1, w2, bias, "gelu", save=save)
    dw1, dw2, db = torch.empty(F_, I), torch.empty(E, F_), torch.empty(F_ + E)
    with pytest.raises(ValueError, match="unknown activation"):
        ops.ffn_fwd(x, w1, w2, bias, "relu")
    with pytest.raises(ValueError, match="unknown activation"):
        ops.ffn_act_fwd(x, "tanh")
    with pytest.raises(ValueError, match="w1 must be"):
        ops.ffn_fwd(x, w1[:, :8], w2, bias)
    with pytest.raises(ValueError, match="w2 must be"):
        ops.ffn_fwd(x, w1, w2[:, :8], bias)
    with pytest.raises(ValueError, match="bias must be"):
        ops.ffn_fwd(x, w1, w2, bias[:-1])
    with pytest.raises(TypeError):
        ops.ffn_fwd(x.double(), w1, w2, bias)
    with pytest.raises(TypeError):
        ops.ffn_fwd(x, w1.to(torch.bfloat16), w2, bias)
    with pytest.raises(ValueError, match="out must be"):
        ops.ffn_fwd(x, w1, w2, bias, out=torch.empty(P, E + 1))
    with pytest.raises(ValueError, match="err must be"):
        ops.ffn_bwd(err[:, :-1], x, w1, w2, save, dw1, dw2, db)
    with pytest.raises(ValueError, match="dw1 must be"):
        ops.ffn_bwd(err, x, w1, w2, save, dw2, dw2, db)
    with pytest.raises(ValueError, match="dbias must be"):
        ops.ffn_bwd(err, x, w1, w2, save, dw1, dw2, db[:-1])
    with pytest.raises(ValueError, match="save"):
        ops.ffn_bwd(err, x, w1, w2, {}, dw1, dw2, db)
    with pytest.raises(ValueError, match="accumulate"):
        ops.ffn_bwd(err, x, w1, w2, save, dw1, dw2, db, accumulate=False)
    with pytest.raises(ValueError, match="aux_act without aux"):
        ops.ffn_bwd(err, x, w1, w2, save, dw1, dw2, db, aux_act="tanh")
    with pytest.raises(ValueError, match="err_input must be"):
        ops.ffn_bwd(err, x, w1, w2, save, dw1, dw2, db,
                    err_input=torch.empty(P, I + 1))
    u = save["u"]
    with pytest.raises(ValueError):
        ops.ffn_act_bwd(u[:, :-1], u)                    # mismatched shapes
    with pytest.raises(ValueError, match="out_t must be"):
        ops.ffn_act_bwd(u, u, out_t=torch.empty(P, F_))
    with pytest.raises(ValueError, match="db1"):
        ops.ffn_act_bwd(u, u, db1=torch.empty(F_ + 1))
    with pytest.raises(ValueError):
        ops.ffn_act_fwd(u.t())                           # rows not contiguous
    # 2^31 elements or more: rejected from the shape alone, before any work
    big = torch.empty(1 << 16, 1 << 15, device="meta")
    with pytest.raises(ValueError):
        ops.ffn_act_fwd(big)
