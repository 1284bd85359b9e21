"""Layer normalisation with a fused residual add: a float64 NumPy oracle,
pinned to float64 ``torch.nn.LayerNorm``, and the CPU path of
``ops.layernorm_fwd`` / ``layernorm_bwd`` / ``ops.add`` against it.

Every bound below is first-order float32 error analysis (unit roundoff U =
2^-24, gamma(k) = kU / (1 - kU) for a sum whose longest chain has k
additions) of the rule the code under test follows, evaluated on the float64
values of the case (the oracle's companion pass over absolute values); 1 % is
added for the second-order terms.  The rule:

    s = fl(x + r) (one rounding; exact without a residual)
    mean = fl(sum s) / C                       row sums of depth ``Drow``
    d = fl(s - mean), var = fl(sum d^2) / C    (two passes: no cancellation)
    invstd = 1 / sqrt(var + eps)               3 U, as test_batchnorm_ref
    sh = d invstd, y = sh gamma + beta
    dbeta = sum_P err, dgamma = sum_P err sh   column sums of depth ``Dcol``
    gh = err gamma, c1 = sum gh / C, c2 = sum gh sh / C
    dx = invstd (gh - c1 - sh c2)

A float32 division is taken as accurate to 2.5 ulp.  The error of the mean
is the same for every column of a row, so it drops out of sum d^2 to first
order (sum d = 0) and enters the variance only through its square.

Depths.  CPU (``ops._ln_row_sum``): LN_CPU_CHAIN = 16 neighbours per level,
ceil(log16 C) levels; columns: ``ops._bn_chain_sum``.  GPU: ``path`` /
``slices`` below mirror ln_path / ln_slices of csrc/kernels/layernorm.hip.
"""
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from veles_amd import ops
from veles_amd.error import KernelLibraryMissing
from veles_amd.ops import _lib
from test_step_tail_ref import U, Ratios, bf_half_ulp, f64, gamma

EPS = 1e-5
SECOND_ORDER = 1.01
DIV = 3           # a division: 2.5 ulp, rounded up


# ------------------------------------------------------------------ oracle
def ln_ref(x, r, g, b, eps=EPS):
    """x, r (or None) float64 [P][C] -> dict of float64 results"""
    s = x if r is None else x + r
    mu = s.mean(1, keepdims=True)
    d = s - mu
    var = (d * d).mean(1, keepdims=True)
    invstd = 1 / np.sqrt(var + eps)
    sh = d * invstd
    return {"s": s, "mu": mu[:, 0], "var": var[:, 0], "invstd": invstd[:, 0],
            "d": d, "sh": sh, "y": g * sh + b, "res": r is not None}


def ln_bwd_ref(err, f, g):
    gh = err * g
    c1 = gh.mean(1, keepdims=True)
    c2 = (gh * f["sh"]).mean(1, keepdims=True)
    inner = gh - c1 - f["sh"] * c2
    return {"db": err.sum(0), "dg": (err * f["sh"]).sum(0), "gh": gh,
            "c1": c1, "c2": c2, "inner": inner,
            "dx": f["invstd"][:, None] * inner}


def fwd_bounds(f, g, b, Drow, eps=EPS):
    """Bounds on |computed - oracle| of a forward pass whose row sums have
    depth ``Drow``"""
    e = {}
    a_s, a_d = np.abs(f["s"]), np.abs(f["d"])
    e_s = U * a_s if f["res"] else np.zeros_like(a_s)
    e["mu"] = gamma(Drow + DIV) * a_s.mean(1) + e_s.mean(1)
    ed = e_s + e["mu"][:, None]               # |computed d - d|, sans U |d|
    e["var"] = gamma(Drow + DIV + 3) * ((a_d + ed) ** 2).mean(1) + \
        (2 * a_d * e_s).mean(1) + 2 * U * f["var"] + (ed * ed).mean(1)
    ve = f["var"] + eps
    e["invstd"] = f["invstd"] * ((e["var"] + U * eps) / (2 * ve) + 3 * U)
    e["sh"] = ed * f["invstd"][:, None] + a_d * e["invstd"][:, None] + \
        2 * U * np.abs(f["sh"])
    e["y"] = np.abs(g) * e["sh"] + U * (np.abs(g * f["sh"]) + np.abs(f["y"]))
    return {k: v * SECOND_ORDER for k, v in e.items()}


def bwd_bounds(err, f, fe, r, g, Drow, Dcol):
    """fe: fwd_bounds of the pass that saved mean / invstd; r: ln_bwd_ref"""
    a_e, a_sh, a_gh = np.abs(err), np.abs(f["sh"]), np.abs(r["gh"])
    e = {}
    e["db"] = gamma(Dcol) * a_e.sum(0)
    e["dg"] = gamma(Dcol + 2) * (a_e * a_sh).sum(0) + (a_e * fe["sh"]).sum(0)
    e_c1 = gamma(Drow + DIV + 1) * a_gh.mean(1, keepdims=True)
    e_c2 = gamma(Drow + DIV + 2) * (a_gh * a_sh).mean(1, keepdims=True) + \
        (a_gh * fe["sh"]).mean(1, keepdims=True)
    parts = a_gh + np.abs(r["c1"]) + a_sh * np.abs(r["c2"])
    e_inner = e_c1 + fe["sh"] * np.abs(r["c2"]) + a_sh * e_c2 + 8 * U * parts
    e["dx"] = fe["invstd"][:, None] * np.abs(r["inner"]) + \
        f["invstd"][:, None] * e_inner + 2 * U * np.abs(r["dx"])
    return {k: v * SECOND_ORDER for k, v in e.items()}


def cpu_row_depth(C):
    levels = 1
    while ops.LN_CPU_CHAIN ** levels < C:
        levels += 1
    return ops.LN_CPU_CHAIN * levels


def cpu_col_depth(P):
    return ops.BN_CPU_CHAIN + P // ops.BN_CPU_CHAIN + 1


# --------------------------- the grids of csrc/kernels/layernorm.hip (GPU)
LN_REG_C = 8192


def path(C, vec):
    """ln_path: L lanes own a row and keep K groups of NV columns each
    (K = 0: a column loop per lane, over a row staged in LDS on the element
    path up to 8192 columns, re-reading past that); RPB rows per workgroup
    pass.  ``kind``: wave / workgroup / reread.  ``Drow``: a lane's K NV values (re-reading:
    ceil(CG / 256) NV), the exchange levels, the four waves of a
    workgroup."""
    NV = 8 if vec else 1
    CG = C // NV
    if C > LN_REG_C:
        L, K = 256, 0
    elif vec:
        L, K = next(lk for cap, lk in (
            (16, (16, 1)), (32, (32, 1)), (64, (64, 1)), (128, (64, 2)),
            (256, (64, 4)), (512, (256, 2)), (1024, (256, 4))) if CG <= cap)
    else:
        L, K = next(lk for cap, lk in (
            (16, (16, 1)), (64, (64, 1)), (256, (64, 4)), (1024, (256, 4)),
            (8192, (256, 0))) if CG <= cap)
    serial = (K if K else -(-CG // 256)) * NV
    Drow = serial + int(math.log2(min(L, 64))) + (3 if L == 256 else 0)
    return {"L": L, "K": K, "CG": CG, "RPB": 256 // L, "Drow": Drow,
            "kind": "reread" if C > LN_REG_C else
            "workgroup" if L == 256 else "wave"}


def slices(P, C, vec):
    """ln_slices (one per 4 RPB rows, at most 1024) and the depth of a
    column sum: a row group's rows, the RPB groups, a finishing lane's
    slices (16 lanes share a column), the 16 lanes"""
    p = path(C, vec)
    G = max(1, min(-(-P // (p["RPB"] * 4)), 1024))
    Dcol = -(-P // (G * p["RPB"])) + p["RPB"] + -(-G // 16) + 16
    return G, Dcol


# ------------------------------------------------------------------- cases
def make_case(shape, seed, residual=True, mean=0.3, std=1.2,
              dtype=torch.float32):
    gen = torch.Generator().manual_seed(seed)
    C = shape[-1]
    x = (mean + std * torch.randn(shape, generator=gen)).to(dtype)
    r = (0.5 * torch.randn(shape, generator=gen) - 0.2).to(dtype) \
        if residual else None
    err = (0.1 * torch.randn(shape, generator=gen)).to(dtype)
    g = 0.5 + torch.rand(C, generator=gen)
    b = 0.3 * torch.randn(C, generator=gen)
    return x, r, err, g, b


def large_mean_case(P, C, seed=0, residual=False, std=0.5):
    """rows of mean 64, std 0.5, bfloat16 values (float32 tensors); with a
    residual: two halves of mean 32"""
    gen = torch.Generator().manual_seed(seed)
    m = 32.0 if residual else 64.0
    s = std * (0.5 ** 0.5 if residual else 1.0)
    x = (m + s * torch.randn(P, C, generator=gen)).bfloat16().float()
    r = (m + s * torch.randn(P, C, generator=gen)).bfloat16().float() \
        if residual else None
    err = torch.randn(P, C, generator=gen).bfloat16().float()
    g = 0.5 + torch.rand(C, generator=gen)
    b = 0.3 * torch.randn(C, generator=gen)
    return x, r, err, g, b


def rows(t):
    return f64(t).reshape(-1, t.shape[-1])


def run(case, accumulate="overwrite", grads=None, need_dx=True, save=None,
        ws=None):
    """forward + backward through ops.* on the case's own device"""
    x, r, err, g, b = case
    save = {} if save is None else save
    y = ops.layernorm_fwd(x, g, b, residual=r, save=save)
    C = x.shape[-1]
    dg, db = grads if grads is not None else (
        torch.full((C,), 9.0, device=x.device),
        torch.full((C,), -9.0, device=x.device))
    dx = ops.layernorm_bwd(err, x, g, save, dg, db, residual=r,
                           accumulate=accumulate, ws=ws, need_dx=need_dx)
    return {"y": y, "save": save, "dx": dx, "dg": dg, "db": db}


def check_case(ratios, tag, got, case, Drow, Dcol, out_bf16, dg0=None,
               db0=None):
    """``got`` (tensors of the code under test) against the oracle of
    ``case`` (CPU tensors holding the values the code was given)"""
    x, r, err, g, b = case
    G, B = f64(g), f64(b)
    f = ln_ref(rows(x), None if r is None else rows(r), G, B)
    fe = fwd_bounds(f, G, B, Drow)

    def half(v, e):
        return bf_half_ulp(np.abs(v) + e) if out_bf16 else 0.0
    ratios.see(tag + "mu", np.abs(f64(got["save"]["mean"]) - f["mu"]),
               fe["mu"])
    ratios.see(tag + "invstd",
               np.abs(f64(got["save"]["invstd"]) - f["invstd"]), fe["invstd"])
    ratios.see(tag + "y", np.abs(rows(got["y"]) - f["y"]),
               fe["y"] + half(f["y"], fe["y"]))
    E = rows(err)
    rb = ln_bwd_ref(E, f, G)
    be = bwd_bounds(E, f, fe, rb, G, Drow, Dcol)
    for k, base in (("dg", dg0), ("db", db0)):
        want = rb[k] + (0 if base is None else f64(base))
        extra = 0 if base is None else U * np.abs(want)
        ratios.see(tag + k, np.abs(f64(got[k]) - want), be[k] + extra)
    if got.get("dx") is not None:
        ratios.see(tag + "dx", np.abs(rows(got["dx"]) - rb["dx"]),
                   be["dx"] + half(rb["dx"], be["dx"]))
    return f, fe, rb, be


def check_cpu(case, **kw):
    x = case[0]
    C = x.shape[-1]
    P = x.numel() // C
    ratios = Ratios()
    got = run(case, **{k: v for k, v in kw.items() if k in (
        "accumulate", "grads")})
    res = check_case(ratios, "", got, case, cpu_row_depth(C),
                     cpu_col_depth(P), False,
                     **{k: v for k, v in kw.items() if k in ("dg0", "db0")})
    print(tuple(x.shape), "residual" if case[1] is not None else "plain",
          {k: round(v, 4) for k, v in ratios.items()})
    return (got,) + res


# ------------------------------------------------------------------ oracle
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("shape", [(6, 5), (2, 3, 4, 7), (3, 4, 6)])
def test_oracle_matches_float64_torch(shape, residual):
    x, r, err, g, b = make_case(shape, 1, residual, dtype=torch.float64)
    C = shape[-1]
    xt = x.clone().requires_grad_(True)
    rt = r.clone().requires_grad_(True) if residual else None
    ln = torch.nn.LayerNorm(C, eps=EPS, elementwise_affine=True).double()
    with torch.no_grad():
        ln.weight.copy_(g)
        ln.bias.copy_(b)
    y = ln(xt + rt if residual else xt)
    y.backward(err)
    f = ln_ref(rows(x), rows(r) if residual else None, f64(g), f64(b))
    rb = ln_bwd_ref(rows(err), f, f64(g))
    pairs = [("y", f["y"], rows(y)), ("dx", rb["dx"], rows(xt.grad)),
             ("dg", rb["dg"], f64(ln.weight.grad)),
             ("db", rb["db"], f64(ln.bias.grad))]
    if residual:    # the residual branch's gradient is the same tensor
        pairs.append(("dr", rb["dx"], rows(rt.grad)))
    for name, got, want in pairs:
        d = np.abs(got - want).max()
        assert d <= 1e-12 * max(1.0, np.abs(want).max()), (name, d)


# ---------------------------------------------------------------- CPU path
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("shape", [
    (6, 5), (2, 3, 4, 7), (3, 4, 6), (65, 8), (7, 3), (1, 50), (300, 20),
    (5, 17), (4, 9, 257), (2, 1000)])
def test_cpu_path_against_the_oracle(shape, residual):
    check_cpu(make_case(shape, 7, residual))


def test_one_column_gives_beta():
    """C = 1: s - mean = 0, y = beta, dx = 0"""
    for residual in (False, True):
        case = make_case((9, 1), 3, residual)
        got = check_cpu(case)[0]
        assert torch.equal(got["y"], case[4].expand(9, 1))
        assert torch.equal(got["dx"], torch.zeros(9, 1))
        assert (got["save"]["invstd"] == float(
            1 / np.sqrt(np.float32(EPS)))).all()


def test_cpu_accumulate_adds_and_overwrite_replaces():
    case = make_case((50, 6), 9)
    base = torch.full((6,), 3.0), torch.full((6,), -2.0)
    check_cpu(case, accumulate=True, grads=tuple(t.clone() for t in base),
              dg0=base[0], db0=base[1])
    check_cpu(case, grads=tuple(t.clone() for t in base))
    with pytest.raises(ValueError):
        run(case, accumulate=False)


# ----------------------------------------------- inputs that tell rules apart
def ratio(err, bound):
    return float((np.abs(err) / bound).max())


@pytest.mark.parametrize("C", [2000, 8192])
def test_large_mean_rows_tell_the_variance_rules_apart(C):
    """Rows of mean 64, std 0.5.  The CPU path stays inside the bounds; a
    float32 E[s^2] - mean^2 (with the same chained sums) and the unbiased
    variance each leave the bound on invstd by more than 10 x."""
    case = large_mean_case(16, C)
    got, f, fe, rb, be = check_cpu(case)
    x = case[0]
    m = ops._ln_row_sum(x) / C
    naive = ops._ln_row_sum(x * x) / C - m * m
    bad = 1 / np.sqrt(f64(naive) + EPS)
    print("naive: %.1f x the bound" % ratio(bad - f["invstd"], fe["invstd"]))
    assert ratio(bad - f["invstd"], fe["invstd"]) > 10
    unbiased = 1 / np.sqrt(f["var"] * C / (C - 1) + EPS)
    print("unbiased: %.1f x" % ratio(unbiased - f["invstd"], fe["invstd"]))
    assert (np.abs(unbiased - f["invstd"]) > 10 * fe["invstd"]).all()
    # the GPU paths' depths give bounds that tell the same two apart
    for vec in (True, False):
        fg = fwd_bounds(f, f64(case[3]), f64(case[4]), path(C, vec)["Drow"])
        assert ratio(bad - f["invstd"], fg["invstd"]) > 10
        assert (np.abs(unbiased - f["invstd"]) > 10 * fg["invstd"]).all()


@pytest.mark.parametrize("C", [2000, 8192])
def test_small_variance_rows_tell_where_eps_goes(C):
    """std 0.01: sqrt(var + eps) and sqrt(var) + eps differ by 4 %.  (At std
    0.5 the two agree to first order: d sqrt(v) / dv = 1 at v = 1 / 4.)"""
    case = large_mean_case(8, C, std=0.01)
    x = (case[0] - 64).contiguous()      # mean 0: the values stay distinct
    case = (x,) + case[1:]
    got, f, fe, rb, be = check_cpu(case)
    outside = 1 / (np.sqrt(f["var"]) + EPS)
    print("eps outside: %.0f x" % ratio(outside - f["invstd"], fe["invstd"]))
    assert (np.abs(outside - f["invstd"]) > 10 * fe["invstd"]).all()


@pytest.mark.parametrize("C", [2000, 8192])
def test_dx_needs_its_projection_on_the_normalised_row(C):
    case = large_mean_case(8, C)
    got, f, fe, rb, be = check_cpu(case)
    short = f["invstd"][:, None] * (rb["gh"] - rb["c1"])
    print("no sh mean(gh sh): %.0f x" % ratio(short - rb["dx"], be["dx"]))
    assert ratio(short - rb["dx"], be["dx"]) > 10
    assert (np.abs(short - rb["dx"]) > 10 * be["dx"]).mean() > 0.5


@pytest.mark.parametrize("C", [2000, 8192])
def test_a_residual_rounded_to_bf16_before_the_statistics_is_seen(C):
    """x and r of mean 32: bf16(x + r) is off by up to 1 / 4 at 64"""
    case = large_mean_case(8, C, residual=True)
    got, f, fe, rb, be = check_cpu(case)
    x, r, err, g, b = case
    s16 = (x + r).bfloat16().float()
    save = {}
    y = ops.layernorm_fwd(s16, g, b, save=save)
    for name, bad, want, bound in (
            ("mu", f64(save["mean"]), f["mu"], fe["mu"]),
            ("invstd", f64(save["invstd"]), f["invstd"], fe["invstd"]),
            ("y", rows(y), f["y"], fe["y"])):
        print("rounded s, %s: %.0f x" % (name, ratio(bad - want, bound)))
        assert ratio(bad - want, bound) > 10, name
    # ... also past the half bf16 ulp that a bf16 y is allowed on the GPU
    assert ratio(rows(y) - f["y"], fe["y"] + bf_half_ulp(
        np.abs(f["y"]) + fe["y"])) > 10


# -------------------------------------------------------------- ops.add
def test_add_on_the_cpu():
    a, b = torch.randn(5, 7), torch.randn(5, 7)
    assert torch.equal(ops.add(a, b), a + b)
    out = torch.zeros(5, 12)
    ops.add(a, b, out=out[:, 2:9])
    assert torch.equal(out[:, 2:9], a + b) and (out[:, :2] == 0).all()
    ops.add(a, b, out=a)                      # in place
    assert torch.equal(a, out[:, 2:9])
    with pytest.raises(ValueError):
        ops.add(a, b[:4])
    with pytest.raises(TypeError):
        ops.add(a, b.double())
    with pytest.raises(TypeError):
        ops.add(a.bfloat16(), b.bfloat16())   # bf16 is the GPU's


# ---------------------------------------------------------- host checks
def test_host_checks():
    x = torch.randn(6, 4)
    g, b = torch.ones(4), torch.zeros(4)
    with pytest.raises(TypeError):
        ops.layernorm_fwd(x.double(), g, b)
    with pytest.raises(TypeError):
        ops.layernorm_fwd(x.numpy(), g, b)
    with pytest.raises(TypeError):
        ops.layernorm_fwd(x, g.double(), b)
    with pytest.raises(ValueError):
        ops.layernorm_fwd(x, torch.ones(5), b)
    with pytest.raises(ValueError):
        ops.layernorm_fwd(x, g, torch.ones(8)[::2])
    with pytest.raises(ValueError):      # the last axis is not contiguous
        ops.layernorm_fwd(torch.randn(4, 6).t(), g, b)
    with pytest.raises(ValueError):
        ops.layernorm_fwd(x, g, b, out=torch.empty(6, 5))
    with pytest.raises(ValueError):      # residual mismatches
        ops.layernorm_fwd(x, g, b, residual=torch.randn(5, 4))
    with pytest.raises(TypeError):
        ops.layernorm_fwd(x, g, b, residual=x.double())
    with pytest.raises(ValueError):
        ops.layernorm_fwd(x, g, b, residual=torch.randn(4, 6).t())
    save = {}
    ops.layernorm_fwd(x, g, b, save=save)
    dg, db = torch.zeros(4), torch.zeros(4)
    with pytest.raises(ValueError):
        ops.layernorm_bwd(x[:5], x, g, save, dg, db)
    with pytest.raises(ValueError):
        ops.layernorm_bwd(x, x, g, {}, dg, db)
    with pytest.raises(ValueError):      # the save of another shape
        ops.layernorm_bwd(x[:5], x[:5], g, save, dg, db)
    with pytest.raises(ValueError):
        ops.layernorm_bwd(x, x, g, save, dg, db, accumulate=False)
    with pytest.raises(ValueError):
        ops.layernorm_bwd(x, x, g, save, dg, db, residual=x[:5])
    with pytest.raises(TypeError):
        ops.layernorm_bwd(x, x, g, save, dg.double(), db)
    assert ops.layernorm_bwd(x, x, g, save, dg, db, need_dx=False) is None
    # a 2-D view with a row pitch is taken as it is
    wide = torch.randn(6, 10)
    y2 = ops.layernorm_fwd(wide[:, :4], g, b, residual=wide[:, 5:9])
    y3 = ops.layernorm_fwd(wide[:, :4].contiguous(), g, b,
                           residual=wide[:, 5:9].contiguous())
    assert torch.equal(y2, y3)


def test_two_to_the_31_elements_are_rejected():
    """no memory behind it: a contiguous [2^28][8] tensor on the meta
    device"""
    g, b = torch.ones(8, device="meta"), torch.zeros(8, device="meta")
    big = torch.empty((2 ** 28, 8), device="meta")
    assert big.numel() == 2 ** 31 and big.is_contiguous()
    for fn in (lambda: ops.layernorm_fwd(big, g, b),
               lambda: ops.layernorm_fwd(big[:5], g, b, residual=big),
               lambda: ops.add(big, big)):
        with pytest.raises(ValueError, match=r"2\^31"):
            fn()
    for vec in (0, 1):
        assert _lib.lib().hvk_ln_partials(2 ** 28, 8, vec) == -1
        assert _lib.lib().hvk_ln_partials(2 ** 28 - 1, 8, vec) >= 1
    with pytest.raises(ValueError):
        ops.ln_partials(2 ** 28, 8, True)
    with pytest.raises(ValueError):
        ops.ln_partials(4, 12, True)      # no vector path at C % 8 != 0


def test_buffers_live_in_the_callers_dicts():
    case = make_case((20, 8), 2)
    x, r, err, g, b = case
    save = {}
    out = torch.empty_like(x)
    ops.layernorm_fwd(x, g, b, residual=r, save=save, out=out)
    kept = {k: v.data_ptr() for k, v in save.items()}
    assert set(kept) == {"mean", "invstd"}
    assert tuple(save["mean"].shape) == (20,)
    y = ops.layernorm_fwd(x, g, b, residual=r, save=save, out=out)
    assert y is out
    assert kept == {k: v.data_ptr() for k, v in save.items()}
    dx = torch.empty_like(x)
    dg, db = torch.zeros(8), torch.zeros(8)
    assert ops.layernorm_bwd(err, x, g, save, dg, db, residual=r,
                             out=dx) is dx


def test_a_stale_library_names_the_symbol_and_the_rebuild(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: types.SimpleNamespace())
    with pytest.raises(KernelLibraryMissing) as e:
        ops.ln_partials(4, 8, True)
    assert "hvk_ln_partials" in str(e.value)
    assert "python -m veles_amd.ops.build" in str(e.value)


LN_NAMES = ("hvk_ln_partials", "hvk_ln_vec", "hvk_ln_colsum", "hvk_ln_fwd",
            "hvk_ln_bwd", "hvk_add")


def test_abi_of_the_layernorm_entry_points():
    """tests/test_abi.py's comparison, for the bindings of layernorm.hip"""
    import test_abi
    decls = test_abi._decls()
    for name in LN_NAMES:
        assert name in decls and name in _lib._OPTIONAL, name
        ret, args = decls[name]
        assert ret == "int"
        assert _lib._OPTIONAL[name] == [test_abi._kind(a) for a in args], name
    with open(os.path.join(test_abi.ROOT, "csrc", "kernels",
                           "hvk_api.h")) as h:
        src = h.read()
    for name in LN_NAMES:
        assert re.search(r"\b%s\(" % name, src), name


def test_partials_are_a_function_of_the_shape():
    """the grid formula of csrc/kernels/layernorm.hip (ln_slices)"""
    for P, C, vec in ((1, 8, 1), (65, 256, 1), (2049, 256, 1), (100, 4096, 1),
                      (65537, 8, 1), (63, 3, 0), (10 ** 6, 50, 0),
                      (5, 8200, 1), (5000, 8193, 0), (2 * 10 ** 6, 256, 1)):
        assert ops.ln_partials(P, C, vec) == slices(P, C, vec)[0], (P, C)
    assert [path(C, True)["kind"] for C in (2048, 2056, 8192, 8200)] == [
        "wave", "workgroup", "workgroup", "reread"]
    assert [path(C, False)["kind"] for C in (256, 257, 8192, 8193)] == [
        "wave", "workgroup", "workgroup", "reread"]
