"""Batch normalisation: a float64 NumPy oracle, pinned to float64 torch, and
the CPU path of ``ops.batchnorm_fwd`` / ``batchnorm_bwd`` against it.

Every bound below is first-order float32 error analysis (unit roundoff U =
2^-24, gamma(k) = kU / (1 - kU) for a sum whose longest chain has k
additions) of the rule the code under test follows, evaluated on the float64
values of the case; 1 % is added for the second-order terms.  Two rules:

* ``two_pass`` (CPU): mean = sum x / P, var = sum (x - mean)^2 / P;
* ``shifted`` (GPU): sums of d = x - K and d^2 with K = the mean of the
  first min(P, 8) rows (any K gives the exact result in exact arithmetic; the
  float32 K the kernels share differs from this one by parts in 10^7 of the
  sums below), mean = K + S1 / P, var = (S2 - S1^2 / P) / P.

Transcendental activations: the library functions are taken as accurate to
ACT_ULPS units in the last place (float32 expf / tanhf / log1pf)."""
import os
import re

import numpy as np
import pytest
import torch

from veles_amd import ops
from veles_amd.ops import _lib
from test_step_tail_ref import U, Ratios, bf_half_ulp, f64, gamma

EPS, MOM = 1e-5, 0.1
ACT_ULPS = 16
SECOND_ORDER = 1.01
SHIFT_ROWS = 8        # BN_SHIFT_ROWS of csrc/kernels/batchnorm.hip
# Lipschitz constants of the five activations and the largest |f'| of each
LIP = {0: 1.0, 1: 1.7159 * 0.6666, 2: 1.0, 3: 1.0, 4: 0.25}


def act_f(z, act):
    if act == 1:
        return 1.7159 * np.tanh(0.6666 * z)
    if act == 2:
        return np.where(z > 15, z, np.log1p(np.exp(np.minimum(z, 15))))
    if act == 3:
        return np.maximum(z, 0)
    if act == 4:
        return 1 / (1 + np.exp(-z))
    return z


def act_df(y, act):
    """f' through the output y, as the project defines it"""
    if act == 1:
        return 0.6666 * 1.7159 - (0.6666 / 1.7159) * y * y
    if act == 2:
        return 1 - np.exp(-y)
    if act == 3:
        return (y > 0).astype(np.float64)
    if act == 4:
        return y * (1 - y)
    return np.ones_like(y)


def bn_ref(x, g, b, rm, rv, act=0, training=True, eps=EPS, mom=MOM):
    """x float64 [P][C] -> dict of float64 results"""
    P = x.shape[0]
    r = {"P": P}
    if training:
        mu = x.mean(0)
        var = ((x - mu) ** 2).mean(0)
        r["rm"] = (1 - mom) * rm + mom * mu
        r["rv"] = (1 - mom) * rv + mom * var * P / (P - 1)
    else:
        mu, var = rm, rv
        r["rm"], r["rv"] = rm, rv
    r["mu"], r["var"] = mu, var
    r["invstd"] = 1 / np.sqrt(var + eps)
    r["xh"] = (x - mu) * r["invstd"]
    r["sc"] = g * r["invstd"]
    r["sh"] = b - mu * r["sc"]
    r["z"] = g * r["xh"] + b
    r["y"] = act_f(r["z"], act)
    return r


def bn_bwd_ref(err, y, f, g, act=0, aux=None, aux_act=0):
    """err, y (the layer's output as the backward reads it), aux float64"""
    P = f["P"]
    gr = err * act_df(y, act) if act else err
    db = gr.sum(0)
    dg = (gr * f["xh"]).sum(0)
    dx0 = g * f["invstd"] * (gr - db / P - f["xh"] * dg / P)
    fa = act_df(aux, aux_act) if aux_act else np.ones_like(dx0)
    return {"g": gr, "db": db, "dg": dg, "dx0": dx0, "fa": fa,
            "dx": dx0 * fa}


def cpu_depth(P):
    """longest float32 chain of ops._bn_chain_sum"""
    return ops.BN_CPU_CHAIN + P // ops.BN_CPU_CHAIN + 1


def fwd_bounds(x, g, b, rm, rv, f, act, rule, D, training=True, eps=EPS,
               mom=MOM):
    """Bounds on |computed - oracle| of a forward pass that follows ``rule``
    with sums of depth ``D``"""
    P = x.shape[0]
    e = {}
    if not training:
        e["mu"] = e["var"] = np.zeros_like(f["mu"])
    elif rule == "two_pass":
        e["mu"] = gamma(D + 1) * np.abs(x).sum(0) / P
        e["var"] = gamma(D + 4) * (f["var"] + e["mu"] ** 2) + e["mu"] ** 2
    else:
        d = x - x[:SHIFT_ROWS].mean(0)
        A1, S1, S2 = np.abs(d).sum(0), d.sum(0), (d * d).sum(0)
        t = S1 * S1 / P
        e["mu"] = gamma(D + 3) * A1 / P + U * np.abs(f["mu"])
        e["var"] = (gamma(D + 3) * S2 + gamma(D + 4) * 2 * np.abs(S1) * A1 / P
                    + gamma(5) * (S2 + t)) / P
    ve = f["var"] + eps
    e["invstd"] = f["invstd"] * ((e["var"] + U * eps) / (2 * ve) + 3 * U)
    e["rm"] = mom * e["mu"] + 5 * U * (np.abs((1 - mom) * rm) +
                                       np.abs(mom * f["mu"]))
    e["rv"] = mom * e["var"] * P / (P - 1.0) + 6 * U * (
        np.abs((1 - mom) * rv) + mom * f["var"] * P / (P - 1.0)) \
        if training else np.zeros_like(rv)
    e["sc"] = np.abs(g) * e["invstd"] + U * np.abs(f["sc"])
    xc = np.abs(x - f["mu"])
    e["z"] = xc * e["sc"] + np.abs(f["sc"]) * e["mu"] + U * (
        np.abs(f["sh"]) + 2 * np.abs(f["z"]) + np.abs(f["sc"]) * xc)
    e["y"] = LIP[act] * e["z"] + (ACT_ULPS * U * np.abs(f["y"])
                                  if act in (1, 2, 4) else 0)
    e["xh"] = xc * e["invstd"] + f["invstd"] * e["mu"] + 2 * U * np.abs(
        f["xh"])
    return {k: v * SECOND_ORDER for k, v in e.items()}


def bwd_bounds(err, f, fe, r, g, act, aux_act, D):
    """fe: fwd_bounds of the pass that saved mean / invstd; r: bn_bwd_ref"""
    P = f["P"]
    e_g = 8 * U * np.abs(err) if act in (1, 2, 4) else np.zeros_like(err)
    ag, axh = np.abs(r["g"]), np.abs(f["xh"])
    e = {}
    e["db"] = gamma(D) * ag.sum(0) + e_g.sum(0)
    e["dg"] = gamma(D + 2) * (ag * axh).sum(0) + (
        ag * fe["xh"] + e_g * axh).sum(0)
    A = np.abs(g * f["invstd"])
    inner = r["g"] - r["db"] / P - f["xh"] * r["dg"] / P
    e0 = np.abs(g) * fe["invstd"] * np.abs(inner) + A * (
        e_g + e["db"] / P + fe["xh"] * np.abs(r["dg"]) / P +
        axh * e["dg"] / P) + 8 * U * A * (
        ag + np.abs(r["db"]) / P + axh * np.abs(r["dg"]) / P)
    e["dx"] = e0 * np.abs(r["fa"]) + (8 * U * LIP[1] * np.abs(r["dx0"])
                                      if aux_act else 0)
    return {k: v * SECOND_ORDER for k, v in e.items()}


def large_mean_case(P, C=16, seed=0):
    """mean 64, std 0.5, rounded to bfloat16 (float32 tensor)"""
    gen = torch.Generator().manual_seed(seed)
    return (64 + 0.5 * torch.randn(P, C, generator=gen)).bfloat16().float()


def make_case(shape, seed, mean=0.3, std=1.2, dtype=torch.float32):
    gen = torch.Generator().manual_seed(seed)
    C = shape[-1]
    x = (mean + std * torch.randn(shape, generator=gen)).to(dtype)
    err = (0.1 * torch.randn(shape, generator=gen)).to(dtype)
    aux = torch.randn(shape, generator=gen).to(dtype)
    g = 0.5 + torch.rand(C, generator=gen)
    b = 0.3 * torch.randn(C, generator=gen)
    rm = 0.2 * torch.randn(C, generator=gen)
    rv = 0.5 + torch.rand(C, generator=gen)
    return x, err, aux, g, b, rm, rv


def rows(t):
    return f64(t).reshape(-1, t.shape[-1])


# ------------------------------------------------------------------ oracle
@pytest.mark.parametrize("shape", [(6, 5), (2, 3, 4, 7), (3, 4, 6)])
def test_oracle_matches_float64_torch(shape):
    x, err, _, g, b, rm, rv = make_case(shape, 1, dtype=torch.float64)
    C = shape[-1]
    xt = x.reshape(-1, C).clone().requires_grad_(True)
    gt, bt = (t.double().clone().requires_grad_(True) for t in (g, b))
    rmt, rvt = rm.double().clone(), rv.double().clone()
    y = torch.nn.functional.batch_norm(xt, rmt, rvt, gt, bt, True, MOM, EPS)
    y.backward(err.reshape(-1, C))
    f = bn_ref(rows(x), f64(g), f64(b), f64(rm), f64(rv))
    r = bn_bwd_ref(rows(err), None, f, f64(g))
    for name, got, want in (("y", f["y"], y), ("mu", f["mu"], xt.mean(0)),
                            ("rm", f["rm"], rmt), ("rv", f["rv"], rvt),
                            ("dx", r["dx"], xt.grad), ("dg", r["dg"], gt.grad),
                            ("db", r["db"], bt.grad)):
        d = np.abs(got - f64(want)).max()
        assert d <= 1e-12 * max(1.0, np.abs(f64(want)).max()), (name, d)
    # evaluation mode
    ye = torch.nn.functional.batch_norm(xt, rmt, rvt, gt, bt, False, MOM, EPS)
    fe = bn_ref(rows(x), f64(g), f64(b), f64(rmt), f64(rvt), training=False)
    assert np.abs(fe["y"] - f64(ye)).max() <= 1e-12


# ---------------------------------------------------------------- CPU path
def run_cpu(x, err, aux, g, b, rm, rv, act, aux_act, training=True,
            accumulate="overwrite", grads=None):
    rm, rv = rm.clone(), rv.clone()
    save = {}
    y = ops.batchnorm_fwd(x, g, b, rm, rv, training=training, act=act,
                          save=save)
    out = {"y": y, "rm": rm, "rv": rv, "save": save}
    if training:
        C = x.shape[-1]
        dg, db = grads if grads is not None else (torch.zeros(C),
                                                  torch.zeros(C))
        out["dx"] = ops.batchnorm_bwd(err, x, y, g, save, dg, db, act=act,
                                      accumulate=accumulate, aux=aux,
                                      aux_act=aux_act)
        out["dg"], out["db"] = dg, db
    return out


def check_case(ratios, tag, got, x, err, aux, g, b, rm, rv, act, aux_act,
               rule, D, out_bf16, training=True, dg0=None, db0=None):
    """``got`` (tensors of the code under test) against the oracle"""
    X = rows(x)
    f = bn_ref(X, f64(g), f64(b), f64(rm), f64(rv), act, training)
    fe = fwd_bounds(X, f64(g), f64(b), f64(rm), f64(rv), f, act, rule, D,
                    training)

    def half(v, e):
        return bf_half_ulp(np.abs(v) + e) if out_bf16 else 0.0
    ratios.see(tag + "y", np.abs(rows(got["y"]) - f["y"]),
               fe["y"] + half(f["y"], fe["y"]))
    for k, name in (("rm", "rm"), ("rv", "rv")):
        ratios.see(tag + name, np.abs(f64(got[k]) - f[k]), fe[k])
    if not training:
        return f, None
    ratios.see(tag + "mu", np.abs(f64(got["save"]["mean"]) - f["mu"]),
               fe["mu"])
    ratios.see(tag + "invstd",
               np.abs(f64(got["save"]["invstd"]) - f["invstd"]), fe["invstd"])
    E = rows(err)
    r = bn_bwd_ref(E, rows(got["y"]), f, f64(g), act,
                   None if aux is None else rows(aux), aux_act)
    be = bwd_bounds(E, f, fe, r, f64(g), act, aux_act, D)
    for k, base in (("dg", dg0), ("db", db0)):
        want = r[k] + (0 if base is None else f64(base))
        extra = 0 if base is None else U * np.abs(want)
        ratios.see(tag + k, np.abs(f64(got[k]) - want), be[k] + extra)
    if got.get("dx") is not None:
        ratios.see(tag + "dx", np.abs(rows(got["dx"]) - r["dx"]),
                   be["dx"] + half(r["dx"], be["dx"]))
    return f, fe


@pytest.mark.parametrize("shape,act,aux_act", [
    ((65, 8), 0, 0), ((7, 3), 1, 3), ((2, 5), 2, 1), ((2, 5, 7, 16), 3, 4),
    ((4, 9, 24), 4, 2), ((300, 20), 3, 3), ((100, 40), 1, 0)])
def test_cpu_path_against_the_oracle(shape, act, aux_act):
    case = make_case(shape, 7)
    x, err, aux = case[:3]
    P = x.numel() // shape[-1]
    ratios = Ratios()
    got = run_cpu(*case, act, aux_act)
    check_case(ratios, "", got, *case, act, aux_act, "two_pass", cpu_depth(P),
               False)
    print(shape, act, aux_act, dict(ratios))


def test_cpu_eval_mode_uses_and_keeps_the_running_statistics():
    case = make_case((33, 12), 5)
    for act in range(5):
        got = run_cpu(*case, act, 0, training=False)
        ratios = Ratios()
        check_case(ratios, "", got, *case, act, 0, "two_pass", 1, False,
                   training=False)
        assert torch.equal(got["rm"], case[5])
        assert torch.equal(got["rv"], case[6])


def test_cpu_accumulate_adds_and_overwrite_replaces():
    case = make_case((50, 6), 9)
    base = torch.full((6,), 3.0), torch.full((6,), -2.0)
    ratios = Ratios()
    got = run_cpu(*case, 1, 0, accumulate=True,
                  grads=tuple(t.clone() for t in base))
    check_case(ratios, "", got, *case, 1, 0, "two_pass", cpu_depth(50), False,
               dg0=base[0], db0=base[1])
    got = run_cpu(*case, 1, 0, grads=tuple(t.clone() for t in base))
    check_case(ratios, "", got, *case, 1, 0, "two_pass", cpu_depth(50), False)


@pytest.mark.parametrize("P", [2000, 8192])
def test_large_mean_inputs_tell_the_rules_apart(P):
    """mean 64, std 0.5: the CPU path stays inside the bounds; E[x^2] -
    mean^2 in float32, the unbiased variance under the root, and the biased
    one in running_var each leave theirs."""
    x = large_mean_case(P)
    C = x.shape[1]
    g, b = torch.ones(C), torch.zeros(C)
    rm, rv = torch.zeros(C), torch.ones(C)
    err = torch.randn(P, C, generator=torch.Generator().manual_seed(1))
    ratios = Ratios()
    got = run_cpu(x, err, None, g, b, rm, rv, 0, 0)
    f, fe = check_case(ratios, "", got, x, err, None, g, b, rm, rv, 0, 0,
                       "two_pass", cpu_depth(P), False)
    print(P, dict(ratios))
    x32 = x.numpy()
    naive = (x32 * x32).mean(0, dtype=np.float32) - \
        x32.mean(0, dtype=np.float32) ** 2
    rel = np.abs(naive.astype(np.float64) - f["var"]) / f["var"]
    print("naive float32 variance: relative error up to %.2e, bound %.2e" %
          (rel.max(), (fe["var"] / f["var"]).max()))
    assert (np.abs(naive - f["var"]) > fe["var"]).any()
    unbiased = f["var"] * P / (P - 1)
    assert (np.abs(1 / np.sqrt(unbiased + EPS) - f["invstd"]) >
            fe["invstd"]).all()
    biased_rv = (1 - MOM) * f64(rv) + MOM * f["var"]
    assert (np.abs(biased_rv - f["rv"]) > fe["rv"]).all()
    # and the shifted rule's bounds tell the same three apart
    fs = fwd_bounds(rows(x), f64(g), f64(b), f64(rm), f64(rv), f, 0,
                    "shifted", 256)
    assert (np.abs(naive - f["var"]) > fs["var"]).any()
    assert (np.abs(1 / np.sqrt(unbiased + EPS) - f["invstd"]) >
            fs["invstd"]).any()
    assert (np.abs(biased_rv - f["rv"]) > fs["rv"]).any()


def test_one_row_raises_in_training_only():
    x = torch.randn(1, 4)
    v = [torch.ones(4), torch.zeros(4), torch.zeros(4), torch.ones(4)]
    with pytest.raises(ValueError):
        ops.batchnorm_fwd(x, *v)
    y = ops.batchnorm_fwd(x, *v, training=False)
    assert y.shape == x.shape


def test_host_checks():
    x = torch.randn(6, 4)
    g, b, rm, rv = torch.ones(4), torch.zeros(4), torch.zeros(4), torch.ones(4)
    with pytest.raises(TypeError):
        ops.batchnorm_fwd(x.double(), g, b, rm, rv)
    with pytest.raises(TypeError):
        ops.batchnorm_fwd(x.numpy(), g, b, rm, rv)
    with pytest.raises(TypeError):
        ops.batchnorm_fwd(x, g.double(), b, rm, rv)
    with pytest.raises(ValueError):
        ops.batchnorm_fwd(x, torch.ones(5), b, rm, rv)
    with pytest.raises(ValueError):
        ops.batchnorm_fwd(x, g, b, rm, torch.ones(8)[::2])
    with pytest.raises(ValueError):
        ops.batchnorm_fwd(torch.randn(4, 6).t(), g, b, rm, rv)
    with pytest.raises(ValueError):
        ops.batchnorm_fwd(x, g, b, rm, rv, out=torch.empty(6, 5))
    with pytest.raises(ValueError):
        ops.batchnorm_fwd(x, g, b, rm, rv, act=7)
    save = {}
    y = ops.batchnorm_fwd(x, g, b, rm, rv, save=save)
    dg, db = torch.zeros(4), torch.zeros(4)
    with pytest.raises(ValueError):
        ops.batchnorm_bwd(x[:5], x, y, g, save, dg, db)
    with pytest.raises(ValueError):
        ops.batchnorm_bwd(x, x, y, g, {}, dg, db)
    with pytest.raises(ValueError):
        ops.batchnorm_bwd(x, x, None, g, save, dg, db, act=1)
    with pytest.raises(ValueError):
        ops.batchnorm_bwd(x, x, y, g, save, dg, db, accumulate=False)
    with pytest.raises(ValueError):
        ops.batchnorm_bwd(x, x, y, g, save, dg, db, aux_act=1)
    with pytest.raises(TypeError):
        ops.batchnorm_bwd(x, x, y, g, save, dg.double(), db)
    # a 2-D view with a row pitch is taken as it is
    wide = torch.randn(6, 10)
    y2 = ops.batchnorm_fwd(wide[:, :4], g, b, rm.clone(), rv.clone())
    y3 = ops.batchnorm_fwd(wide[:, :4].contiguous(), g, b, rm.clone(),
                           rv.clone())
    assert torch.equal(y2, y3)


def test_buffers_live_in_the_callers_dicts():
    case = make_case((20, 8), 2)
    x, err, aux, g, b, rm, rv = case
    save, ws = {}, {}
    out = torch.empty_like(x)
    ops.batchnorm_fwd(x, g, b, rm, rv, save=save, out=out, ws=ws)
    kept = {k: v.data_ptr() for k, v in save.items()}
    assert set(kept) == {"mean", "invstd", "table"}
    ops.batchnorm_fwd(x, g, b, rm, rv, save=save, out=out, ws=ws)
    assert kept == {k: v.data_ptr() for k, v in save.items()}
    assert tuple(save["table"].shape) == (2, 8)


def test_abi_of_the_batchnorm_entry_points():
    """tests/test_abi.py's comparison, for the bindings of batchnorm.hip"""
    import test_abi
    decls = test_abi._decls()
    names = [n for n in decls if n.startswith("hvk_bn_")]
    assert len(names) == 6
    table = dict(_lib._SIGS)
    table.update(_lib._OPTIONAL)
    for name in names:
        ret, args = decls[name]
        assert ret == "int"
        assert table[name] == [test_abi._kind(a) for a in args], name
    with open(os.path.join(test_abi.ROOT, "csrc", "kernels",
                           "hvk_api.h")) as h:
        src = h.read()
    for name in names:
        assert re.search(r"\b%s\(" % name, src), name


def test_partials_are_a_function_of_the_shape():
    """the grid formula of csrc/kernels/batchnorm.hip (bn_geom)"""
    for P, C, vec in ((2, 8, 1), (65, 256, 1), (2049, 256, 1), (100, 4096, 1),
                      (65537, 8, 1), (63, 3, 0), (10 ** 6, 50, 0),
                      (2 * 10 ** 6, 256, 1)):
        assert ops.bn_partials(P, C, vec) == geom(P, C, vec)["G"], (P, C)


def geom(P, C, vec):
    """bn_geom of csrc/kernels/batchnorm.hip: channel groups CG of NV
    channels, NTX tiles of TX <= 64 groups, RY = 256 // TX row lanes, and G
    row slices: one per 4 * RY rows, at most 1024 // NTX.  ``depth``: the
    longest chain of a reduction: a lane's rows, the RY row lanes in LDS,
    a finishing lane's slices (64 lanes share a channel), the wave tree."""
    CG = C // 8 if vec else C
    NTX = -(-CG // 64)
    TX = -(-CG // NTX)
    RY = 256 // TX
    G = max(1, min(-(-P // (RY * 4)), max(1, 1024 // NTX)))
    depth = -(-P // (G * RY)) + RY + -(-G // 64) + 6
    return {"CG": CG, "NTX": NTX, "TX": TX, "RY": RY, "G": G, "depth": depth}
