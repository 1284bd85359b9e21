"""Grouped-query heads (``kv_heads``; docs/OPS.md "Attention", "Grouped-query
heads") on the float32 CPU path; tests/test_attention_gqa_gpu.py runs the same
helpers on the hvk_gqa_* kernels.

Reference: test_attention_ref.oracle on K/V expanded per group (query head h
reads K/V head h // G, ``repeat_interleave``), dk and dv summed over the group
in float64.  Bounds: for o, lse and dq those of test_attention_ref.bounds on
the expanded case; for dk and dv see ``gqa_bounds``."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import veles_amd.ops as ops
from test_attention_ref import bounds, heads_of, make_case, oracle, unheads
from test_step_tail_ref import U, Ratios, bf_half_ulp, f64, gamma

NAMES = ("o", "lse", "dq", "dk", "dv")


def expand(t, KVH, G, rule=None):
    """[B][T][KVH*D] -> [B][T][KVH*G*D]: head h = K/V head h // G (``rule``
    "mod": the wrong h % KVH)"""
    B, T, EK = t.shape
    t = t.reshape(B, T, KVH, 1, EK // KVH)
    t = np.repeat(t, G, 3) if rule is None else \
        np.repeat(t.transpose(0, 1, 3, 2, 4), G, 2)
    return t.reshape(B, T, G * EK)


def group_sum(t, KVH, G):
    B, T, E = t.shape
    return t.reshape(B, T, KVH, G, E // (KVH * G)).sum(3).reshape(B, T, E // G)


def gqa_case(B, T, NH, KVH, D, seed=0):
    q, k, v, do = make_case(B, T, NH, D, seed=seed)
    return q, k[:, :, :KVH * D].contiguous(), v[:, :, :KVH * D].contiguous(), do


def gqa_oracle(case, NH, KVH, causal, rule=None):
    """(expanded float64 case, oracle's dict with dk, dv summed per group)"""
    q, k, v, do = (f64(t) if torch.is_tensor(t) else t for t in case)
    G = NH // KVH
    wide = (q, expand(k, KVH, G, rule), expand(v, KVH, G, rule), do)
    ref = oracle(*wide, NH, causal)
    ref["dk_heads"], ref["dv_heads"] = ref["dk"], ref["dv"]
    ref["dk"], ref["dv"] = (group_sum(ref[n], KVH, G) for n in ("dk", "dv"))
    return wide, ref


def gqa_bounds(wide, ref, NH, KVH, causal, gpu, tk=None):
    """o, lse, dq: ``bounds`` on the expanded case.  dk, dv of a K/V head are
    one float32 sum over the G T terms of its group, rounded once:
    * ``bounds`` given a result of 0 returns, per expanded head, every error
      of the terms (the bf16 rounding of P / dS, their own errors) plus
      gamma(T) sum |term| for the float32 sum and half a bf16 ulp OF THAT
      BOUND (at most 2^-8 of it) in place of the result's rounding; these
      are summed over the group;
    * the float32 sum runs over G T terms: (gamma(G T) - gamma(T)) sum |term|
      more, with sum |term| = sum_i |dS_ij| |q_id| (dk), sum_i P_ij |dO_id|
      (dv), from the oracle;
    * ONE half bf16 ulp of the summed result (GPU); on the CPU the G float32
      head results are rounded (4 u each) and added in float32 (gamma(G))."""
    G, T = NH // KVH, wide[0].shape[1]
    zero = {n: np.zeros_like(ref[n + "_heads"]) for n in ("dk", "dv")}
    bd = bounds(*wide, NH, causal, dict(ref, **zero), gpu, tk)
    qh, doh = (heads_of(np.abs(t), NH) for t in (wide[0], wide[3]))
    terms = {"dk": np.einsum("bhij,bhid->bhjd", np.abs(ref["dS"]), qh),
             "dv": np.einsum("bhij,bhid->bhjd", ref["P"], doh)}
    for n in ("dk", "dv"):
        b = group_sum(bd[n] + (gamma(G * T) - gamma(T)) * unheads(terms[n]),
                      KVH, G)
        bd[n] = b + (bf_half_ulp(np.abs(ref[n]) + b) if gpu else
                     (4 * U + gamma(G)) *
                     group_sum(np.abs(ref[n + "_heads"]), KVH, G))
    return bd


def check_gqa(r, got, case, NH, KVH, causal, gpu, tk=None):
    wide, ref = gqa_oracle(case, NH, KVH, causal)
    bd = gqa_bounds(wide, ref, NH, KVH, causal, gpu, tk)
    for n in NAMES:
        r.see(n, np.abs(f64(got[n]) - ref[n]), bd[n])


def run_gqa(case, NH, KVH, causal, **kw):
    """forward + backward on the device and in the dtype of ``case``"""
    q, k, v, do = case
    save = {}
    o = ops.attention_fwd(q, k, v, NH, causal=causal, save=save, kv_heads=KVH,
                          **kw)
    dq, dk, dv = ops.attention_bwd(do, q, k, v, o, save, NH, causal=causal,
                                   kv_heads=KVH, **kw)
    return {"o": o, "lse": save["lse"], "dq": dq, "dk": dk, "dv": dv}


@pytest.mark.parametrize("causal", (False, True))
def test_oracle_against_torch_sdpa(causal):
    B, T, NH, KVH, D = 2, 37, 4, 2, 32
    case = gqa_case(B, T, NH, KVH, D, seed=3)
    q, k, v, do = (t.double().requires_grad_(True) for t in case)
    hq, hk, hv = (t.view(B, T, -1, D).transpose(1, 2) for t in (q, k, v))
    try:
        o = F.scaled_dot_product_attention(hq, hk, hv, is_causal=causal,
                                           enable_gqa=True)
    except TypeError:      # a torch without the argument
        o = F.scaled_dot_product_attention(
            hq, *(t.repeat_interleave(NH // KVH, 1) for t in (hk, hv)),
            is_causal=causal)
    o = o.transpose(1, 2).reshape(B, T, NH * D)
    o.backward(do.detach())
    _, ref = gqa_oracle(case, NH, KVH, causal)
    for name, t in (("o", o), ("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
        err = np.abs(ref[name] - f64(t)).max() / np.abs(f64(t)).max()
        assert err < 1e-12, (name, err)


@pytest.mark.parametrize("causal", (False, True))
@pytest.mark.parametrize("B,T,NH,KVH,D", ((2, 33, 4, 2, 32), (1, 31, 6, 3, 64),
                                          (2, 1, 3, 1, 32), (1, 129, 4, 1, 32)))
def test_cpu_core_within_the_bound(B, T, NH, KVH, D, causal):
    case = gqa_case(B, T, NH, KVH, D)
    r = Ratios()
    check_gqa(r, run_gqa(case, NH, KVH, causal), case, NH, KVH, causal, False)
    print((B, T, NH, KVH, D, causal), {k: round(v, 4) for k, v in r.items()})


def test_wrong_head_mapping_leaves_the_bound():
    """h % KVH in place of h // G, against the GPU bound (the wider one)"""
    NH, KVH, causal = 4, 2, True
    case = gqa_case(1, 33, NH, KVH, 32)
    wide, ref = gqa_oracle(case, NH, KVH, causal)
    bd = gqa_bounds(wide, ref, NH, KVH, causal, True, tk=ops.ATTN_TK)
    _, bad = gqa_oracle(case, NH, KVH, causal, rule="mod")
    worst = max(float((np.abs(bad[n] - ref[n]) / bd[n]).max()) for n in NAMES)
    assert worst > 10.0, worst


def test_kv_heads_equal_to_heads_is_the_call_without_it():
    case = make_case(2, 33, 2, 32, seed=1)
    q, k, v, do = case
    a = run_gqa(case, 2, None, True)
    b = run_gqa(case, 2, 2, True)
    save = {}
    o = ops.attention_fwd(q, k, v, 2, causal=True, save=save)
    c = ops.attention_bwd(do, q, k, v, o, save, 2, causal=True)
    for n, t in zip(NAMES, (o, save["lse"]) + tuple(c)):
        assert torch.equal(a[n], t) and torch.equal(b[n], t), n


@pytest.mark.parametrize("bad", (0, 3, 8))
def test_bad_kv_heads_raise_before_any_launch(bad):
    q, k, v, do = make_case(1, 5, 4, 32)
    with pytest.raises(ValueError, match="kv_heads"):
        ops.attention_fwd(q, k, v, 4, kv_heads=bad)
    with pytest.raises(ValueError, match="kv_heads"):
        ops.attention_bwd(do, q, k, v, q, {"lse": torch.zeros(1, 4, 5)}, 4,
                          kv_heads=bad)
    with pytest.raises(ValueError):       # k as wide as q under kv_heads = 2
        ops.attention_fwd(q, k, v, 4, kv_heads=2)


def mha_gqa_case(B, T, I, E, NH, KVH, seed=0):
    """x, flat weights [(E + 2 EK) I + E E], bias [E + 2 EK + E], err on the
    bf16 grid (float32 CPU tensors)"""
    W = E + 2 * KVH * (E // NH)
    g = torch.Generator().manual_seed(seed + 31 * T + E)
    rnd = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    return tuple(t.to(torch.bfloat16).float() for t in (
        rnd(B, T, I), torch.cat((rnd(W * I) / I ** 0.5, rnd(E * E) / E ** 0.5)),
        rnd(W + E) * 0.1, rnd(B, T, E)))


def run_mha_gqa(x, w, b, err, E, NH, KVH, causal, save=None):
    """The layer ops on the device of ``x`` -> y, dw (flat), db, dx"""
    I, n = x.shape[2], w.numel() - E * E
    w_in, w_out = w[:n].view(n // I, I), w[n:].view(E, E)
    save = {} if save is None else save
    y = ops.mha_fwd(x, w_in, w_out, b, NH, causal=causal, save=save,
                    kv_heads=KVH)
    dw = torch.full((n + E * E,), 7.0, device=x.device)
    db = torch.full((n // I + E,), -7.0, device=x.device)
    dx = ops.mha_bwd(err, x, w_in, w_out, save, dw[:n].view(n // I, I),
                     dw[n:].view(E, E), db, NH, causal=causal, kv_heads=KVH)
    return {"y": y, "dw": dw, "db": db, "dx": dx}


def check_mha_gqa(r, got, x, w, b, err, E, NH, KVH, causal, gpu, tk=None):
    """The layer in float64 with the three projections by hand (rows q: E,
    k: EK, v: EK of W_in, bias offsets E, E + EK, W), and the bound of
    test_attention_ref.check_mha term by term at the narrow widths: qkv and
    do carry gamma(K) of their GEMM and one rounding; the core is held to
    ``gqa_bounds`` plus its sensitivity to those input errors (differences
    of the oracle along four random sign patterns, scaled by sqrt(4 n) for
    the worst signs, n = max(G T, D) the terms of one output element,
    doubled); the outer GEMMs add gamma(K) of their absolute sums and the
    rounding of the result."""
    x, w, b, err = (f64(t) for t in (x, w, b, err))
    B, T, I = x.shape
    D, rows = E // NH, B * T
    EK, G = KVH * D, NH // KVH
    W = E + 2 * EK
    w_in, w_out = w[:W * I].reshape(W, I), w[W * I:].reshape(E, E)
    x2, e2 = x.reshape(rows, I), err.reshape(rows, E)
    cut = lambda a: [a[:, lo:hi].reshape(B, T, hi - lo)    # noqa: E731
                     for lo, hi in ((0, E), (E, E + EK), (E + EK, W))]
    qkv = x2 @ w_in.T + b[:W]
    q, k, v = cut(qkv)
    do = (e2 @ w_out).reshape(B, T, E)
    wide, core = gqa_oracle((q, k, v, do), NH, KVH, causal)
    o2 = core["o"].reshape(rows, E)
    dqkv = np.concatenate([core[n].reshape(rows, -1)
                           for n in ("dq", "dk", "dv")], 1)
    ref = {"y": o2 @ w_out.T + b[W:], "dx": dqkv @ w_in,
           "dw": np.concatenate(((dqkv.T @ x2).ravel(), (e2.T @ o2).ravel())),
           "db": np.concatenate((dqkv.sum(0), e2.sum(0)))}
    ax, ae, aw_in, aw_out = (np.abs(t) for t in (x2, e2, w_in, w_out))
    rnd = 2.0 ** -9 if gpu else 2 * U
    tiny = 1e-30
    e_q, e_k, e_v = cut(gamma(I + 2) * (ax @ aw_in.T + np.abs(b[:W])) +
                        rnd * np.abs(qkv) + tiny)
    e_do = (gamma(E + 1) * (ae @ aw_out)).reshape(B, T, E) + \
        rnd * np.abs(do) + tiny
    bd = gqa_bounds(wide, core, NH, KVH, causal, gpu, tk)
    rng = np.random.default_rng(7)
    tot = {n: 0.0 for n in ("o", "dq", "dk", "dv")}
    for _ in range(4):
        moved = [t + rng.choice((-1.0, 1.0), size=t.shape) * e for t, e in
                 ((q, e_q), (k, e_k), (v, e_v), (do, e_do))]
        pert = gqa_oracle(moved, NH, KVH, causal)[1]
        tot = {n: np.maximum(tot[n], np.abs(pert[n] - core[n])) for n in tot}
    grow = 2.0 * (4.0 * max(G * T, D)) ** 0.5
    tot = {n: (bd[n] + grow * s).reshape(rows, -1) for n, s in tot.items()}
    t_dqkv = np.concatenate([tot[n] for n in ("dq", "dk", "dv")], 1)
    ao, adqkv = np.abs(o2), np.abs(dqkv)

    def rounded(bnd, val):
        val = np.abs(val)
        return bnd + (bf_half_ulp(val + bnd) if gpu else 4 * U * val)
    bnd = {"y": rounded(tot["o"] @ aw_out.T + gamma(E + 2) * (
               ao @ aw_out.T + np.abs(b[W:])) + tiny, ref["y"]),
           "dx": rounded(t_dqkv @ aw_in + gamma(W + 2) * (adqkv @ aw_in) +
                         tiny, ref["dx"]),
           "dw": np.concatenate((
               (t_dqkv.T @ ax + gamma(rows + 2) * (adqkv.T @ ax)).ravel(),
               (ae.T @ tot["o"] + gamma(rows + 2) * (ae.T @ ao)).ravel())) +
           tiny,
           "db": np.concatenate((t_dqkv.sum(0) + gamma(rows + 2) *
                                 adqkv.sum(0), gamma(rows + 2) * ae.sum(0))) +
           tiny}
    for n in ("y", "dw", "db", "dx"):
        r.see("mha_" + n, np.abs(f64(got[n]).reshape(ref[n].shape) - ref[n]),
              bnd[n])


@pytest.mark.parametrize("causal", (False, True))
@pytest.mark.parametrize("B,T,I,E,NH,KVH", ((2, 9, 8, 128, 4, 2),
                                            (1, 33, 64, 64, 2, 1)))
def test_cpu_mha_within_the_bound(B, T, I, E, NH, KVH, causal):
    case = mha_gqa_case(B, T, I, E, NH, KVH)
    r = Ratios()
    check_mha_gqa(r, run_mha_gqa(*case, E, NH, KVH, causal), *case, E, NH,
                  KVH, causal, False)
    print((B, T, I, E, NH, KVH, causal), {k: round(v, 4) for k, v in r.items()})


def layer(**att):
    from test_attention_units import _wf
    gd = {"solvers": ("adam",), "learning_rate": 1e-2}
    return _wf([{"type": "attention", "->": dict(output_sample_shape=64, **att),
                 "<-": dict(gd)},
                {"type": "softmax", "->": {"output_sample_shape": 8},
                 "<-": dict(gd)}])


def test_layer_parameters_and_kv_heads_equal_to_heads():
    from test_attention_units import _state
    wf = layer(heads=2, kv_heads=1)
    att = wf.forwards[0]
    I, E, W = att.n_in, 64, 64 + 2 * 32
    assert att.weights.mem.shape == (W * I + E * E,)
    assert att.bias.mem.shape == (W + E,)
    w_in, w_out = att.split(torch.zeros(W * I + E * E), I)
    assert tuple(w_in.shape) == (W, I) and tuple(w_out.shape) == (E, E)
    wf.run_steps(2)
    assert torch.isfinite(_state(wf)).all()
    for bad in (0, 3):
        with pytest.raises(ValueError, match="kv_heads"):
            layer(heads=2, kv_heads=bad)
    a, b = layer(heads=2), layer(heads=2, kv_heads=2)
    a.run_steps(3)
    b.run_steps(3)
    assert torch.equal(_state(a), _state(b))


# samples/seq_recall_gqa_config.py on the CPU device, measured as in
# tests/test_ffn_sample.py: seeds 1 .. 5 ran 36 epochs; the validation errors
# (of 256) start at 220, 229, 227, 228, 205, first fall below 20 at epochs 13,
# 14, 11, 13, 11 and over epochs 30 .. 36 stay within the ranges below; each
# seed is held to its plateau widened by 2 samples either way
SAMPLE_PLATEAU = ((10, 11), (12, 13), (4, 4), (13, 13), (9, 9))


@pytest.mark.parametrize("seed", (1, 2, 3, 4, 5))
def test_gqa_sample_trains_on_cpu(tmp_path, seed):
    import json
    from test_ffn_sample import cli
    res = tmp_path / "results.json"
    out = cli("samples/seq_recall.py", "samples/seq_recall_gqa_config.py",
              "-a", "cpu", "-r", str(seed), "--result-file", str(res),
              "root.common.disable.snapshotting=True")
    assert "Workflow wall time" in out
    h = json.loads(res.read_text())["Epoch history"]
    assert len(h) == 30
    errors = [round(e["validation_err_pt"] * 256 / 100.0) for e in h]
    assert errors[0] > 128, errors        # it starts near chance (7/8)
    lo, hi = SAMPLE_PLATEAU[seed - 1]
    assert lo - 2 <= errors[-1] <= hi + 2, errors
