"""Float64 oracle of self-attention (docs/OPS.md "Attention"), the checks on
it, and the error bounds that hold ``ops.attention_fwd`` / ``attention_bwd``
/ ``mha_fwd`` / ``mha_bwd`` to it: here for the float32 CPU path,
tests/test_attention_gpu.py imports the same helpers for the HIP kernels.

The oracle is plain NumPy: per (batch, head) it materialises S = q k^T /
sqrt(D), P = softmax(S) (key j hidden from query i when j > i under
``causal``), o = P v, lse = ln sum exp(S) and all five gradients
(dV = P^T dO, dP = dO V^T, delta = rowsum(dO o), dS = P (dP - delta) /
sqrt(D), dQ = dS K, dK = dS^T Q).  It is held to float64
``F.scaled_dot_product_attention`` and, with the projections around it, to
float64 ``torch.nn.MultiheadAttention`` with autograd at 1e-12 relative.

Error bounds (u = 2^-24 one float32 rounding, gamma(n) = n u / (1 - n u);
all derived, none measured).  A companion pass of the oracle over absolute
values gives the sums the rounding errors scale with:

    A_ij  = sum_d |q_id| |k_jd| / sqrt(D)     R_i = max_j A_ij  (>= |S_ij|)
    AO_id = sum_j P_ij |v_jd|                 ADP_ij = sum_d |dO_id| |v_jd|

* score: the float32 product chain of D terms and the multiplication by the
  scale, es_ij = gamma(D + 2) A_ij.
* P before normalisation: the score's error, the rounding of the difference
  to the running maximum (|S - m| <= 2 R_i), and the float32 exponential
  (EXP_REL = 2^-22: the hardware base-2 exponential and torch's are good to
  1 ulp = 2^-23; twice that): eP_i = max_j es_ij + 2 u R_i + EXP_REL.
* online softmax: every key tile rescales l and O by exp(m_old - m_new): nt
  exponentials and multiplications and the roundings of the differences,
  which add up to the spread of the row: eR_i = nt (EXP_REL + 2 u) + 2 u R_i
  (nt = ceil(T / TK) on the GPU, 1 on the CPU).
* l: eL_i = eP_i + gamma(T) + eR_i; lse = m + ln l in float32:
  b_lse = eL_i + 4 u (R_i + ln T + 1).
* o = (sum_j bf16(P~_ij) v_jd) / l:
  b_o = AO_id (BFU + eP_i + gamma(T) + eR_i + eL_i + 4 u) + half a bf16
  ulp of the result.  BFU = 2^-8 is the unit roundoff of bfloat16 (8
  significant bits): half a bf16 ulp h(x) = 2^(e-9) for x in [2^(e-1), 2^e)
  is between 2^-9 and 2^-8 of x, and what the kernel rounds is the
  unnormalised exp(S_ij - m), whose place in its binade is not P's.  (A plain
  2^-9 sum_j |p_ij| |v_jd| is met only when every p sits at the top of its
  binade: a correctly rounding kernel exceeded it by up to 1.27 x on the
  first run of these tests, on rows with few visible keys.)  On the CPU this
  term is 0 and the results are float32: 4 u |o| instead of the half ulp.
* backward: P is recomputed from the forward's lse:
  ePb_ij = es_ij + b_lse_i + 2 u (2 R_i + ln T) + EXP_REL;
  delta from the forward's o: ed_i = sum_d |dO_id| b_o_id +
  gamma(D + 1) sum_d |dO_id o_id|;
  dS before its rounding: eds_ij = P_ij / sqrt(D) (ePb_ij |dP_ij - delta_i| +
  gamma(D) ADP_ij + ed_i + 3 u (|dP_ij| + |delta_i|));
  dV_jd: sum_i (h(P_ij) + P_ij (ePb_ij + gamma(T))) |dO_id| + half ulp
  (here the rounded value is P itself up to ePb, so h applies, taken at
  P (1 + ePb));
  dK_jd: sum_i (eds_ij + h(|dS_ij| + eds_ij) + gamma(T) |dS_ij|) |q_id| +
  half ulp;
  dQ_id: the same sum over j with |k_jd|.
  A flushed subnormal (the kernels are built with denormals flushed) moves a
  product by less than 2^-126 T: TINY = 1e-30 covers it.

The wrong rules (no 1 / sqrt(D); a mask of j < i; lse without the maximum;
dS without - delta) leave these bounds on the test inputs
(``test_wrong_rules_leave_the_bound``).

The worst |error| / bound of the CPU path goes to
profiles/attention/cpu_tests_figures.txt.
"""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import veles_amd.ops as ops
from veles_amd.ops import _lib
from test_step_tail_ref import Ratios, U, bf_half_ulp, f64, gamma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIGURES = os.path.join(ROOT, "profiles", "attention", "cpu_tests_figures.txt")
WORST = Ratios()
EXP_REL = 2.0 ** -22
BF_REL = 2.0 ** -9      # half a bf16 ulp relative to the top of a binade
BF_U = 2.0 ** -8        # ... to its bottom: the unit roundoff of bfloat16
TINY = 1e-30
RULES = ("no_scale", "mask_lt", "lse_no_max", "ds_no_delta")


@pytest.fixture(scope="module", autouse=True)
def figures():
    yield
    if not WORST:
        return
    os.makedirs(os.path.dirname(FIGURES), exist_ok=True)
    with open(FIGURES, "w") as f:
        f.write("# worst |error| / bound per quantity over "
                "tests/test_attention_ref.py (float32 CPU path)\n")
        for k in sorted(WORST):
            f.write("%-8s %.4f\n" % (k, WORST[k]))


# ------------------------------------------------------------------ oracle
def heads_of(t, NH):
    """[B][T][NH*D] -> [B][NH][T][D]"""
    B, T, E = t.shape
    return t.reshape(B, T, NH, E // NH).transpose(0, 2, 1, 3)


def unheads(t):
    B, NH, T, D = t.shape
    return t.transpose(0, 2, 1, 3).reshape(B, T, NH * D)


def oracle(q, k, v, do, NH, causal, rule=None):
    """float64 [B][T][E] arrays -> dict of o, lse [B][NH][T], dq, dk, dv and
    the per-head intermediates P, S, dS, dP, delta.  ``rule``: one of RULES,
    a deliberately wrong variant."""
    qh, kh, vh, doh = (heads_of(t, NH) for t in (q, k, v, do))
    T, D = qh.shape[2], qh.shape[3]
    scale = 1.0 if rule == "no_scale" else 1.0 / math.sqrt(D)
    S = np.einsum("bhid,bhjd->bhij", qh, kh) * scale
    i = np.arange(T)
    hidden = np.zeros((T, T), bool)
    if causal:
        hidden = (i[None, :] >= i[:, None]) if rule == "mask_lt" else \
            (i[None, :] > i[:, None])
        if rule == "mask_lt":
            hidden[0, 0] = False    # row 0 would be empty
    S = np.where(hidden, -np.inf, S)
    m = S.max(3, keepdims=True)
    e = np.exp(S - m)
    l = e.sum(3, keepdims=True)
    P = e / l
    lse = (m + np.log(l))[..., 0]
    oh = P @ vh
    Pb = P
    if rule == "lse_no_max":
        lse = np.log(l)[..., 0]
        Pb = np.where(hidden, 0.0, np.exp(np.where(hidden, 0.0, S) -
                                          lse[..., None]))
    dP = doh @ vh.transpose(0, 1, 3, 2)
    delta = (doh * oh).sum(3, keepdims=True)
    dS = Pb * (dP - (0.0 if rule == "ds_no_delta" else delta)) * scale
    return {"o": unheads(oh), "lse": lse, "dq": unheads(dS @ kh),
            "dk": unheads(dS.transpose(0, 1, 3, 2) @ qh),
            "dv": unheads(Pb.transpose(0, 1, 3, 2) @ doh),
            "P": P, "S": S, "dS": dS, "dP": dP, "delta": delta[..., 0]}


def bounds(q, k, v, do, NH, causal, ref, gpu, tk=None):
    """Per-element bounds of o, lse, dq, dk, dv (the module docstring);
    ``gpu``: bf16 operands of the second products and bf16 results, online
    softmax over key tiles of ``tk``."""
    qh, kh, vh, doh = (heads_of(np.abs(t), NH) for t in (q, k, v, do))
    T, D = qh.shape[2], qh.shape[3]
    scale = 1.0 / math.sqrt(D)
    nt = -(-T // tk) if gpu else 1
    P, dS = ref["P"], np.abs(ref["dS"])
    A = np.einsum("bhid,bhjd->bhij", qh, kh) * scale
    R = A.max(3)                                         # [B][NH][T]
    es = gamma(D + 2) * A
    eP = es.max(3) + 2 * U * R + EXP_REL
    eR = nt * (EXP_REL + 2 * U) + 2 * U * R
    eL = eP + gamma(T) + eR
    b_lse = eL + 4 * U * (R + math.log(T) + 1.0)
    AO = P @ vh
    b_o = AO * ((BF_U if gpu else 0.0) + eP + gamma(T) + eR + eL +
                4 * U)[..., None] + TINY
    oh = heads_of(ref["o"], NH)

    def finish(b, val):
        """+ the rounding of the result itself"""
        val = np.abs(val)
        return b + (bf_half_ulp(val + b) if gpu else 4 * U * val)
    b_o = finish(b_o, oh)
    ePb = es + (b_lse + 2 * U * (2 * R + math.log(T)) + EXP_REL)[..., None]
    ed = (doh * b_o).sum(3) + gamma(D + 1) * (doh * np.abs(oh)).sum(3)
    ADP = np.einsum("bhid,bhjd->bhij", doh, vh)
    dPd = np.abs(ref["dP"] - ref["delta"][..., None])
    eds = P * scale * (ePb * dPd + gamma(D) * ADP + ed[..., None] +
                       3 * U * (np.abs(ref["dP"]) +
                                np.abs(ref["delta"])[..., None]))
    edsr = eds + gamma(T) * dS + (bf_half_ulp(dS + eds) if gpu else 0.0)
    # |bf16(P~) - P~| at the largest P~ the kernel may hold
    HP = bf_half_ulp(P * (1.0 + ePb)) if gpu else 0.0
    b_dv = np.einsum("bhij,bhid->bhjd", HP + P * (ePb + gamma(T)), doh) + TINY
    b_dk = np.einsum("bhij,bhid->bhjd", edsr, qh) + TINY
    b_dq = np.einsum("bhij,bhjd->bhid", edsr, kh) + TINY
    return {"o": unheads(b_o), "lse": b_lse,
            "dq": unheads(finish(b_dq, heads_of(ref["dq"], NH))),
            "dk": unheads(finish(b_dk, heads_of(ref["dk"], NH))),
            "dv": unheads(finish(b_dv, heads_of(ref["dv"], NH)))}


def make_case(B, T, NH, D, seed=0, std=1.0):
    """Independent Gaussian q, k, v, do [B][T][NH*D] on the bf16 grid (exact
    in float32 and bfloat16), float32 CPU tensors"""
    g = torch.Generator().manual_seed(1000 * seed + 17 * T + D + NH + B)
    return tuple((torch.randn(B, T, NH * D, generator=g) * s)
                 .to(torch.bfloat16).float()
                 for s in (std, std, 1.0, 1.0))


def check_core(r, tag, got, case, NH, causal, gpu, tk=None, ref=None):
    """got: dict of o, lse, dq, dk, dv tensors; asserts every bound"""
    q, k, v, do = (f64(t) for t in case)
    ref = ref if ref is not None else oracle(q, k, v, do, NH, causal)
    bd = bounds(q, k, v, do, NH, causal, ref, gpu, tk)
    for name in ("o", "lse", "dq", "dk", "dv"):
        if name in got:
            r.see(tag + name, np.abs(f64(got[name]) - ref[name]), bd[name])
    return ref, bd


def run_core_cpu(case, NH, causal):
    q, k, v, do = case
    save = {}
    o = ops.attention_fwd(q, k, v, NH, causal=causal, save=save)
    dq, dk, dv = ops.attention_bwd(do, q, k, v, o, save, NH, causal=causal)
    return {"o": o, "lse": save["lse"], "dq": dq, "dk": dk, "dv": dv}


# ------------------------------------------------------ oracle against torch
def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("causal", (False, True))
def test_oracle_against_torch_sdpa(causal):
    B, T, NH, D = 2, 37, 3, 32
    q, k, v, do = (t.double().requires_grad_(True)
                   for t in make_case(B, T, NH, D, seed=3))
    hs = [t.view(B, T, NH, D).transpose(1, 2) for t in (q, k, v)]
    o = F.scaled_dot_product_attention(*hs, is_causal=causal)
    o = o.transpose(1, 2).reshape(B, T, NH * D)
    o.backward(do.detach())
    ref = oracle(*(f64(t) for t in (q, k, v, do)), NH, causal)
    assert rel(ref["o"], f64(o)) < 1e-12
    for name, t in (("dq", q), ("dk", k), ("dv", v)):
        assert rel(ref[name], f64(t.grad)) < 1e-12, name
    s = (hs[0] @ hs[1].transpose(2, 3)) / math.sqrt(D)
    if causal:
        s = s.masked_fill(torch.ones(T, T).triu(1).bool(), float("-inf"))
    assert rel(ref["lse"], f64(torch.logsumexp(s, 3))) < 1e-12


def mha_oracle(x, w, b, err, I, E, NH, causal):
    """The layer in float64 from the flat ``weights`` [3E*I + E*E] and
    ``bias`` [4E]: y, dweights, dbias, dx"""
    w_in, w_out = w[:3 * E * I].reshape(3 * E, I), w[3 * E * I:].reshape(E, E)
    B, T, _ = x.shape
    x2 = x.reshape(B * T, I)
    qkv = x2 @ w_in.T + b[:3 * E]
    q, k, v = (qkv[:, n * E:(n + 1) * E].reshape(B, T, E) for n in range(3))
    e2 = err.reshape(B * T, E)
    do = (e2 @ w_out).reshape(B, T, E)
    ref = oracle(q, k, v, do, NH, causal)
    o2 = ref["o"].reshape(B * T, E)
    y = o2 @ w_out.T + b[3 * E:]
    dqkv = np.concatenate([ref[n].reshape(B * T, E)
                           for n in ("dq", "dk", "dv")], 1)
    dw = np.concatenate(((dqkv.T @ x2).reshape(-1), (e2.T @ o2).reshape(-1)))
    db = np.concatenate((dqkv.sum(0), e2.sum(0)))
    return {"y": y.reshape(B, T, E), "dw": dw, "db": db,
            "dx": (dqkv @ w_in).reshape(B, T, I), "core": ref,
            "qkv": (q, k, v), "do": do}


def torch_mha(x, w, b, err, I, E, NH, causal):
    """float64 torch.nn.MultiheadAttention fed through the documented
    layout; returns y, dweights, dbias, dx as arrays"""
    assert I == E      # in_proj_weight is [3E][E]
    mha = torch.nn.MultiheadAttention(E, NH, bias=True, dropout=0.0,
                                      batch_first=True).double()
    wt, bt = torch.from_numpy(w), torch.from_numpy(b)
    with torch.no_grad():
        mha.in_proj_weight.copy_(wt[:3 * E * I].view(3 * E, I))
        mha.out_proj.weight.copy_(wt[3 * E * I:].view(E, E))
        mha.in_proj_bias.copy_(bt[:3 * E])
        mha.out_proj.bias.copy_(bt[3 * E:])
    xt = torch.from_numpy(x).requires_grad_(True)
    T = x.shape[1]
    mask = torch.ones(T, T).triu(1).bool() if causal else None
    y, _ = mha(xt, xt, xt, attn_mask=mask, need_weights=False,
               is_causal=causal)
    y.backward(torch.from_numpy(err))
    dw = torch.cat((mha.in_proj_weight.grad.reshape(-1),
                    mha.out_proj.weight.grad.reshape(-1)))
    db = torch.cat((mha.in_proj_bias.grad, mha.out_proj.bias.grad))
    return f64(y), f64(dw), f64(db), f64(xt.grad)


def mha_case(B, T, I, E, seed=0):
    g = torch.Generator().manual_seed(seed + 31 * T + E)
    bfr = lambda t: t.to(torch.bfloat16).float()   # noqa: E731
    x = bfr(torch.randn(B, T, I, generator=g))
    w = bfr(torch.cat((torch.randn(3 * E * I, generator=g) / math.sqrt(I),
                       torch.randn(E * E, generator=g) / math.sqrt(E))))
    b = bfr(torch.randn(4 * E, generator=g) * 0.1)
    err = bfr(torch.randn(B, T, E, generator=g))
    return x, w, b, err


@pytest.mark.parametrize("causal", (False, True))
def test_oracle_against_torch_mha(causal):
    """the weights / bias layout and all of y, dW, db, dx"""
    B, T, E, NH = 2, 9, 64, 2
    x, w, b, err = (f64(t) for t in mha_case(B, T, E, E, seed=5))
    ref = mha_oracle(x, w, b, err, E, E, NH, causal)
    y, dw, db, dx = torch_mha(x, w, b, err, E, E, NH, causal)
    assert rel(ref["y"], y) < 1e-12
    assert rel(ref["dw"], dw) < 1e-12
    assert rel(ref["db"], db) < 1e-12
    assert rel(ref["dx"], dx) < 1e-12


# ------------------------------------------------------------ the CPU path
CPU_SHAPES = [(1, 1, 1, 32), (1, 2, 1, 64), (2, 31, 3, 32), (1, 33, 1, 64),
              (3, 33, 3, 128), (1, 129, 2, 64)]


@pytest.mark.parametrize("causal", (False, True))
@pytest.mark.parametrize("shape", CPU_SHAPES)
def test_cpu_core_within_the_bound(shape, causal):
    B, T, NH, D = shape
    case = make_case(B, T, NH, D)
    r = Ratios()
    check_core(r, "", run_core_cpu(case, NH, causal), case, NH, causal, False)
    WORST.merge(r)


def spike_case(T, D, qi, kj, NH=1, seed=0):
    """Every score near 0 except (qi, kj): q_qi = k_kj = c 1 with c^2 sqrt(D)
    about 120 (on the bf16 grid), above ln FLT_MAX = 88.7: a softmax without
    the running maximum overflows"""
    q, k, v, do = make_case(1, T, NH, D, seed=seed, std=0.05)
    c = float(torch.tensor(math.sqrt(120.0 / math.sqrt(D)))
              .to(torch.bfloat16))
    q[:, qi, :] = c
    k[:, kj, :] = c
    return q, k, v, do


@pytest.mark.parametrize("causal,qi,kj", ((False, 5, 3), (False, 5, 70),
                                          (True, 40, 40)))
def test_cpu_spiked_score(causal, qi, kj):
    case = spike_case(97, 64, qi, kj)
    ref = oracle(*(f64(t) for t in case), 1, causal)
    assert ref["S"][0, 0, qi, kj] > 100.0
    r = Ratios()
    got = run_core_cpu(case, 1, causal)
    for t in got.values():
        assert torch.isfinite(t).all()
    check_core(r, "spike_", got, case, 1, causal, False, ref=ref)
    WORST.merge(r)


def check_mha(r, tag, got, x, w, b, err, I, E, NH, causal, gpu, tk=None):
    """got: y, dw, db, dx (tensors) of the layer ops.  On the GPU path qkv,
    o, do and dqkv are bf16 tensors: each is held to the core bounds around
    half a bf16 ulp of its inputs, and the GEMMs to gamma(K) of their
    absolute sums plus the propagated error of their operands."""
    xr, wr, br, er = (f64(t) for t in (x, w, b, err))
    ref = mha_oracle(xr, wr, br, er, I, E, NH, causal)
    B, T, _ = xr.shape
    w_in = np.abs(wr[:3 * E * I].reshape(3 * E, I))
    w_out = np.abs(wr[3 * E * I:].reshape(E, E))
    ax = np.abs(xr.reshape(B * T, I))
    ae = np.abs(er.reshape(B * T, E))
    rnd = BF_REL if gpu else 2 * U
    q, k, v = ref["qkv"]
    # qkv and do: a GEMM and one rounding of the result
    e_qkv = gamma(I + 2) * (ax @ w_in.T + np.abs(br[:3 * E])) + \
        rnd * np.abs(np.concatenate([t.reshape(B * T, E)
                                     for t in (q, k, v)], 1)) + TINY
    e_do = (gamma(E + 1) * (ae @ w_out) +
            rnd * np.abs(ref["do"].reshape(B * T, E)) + TINY)
    eq, ek, ev = (e_qkv[:, n * E:(n + 1) * E].reshape(B, T, E)
                  for n in range(3))
    e_do = e_do.reshape(B, T, E)
    # the core at inputs moved by their errors: first order, through the
    # oracle evaluated at the corners would be 2^4 passes; the core is
    # smooth, so its sensitivity is bounded by central differences along
    # the worst-sign direction of every input, doubled
    core = ref["core"]
    bd = bounds(q, k, v, ref["do"], NH, causal, core, gpu, tk)
    sens = {n: np.zeros_like(core[n]) for n in ("o", "dq", "dk", "dv")}
    rng = np.random.default_rng(7)
    for _ in range(4):
        sg = [rng.choice((-1.0, 1.0), size=eq.shape) for _ in range(4)]
        pert = oracle(q + sg[0] * eq, k + sg[1] * ek, v + sg[2] * ev,
                      ref["do"] + sg[3] * e_do, NH, causal)
        for n in sens:
            sens[n] = np.maximum(sens[n], np.abs(pert[n] - core[n]))
    # random signs add up like sqrt(n) where the worst signs add up like n:
    # n is at most the terms of one output element
    grow = math.sqrt(4.0 * max(T, E // NH))
    tot = {n: bd[n] + 2.0 * grow * sens[n] for n in sens}
    ao = np.abs(core["o"].reshape(B * T, E))
    b_y = tot["o"].reshape(B * T, E) @ w_out.T + \
        gamma(E + 2) * (ao @ w_out.T + np.abs(br[3 * E:])) + TINY
    yv = np.abs(ref["y"].reshape(B * T, E))
    b_y = b_y + (bf_half_ulp(yv + b_y) if gpu else 4 * U * yv)
    r.see(tag + "y", np.abs(f64(got["y"]).reshape(B * T, E) -
                            ref["y"].reshape(B * T, E)), b_y)
    dqkv = np.concatenate([core[n].reshape(B * T, E)
                           for n in ("dq", "dk", "dv")], 1)
    t_dqkv = np.concatenate([tot[n].reshape(B * T, E)
                             for n in ("dq", "dk", "dv")], 1)
    rows = B * T
    b_dw = np.concatenate((
        (t_dqkv.T @ ax + gamma(rows + 2) * (np.abs(dqkv).T @ ax)).reshape(-1),
        (ae.T @ tot["o"].reshape(rows, E) +
         gamma(rows + 2) * (ae.T @ ao)).reshape(-1))) + TINY
    r.see(tag + "dw", np.abs(f64(got["dw"]) - ref["dw"]), b_dw)
    b_db = np.concatenate((t_dqkv.sum(0) +
                           gamma(rows + 2) * np.abs(dqkv).sum(0),
                           gamma(rows + 2) * ae.sum(0))) + TINY
    r.see(tag + "db", np.abs(f64(got["db"]) - ref["db"]), b_db)
    if "dx" in got:
        dxv = np.abs(ref["dx"].reshape(rows, I))
        b_dx = t_dqkv @ w_in + gamma(3 * E + 2) * (np.abs(dqkv) @ w_in) + TINY
        b_dx = b_dx + (bf_half_ulp(dxv + b_dx) if gpu else 4 * U * dxv)
        r.see(tag + "dx", np.abs(f64(got["dx"]).reshape(rows, I) -
                                 ref["dx"].reshape(rows, I)), b_dx)
    return ref


def run_mha(x, w, b, err, I, E, NH, causal, accumulate="overwrite",
            need_err_input=True, grads=None, save=None):
    """The layer ops on the device of ``x`` (weights in its dtype)"""
    w_in, w_out = w[:3 * E * I].view(3 * E, I), w[3 * E * I:].view(E, E)
    save = {} if save is None else save
    y = ops.mha_fwd(x, w_in, w_out, b, NH, causal=causal, save=save)
    if grads is None:
        grads = (torch.full((3 * E * I + E * E,), 7.0, device=x.device),
                 torch.full((4 * E,), -7.0, device=x.device))
    dw, db = grads
    dx = ops.mha_bwd(err, x, w_in, w_out, save, dw[:3 * E * I].view(3 * E, I),
                     dw[3 * E * I:].view(E, E), db, NH, causal=causal,
                     accumulate=accumulate, need_err_input=need_err_input)
    out = {"y": y, "dw": dw, "db": db}
    if dx is not None:
        out["dx"] = dx
    return out


@pytest.mark.parametrize("causal", (False, True))
@pytest.mark.parametrize("B,T,I,E,NH", ((2, 9, 8, 64, 2), (1, 33, 64, 64, 1)))
def test_cpu_mha_within_the_bound(B, T, I, E, NH, causal):
    x, w, b, err = mha_case(B, T, I, E)
    r = Ratios()
    got = run_mha(x, w, b, err, I, E, NH, causal)
    check_mha(r, "mha_", got, x, w, b, err, I, E, NH, causal, False)
    WORST.merge(r)
    # accumulate=True adds to what the buffers hold; no err_input on request
    g2 = (got["dw"].clone(), got["db"].clone())
    got2 = run_mha(x, w, b, err, I, E, NH, causal, accumulate=True,
                   need_err_input=False, grads=g2)
    assert "dx" not in got2
    assert torch.allclose(got2["dw"], 2 * got["dw"], rtol=1e-6, atol=1e-30)
    assert torch.allclose(got2["db"], 2 * got["db"], rtol=1e-6, atol=1e-30)


# -------------------------------------------------------------- wrong rules
@pytest.mark.parametrize("rule", RULES)
def test_wrong_rules_leave_the_bound(rule):
    """each wrong rule is outside the GPU bound (the wider one) somewhere"""
    B, T, NH, D = 1, 33, 1, 64
    case = tuple(f64(t) for t in make_case(B, T, NH, D))
    causal = True
    ref = oracle(*case, NH, causal)
    bd = bounds(*case, NH, causal, ref, True, tk=ops.ATTN_TK)
    bad = oracle(*case, NH, causal, rule=rule)
    worst = max(float((np.abs(bad[n] - ref[n]) / bd[n]).max())
                for n in ("o", "lse", "dq", "dk", "dv"))
    assert worst > 10.0, (rule, worst)


# -------------------------------------------------------------- host checks
def test_host_checks_raise_before_any_launch():
    q, k, v, do = make_case(2, 5, 2, 32)
    with pytest.raises(TypeError):
        ops.attention_fwd(q.numpy(), k, v, 2)
    with pytest.raises(TypeError):
        ops.attention_fwd(q.double(), k.double(), v.double(), 2)
    with pytest.raises(TypeError):
        ops.attention_fwd(q, k.double(), v, 2)
    with pytest.raises(ValueError):
        ops.attention_fwd(q[0], k[0], v[0], 2)
    with pytest.raises(ValueError):
        ops.attention_fwd(q, k[:, :4], v, 2)
    with pytest.raises(ValueError):
        ops.attention_fwd(q, k, v, 3)                 # 64 / 3
    with pytest.raises(ValueError, match=r"\[32, 64, 128\]"):
        ops.attention_fwd(q, k, v, 4)                 # D = 16
    with pytest.raises(ValueError):
        ops.attention_fwd(q.transpose(1, 2).contiguous().transpose(1, 2), k,
                          v, 2)
    with pytest.raises(ValueError):
        ops.attention_fwd(q, k, v, 2, out=torch.empty(2, 5, 32))
    save = {}
    o = ops.attention_fwd(q, k, v, 2, save=save)
    with pytest.raises(ValueError):
        ops.attention_bwd(do, q, k, v, o, {}, 2)
    with pytest.raises(ValueError):
        ops.attention_bwd(do, q, k, v, o, {"lse": save["lse"][:, :1]}, 2)
    with pytest.raises(ValueError):
        ops.attention_bwd(do[:, :4], q, k, v, o, save, 2)
    with pytest.raises(ValueError):
        ops.attention_bwd(do, q, k, v, o, save, 2, dq=torch.empty(2, 5, 32))
    x, w, b, err = mha_case(2, 5, 8, 64)
    w_in, w_out = w[:3 * 64 * 8].view(192, 8), w[3 * 64 * 8:].view(64, 64)
    with pytest.raises(ValueError):
        ops.mha_fwd(x, w_in[:100], w_out, b, 2)
    with pytest.raises(ValueError):
        ops.mha_fwd(x, w_in, w_out, b[:5], 2)
    with pytest.raises(ValueError):
        ops.mha_fwd(x, w_in, w_out, b, 8)             # D = 8
    with pytest.raises(TypeError):
        ops.mha_fwd(x.numpy(), w_in, w_out, b, 2)
    save = {}
    ops.mha_fwd(x, w_in, w_out, b, 2, save=save)
    dwi, dwo, db = torch.zeros(192, 8), torch.zeros(64, 64), torch.zeros(256)
    with pytest.raises(ValueError):
        ops.mha_bwd(err, x, w_in, w_out, {}, dwi, dwo, db, 2)
    with pytest.raises(ValueError):
        ops.mha_bwd(err, x, w_in, w_out, save, dwi, dwo, db, 2,
                    accumulate=False)
    with pytest.raises(ValueError):
        ops.mha_bwd(err[:, :4], x, w_in, w_out, save, dwi, dwo, db, 2)
    with pytest.raises(ValueError):
        ops.mha_bwd(err, x, w_in, w_out, save, dwi.double(), dwo, db, 2)
    with pytest.raises(ValueError):
        ops.mha_bwd(err, x, w_in, w_out, save, dwi, dwo, db, 2, aux_act=1)
    # column slices of a fused buffer are taken as they are
    fused = torch.cat((q, k, v), 2)
    o2 = ops.attention_fwd(fused[:, :, :64], fused[:, :, 64:128],
                           fused[:, :, 128:], 2)
    assert torch.equal(o, o2)


def test_buffers_live_in_the_callers_dicts():
    x, w, b, err = mha_case(2, 5, 8, 64)
    save = {}
    run_mha(x, w, b, err, 8, 64, 2, False, save=save)
    kept = {k_: t.data_ptr() for k_, t in save.items()}
    assert set(kept) == {"qkv", "o", "lse", "do", "dqkv", "delta"}
    run_mha(x, w, b, err, 8, 64, 2, False, save=save)
    assert kept == {k_: t.data_ptr() for k_, t in save.items()}


def test_abi_of_the_attention_entry_points():
    """tests/test_abi.py's comparison, for the bindings of attention.hip"""
    import test_abi
    decls = test_abi._decls()
    names = [n for n in decls if n.startswith("hvk_attn_")]
    assert len(names) == 5
    for name in names:
        assert name in _lib._OPTIONAL and name not in _lib._SIGS
        ret, args = decls[name]
        assert ret == "int"
        assert _lib._OPTIONAL[name] == [test_abi._kind(a) for a in args], name
    with open(os.path.join(test_abi.ROOT, "csrc", "kernels",
                           "hvk_api.h")) as h:
        src = h.read()
    for name in names:
        assert re.search(r"\b%s\(" % name, src), name
