"""The grouped-query kernels (hvk_gqa_fwd / _bwd_dkv / _bwd_dq) through the
oracle and bounds of tests/test_attention_gqa.py, on bf16.  T in {1, TK - 1,
TK + 1, TQ + 1}: the sweep-tile and owner-tile edges; at G = 2 and T = TK + 1
the four slots of a workgroup straddle two query blocks.  The worst |error| /
bound goes to profiles/attention/gqa_gpu_tests_figures.txt.

With dropout the five results are held to test_attention_dropout.check_drop on
the expanded case: dk and dv of the G heads of a group come from G backward
runs with do zeroed outside one head (every other head then adds exact
zeros), so each head's share, with its own mask rows, meets the per-head
bound.  The summed dk / dv of the full run is then held to the sum of those
pieces: both are bf16 roundings of float32 sums over the same products, one
chain of G T terms against G chains of T, so they differ by the G + 1 half
ulps and 2 gamma(G T) sum |term|; sum |term| is bounded from the p = 0 oracle
(P~ <= P / (1 - p); |dS~| <= P (|dP| + sum_j P |dP|) / ((1 - p) sqrt(D))).

One group (KVH = NH) through the same entries gives the bits of hvk_attn_* and
hvk_adrop_*: the kernels are one code, and ops never takes that route."""
import math
import os

import numpy as np
import pytest
import torch

from veles_amd import ops
from test_attention_dropout import check_drop, keep_inv
from test_attention_gqa import (NAMES, check_gqa, check_mha_gqa, gqa_case,
                                gqa_oracle, group_sum, mha_gqa_case,
                                run_gqa, run_mha_gqa)
from test_attention_ref import heads_of, unheads
from test_step_tail_ref import (BF, Ratios, bf_half_ulp, f64, gamma,
                                same_bits)

pytestmark = pytest.mark.gpu
FIGURES = os.path.join(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))), "profiles", "attention",
    "gqa_gpu_tests_figures.txt")
TQ, TK = ops.ATTN_TQ, ops.ATTN_TK
WORST = Ratios()
EDGES = (1, TK - 1, TK + 1, TQ + 1)
CORE = [(4, 2, T, 32, c) for T in EDGES for c in (False, True)] + [
    (6, 3, TK + 1, 64, True), (3, 1, TQ + 1, 128, False),
    (4, 1, TK - 1, 32, True), (4, 1, TQ + 1, 64, True), (3, 1, 1, 64, False)]


@pytest.fixture(scope="module", autouse=True)
def figures():
    yield
    os.makedirs(os.path.dirname(FIGURES), exist_ok=True)
    with open(FIGURES, "w") as f:
        f.write("# worst |error| / bound per quantity over "
                "tests/test_attention_gqa_gpu.py\n")
        f.writelines("%-8s %.4f\n" % kv for kv in sorted(WORST.items()))


def seed_tensor(v):
    return torch.tensor([v], dtype=torch.int32, device="cuda")


def views(case, pad=0):
    """q, k, v as column slices of one [B][T][E + 2 EK + pad] bf16 buffer, do
    with the same padding"""
    q, k, v, do = case
    B, T, E = q.shape
    qkv = torch.zeros(B, T, E + 2 * k.shape[2] + pad, dtype=BF, device="cuda")
    d = torch.zeros(B, T, E + pad, dtype=BF, device="cuda")
    out, c0 = [], 0
    for t in (q, k, v):
        out.append(qkv[:, :, c0:c0 + t.shape[2]])
        out[-1].copy_(t)
        c0 += t.shape[2]
    d[:, :, :E].copy_(do)
    return out + [d[:, :, :E]]


def merge(tag, r):
    print(tag, {k: round(v, 4) for k, v in r.items()})
    WORST.merge(r)


@pytest.mark.parametrize("NH,KVH,T,D,causal", CORE)
def test_core_within_the_bound(NH, KVH, T, D, causal):
    case = gqa_case(2, T, NH, KVH, D, seed=2)
    got = run_gqa(views(case), NH, KVH, causal)
    r = Ratios()
    check_gqa(r, got, case, NH, KVH, causal, True, tk=TK)
    merge((NH, KVH, T, D, causal), r)


def test_element_path_within_the_bound():
    """a pitch 2 bytes off the 16-byte grid"""
    case = gqa_case(2, TK + 1, 4, 2, 64, seed=4)
    gv = views(case, pad=1)
    assert gv[1].stride(1) % 8 == 1
    r = Ratios()
    check_gqa(r, run_gqa(gv, 4, 2, True), case, 4, 2, True, True, tk=TK)
    merge("element", r)


@pytest.mark.parametrize("NH,KVH,T,D,causal", (
    (4, 2, 1, 32, False), (4, 2, TK - 1, 128, True), (4, 2, TK + 1, 32, True),
    (4, 1, TQ + 1, 64, False)))
def test_dropout_within_the_bound(NH, KVH, T, D, causal):
    G, p, seed = NH // KVH, 0.5, 1234 + T
    case = gqa_case(2, T, NH, KVH, D, seed=3)
    q, k, v, do = views(case)
    kw = dict(dropout=p, seed_dev=seed_tensor(seed))
    got = run_gqa((q, k, v, do), NH, KVH, causal, **kw)
    full = {n: f64(got[n]) for n in ("dk", "dv")}
    B = q.shape[0]
    wide = {n: torch.zeros(B, T, KVH, G, D, dtype=BF, device="cuda")
            for n in ("dk", "dv")}
    for g in range(G):
        one = torch.zeros_like(do).view(B, T, KVH, G, D)
        one[:, :, :, g] = do.reshape(B, T, KVH, G, D)[:, :, :, g]
        part = run_gqa((q, k, v, one.view(B, T, NH * D)), NH, KVH, causal,
                       **kw)
        for n in wide:
            wide[n][:, :, :, g] = part[n].view(B, T, KVH, D)
    got.update({n: t.view(B, T, NH * D) for n, t in wide.items()})
    rep = lambda t: t.view(B, T, KVH, 1, D).expand(  # noqa: E731
        B, T, KVH, G, D).reshape(B, T, NH * D)
    r = Ratios()
    check_drop(r, got, (case[0], rep(case[1]), rep(case[2]), case[3]), NH,
               causal, p, seed, True, tk=TK)
    wide_case, ref = gqa_oracle(case, NH, KVH, causal)
    qh, doh = (heads_of(np.abs(wide_case[i]), NH) for i in (0, 3))
    P, adP = ref["P"], np.abs(ref["dP"])
    terms = {"dv": np.einsum("bhij,bhid->bhjd", P, doh),
             "dk": np.einsum("bhij,bhid->bhjd", P * (adP + (P * adP).sum(
                 3, keepdims=True)), qh) / math.sqrt(D)}
    for n in ("dk", "dv"):
        parts = f64(wide[n]).reshape(B, T, KVH, G, D)
        tol = bf_half_ulp(parts).sum(3).reshape(B, T, KVH * D) + \
            bf_half_ulp(full[n]) + 2 * gamma(G * T + 2) / (1 - p) * group_sum(
                unheads(terms[n]), KVH, G) + 1e-30
        r.see("sum_" + n, np.abs(full[n] - parts.sum(3).reshape(full[n].shape)),
              tol)
    merge(("dropout", NH, KVH, T, D, causal), {"p_" + n: x
                                               for n, x in r.items()})


@pytest.mark.parametrize("base_row", (0, 5))
def test_mask_readout(base_row):
    """q = 0: P is uniform, so with one-hot v the nonzero pattern of o is the
    mask of each QUERY head, and with one-hot do that of dv is the union of
    the masks of a group's heads (each dkv sweep took its own head's rows)"""
    B, NH, KVH, T, D, p, seed = 2, 4, 2, 32, 32, 0.5, 77
    G = NH // KVH
    eye = torch.eye(T).view(1, T, 1, T)
    q = torch.zeros(B, T, NH * D)
    kv = eye.expand(B, T, KVH, T).reshape(B, T, KVH * D)
    do = eye.expand(B, T, NH, T).reshape(B, T, NH * D)
    got = run_gqa(views((q, kv, kv, do)), NH, KVH, False, dropout=p,
                  seed_dev=seed_tensor(seed), base_row=base_row)
    keep, _ = keep_inv(B, NH, T, seed, p, base_row)      # [B][NH][i][j]
    assert np.array_equal(heads_of(f64(got["o"]), NH) != 0, keep)
    union = keep.reshape(B, KVH, G, T, T).any(2).transpose(0, 1, 3, 2)
    assert 0 < union.sum() < union.size
    assert np.array_equal(heads_of(f64(got["dv"]), KVH) != 0, union)


def test_two_runs_give_identical_bits():
    gv = views(gqa_case(2, 2 * TQ + 1, 4, 2, 64, seed=6))
    kw = dict(dropout=0.5, seed_dev=seed_tensor(9))
    a, b = (run_gqa(gv, 4, 2, True, **kw) for _ in "01")
    for n in NAMES:
        assert same_bits(a[n], b[n]), n


def test_layer_within_the_bound_and_graph_replays():
    """mha_fwd + mha_bwd at kv_heads = 2 of 4 heads against the float64 layer
    oracle; then the same chain captured once and replayed three times"""
    B, T, I, E, NH, KVH = 2, TK + 1, 64, 128, 4, 2
    case = mha_gqa_case(B, T, I, E, NH, KVH, seed=8)
    x, w, b, err = case
    dev = (x.to("cuda", BF), w.to("cuda", BF), b.cuda(), err.to("cuda", BF))
    save = {}
    ops.set_deterministic(True)
    try:
        def step():
            return run_mha_gqa(*dev, E, NH, KVH, True, save=save)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            step()       # warm-up: every buffer of ``save`` exists now
        torch.cuda.current_stream().wait_stream(s)
        eager = step()
        torch.cuda.synchronize()
        r = Ratios()
        check_mha_gqa(r, eager, *case, E, NH, KVH, True, True, tk=TK)
        merge("layer", r)
        W = E + 2 * KVH * (E // NH)
        assert tuple(save["qkv"].shape) == (B * T, W) == tuple(
            save["dqkv"].shape)
        kept = [save[n] for n in sorted(save)]
        want = [t.clone() for t in list(eager.values()) + kept]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = step()
        for _ in range(3):
            for t in list(out.values()) + kept:
                t.fill_(3.0)
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(u, v) for u, v in
                       zip(list(out.values()) + kept, want))
    finally:
        ops.set_deterministic(False)


def gqa_direct(case, NH, causal, p=0.0, seed_dev=None):
    """hvk_gqa_* called at KVH = NH, where ops takes hvk_attn_* / hvk_adrop_*"""
    q, k, v, do = case
    B, T, E = q.shape
    o, dq, dk, dv = (torch.empty(B, T, E, dtype=BF, device="cuda")
                     for _ in range(4))
    lse, delta = (torch.empty(B, NH, T, device="cuda") for _ in "01")
    lib, s = ops._lib.lib(), torch.cuda.current_stream().cuda_stream

    def at(*ts):
        return [x for t in ts for x in (t.data_ptr(), t.stride(1))]
    tail = [B, T, NH, NH, E // NH, int(causal),
            None if seed_dev is None else seed_dev.data_ptr(), p, 0, s]
    bwd = at(q, k, v, do) + [lse.data_ptr(), delta.data_ptr()]
    rcs = (lib.hvk_gqa_fwd(*at(q, k, v, o), lse.data_ptr(), *tail),
           lib.hvk_attn_bwd_delta(*at(do, o), delta.data_ptr(), B, T, NH,
                                  E // NH, s),
           lib.hvk_gqa_bwd_dkv(*bwd, *at(dk, dv), *tail),
           lib.hvk_gqa_bwd_dq(*bwd, *at(dq), *tail))
    assert rcs == (0, 0, 0, 0)
    return {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv}


def same_as_the_plain_entries(gv, NH, causal):
    for p, sd in ((0.0, None), (0.5, seed_tensor(4321))):
        kw = dict(dropout=p, seed_dev=sd) if p else {}
        plain = run_gqa(gv, NH, NH, causal, **kw)
        got = gqa_direct(gv, NH, causal, p, sd)
        for n in NAMES:
            assert same_bits(got[n], plain[n]), (n, p)


@pytest.mark.parametrize("D", (32, 128))
@pytest.mark.parametrize("causal", (False, True))
def test_one_group_gives_the_bits_of_the_plain_entries(D, causal):
    """G = 1 is the plain geometry: hvk_gqa_* at KVH = NH against hvk_attn_*
    (p = 0, null seed) and hvk_adrop_* (p = 0.5).  T = TQ + TK + 1: the second
    owned tile has one full wave, one wave with a single row, two idle"""
    same_as_the_plain_entries(
        views(gqa_case(2, TQ + TK + 1, 3, 3, D, seed=7)), 3, causal)


def test_one_group_gives_the_bits_of_the_plain_entries_element_path():
    gv = views(gqa_case(2, TQ + TK + 1, 3, 3, 32, seed=7), pad=1)
    assert gv[0].stride(1) % 8 == 1
    same_as_the_plain_entries(gv, 3, True)


def test_entry_points_reject_before_any_launch():
    """NH % KVH, a K/V or gradient pitch below the width the entry needs
    (KVH D for k, v, dk, dv; E for dq), dropout without a seed"""
    q, k, v, do = views(gqa_case(2, 5, 4, 2, 32))
    o, dq, dk, dv = (torch.empty(2, 5, 128, dtype=BF, device="cuda")
                     for _ in range(4))
    lse, delta = (torch.zeros(2, 4, 5, device="cuda") for _ in "01")
    lib = ops._lib.lib()

    def at(t, ld=None):
        return [t.data_ptr(), t.stride(1) if ld is None else ld]

    def calls(ldk=None, lddk=None, lddq=None, NH=4, KVH=2, p=0.0):
        ins = at(q) + at(k, ldk) + at(v)
        bwd = ins + at(do) + [lse.data_ptr(), delta.data_ptr()]
        tail = [2, 5, NH, KVH, 32, 0, None, p, 0, None]
        return (lib.hvk_gqa_fwd(*ins, *at(o), lse.data_ptr(), *tail),
                lib.hvk_gqa_bwd_dkv(*bwd, *at(dk, lddk), *at(dv), *tail),
                lib.hvk_gqa_bwd_dq(*bwd, *at(dq, lddq), *tail))
    assert calls() == (0, 0, 0)
    for bad in (dict(KVH=3), dict(KVH=0), dict(KVH=8), dict(ldk=63),
                dict(p=0.5)):
        assert all(c != 0 for c in calls(**bad)), bad
    assert calls(lddk=63)[1] != 0 and calls(lddq=127)[2] != 0
    torch.cuda.synchronize()
