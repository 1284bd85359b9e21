"""The attention kernels with dropout on the weights (hvk_adrop_*) through the
oracle, bounds and mask read-out of tests/test_attention_dropout.py, on bf16.
T in {1, TK - 1, TK + 1, TQ + 1}: the sweep-tile and owner-tile edges.  The worst
|error| / bound goes to profiles/attention/dropout_gpu_tests_figures.txt."""
import os

import pytest
import torch

from veles_amd import ops
from test_attention_dropout import (NAMES, READOUT, check_drop, check_readout,
                                    check_resume, run_core)
from test_attention_gpu import fused
from test_attention_ref import make_case
from test_step_tail_ref import BF, Ratios, same_bits

pytestmark = pytest.mark.gpu
FIGURES = os.path.join(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))), "profiles", "attention",
    "dropout_gpu_tests_figures.txt")
TQ, TK = ops.ATTN_TQ, ops.ATTN_TK
WORST = Ratios()


@pytest.fixture(scope="module", autouse=True)
def figures():
    yield
    os.makedirs(os.path.dirname(FIGURES), exist_ok=True)
    with open(FIGURES, "w") as f:
        f.write("# worst |error| / bound per quantity over "
                "tests/test_attention_dropout_gpu.py\n")
        f.writelines("%-8s %.4f\n" % kv for kv in sorted(WORST.items()))


def seed_tensor(v):
    return torch.tensor([v], dtype=torch.int32, device="cuda")


def run_gpu(case, NH, causal, **kw):
    return run_core([t.to("cuda", BF) for t in case], NH, causal, **kw)


@pytest.mark.parametrize("T,D,causal,base_row", READOUT)
def test_mask_readout(T, D, causal, base_row):
    check_readout(T, D, causal, base_row, 77, True, lambda *a, **kw: run_gpu(
        *a, seed_dev=seed_tensor(77), **kw))


@pytest.mark.parametrize("p", (0.1, 0.5))
@pytest.mark.parametrize("causal", (False, True))
@pytest.mark.parametrize("T,D,pad", [(T, D, 0) for T in (1, TK - 1, TK + 1,
                                                         TQ + 1)
                                     for D in (32, 64, 128)] + [(TK + 1, 64, 1)])
def test_general_within_the_bound(T, D, pad, causal, p):
    """pad 1: a pitch 2 bytes and a base 8 bytes off the 16-byte grid, the
    element path"""
    case = make_case(1, T, 2, D, seed=3)
    kw = dict(dropout=p, seed_dev=seed_tensor(1234 + T))
    if pad:
        (q, k, v), do, _, _ = fused(case, pad, 4)
        got = run_core((q, k, v, do), 2, causal, **kw)
    else:
        got = run_gpu(case, 2, causal, **kw)
    r = Ratios()
    check_drop(r, got, case, 2, causal, p, 1234 + T, True, tk=TK)
    print((T, D, pad, causal, p), {k: round(v, 4) for k, v in r.items()})
    WORST.merge(r)


def test_off_is_off_and_the_seed_decides():
    case = make_case(2, TQ + 1, 2, 64, seed=6)
    sd = seed_tensor(4321)
    a, b = run_gpu(case, 2, True), run_gpu(case, 2, True, dropout=0.0,
                                           seed_dev=sd)
    c, d = (run_gpu(case, 2, True, dropout=0.5, seed_dev=sd) for _ in "01")
    for n in NAMES:
        assert same_bits(a[n], b[n]) and same_bits(c[n], d[n]), n
    ops.seed_advance(sd)
    nxt = ops.seed_advance_ref(4321)
    assert int(sd.cpu()[0]) & 0xFFFFFFFF == nxt != 4321
    check_readout(33, 64, False, 0, nxt, True,
                  lambda *a, **kw: run_gpu(*a, seed_dev=sd, **kw))
    assert not torch.equal(ops.attention_dropout_mask_ref(2, 3, 33, nxt, 0.5),
                           ops.attention_dropout_mask_ref(2, 3, 33, 4321, 0.5))
    fn, a = ops._lib.lib().hvk_adrop_fwd, [c["o"].data_ptr(), 128] * 4 + [
        c["lse"].data_ptr(), 2, TQ + 1, 2, 64, 0]
    for seed, p in ((None, 0.5), (sd.data_ptr(), 1.0), (sd.data_ptr(), -0.1)):
        assert fn(*a, seed, p, 0, None) != 0      # rejected before a launch


def test_graph_replays_equal_eager_steps():
    """the step advances the device seed: two replays draw the two masks of
    two eager steps from the same starting seed"""
    (q, k, v), do, o, (dq, dk, dv) = fused(make_case(2, TQ + 1, 2, 64,
                                                     seed=8))
    sd, save = seed_tensor(0), {}
    kw = dict(causal=True, dropout=0.1, seed_dev=sd)

    def step():
        ops.seed_advance(sd)
        ops.attention_fwd(q, k, v, 2, out=o, save=save, **kw)
        ops.attention_bwd(do, q, k, v, o, save, 2, dq=dq, dk=dk, dv=dv,
                          ws=save, **kw)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()       # warm-up: every buffer of ``save`` exists now
    torch.cuda.current_stream().wait_stream(s)
    outs = [o, dq, dk, dv, save["lse"]]
    sd.fill_(555)
    eager = []
    for _ in "01":
        step()
        eager.append([t.clone() for t in outs])
    assert not torch.equal(eager[0][0], eager[1][0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    sd.fill_(555)
    for want in eager:
        for t in outs:
            t.fill_(3.0)
        graph.replay()
        torch.cuda.synchronize()
        assert all(same_bits(u, w) for u, w in zip(outs, want))


def test_unit_snapshot_resumes_the_device_mask_stream():
    ops.set_deterministic(True)
    try:
        check_resume("hip")
    finally:
        ops.set_deterministic(False)
