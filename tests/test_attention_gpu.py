"""The attention kernels (csrc/kernels/attention.hip) and the layer ops
around them against the float64 oracle of test_attention_ref.py, fed with the
GPU's own bf16 tensors; the full tensors are compared, each element with the
bound derived in that file's docstring (bf16 operands of the second products,
online softmax over key tiles of TK, half a bf16 ulp of every bf16 result).

Shapes: TQ = 128 rows a workgroup owns (32 per wave), TK = 32 rows of a swept
tile.  T in {1, 2, TK-1, TK, TK+1, TQ-1, TQ, TQ+1, 2 TQ+1}, causal and not,
meets the diagonal tile, a fully visible tile, a skipped tile, key and query
tails and more than one workgroup per (batch, head); T = TK + 1 with every
head width, 1 and 3 heads and 1 and 3 batch items meets the head and batch
offsets.  Sliced views of a fused [B*T][3E] buffer take the 16-byte vector
path; a base 8 bytes off the 16-byte grid, or a pitch off it, the element
path.  q = k and v = an identity pattern are there for transposed operands;
everything else is independent Gaussians.

The spiked cases carry one score near 120 (above ln FLT_MAX = 88.7) in the
first key tile, in the last of three, and on the diagonal under the causal
mask, so the running maximum jumps at a chosen tile.

The worst |error| / bound per quantity goes to
profiles/attention/gpu_tests_figures.txt."""
import os

import numpy as np
import pytest
import torch

from veles_amd import ops
from test_attention_ref import (check_core, check_mha, make_case, mha_case,
                                oracle, run_mha, spike_case)
from test_step_tail_ref import BF, Ratios, f64, same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIGURES = os.path.join(ROOT, "profiles", "attention", "gpu_tests_figures.txt")
TQ, TK = ops.ATTN_TQ, ops.ATTN_TK
WORST = Ratios()


@pytest.fixture(scope="module", autouse=True)
def figures():
    yield
    if not WORST:
        return
    os.makedirs(os.path.dirname(FIGURES), exist_ok=True)
    with open(FIGURES, "w") as f:
        f.write("# worst |error| / bound per quantity over "
                "tests/test_attention_gpu.py\n")
        for k in sorted(WORST):
            f.write("%-8s %.4f\n" % (k, WORST[k]))


def test_tile_sizes_are_the_kernels():
    lib = ops._lib.lib()
    assert (lib.hvk_attn_tile(0), lib.hvk_attn_tile(1)) == (TQ, TK)


def fused(case, pad=0, shift=0):
    """q, k, v as column slices of one [B][T][3E + pad] bf16 buffer whose
    base is ``shift`` elements off an allocation; do and the gradient buffer
    likewise"""
    q, k, v, do = case
    B, T, E = q.shape
    dev = torch.device("cuda")
    W = 3 * E + pad

    def buf(w):
        flat = torch.zeros(B * T * w + shift, dtype=BF, device=dev)
        return flat[shift:].view(B, T, w)
    qkv, g = buf(W), buf(W)
    for n, t in enumerate((q, k, v)):
        qkv[:, :, n * E:(n + 1) * E].copy_(t)
    d = buf(E + pad)
    d[:, :, :E].copy_(do)
    o = buf(E + pad)
    views = [qkv[:, :, n * E:(n + 1) * E] for n in range(3)]
    grads = [g[:, :, n * E:(n + 1) * E] for n in range(3)]
    return views, d[:, :, :E], o[:, :, :E], grads


def run_core_gpu(case, NH, causal, pad=0, shift=0):
    (q, k, v), do, o, (dq, dk, dv) = fused(case, pad, shift)
    save = {}
    ops.attention_fwd(q, k, v, NH, causal=causal, out=o, save=save)
    ops.attention_bwd(do, q, k, v, o, save, NH, causal=causal, dq=dq, dk=dk,
                      dv=dv)
    torch.cuda.synchronize()
    return {"o": o, "lse": save["lse"], "dq": dq, "dk": dk, "dv": dv}


def check(tag, case, NH, causal, got, ref=None):
    r = Ratios()
    for t in got.values():
        assert torch.isfinite(t).all(), tag
    check_core(r, "", got, case, NH, causal, True, tk=TK, ref=ref)
    print(tag, tuple(case[0].shape), "NH", NH, "causal", causal,
          {k: round(v, 4) for k, v in r.items()})
    WORST.merge(r)


@pytest.mark.parametrize("causal", (False, True))
@pytest.mark.parametrize("T", (1, 2, TK - 1, TK, TK + 1, TQ - 1, TQ, TQ + 1,
                               2 * TQ + 1))
def test_tile_edges(T, causal):
    case = make_case(1, T, 1, 64)
    check("edges", case, 1, causal, run_core_gpu(case, 1, causal))


@pytest.mark.parametrize("causal", (False, True))
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("NH", (1, 3))
@pytest.mark.parametrize("D", (32, 64, 128))
def test_head_widths_and_counts(D, NH, B, causal):
    case = make_case(B, TK + 1, NH, D)
    check("heads", case, NH, causal, run_core_gpu(case, NH, causal))


@pytest.mark.parametrize("causal", (False, True))
@pytest.mark.parametrize("pad,shift", ((0, 0), (0, 4), (4, 0), (1, 0)))
def test_vector_and_element_paths(pad, shift, causal):
    """(0, 0): every base and pitch on the 16-byte grid; shift 4: bases 8
    bytes off it; pad 4 / 1: pitches 8 / 2 bytes off it"""
    case = make_case(2, TQ + 1, 2, 32, seed=2)
    got = run_core_gpu(case, 2, causal, pad, shift)
    on_grid = got["o"].data_ptr() % 16 == 0 and got["o"].stride(1) % 8 == 0
    assert on_grid == (pad == 0 and shift == 0)
    check("paths", case, 2, causal, got)


@pytest.mark.parametrize("causal", (False, True))
def test_layout_q_equals_k_and_identity_v(causal):
    T, D = TK + 1, 64
    q, k, v, do = make_case(1, T, 1, D, seed=4)
    case = (q, q.clone(), v, do)
    check("q=k", case, 1, causal, run_core_gpu(case, 1, causal))
    eye = torch.zeros(1, T, D)
    eye[0, torch.arange(T), torch.arange(T) % D] = 1.0
    case = (q, k, eye, do)
    check("v=I", case, 1, causal, run_core_gpu(case, 1, causal))


@pytest.mark.parametrize("causal,qi,kj", ((False, 5, 3), (False, 5, 90),
                                          (True, 40, 40)))
def test_spiked_score_forces_the_rescale(causal, qi, kj):
    """3 key tiles; the spike sits in the first, in the last, and on the
    diagonal"""
    T = 3 * TK
    case = spike_case(T, 64, qi, kj)
    ref = oracle(*(f64(t) for t in case), 1, causal)
    assert ref["S"][0, 0, qi, kj] > 100.0
    check("spike", case, 1, causal, run_core_gpu(case, 1, causal), ref=ref)


def test_two_runs_give_identical_bits():
    case = make_case(2, 2 * TQ + 1, 2, 64, seed=6)
    a = run_core_gpu(case, 2, True)
    b = run_core_gpu(case, 2, True)
    for name in ("o", "lse", "dq", "dk", "dv"):
        assert same_bits(a[name], b[name]), name


def to_gpu(x, w, b, err):
    dev = torch.device("cuda")
    return x.to(dev, BF), w.to(dev, BF), b.to(dev), err.to(dev, BF)


@pytest.mark.parametrize("causal", (False, True))
@pytest.mark.parametrize("B,T,I,E,NH", ((2, TK + 1, 8, 64, 2),
                                        (1, TQ + 1, 64, 64, 1),
                                        (3, 9, 40, 96, 3)))
def test_mha_layer_ops(B, T, I, E, NH, causal):
    case = mha_case(B, T, I, E)
    x, w, b, err = to_gpu(*case)
    ops.set_deterministic(True)
    try:
        got = run_mha(x, w, b, err, I, E, NH, causal)
        torch.cuda.synchronize()
        r = Ratios()
        check_mha(r, "mha_", got, *case, I, E, NH, causal, True, tk=TK)
        print("mha", (B, T, I, E, NH), causal,
              {k: round(v, 4) for k, v in r.items()})
        WORST.merge(r)
        # accumulate=True adds to what the buffers hold ("overwrite" wrote
        # over the 7s); no err_input on request
        g2 = (got["dw"].clone(), got["db"].clone())
        got2 = run_mha(x, w, b, err, I, E, NH, causal, accumulate=True,
                       need_err_input=False, grads=g2)
        torch.cuda.synchronize()
        assert "dx" not in got2
        for n in ("dw", "db"):
            a, c = f64(got2[n]), 2 * f64(got[n])
            assert np.abs(a - c).max() <= 2.0 ** -22 * np.abs(c).max(), n
    finally:
        ops.set_deterministic(False)


def test_graph_replay_equals_eager():
    """forward + backward captured once as one linear chain, replayed five
    times"""
    B, T, I, E, NH = 2, TQ + 1, 64, 64, 2
    x, w, b, err = to_gpu(*mha_case(B, T, I, E, seed=8))
    w_in, w_out = w[:3 * E * I].view(3 * E, I), w[3 * E * I:].view(E, E)
    dev = x.device
    dw = torch.zeros(3 * E * I + E * E, device=dev)
    db = torch.zeros(4 * E, device=dev)
    y = torch.empty(B, T, E, dtype=BF, device=dev)
    ei = torch.empty(B, T, I, dtype=BF, device=dev)
    save = {}
    ops.set_deterministic(True)
    try:
        def step():
            ops.mha_fwd(x, w_in, w_out, b, NH, causal=True, save=save, out=y)
            ops.mha_bwd(err, x, w_in, w_out, save,
                        dw[:3 * E * I].view(3 * E, I),
                        dw[3 * E * I:].view(E, E), db, NH, causal=True,
                        err_input=ei)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            step()       # warm-up: every buffer of ``save`` exists now
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        kept = {k: t.data_ptr() for k, t in save.items()}
        step()
        torch.cuda.synchronize()
        assert kept == {k: t.data_ptr() for k, t in save.items()}
        names = ("qkv", "o", "lse", "do", "dqkv", "delta")
        eager = [t.clone() for t in [y, ei, dw, db] + [save[n] for n in names]]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step()
        for _ in range(5):
            for t in [y, ei, dw, db] + [save[n] for n in names]:
                t.fill_(3.0)
            graph.replay()
            torch.cuda.synchronize()
            got = [y, ei, dw, db] + [save[n] for n in names]
            for u, v in zip(got, eager):
                assert torch.equal(u, v)
    finally:
        ops.set_deterministic(False)


def test_host_checks_raise_before_any_launch():
    dev = torch.device("cuda")
    q, k, v, do = (t.to(dev, BF) for t in make_case(2, 5, 2, 32))
    with pytest.raises(TypeError):
        ops.attention_fwd(q.float(), k.float(), v.float(), 2)
    with pytest.raises(ValueError):
        ops.attention_fwd(q, k.cpu(), v, 2)
    with pytest.raises(ValueError, match=r"\[32, 64, 128\]"):
        ops.attention_fwd(q, k, v, 4)
    with pytest.raises(ValueError):
        ops.attention_fwd(q, k, v, 2, out=torch.empty(2, 5, 64, dtype=BF))
    lib = ops._lib.lib()
    lse = torch.empty(2, 2, 5, device=dev)
    o = torch.empty_like(q)
    p = [q.data_ptr(), 64, k.data_ptr(), 64, v.data_ptr(), 64, o.data_ptr(),
         64, lse.data_ptr()]
    # the entry points themselves: shapes, D, pitches, the 2^31 limit
    assert lib.hvk_attn_fwd(*p, 2, 5, 2, 16, 0, None) != 0
    assert lib.hvk_attn_fwd(*p, 0, 5, 2, 32, 0, None) != 0
    assert lib.hvk_attn_fwd(*(p[:1] + [32] + p[2:]), 2, 5, 2, 32, 0,
                            None) != 0
    assert lib.hvk_attn_fwd(*p, 1 << 20, 1 << 6, 2, 32, 0, None) != 0
    assert lib.hvk_attn_fwd(*(p[:8] + [None]), 2, 5, 2, 32, 0, None) != 0
    torch.cuda.synchronize()
