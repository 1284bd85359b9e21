"""The ``attention`` layer type in a StandardWorkflow (docs/OPS.md
"Attention"): layout and filling of its parameters, a 20-step Adam trajectory
against float64 torch, snapshot / resume, pickling, the unsupported head
widths, and (GPU) eager against graphs."""
import pickle

import numpy
import pytest
import torch

from test_adam_units import _follow, _workflow

T, I, E = 5, 32, 32


def _layers(heads=1, causal=False, E=E, **gd):
    g = {"solvers": ("adam",), "learning_rate": 1e-3,
         "learning_rate_bias": 1e-3}
    g.update(gd)
    return [{"type": "attention", "->": {"output_sample_shape": E,
                                         "heads": heads, "causal": causal},
             "<-": dict(g)},
            {"type": "softmax", "->": {"output_sample_shape": 8},
             "<-": dict(g)}]


def _wf(layers, backend="cpu", seed=11, **loader):
    from veles_amd.backends import Device
    from veles_amd.prng import random_generator
    random_generator.get().seed(seed)
    cfg = {"steps": T, "features": I}
    cfg.update(loader)
    wf = _workflow(layers, **cfg)
    wf.initialize(device=Device(backend=backend))
    return wf


class Net(torch.nn.Module):
    """MultiheadAttention + Linear in float64, the weights copied through the
    documented layout: weights = (in_proj_weight, out_proj.weight), bias =
    (in_proj_bias, out_proj.bias)"""

    def __init__(self, fwds, heads, causal):
        super().__init__()
        att, sm = fwds
        E = att.width
        self.causal = causal
        self.mha = torch.nn.MultiheadAttention(
            E, heads, bias=True, dropout=0.0, batch_first=True).double()
        self.fc = torch.nn.Linear(*reversed(sm.weights.mem.shape)).double()
        w = torch.from_numpy(att.weights.mem)
        b = torch.from_numpy(att.bias.mem)
        n = 3 * E * E
        with torch.no_grad():
            self.mha.in_proj_weight.copy_(w[:n].view(3 * E, E))
            self.mha.out_proj.weight.copy_(w[n:].view(E, E))
            self.mha.in_proj_bias.copy_(b[:3 * E])
            self.mha.out_proj.bias.copy_(b[3 * E:])
            self.fc.weight.copy_(torch.from_numpy(sm.weights.mem))
            self.fc.bias.copy_(torch.from_numpy(sm.bias.mem))

    def forward(self, x):
        n = x.shape[1]
        mask = torch.ones(n, n).triu(1).bool() if self.causal else None
        y, _ = self.mha(x, x, x, attn_mask=mask, need_weights=False)
        return self.fc(y.reshape(x.shape[0], -1))


def test_layer_type_parameters_and_filling():
    from veles_amd.models import (LAYER_TYPES, LSTM, Attention, GDAttention)
    assert LAYER_TYPES["attention"] == (Attention, GDAttention)
    assert Attention.MAPPING == "attention"
    assert Attention.__id__ != LSTM.__id__
    assert GDAttention.OVERWRITES_GRADS
    wf = _wf(_layers(heads=2, E=64), features=8)
    att = wf.forwards[0]
    assert (att.heads, att.causal, att.width) == (2, False, 64)
    assert att.weights.mem.shape == (3 * 64 * 8 + 64 * 64,)
    assert att.bias.mem.shape == (4 * 64,) and (att.bias.mem == 0).all()
    assert tuple(att.output.shape) == (32, T, 64)
    w = att.weights.mem
    n = 3 * 64 * 8
    # the uniform rule with fan-in I for W_in and E for W_o
    assert 0.9 * 8 ** -0.5 < numpy.abs(w[:n]).max() <= 8 ** -0.5
    assert 0.9 * 64 ** -0.5 < numpy.abs(w[n:]).max() <= 64 ** -0.5
    w0, b0 = att.weights_master.clone(), att.bias_master.clone()
    wf.run_steps(2)
    assert wf.gds[0].err_input.devmem is None       # need_err_input False
    assert torch.isfinite(att.weights_master).all()
    assert (att.weights_master[:n] != w0[:n]).any()
    assert (att.weights_master[n:] != w0[n:]).any()
    assert (att.bias_master[:64] != b0[:64]).any()   # b_q
    assert (att.bias_master[192:] != b0[192:]).any()  # b_o


def test_stacked_attention_passes_the_error_down():
    layers = _layers(heads=1, E=32)
    layers.insert(0, {"type": "all2all_tanh",
                      "->": {"output_sample_shape": (T, 32)},
                      "<-": dict(layers[0]["<-"])})
    wf = _wf(layers, features=8)
    w0 = wf.forwards[0].weights_master.clone()
    wf.run_steps(2)
    assert tuple(wf.gds[1].err_input.shape) == (32, T, 32)
    assert (wf.forwards[0].weights_master != w0).any()


@pytest.mark.parametrize("heads,causal", ((1, False), (1, True)))
def test_trajectory_follows_float64_torch(heads, causal):
    """20 Adam steps (lr 1e-3) of (T, 32) -> attention(32) -> softmax(8) on
    the CPU device against MultiheadAttention + Linear in float64 torch from
    the same initial weights and batches.  Measured worst relative difference
    of the loss over the 20 steps: 7.6e-9 (plain) and 1.1e-8 (causal), eight
    digits; asserted with a factor 10 of margin, 1.1e-7.  The trained
    parameters are held to 1e-5, a hundredth of one Adam step of 1e-3
    (measured: 7e-8)."""
    wf = _wf(_layers(heads, causal))
    net = Net(wf.forwards, heads, causal)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    worst, _ = _follow(wf, net, opt, 20, 0.0)
    print("worst relative loss difference %.2e" % worst)
    assert worst <= 1.1e-7, worst
    att = wf.forwards[0]
    n = 3 * E * E
    # b_k is left out: a shift of every key moves all scores of a row alike,
    # so its true gradient is zero and Adam turns the roundoff in its place
    # into steps
    bm, bt = att.bias_master.double(), net.mha.in_proj_bias.detach()
    for name, got, want in (
            ("W_in", att.weights_master[:n], net.mha.in_proj_weight),
            ("W_o", att.weights_master[n:], net.mha.out_proj.weight),
            ("b_q", bm[:E], bt[:E]), ("b_v", bm[2 * E:3 * E], bt[2 * E:]),
            ("b_o", bm[3 * E:], net.mha.out_proj.bias)):
        d = (got.double().view(-1) - want.detach().reshape(-1)).abs().max()
        print(name, "max difference %.2e" % d)
        assert d <= 1e-5, (name, d)


def _state(wf):
    if wf.param_store_.master.is_cuda:
        torch.cuda.synchronize()
    return wf.param_store_.master.detach().cpu().clone()


def _resumed(backend, k, m, **kw):
    from veles_amd.backends import Device
    from veles_amd.dummy import DummyLauncher
    wf = _wf(_layers(heads=1, causal=True), backend, **kw)
    wf.run_steps(k)
    blob = pickle.dumps(wf, protocol=pickle.HIGHEST_PROTOCOL)
    del wf
    wf2 = pickle.loads(blob)
    wf2.workflow = DummyLauncher()
    wf2.initialize(device=Device(backend=backend))
    att = wf2.forwards[0]
    assert (att.heads, att.causal, att.width) == (1, True, E)
    wf2.run_steps(m)
    return wf2


def test_snapshot_resume_continues_exactly():
    a = _wf(_layers(heads=1, causal=True))
    a.run_steps(7)
    b = _resumed("cpu", 4, 3)
    assert torch.equal(_state(a), _state(b))


def test_unsupported_head_width_raises_on_every_device():
    with pytest.raises(ValueError, match=r"\[32, 64, 128\]"):
        _wf(_layers(heads=2, E=32))                 # D = 16
    with pytest.raises(ValueError, match=r"\[32, 64, 128\]"):
        _wf(_layers(heads=1, E=48))
    with pytest.raises(ValueError):
        _wf(_layers(heads=3, E=64))                 # 64 / 3
    from veles_amd.dummy import DummyLauncher
    from veles_amd.models import Attention
    with pytest.raises(ValueError):
        Attention(DummyLauncher(), output_sample_shape=64,
                  weights_transposed=True)


@pytest.mark.gpu
def test_eager_and_graphs_agree_over_three_steps(monkeypatch):
    from veles_amd import ops
    ops.set_deterministic(True)
    states = []
    try:
        for graphs in ("0", "1"):
            monkeypatch.setenv("VELES_AMD_GRAPHS", graphs)
            wf = _wf(_layers(heads=1, causal=True), backend="hip")
            wf.run_steps(3)
            torch.cuda.synchronize()
            segs = getattr(wf, "graph_segments_", None) or []
            # two warm-up passes run eagerly; the third is captured and run
            # from the graph (a replay proper would be the fourth)
            captures = sum(s.captures for s in segs)
            assert (captures > 0) == (graphs == "1"), captures
            assert not any(s.failures for s in segs)
            assert torch.isfinite(wf.forwards[-1].output.devmem.float()).all()
            states.append(_state(wf))
    finally:
        ops.set_deterministic(False)
    assert torch.equal(states[0], states[1])
