"""The ``ffn`` layer type in a StandardWorkflow (docs/OPS.md "Position-wise
feed-forward"): layout and filling of its parameters, the error passed down
and up, a post-LN block around it, a 20-step Adam trajectory against float64
torch, pickle resume, bad kwargs, and (GPU) eager against graphs."""
import pickle

import numpy
import pytest
import torch

from test_adam_units import _follow, _workflow

T, I, E, H = 5, 32, 32, 64


def _gd(**gd):
    g = {"solvers": ("adam",), "learning_rate": 1e-3,
         "learning_rate_bias": 1e-3}
    g.update(gd)
    return g


def _layers(act="gelu", E=E, hidden=H, **gd):
    return [{"type": "ffn", "->": {"output_sample_shape": E, "hidden": hidden,
                                   "activation": act}, "<-": _gd(**gd)},
            {"type": "softmax", "->": {"output_sample_shape": 8},
             "<-": _gd(**gd)}]


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
    """Sequential(Linear, GELU, Linear) + Linear in float64, the weights
    copied through the documented layout: weights = (W1, W2), bias = (b1,
    b2)"""

    def __init__(self, fwds, act):
        super().__init__()
        ffn, sm = fwds
        F_, E_, I_ = ffn.hidden, ffn.width, ffn.n_in
        self.l1 = torch.nn.Linear(I_, F_).double()
        self.l2 = torch.nn.Linear(F_, E_).double()
        self.act = torch.nn.GELU(
            approximate="tanh" if act == "gelu_tanh" else "none")
        self.fc = torch.nn.Linear(*reversed(sm.weights.mem.shape)).double()
        w = torch.from_numpy(ffn.weights.mem)
        b = torch.from_numpy(ffn.bias.mem)
        n = F_ * I_
        with torch.no_grad():
            self.l1.weight.copy_(w[:n].view(F_, I_))
            self.l2.weight.copy_(w[n:].view(E_, F_))
            self.l1.bias.copy_(b[:F_])
            self.l2.bias.copy_(b[F_:])
            self.fc.weight.copy_(torch.from_numpy(sm.weights.mem))
            self.fc.bias.copy_(torch.from_numpy(sm.bias.mem))

    def forward(self, x):
        y = self.l2(self.act(self.l1(x)))
        return self.fc(y.reshape(x.shape[0], -1))


def test_layer_type_parameters_and_filling():
    from veles_amd.models import (LAYER_TYPES, Attention, FeedForward,
                                  GDFeedForward)
    from veles_amd.models.standard_workflow import _FUSABLE
    assert LAYER_TYPES["ffn"] == (FeedForward, GDFeedForward)
    assert FeedForward.MAPPING == "ffn"
    assert FeedForward.__id__ != Attention.__id__
    assert GDFeedForward.OVERWRITES_GRADS
    assert GDFeedForward in _FUSABLE
    wf = _wf(_layers(E=16, hidden=64), features=8)
    ffn = wf.forwards[0]
    assert (ffn.width, ffn.hidden, ffn.act, ffn.n_in) == (16, 64, "gelu", 8)
    assert ffn.weights.mem.shape == (64 * 8 + 16 * 64,)
    assert ffn.bias.mem.shape == (64 + 16,) and (ffn.bias.mem == 0).all()
    assert tuple(ffn.output.shape) == (32, T, 16)
    w = ffn.weights.mem
    n = 64 * 8
    # the uniform rule with fan-in I for W1 and F for W2
    assert 0.9 * 8 ** -0.5 < numpy.abs(w[:n]).max() <= 8 ** -0.5
    assert 0.9 * 64 ** -0.5 < numpy.abs(w[n:]).max() <= 64 ** -0.5
    w0, b0 = ffn.weights_master.clone(), ffn.bias_master.clone()
    wf.run_steps(2)
    assert wf.gds[0].err_input.devmem is None       # need_err_input False
    assert torch.isfinite(ffn.weights_master).all()
    assert (ffn.weights_master[:n] != w0[:n]).any()
    assert (ffn.weights_master[n:] != w0[n:]).any()
    assert (ffn.bias_master[:64] != b0[:64]).any()   # b1
    assert (ffn.bias_master[64:] != b0[64:]).any()   # b2


def test_defaults_follow_the_input_width():
    wf = _wf([{"type": "ffn", "<-": _gd()},
              {"type": "softmax", "->": {"output_sample_shape": 8},
               "<-": _gd()}], features=8)
    ffn = wf.forwards[0]
    assert (ffn.width, ffn.hidden) == (8, 32)
    assert tuple(ffn.output.shape) == (32, T, 8)


def test_flat_samples_work_too():
    """[B][I] input: an all2all below turns (T, 8) into (24,)"""
    layers = _layers(E=16, hidden=24)
    layers.insert(0, {"type": "all2all", "->": {"output_sample_shape": 24},
                      "<-": _gd()})
    wf = _wf(layers, features=8)
    wf.run_steps(2)
    assert tuple(wf.forwards[1].output.shape) == (32, 16)
    assert tuple(wf.gds[1].err_input.shape) == (32, 24)


def test_ffn_under_and_over_other_layers_passes_the_error_down():
    """all2all_tanh -> ffn -> ffn -> softmax: the upper ffn's err_input feeds
    the lower one, and the lower one's err_input GEMM carries the tanh
    derivative of the layer below (fused aux_act)"""
    layers = _layers(E=32, hidden=48) + []
    layers.insert(0, {"type": "ffn", "->": {"hidden": 40,
                                            "activation": "str"},
                      "<-": _gd()})
    layers.insert(0, {"type": "all2all_tanh",
                      "->": {"output_sample_shape": (T, 32)}, "<-": _gd()})
    wf = _wf(layers, features=8)
    assert wf.gds[1].fused_aux is wf.forwards[0]
    assert wf.gds[1].fused_aux_act and not wf.gds[0].own_derivative
    assert wf.gds[2].fused_aux is None          # an ffn's output is linear
    w0 = [f.weights_master.clone() for f in wf.forwards]
    wf.run_steps(2)
    assert tuple(wf.gds[2].err_input.shape) == (32, T, 32)
    assert tuple(wf.gds[1].err_input.shape) == (32, T, 32)
    for f, w in zip(wf.forwards, w0):
        assert (f.weights_master != w).any(), f.name


def _block(**gd):
    g = _gd(**gd)
    return [{"type": "all2all", "->": {"output_sample_shape": (T, 32)},
             "<-": dict(g)},
            {"type": "skip", "name": "b"},
            {"type": "ffn", "->": {"hidden": 64}, "<-": dict(g)},
            {"type": "layer_norm", "->": {"residual": "b"}, "<-": dict(g)},
            {"type": "softmax", "->": {"output_sample_shape": 8},
             "<-": dict(g)}]


def test_block_with_skip_and_layer_norm_runs_and_matches_autograd():
    """skip b -> ffn -> layer_norm(residual=b): one step's gradients on the
    CPU device against float64 autograd"""
    wf = _wf(_block(), features=8)
    f0, _, ffn, ln, sm = wf.forwards
    w = {k: torch.from_numpy(u.weights.mem.copy()).double().requires_grad_()
         for k, u in (("a", f0), ("f", ffn), ("n", ln), ("s", sm))}
    b = {k: torch.from_numpy(u.bias.mem.copy()).double().requires_grad_()
         for k, u in (("a", f0), ("f", ffn), ("n", ln), ("s", sm))}
    wf.run_steps(1)
    x = wf.loader.minibatch_data.devmem.double()
    lab = wf.loader.minibatch_labels.devmem.long()
    B = x.shape[0]
    a = (x.reshape(B, -1) @ w["a"].t() + b["a"]).view(B, T, 32)
    n = 64 * 32
    u = a @ w["f"][:n].view(64, 32).t() + b["f"][:64]
    y = torch.nn.functional.gelu(u) @ w["f"][n:].view(32, 64).t() + b["f"][64:]
    z = torch.nn.functional.layer_norm(y + a, (32,), w["n"], b["n"], 1e-5)
    logits = z.reshape(B, -1) @ w["s"].t() + b["s"]
    torch.nn.functional.cross_entropy(logits, lab).backward()
    for k, unit in (("a", f0), ("f", ffn), ("n", ln), ("s", sm)):
        for what, p, t in (("weights", unit._pw_, w[k]),
                           ("bias", unit._pb_, b[k])):
            got = p.grad.double().reshape(-1)
            want = t.grad.reshape(-1)
            # the store's gradient is of the summed loss over the batch or of
            # its mean: compare directions and scale in one go
            s = float(got @ want / (want @ want))
            d = float((got - s * want).abs().max() / (s * want).abs().max())
            print(unit.name, what, "scale %.6g relative %.2e" % (s, d))
            assert d <= 1e-5, (unit.name, what, d)


@pytest.mark.parametrize("act", ("gelu", "gelu_tanh"))
def test_trajectory_follows_float64_torch(act):
    """20 Adam steps (lr 1e-3) of (5, 32) -> ffn(32, hidden 64) ->
    softmax(8) on the CPU device against Linear-GELU-Linear + Linear in
    float64 torch from the same initial weights and batches.  Measured worst
    relative difference of the loss over the 20 steps: 9.8e-9 (gelu) and
    1.4e-8 (gelu_tanh); asserted with a factor 10 of margin (BOUND).  The
    trained parameters are held to 1e-5, a hundredth of one Adam step of
    1e-3 (measured: 6.2e-8)."""
    wf = _wf(_layers(act))
    net = Net(wf.forwards, act)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    worst, _ = _follow(wf, net, opt, 20, 0.0)
    print("worst relative loss difference %.2e" % worst)
    assert worst <= BOUND[act], worst
    ffn = wf.forwards[0]
    n = H * I
    bm = ffn.bias_master.double()
    for name, got, want in (
            ("W1", ffn.weights_master[:n], net.l1.weight),
            ("W2", ffn.weights_master[n:], net.l2.weight),
            ("b1", bm[:H], net.l1.bias), ("b2", bm[H:], net.l2.bias)):
        d = (got.double().view(-1) - want.detach().reshape(-1)).abs().max()
        print(name, "max difference %.2e" % d)
        assert d <= 1e-5, (name, d)


BOUND = {"gelu": 9.8e-8, "gelu_tanh": 1.4e-7}   # 10 x the measured values


def _state(wf):
    if wf.param_store_.master.is_cuda:
        torch.cuda.synchronize()
    return wf.param_store_.master.detach().cpu().clone()


def _resumed(backend, k, m):
    from veles_amd.backends import Device
    from veles_amd.dummy import DummyLauncher
    wf = _wf(_layers("gelu_tanh"), backend)
    wf.run_steps(k)
    blob = pickle.dumps(wf, protocol=pickle.HIGHEST_PROTOCOL)
    del wf
    wf2 = pickle.loads(blob)
    wf2.workflow = DummyLauncher()
    wf2.initialize(device=Device(backend=backend))
    ffn = wf2.forwards[0]
    assert (ffn.act, ffn.width, ffn.hidden) == ("gelu_tanh", E, H)
    wf2.run_steps(m)
    return wf2


def test_pickle_resume_continues_exactly():
    a = _wf(_layers("gelu_tanh"))
    a.run_steps(7)
    b = _resumed("cpu", 4, 3)
    assert torch.equal(_state(a), _state(b))


def test_bad_kwargs_raise():
    from veles_amd.dummy import DummyLauncher
    from veles_amd.models import FeedForward
    with pytest.raises(ValueError, match="unknown activation"):
        FeedForward(DummyLauncher(), activation="swish")
    with pytest.raises(ValueError, match="unknown activation"):
        _wf(_layers("relu"))
    with pytest.raises(ValueError, match="weights_transposed"):
        FeedForward(DummyLauncher(), weights_transposed=True)
    with pytest.raises(ValueError, match="hidden"):
        FeedForward(DummyLauncher(), hidden=0)
    with pytest.raises(ValueError, match="output_sample_shape"):
        FeedForward(DummyLauncher(), output_sample_shape=(4, 8))


@pytest.mark.gpu
def test_eager_and_graphs_agree_over_three_steps(monkeypatch):
    from veles_amd import ops
    ops.set_deterministic(True)
    states = []
    try:
        for graphs in ("0", "1"):
            monkeypatch.setenv("VELES_AMD_GRAPHS", graphs)
            wf = _wf(_block(), backend="hip", features=8)
            wf.run_steps(3)
            torch.cuda.synchronize()
            segs = getattr(wf, "graph_segments_", None) or []
            # two warm-up passes run eagerly; the third is captured and run
            # from the graph
            captures = sum(s.captures for s in segs)
            assert (captures > 0) == (graphs == "1"), captures
            if graphs == "1":
                assert len(segs) == 2       # forward and backward chains
            assert not any(s.failures for s in segs)
            assert torch.isfinite(wf.forwards[-1].output.devmem.float()).all()
            states.append(_state(wf))
    finally:
        ops.set_deterministic(False)
    assert torch.equal(states[0], states[1])
