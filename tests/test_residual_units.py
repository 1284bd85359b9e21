"""Residual connections through the units: ``skip`` / ``layer_norm`` (with
``residual=``) / ``residual`` layers in a StandardWorkflow against float64
torch autograd on the same weights and the same minibatch.

Gradient of one step: learning rate 1, no momentum, no weight decay, so the
first update is exactly w1 = w0 - g on the float32 masters (the method of
tests/test_alexnet_bench_scale_gpu.py).  EVERY layer's weight and bias
gradient is compared:

* the layer below a ``skip`` gets err_output + every consumer's skip
  gradient; with the fan-in dropped its gradient is wrong (shown below by
  dropping it);
* the tanh layer below a residual consumer keeps its own derivative: the
  consumer's err_input doubles as the skip gradient, so a derivative fused
  into it would reach the skip branch too.

CPU tolerance: the float32 path against float64, per tensor
||g - g64|| <= 1e-4 ||g64||.  A float32 dot product of n = 784 terms is off
by at most gamma(n) ~ 5e-5 of the sum of its absolute terms and the
difference w0 - w1 adds U |w| / |g| ~ 1e-5 for |w| ~ 100 |g|; both are worst
cases that random signs do not reach, and a dropped fan-in or a wrongly
placed derivative is off by tens of per cent.

GPU tolerance: the bf16 noise floor as tests/test_alexnet_bench_scale_gpu.py
words it: the float64 reference run again with every layer's output and
back-propagated error rounded to bf16 at the layer boundaries gives r_floor
per tensor; the HIP step must stay within 1.5 r_floor + 0.02 and point the
same way (cosine >= the floor's - 0.05)."""
import pickle

import numpy
import pytest
import torch
import torch.nn.functional as F

from veles_amd import ops

LR1 = {"learning_rate": 1.0, "learning_rate_bias": 1.0,
       "gradient_moment": 0.0, "gradient_moment_bias": 0.0,
       "weights_decay": 0.0, "weights_decay_bias": 0.0}
TRAIN = {"learning_rate": 0.01, "learning_rate_bias": 0.01,
         "gradient_moment": 0.9, "gradient_moment_bias": 0.9}


def a2a(n, gd):
    return {"type": "all2all_tanh", "->": {"output_sample_shape": n},
            "<-": dict(gd)}


def sm(gd):
    return {"type": "softmax", "->": {"output_sample_shape": 10},
            "<-": dict(gd)}


def ln(gd, residual=None, **kw):
    fwd = dict(kw)
    if residual:
        fwd["residual"] = residual
    return {"type": "layer_norm", "->": fwd, "<-": dict(gd)}


def skip(name):
    return {"type": "skip", "name": name}


def res(name):
    return {"type": "residual", "->": {"residual": name}}


def post_ln(gd, n=16):
    return [a2a(n, gd), skip("s"), a2a(n, gd), ln(gd, "s"), sm(gd)]


def pre_ln(gd, n=16):
    return [a2a(n, gd), skip("s"), ln(gd), a2a(n, gd), res("s"), sm(gd)]


def two_consumers(gd, n=16):
    return [a2a(n, gd), skip("s"), a2a(n, gd), res("s"), a2a(n, gd),
            ln(gd, "s"), sm(gd)]


def nested(gd, n=16):
    return [a2a(n, gd), skip("a"), a2a(n, gd), skip("b"), a2a(n, gd),
            res("b"), ln(gd, "a", eps=1e-3), sm(gd)]


def skip_first(gd, n=16):
    return [skip("s"), ln(gd, "s"), a2a(n, gd), sm(gd)]


NETS = {"post_ln": post_ln, "pre_ln": pre_ln, "two_consumers": two_consumers,
        "nested": nested, "skip_first": skip_first}


def _workflow(layers, backend="cpu", lengths=(0, 0, 16 * 8), mb=16,
              epochs=None, init=True):
    # a skip at layer 0 marks the images themselves: cifar10's 3 channels
    # (mnist's single one would leave layer_norm nothing to normalise)
    dataset = "cifar10" if layers[0]["type"] == "skip" else "mnist"
    from veles_amd.backends import Device
    from veles_amd.dummy import DummyLauncher
    from veles_amd.models import StandardWorkflow
    from veles_amd.prng import random_generator
    import veles_amd.loader  # noqa: F401
    random_generator.get().seed(17)
    numpy.random.seed(17)
    torch.manual_seed(17)
    wf = StandardWorkflow(
        DummyLauncher(), loader_name="synthetic_images",
        loader_config={"dataset": dataset, "class_lengths": lengths,
                       "minibatch_size": mb, "normalization_type":
                       "mean_disp", "seed": 5, "noise": 110.0,
                       "generate_on_device": False},
        layers=layers, decision_config={"max_epochs": epochs,
                                        "fail_iterations": None})
    if init:
        wf.initialize(device=Device(backend=backend))
    return wf


class _RoundBF16(torch.autograd.Function):
    """bf16 storage of an activation (forward) and of its error (backward)"""

    @staticmethod
    def forward(ctx, x):
        return x.bfloat16().double()

    @staticmethod
    def backward(ctx, g):
        return g.bfloat16().double()


def reference(wf, params, x, emu=False):
    """float64 logits of the workflow's layer list on minibatch x"""
    rb = _RoundBF16.apply if emu else (lambda t: t)
    kept = {}
    h = rb(x.double())
    B = h.shape[0]
    for layer, f in zip(wf.layers, wf.forwards):
        typ = layer["type"]
        if typ == "skip":
            kept[f.name] = h
            continue
        if typ == "residual":
            h = rb(h + kept[f.residual])
            continue
        w, b = params[f.name + ".w"], params[f.name + ".b"]
        if typ == "layer_norm":
            s = h if f.residual is None else h + kept[f.residual]
            h = rb(F.layer_norm(s, (s.shape[-1],), w, b, f.eps))
            continue
        h = F.linear(h.reshape(B, -1), w, b)
        if typ == "all2all_tanh":
            h = rb(1.7159 * torch.tanh(0.6666 * h))
        else:
            assert typ == "softmax"
    return h


def weighted(wf):
    return [f for f in wf.forwards if getattr(f, "_pw_", None) is not None]


def weights_of(wf, lp=False):
    """float64 copies of the parameters the step computes with (``lp``: the
    all2all layers multiply with the bf16 copy of their weights)"""
    out = {}
    for f in weighted(wf):
        w = f.weights_master.detach().cpu()
        if lp and w.dim() == 2:
            w = w.bfloat16()
        out[f.name + ".w"] = w.double()
        out[f.name + ".b"] = f.bias_master.detach().cpu().double()
    return out


def one_step_gradients(wf):
    """(g = w0 - w1 per tensor, the minibatch, its labels) of one step"""
    first = wf.forwards[0]
    seen = {}
    cls = type(first)
    orig = cls.run

    def spy(unit):
        if unit is first:
            seen["x"] = unit.input.devmem.detach().cpu().clone()
            seen["labels"] = \
                wf.loader.minibatch_labels.devmem.detach().cpu().clone()
        return orig(unit)
    w0 = weights_of(wf)
    cls.run = spy
    try:
        wf.run_steps(1)
    finally:
        cls.run = orig
    if wf.param_store_.master.is_cuda:
        torch.cuda.synchronize()
    assert wf.param_store_.steps == 1
    w1 = weights_of(wf)
    return {k: w0[k] - w1[k] for k in w0}, seen["x"], seen["labels"]


def reference_gradients(wf, params, x, labels, emu=False):
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    logits = reference(wf, p, x, emu)
    B = logits.shape[0]
    F.cross_entropy(logits, labels[:B].long()).backward()
    return {k: v.grad.detach() for k, v in p.items()}


def relative(got, want):
    return {k: float((got[k] - want[k]).norm() / (want[k].norm() + 1e-300))
            for k in want}


CPU_TOL = 1e-4


@pytest.mark.parametrize("net", sorted(NETS))
def test_every_gradient_matches_float64_autograd(net):
    wf = _workflow(NETS[net](LR1))
    params = weights_of(wf)
    got, x, labels = one_step_gradients(wf)
    want = reference_gradients(wf, params, x, labels)
    rel = relative(got, want)
    print(net, {k: "%.1e" % v for k, v in rel.items()})
    assert len(rel) == 2 * len(weighted(wf)) >= 6
    for k, v in want.items():
        assert float(v.norm()) > 0, k
        assert rel[k] <= CPU_TOL, (k, rel[k])
    # structure: the chain is linear, one GD unit per layer, nothing fused
    # into a tensor that doubles as a skip gradient
    from veles_amd.graphs import _is_chain
    from veles_amd.models import GDLayerNorm, GDResidual, GDSkip
    assert len(wf.gds) == len(wf.forwards) == len(wf.layers)
    assert _is_chain(list(reversed(wf.gds)))
    for i, gd in enumerate(wf.gds):
        if isinstance(gd, (GDLayerNorm, GDResidual, GDSkip)):
            assert gd.fused_aux is None and not gd.fused_aux_act
            if i:
                assert wf.gds[i - 1].own_derivative
    if net == "skip_first":
        assert not wf.gds[0].need_err_input
        assert wf.gds[0].err_input.devmem is None
        assert wf.forwards[0].output.devmem is wf.forwards[0].input.devmem


@pytest.mark.parametrize("net", ["post_ln", "pre_ln"])
def test_a_dropped_fan_in_is_seen_below_the_skip(net, monkeypatch):
    """GDSkip passing err_output on alone: the gradients of the layer below
    the skip leave the tolerance, those above it stay inside"""
    from veles_amd.models import GDSkip

    def no_fan_in(self):
        self.err_input.devmem = self.err_output.devmem
    monkeypatch.setattr(GDSkip, "run", no_fan_in)
    wf = _workflow(NETS[net](LR1))
    params = weights_of(wf)
    got, x, labels = one_step_gradients(wf)
    rel = relative(got, reference_gradients(wf, params, x, labels))
    below = wf.forwards[0].name
    for k, v in rel.items():
        assert (v > 100 * CPU_TOL) == k.startswith(below + "."), (k, v)


def test_a_derivative_fused_into_the_shared_tensor_is_seen():
    """the tanh layer below ``residual`` with its derivative left to the
    unit above (which does not apply it): its gradients leave the
    tolerance"""
    wf = _workflow(pre_ln(LR1))
    i = [type(f).__name__ for f in wf.forwards].index("Residual")
    wf.gds[i - 1].own_derivative = False
    params = weights_of(wf)
    got, x, labels = one_step_gradients(wf)
    rel = relative(got, reference_gradients(wf, params, x, labels))
    assert rel[wf.forwards[i - 1].name + ".w"] > 100 * CPU_TOL


def test_defaults_are_torchs_and_the_parameters_live_in_the_store():
    wf = _workflow(post_ln(TRAIN))
    f = wf.forwards[3]
    ref = torch.nn.LayerNorm(16)
    assert f.eps == ref.eps == 1e-5
    assert f.weights.mem.shape == (16,) and (f.weights.mem == 1).all()
    assert (f.bias.mem == 0).all()
    assert type(wf.gds[3]).OVERWRITES_GRADS
    assert not hasattr(f, "training")
    wf.run_steps(3)
    assert not torch.equal(f.weights_master, torch.ones(16))
    assert not torch.equal(f.bias_master, torch.zeros(16))
    assert nested(TRAIN)[6]["->"]["eps"] == 1e-3
    assert _workflow(nested(TRAIN)).forwards[6].eps == 1e-3


@pytest.mark.parametrize("layers,what", [
    ([a2a(16, LR1), skip("s"), a2a(16, LR1), ln(LR1, "t"), sm(LR1)],
     "no layer"),
    ([a2a(16, LR1), ln(LR1, "s"), skip("s"), a2a(16, LR1), res("s"),
      sm(LR1)], "later"),
    ([dict(a2a(16, LR1), name="s"), a2a(16, LR1), ln(LR1, "s"), sm(LR1)],
     "not a skip"),
    ([a2a(16, LR1), skip("s"), a2a(16, LR1), sm(LR1)], "no later layer"),
    ([a2a(16, LR1), skip("s"), a2a(16, LR1), {"type": "residual"}, sm(LR1)],
     "names its skip"),
    # a later layer under its default name (type + index)
    ([a2a(16, LR1), ln(LR1, "skip2"), {"type": "skip"}, a2a(16, LR1),
      res("skip2"), sm(LR1)], "later"),
])
def test_wrong_residual_names_raise_at_construction(layers, what):
    with pytest.raises(ValueError, match=what):
        _workflow(layers, init=False)


@pytest.mark.parametrize("consumer", [ln, lambda gd, name: res(name)])
def test_a_shape_mismatch_raises_at_initialize(consumer):
    layers = [a2a(16, LR1), skip("s"), a2a(24, LR1), consumer(LR1, "s"),
              sm(LR1)]
    wf = _workflow(layers, init=False)            # construction passes
    from veles_amd.backends import Device
    with pytest.raises(ValueError, match="skip tensor"):
        wf.initialize(device=Device(backend="cpu"))


@pytest.mark.gpu
@pytest.mark.parametrize("consumer", [ln, lambda gd, name: res(name)])
def test_a_shape_mismatch_raises_at_initialize_on_the_gpu(consumer):
    layers = [a2a(64, LR1), skip("s"), a2a(128, LR1), consumer(LR1, "s"),
              sm(LR1)]
    wf = _workflow(layers, init=False)
    from veles_amd.backends import Device
    with pytest.raises(ValueError, match="skip tensor"):
        wf.initialize(device=Device(backend="hip"))


def _state(wf):
    weighted(wf)[0].ensure_params()
    if wf.param_store_.master.is_cuda:
        torch.cuda.synchronize()
    return [wf.param_store_.master.detach().cpu().clone()]


def _resumed(layers, backend, k, m):
    from veles_amd.backends import Device
    from veles_amd.dummy import DummyLauncher
    wf = _workflow(layers, backend)
    wf.run_steps(k)
    blob = pickle.dumps(wf, protocol=pickle.HIGHEST_PROTOCOL)
    del wf
    wf2 = pickle.loads(blob)
    wf2.workflow = DummyLauncher()
    wf2.initialize(device=Device(backend=backend))
    wf2.run_steps(m)
    return wf2


@pytest.mark.parametrize("net", ["post_ln", "nested"])
def test_snapshot_resume_continues_exactly(net):
    a = _workflow(NETS[net](TRAIN))
    w0 = _state(a)[0]
    a.run_steps(7)
    b = _resumed(NETS[net](TRAIN), "cpu", 4, 3)
    assert not torch.equal(w0, _state(a)[0])
    for x, y in zip(_state(a), _state(b)):
        assert torch.equal(x, y)
    # the links survive the pickle
    i = [type(f).__name__ for f in b.forwards].index("LayerNorm")
    assert b.forwards[i].skip_unit in b.forwards
    assert b.forwards[i] in b.forwards[i].skip_unit.consumers


@pytest.mark.parametrize("net", ["post_ln", "pre_ln"])
def test_extracted_forward_workflow_reproduces_the_trained_outputs(net):
    from veles_amd.backends import Device
    wf = _workflow(NETS[net](TRAIN), lengths=(0, 16, 64), epochs=2)
    wf.run()
    fw = wf.extract_forward_workflow(loader_config={
        "dataset": "mnist", "class_lengths": (32, 0, 0), "minibatch_size": 16,
        "seed": 5, "normalization_type": "mean_disp"})
    fw.initialize(device=Device(backend="cpu"))
    for src, dst in zip(weighted(wf), weighted(fw)):
        assert numpy.array_equal(src.weights.mem, dst.weights.mem)
        assert numpy.array_equal(src.bias.mem, dst.bias.mem)
    assert not (weighted(wf)[1].weights.mem == 1).all() or net == "post_ln"
    fw.run()
    out = numpy.array(fw.gather_results()["Output"])
    assert out.shape == (32, 10) and numpy.isfinite(out).all()
    # the last minibatch, through float64 torch with the TRAINED weights
    x = fw.forwards[0].input.devmem.detach().clone()
    want = torch.softmax(reference(wf, weights_of(wf), x), 1)
    got = fw.forwards[-1].output.devmem.double()
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-5


# --------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("net", ["post_ln", "pre_ln"])
def test_both_graph_segments_are_installed(net):
    wf = _workflow(NETS[net](TRAIN, 64), "hip")
    assert sorted(s.name for s in wf.graph_segments_) == ["backward",
                                                          "forward"]
    wf.run_steps(6)
    torch.cuda.synchronize()
    assert all(s.replays > 0 for s in wf.graph_segments_)


@pytest.mark.gpu
@pytest.mark.parametrize("net", ["post_ln", "pre_ln", "two_consumers"])
def test_eager_and_graph_trajectories_are_bit_identical(net, monkeypatch):
    ops.set_deterministic(True)
    out = []
    try:
        for graphs in ("0", "1"):
            monkeypatch.setenv("VELES_AMD_GRAPHS", graphs)
            wf = _workflow(NETS[net](TRAIN, 64), "hip")
            w0 = _state(wf)[0]
            wf.run_steps(6)
            torch.cuda.synchronize()
            segs = getattr(wf, "graph_segments_", None) or []
            replays = sum(s.replays for s in segs)
            assert (replays > 0) == (graphs == "1"), replays
            out.append(_state(wf))
            assert not torch.equal(w0, out[-1][0])
    finally:
        ops.set_deterministic(False)
    for a, b in zip(*out):
        assert torch.isfinite(a).all() and torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("net", sorted(NETS))
def test_gpu_gradients_stay_within_the_bf16_floor(net):
    wf = _workflow(NETS[net](LR1, 64), "hip")
    params = weights_of(wf, lp=True)
    got, x, labels = one_step_gradients(wf)
    x = x.bfloat16()
    ref = reference_gradients(wf, params, x, labels)
    emu = reference_gradients(wf, params, x, labels, emu=True)

    def cos(a, b):
        return float((a * b).sum() / (a.norm() * b.norm() + 1e-300))
    rows = []
    for k in ref:
        n = float(ref[k].norm()) + 1e-300
        rows.append((k, float((got[k] - ref[k]).norm()) / n,
                     float((emu[k] - ref[k]).norm()) / n,
                     cos(got[k], ref[k]), cos(emu[k], ref[k])))
    print(net, "per tensor: relative error HIP / bf16 floor, cosine HIP / "
          "floor")
    for r in rows:
        print("  %-20s %.4f / %.4f   %.4f / %.4f" % r)
    for k, r_hip, r_flo, c_hip, c_flo in rows:
        assert r_hip <= 1.5 * r_flo + 0.02 and c_hip >= c_flo - 0.05, \
            "%s: HIP %.4f vs bf16 floor %.4f, cosine %.4f vs %.4f" % (
                k, r_hip, r_flo, c_hip, c_flo)
