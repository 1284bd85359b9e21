"""Batch normalisation through the units: the ``batch_norm*`` layer types in a
StandardWorkflow against float64 torch (``nn.BatchNorm2d``, same initial
weights), the train / evaluate rule, snapshots, Adam, and on the GPU HIP
graphs, exact resume and a float8 workflow.

The trajectories are held to the 6 digits of the loss that
tests/test_adam_units.py asks of its own."""
import pickle

import numpy
import pytest
import torch

from veles_amd import ops
from veles_amd.utils.config import root
from test_adam_units import DIGITS, _follow

G = {"learning_rate": 0.01, "learning_rate_bias": 0.01}
EPS, MOM = 1e-4, 0.2


def _layers(gd=None, n=8):
    g = dict(G)
    g.update(gd or {})
    return [
        # no conv bias: batch normalisation removes it, so its true gradient
        # is zero and Adam would turn the roundoff in its place into steps
        {"type": "conv", "->": {"n_kernels": n, "kx": 3, "ky": 3,
                                "padding": 1, "include_bias": False},
         "<-": dict(g)},
        {"type": "batch_norm_str", "->": {"eps": EPS, "momentum": MOM},
         "<-": dict(g)},
        {"type": "max_pooling", "->": {"kx": 2, "ky": 2, "sliding": 2}},
        {"type": "all2all", "->": {"output_sample_shape": 16}, "<-": dict(g)},
        {"type": "softmax", "->": {"output_sample_shape": 10}, "<-": dict(g)}]


def _workflow(layers, backend="cpu", lengths=(0, 0, 16 * 24), mb=16,
              dataset="mnist", epochs=None):
    from veles_amd.backends import Device
    from veles_amd.dummy import DummyLauncher
    from veles_amd.models import StandardWorkflow
    from veles_amd.ops import fp8
    from veles_amd.prng import random_generator
    import veles_amd.loader  # noqa: F401
    fp8._REGISTRIES.clear()
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
    wf.initialize(device=Device(backend=backend))
    return wf


class Net(torch.nn.Module):
    """conv -> BatchNorm2d -> strict ReLU -> 2x2 max pooling -> linear ->
    linear, float64, on the workflow's NHWC minibatches"""

    def __init__(self, fwds):
        super().__init__()
        conv, bn, _, fc, sm = fwds
        w = torch.from_numpy(conv.weights.mem)          # [OC][KH][KW][C]
        self.conv = torch.nn.Conv2d(w.shape[3], w.shape[0], 3, padding=1,
                                    bias=False).double()
        self.bn = torch.nn.BatchNorm2d(w.shape[0], eps=bn.eps,
                                       momentum=bn.momentum).double()
        self.fc = torch.nn.Linear(*reversed(fc.weights.mem.shape)).double()
        self.sm = torch.nn.Linear(*reversed(sm.weights.mem.shape)).double()
        with torch.no_grad():
            self.conv.weight.copy_(w.permute(0, 3, 1, 2))
            self.bn.weight.copy_(torch.from_numpy(bn.weights.mem))
            self.bn.bias.copy_(torch.from_numpy(bn.bias.mem))
            for lin, f in ((self.fc, fc), (self.sm, sm)):
                lin.weight.copy_(torch.from_numpy(f.weights.mem))
                lin.bias.copy_(torch.from_numpy(f.bias.mem))

    def forward(self, x):
        B = x.shape[0]
        x = x.reshape(B, x.shape[1], x.shape[2], -1).permute(0, 3, 1, 2)
        h = torch.relu(self.bn(self.conv(x)))
        h = torch.nn.functional.max_pool2d(h, 2)
        return self.sm(self.fc(h.permute(0, 2, 3, 1).reshape(B, -1)))


def test_defaults_are_torchs():
    wf = _workflow([{"type": "batch_norm", "<-": dict(G)},
                    {"type": "softmax", "->": {"output_sample_shape": 10},
                     "<-": dict(G)}])
    bn = wf.forwards[0]
    ref = torch.nn.BatchNorm2d(1)
    assert (bn.eps, bn.momentum) == (ref.eps, ref.momentum) == (1e-5, 0.1)
    assert (bn.weights.mem == 1).all() and (bn.bias.mem == 0).all()
    assert (bn.running_mean.mem == 0).all()
    assert (bn.running_var.mem == 1).all()
    assert bn.weights.mem.shape == (1,)


@pytest.mark.parametrize("solver", ["momentum", "adam"])
def test_trajectory_follows_float64_torch(solver):
    """20 steps; gamma, beta and the running statistics end where torch's
    do.  Step sizes at which the loss falls steadily (SGD 0.01, Adam at
    torch's default 0.001): at ten times those the loss of this net swings
    between 1 and 6 from step to step, and a trajectory that unstable
    multiplies the float32 roundoff of any layer (measured worst relative
    difference of the loss there: 1.0e-5 under SGD, 2.4e-5 under Adam)."""
    lr = 0.01 if solver == "momentum" else 1e-3
    gd = {"solvers": (solver,), "learning_rate": lr,
          "learning_rate_bias": lr}
    wf = _workflow(_layers(gd))
    bn = wf.forwards[1]
    assert bn.weights.mem.shape == (8,) and (bn.weights.mem == 1).all()
    ref = Net(wf.forwards)
    opt = torch.optim.SGD(ref.parameters(), lr=lr) if solver == "momentum" \
        else torch.optim.Adam(ref.parameters(), lr=lr)
    worst, _ = _follow(wf, ref, opt, 20, 0.0)
    assert worst <= DIGITS, worst
    rm, rv = bn.running_stats()
    for got, want in ((rm, ref.bn.running_mean), (rv, ref.bn.running_var),
                      (bn.weights_master, ref.bn.weight),
                      (bn.bias_master, ref.bn.bias)):
        assert torch.allclose(got.double(), want.detach(), rtol=1e-4,
                              atol=1e-5)
    assert not torch.equal(bn.weights_master, torch.ones(8))
    assert not torch.equal(bn.bias_master, torch.zeros(8))


def test_validation_uses_the_running_statistics_and_keeps_them(monkeypatch):
    wf = _workflow(_layers(), lengths=(0, 32, 64), epochs=2)
    bn = wf.forwards[1]
    seen = []
    real = ops.batchnorm_fwd

    def spy(x, g, b, rm, rv, **kw):
        before = [rm.clone(), rv.clone()]
        y = real(x, g, b, rm, rv, **kw)
        seen.append((int(bn.minibatch_class), kw["training"], before,
                     [rm.clone(), rv.clone()], x.clone(), y.clone(),
                     g.clone(), b.clone()))
        return y
    monkeypatch.setattr(ops, "batchnorm_fwd", spy)
    wf.run()
    classes = [s[0] for s in seen]
    assert 1 in classes and 2 in classes
    for mc, trained, before, after, x, y, g, b in seen:
        assert trained == (mc == 2)
        same = all(torch.equal(a, b) for a, b in zip(before, after))
        assert same == (mc != 2)
        if mc != 2:
            want = torch.relu(torch.nn.functional.batch_norm(
                x.double().permute(0, 3, 1, 2), before[0].double(),
                before[1].double(), g.double(), b.double(), False, MOM,
                EPS)).permute(0, 2, 3, 1)
            assert torch.allclose(y.double(), want, rtol=1e-5, atol=1e-5)
    # a testing workflow and forward_mode evaluate too
    wf.loader.minibatch_class = 2
    bn.forward_mode = True
    assert not bn.training()
    bn.forward_mode = False
    assert bn.training()
    wf.testing = True
    assert not bn.training()


def _state(wf):
    if wf.param_store_.master.is_cuda:
        torch.cuda.synchronize()
    out = [wf.param_store_.master.detach().cpu().clone()]
    for f in wf.forwards:
        if hasattr(f, "running_stats"):
            out += [t.detach().cpu().clone() for t in f.running_stats()]
    return out


def _resumed(layers, backend, k, m, **kw):
    from veles_amd.backends import Device
    from veles_amd.dummy import DummyLauncher
    wf = _workflow(layers, backend, **kw)
    wf.run_steps(k)
    blob = pickle.dumps(wf, protocol=pickle.HIGHEST_PROTOCOL)
    del wf
    wf2 = pickle.loads(blob)
    wf2.workflow = DummyLauncher()
    wf2.initialize(device=Device(backend=backend))
    wf2.run_steps(m)
    return wf2


def test_snapshot_resume_continues_exactly():
    a = _workflow(_layers({"gradient_moment": 0.9}))
    a.run_steps(7)
    b = _resumed(_layers({"gradient_moment": 0.9}), "cpu", 4, 3)
    bn = b.forwards[1]
    assert not (bn.running_mean.mem == 0).all()
    for x, y in zip(_state(a), _state(b)):
        assert torch.equal(x, y)


def test_extracted_forward_workflow_carries_the_running_statistics():
    from veles_amd.backends import Device
    wf = _workflow(_layers(), lengths=(0, 16, 64), epochs=2)
    wf.run()
    fw = wf.extract_forward_workflow(loader_config={
        "dataset": "mnist", "class_lengths": (32, 0, 0), "minibatch_size": 16,
        "seed": 5, "normalization_type": "mean_disp"})
    fw.initialize(device=Device(backend="cpu"))
    src, dst = wf.forwards[1], fw.forwards[1]
    assert numpy.abs(src.running_mean.mem).max() > 0
    for name in ("running_mean", "running_var", "weights", "bias"):
        assert numpy.array_equal(getattr(src, name).mem,
                                 getattr(dst, name).mem), name
    assert not dst.training()
    fw.run()
    out = numpy.array(fw.gather_results()["Output"])
    assert out.shape == (32, 10) and numpy.isfinite(out).all()
    for a, b in zip(dst.running_stats(), (src.running_mean.mem,
                                          src.running_var.mem)):
        assert numpy.array_equal(a.numpy(), b)


def test_bias_is_required_and_one_row_raises():
    with pytest.raises(ValueError):
        _workflow([{"type": "batch_norm", "->": {"include_bias": False},
                    "<-": dict(G)},
                   {"type": "softmax", "->": {"output_sample_shape": 10},
                    "<-": dict(G)}])
    wf = _workflow([{"type": "all2all", "->": {"output_sample_shape": 6},
                     "<-": dict(G)},
                    {"type": "batch_norm_tanh", "<-": dict(G)},
                    {"type": "softmax", "->": {"output_sample_shape": 10},
                     "<-": dict(G)}], lengths=(0, 0, 4), mb=1)
    with pytest.raises(ValueError):
        wf.run_steps(1)


def _fp8_layers():
    def conv(n):
        return {"type": "conv", "->": {"n_kernels": n, "kx": 3, "ky": 3,
                                       "padding": 1}, "<-": dict(G)}
    bn = {"type": "batch_norm_str", "<-": dict(G)}
    return [conv(16), dict(bn), conv(32), dict(bn),
            {"type": "max_pooling", "->": {"kx": 2, "ky": 2, "sliding": 2}},
            {"type": "all2all", "->": {"output_sample_shape": 64},
             "<-": dict(G)},
            {"type": "batch_norm_tanh", "<-": dict(G)},
            {"type": "softmax", "->": {"output_sample_shape": 10},
             "<-": dict(G)}]


def _fp8_case(backend):
    """A float8 workflow: the fp8 conv and the fp8 all2all above a batch
    normalisation quantise their bf16 input themselves (nothing wrote their
    e4m3 copy for them), and the net trains."""
    old = root.common.engine.precision_type
    root.common.engine.precision_type = "float8"
    try:
        wf = _workflow(_fp8_layers(), backend, lengths=(0, 0, 32 * 8), mb=32,
                       dataset="cifar10")
        f = wf.forwards
        # (a thin all2all stays on the bf16 GEMM on the GPU: FP8_MIN_TILES)
        assert f[2].fp8_ and (f[5].fp8_ or backend == "hip")
        quantized = []
        from veles_amd.ops import fp8
        real = fp8.quantize

        def spy(x, *a, **kw):
            quantized.append(x)
            return real(x, *a, **kw)
        fp8.quantize = spy
        try:
            wf.run_steps(4)
        finally:
            fp8.quantize = real
        assert not f[2].x8_fresh_
        bn_out = f[1].output.devmem
        assert any(q is bn_out for q in quantized)
        assert bn_out.dtype == (torch.bfloat16 if backend == "hip"
                                else torch.float32)
        for t in _state(wf):
            assert torch.isfinite(t).all()
        assert not torch.equal(f[1].weights_master.cpu(), torch.ones(16))
    finally:
        root.common.engine.precision_type = old


def test_float8_consumers_quantise_their_own_input_cpu():
    _fp8_case("cpu")


# --------------------------------------------------------------------- GPU
def _gpu_layers():
    la = _layers({"gradient_moment": 0.9}, n=16)
    la.insert(4, {"type": "batch_norm_tanh", "<-": dict(G)})
    return la


@pytest.mark.gpu
def test_eager_and_graph_trajectories_are_bit_identical(monkeypatch):
    ops.set_deterministic(True)
    out = []
    try:
        for graphs in ("0", "1"):
            monkeypatch.setenv("VELES_AMD_GRAPHS", graphs)
            wf = _workflow(_gpu_layers(), "hip", dataset="cifar10")
            wf.run_steps(6)
            torch.cuda.synchronize()
            segs = getattr(wf, "graph_segments_", None) or []
            replays = sum(s.replays for s in segs)
            assert (replays > 0) == (graphs == "1"), replays
            assert all(getattr(u, "graph_safe", True) for u in wf.forwards)
            out.append(_state(wf))
    finally:
        ops.set_deterministic(False)
    assert len(out[0]) == 5
    for a, b in zip(*out):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    assert not (out[0][1] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("graphs", [False, True])
def test_resume_is_bit_identical_on_the_gpu(graphs):
    old = root.common.engine.graphs
    root.common.engine.graphs = graphs
    ops.set_deterministic(True)
    try:
        a = _workflow(_gpu_layers(), "hip", dataset="cifar10")
        a.run_steps(6)
        ref = _state(a)
        got = _state(_resumed(_gpu_layers(), "hip", 3, 3, dataset="cifar10"))
    finally:
        ops.set_deterministic(False)
        root.common.engine.graphs = old
    for x, y in zip(ref, got):
        assert torch.equal(x, y)


@pytest.mark.gpu
def test_float8_consumers_quantise_their_own_input_gpu():
    _fp8_case("hip")
