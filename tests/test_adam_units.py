"""Adam, AdamW and RMSProp through the units: ``solvers=("adam",)`` on the GD
units, the parameter store's update number, clipping by the global gradient
norm (``root.common.engine.clip_gradient_norm``), resume, and HIP graphs.

The trajectories follow the same net in float64 torch with torch.optim and
``clip_grad_norm_`` to 6 digits of the loss."""
import os

import numpy
import pytest
import torch

from veles_amd import ops

HERE = os.path.dirname(os.path.abspath(__file__))
DIGITS = 1e-6


@pytest.fixture
def engine():
    """root.common.engine, with clip_gradient_norm put back afterwards."""
    from veles_amd.utils.config import root
    root.common.engine.clip_gradient_norm = 0.0
    yield root.common.engine
    root.common.engine.clip_gradient_norm = 0.0


def _workflow(layers, snap=None, epochs=None, **loader):
    from veles_amd.dummy import DummyLauncher
    from veles_amd.models import StandardWorkflow
    import veles_amd.loader  # noqa: F401
    cfg = {"steps": 4, "features": 8, "class_lengths": (0, 0, 32 * 20),
           "minibatch_size": 32, "seed": 3}
    cfg.update(loader)
    return StandardWorkflow(
        DummyLauncher(), loader_name="seq_recall", loader_config=cfg,
        layers=layers, decision_config={"max_epochs": epochs,
                                        "fail_iterations": 100},
        snapshotter_config=snap)


def _tiny(**gd):
    g = {"learning_rate": 1e-2}
    g.update(gd)
    return [{"type": "all2all_tanh", "->": {"output_sample_shape": 16},
             "<-": dict(g)},
            {"type": "softmax", "->": {"output_sample_shape": 8},
             "<-": dict(g)}]


def _sample_layers():
    """The layers and the clip of samples/seq_recall_adam_config.py."""
    from veles_amd.utils.config import root
    path = os.path.join(os.path.dirname(HERE), "samples",
                        "seq_recall_adam_config.py")
    with open(path) as f:
        exec(compile(f.read(), path, "exec"), {"root": root})
    clip = float(root.common.engine.clip_gradient_norm)
    root.common.engine.clip_gradient_norm = 0.0
    return [dict(la) for la in root.seq_recall.layers], clip


class TanhNet(torch.nn.Module):
    """all2all_tanh (1.7159 tanh(0.6666 x)) -> softmax, float64."""

    def __init__(self, f0, f1):
        super().__init__()
        self.a = torch.nn.Linear(*reversed(f0.weights.mem.shape)).double()
        self.b = torch.nn.Linear(*reversed(f1.weights.mem.shape)).double()
        with torch.no_grad():
            for lin, f in ((self.a, f0), (self.b, f1)):
                lin.weight.copy_(torch.from_numpy(f.weights.mem))
                lin.bias.copy_(torch.from_numpy(f.bias.mem))

    def forward(self, x):
        h = 1.7159 * torch.tanh(0.6666 * self.a(x.reshape(x.shape[0], -1)))
        return self.b(h)


class LstmNet(torch.nn.Module):
    """lstm -> softmax, float64 (the project's one LSTM bias is bias_ih)."""

    def __init__(self, f0, f1):
        super().__init__()
        H = f0.weights.mem.shape[0] // 4
        I = f0.weights.mem.shape[1] - H
        self.lstm = torch.nn.LSTM(I, H, batch_first=True).double()
        self.fc = torch.nn.Linear(H, f1.weights.mem.shape[0]).double()
        with torch.no_grad():
            w = torch.from_numpy(f0.weights.mem).double()
            self.lstm.weight_ih_l0.copy_(w[:, :I])
            self.lstm.weight_hh_l0.copy_(w[:, I:])
            self.lstm.bias_ih_l0.copy_(torch.from_numpy(f0.bias.mem))
            self.lstm.bias_hh_l0.zero_()
            self.fc.weight.copy_(torch.from_numpy(f1.weights.mem))
            self.fc.bias.copy_(torch.from_numpy(f1.bias.mem))
        self.lstm.bias_hh_l0.requires_grad_(False)

    def forward(self, x):
        y, _ = self.lstm(x)
        return self.fc(y[:, -1])


def _follow(wf, net, opt, steps, clip):
    """``steps`` minibatches through the workflow and through ``net`` in
    float64 on the same batches.  Returns (worst relative loss difference,
    the oracle's pre-clip gradient norms)."""
    params = [p for p in net.parameters() if p.requires_grad]
    worst, norms = 0.0, []
    B = wf.loader.max_minibatch_size
    for k in range(1, steps + 1):
        wf.run_steps(1)
        x = wf.loader.minibatch_data.devmem.double().clone()
        lab = wf.loader.minibatch_labels.devmem.long().clone()
        p = wf.forwards[-1].output.devmem.double()
        got = -torch.log(p[torch.arange(B), lab]).mean().item()
        loss = torch.nn.functional.cross_entropy(net(x), lab)
        d = abs(got - loss.item()) / abs(loss.item())
        worst = max(worst, d)
        opt.zero_grad()
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(
            params, clip if clip > 0 else float("inf"))))
        if clip > 0:
            mine = wf.param_store_.last_grad_norm()
            assert abs(mine - norms[-1]) <= 1e-5 * norms[-1], (mine, norms)
        opt.step()
        print("step %2d loss %.7f / %.7f, relative difference %.2e, "
              "gradient norm %.4f" % (k, got, loss.item(), d, norms[-1]))
    return worst, norms


# the clips sit inside the range of the 20 gradient norms of each net
@pytest.mark.parametrize("net,clip", [("tiny", 0.0), ("tiny", 0.45),
                                      ("lstm", 0.0), ("lstm", 0.2)])
def test_adam_trajectory_matches_float64_torch(engine, net, clip):
    from veles_amd.backends import Device
    from veles_amd.prng import random_generator
    engine.clip_gradient_norm = clip
    random_generator.get().seed(11)
    if net == "tiny":
        wf = _workflow(_tiny(solvers=("adam",)))
        make = TanhNet
    else:
        layers, sample_clip = _sample_layers()
        assert sample_clip == 1.0
        assert all(la["<-"]["solvers"] == ("adam",) for la in layers)
        engine.clip_gradient_norm = clip
        wf = _workflow(layers, steps=8, class_lengths=(0, 0, 64 * 20),
                       minibatch_size=64)
        make = LstmNet
    wf.initialize(device=Device(backend="cpu"))
    store = wf.param_store_
    assert store.clip_norm == clip
    ref = make(*wf.forwards)
    opt = torch.optim.Adam([p for p in ref.parameters() if p.requires_grad],
                           lr=1e-2, betas=(0.9, 0.999), eps=1e-8)
    worst, norms = _follow(wf, ref, opt, 20, clip)
    assert store.t0 == 0 and store.steps == 20
    assert worst <= DIGITS, worst
    if clip > 0:
        assert min(norms) < clip < max(norms), (clip, norms)


def test_momentum_with_clipping_takes_the_solver_path(engine):
    """An all-momentum table with clipping on: the solver path, matching
    float64 SGD with momentum after clip_grad_norm_."""
    from veles_amd.backends import Device
    from veles_amd.prng import random_generator
    clip = 0.45
    engine.clip_gradient_norm = clip
    random_generator.get().seed(11)
    wf = _workflow(_tiny(learning_rate=0.1, gradient_moment=0.9))
    wf.initialize(device=Device(backend="cpu"))
    store = wf.param_store_
    ref = TanhNet(*wf.forwards)
    opt = torch.optim.SGD(ref.parameters(), lr=0.1, momentum=0.9)
    worst, norms = _follow(wf, ref, opt, 20, clip)
    assert store._solver_segs is not None and store.t0 is None
    assert all(sg[6] == 0 for sg in store._solver_segs)
    assert worst <= DIGITS, worst
    assert min(norms) < clip < max(norms), (clip, norms)


@pytest.mark.parametrize("rule", ["adamw", "rmsprop"])
def test_adamw_and_rmsprop_units(engine, rule):
    """The other two rules through the units, with weight decay."""
    from veles_amd.backends import Device
    from veles_amd.prng import random_generator
    random_generator.get().seed(11)
    wf = _workflow(_tiny(solvers=(rule,), learning_rate=3e-3,
                         weights_decay=1e-2, weights_decay_bias=1e-2,
                         gradient_moment=0.5))
    wf.initialize(device=Device(backend="cpu"))
    ref = TanhNet(*wf.forwards)
    opt = torch.optim.AdamW(ref.parameters(), lr=3e-3, weight_decay=1e-2) \
        if rule == "adamw" else torch.optim.RMSprop(
            ref.parameters(), lr=3e-3, alpha=0.99, eps=1e-8,
            weight_decay=1e-2)
    worst, _ = _follow(wf, ref, opt, 20, 0.0)
    assert worst <= DIGITS, worst


def test_solver_names(engine):
    from veles_amd.backends import Device
    with pytest.raises(ValueError):
        _workflow(_tiny(solvers=("adam", "adagrad")))
    with pytest.raises(ValueError):
        _workflow(_tiny(solvers=("adamw", "adam")))
    with pytest.raises(ValueError):
        _workflow(_tiny(solvers=("rmsprop", "adadelta")))
    with pytest.raises(ValueError):
        _workflow(_tiny(solvers=("adamax",)))
    want = {("momentum",): (0, 0.0, 0.0),
            ("adagrad",): (1, 1e-8, 0.0),
            ("adadelta",): (2, 1e-8, 0.9),
            ("adagrad", "adadelta"): (2, 1e-8, 0.9),
            ("momentum", "adagrad", "fast"): (1, 1e-8, 0.0),
            ("adam",): (4, 1e-8, 0.999),
            ("adam", "momentum"): (4, 1e-8, 0.999),
            ("adamw",): (5, 1e-8, 0.999),
            ("rmsprop",): (6, 1e-8, 0.99)}
    for names, tup in want.items():
        wf = _workflow(_tiny(solvers=names, gradient_moment=0.7))
        wf.initialize(device=Device(backend="cpu"))
        for gd in wf.gds:
            assert gd.solver() == tup, names
            assert gd.solver_moment(0.7) == (
                0.9 if tup[0] in (4, 5) else 0.0 if tup[0] == 6 else 0.7)
    wf = _workflow(_tiny(solvers="adam", adam_beta1=0.8, adam_beta2=0.99,
                         adam_epsilon=1e-6))
    assert wf.gds[0].solver() == (4, 1e-6, 0.99)
    assert wf.gds[0].solver_moment(0.0) == 0.8


def test_switching_to_adam_starts_the_bias_correction(engine, monkeypatch):
    """Five momentum updates, then Adam: its first update is number 1."""
    from veles_amd.backends import Device
    wf = _workflow(_tiny(learning_rate=0.05, gradient_moment=0.9))
    wf.initialize(device=Device(backend="cpu"))
    store = wf.param_store_
    wf.run_steps(5)
    assert store.steps == 5 and store.t0 is None
    seen = []
    real = ops.solver_update

    def spy(*a, **kw):
        seen.append(kw.get("step"))
        return real(*a, **kw)
    monkeypatch.setattr(ops, "solver_update", spy)
    for gd in wf.gds:
        gd.solvers = {"adam"}
    wf.run_steps(2)
    assert seen == [1, 2] and store.t0 == 5 and store.steps == 7
    st = store.state_dict()
    assert st["t0"] == 5 and st["steps"] == 7 and st["mom2"].any()


def test_state_dict_restores_the_update_number(engine):
    """k updates, state_dict into a fresh store, the same gradients into
    both: the next update is bit-identical (steps, t0 and mom2 are back)."""
    from veles_amd.backends import Device
    from veles_amd.prng import random_generator
    engine.clip_gradient_norm = 0.45
    stores = []
    for k in (4, 0):
        random_generator.get().seed(11)
        wf = _workflow(_tiny(solvers=("adam",)))
        wf.initialize(device=Device(backend="cpu"))
        wf.run_steps(k) if k else wf.param_store_.finalize()
        stores.append(wf.param_store_)
    a, b = stores
    assert not torch.equal(a.master, b.master)
    b.load_state_dict(a.state_dict())
    assert (b.steps, b.t0) == (a.steps, a.t0) == (4, 0)
    g = torch.randn(a.total, generator=torch.Generator().manual_seed(1))
    for s in stores:
        s.grad.copy_(g)
        s.apply()
    assert a.steps == b.steps == 5
    for name in ("master", "mom", "mom2"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.last_grad_norm() == b.last_grad_norm() > 0.45


def test_snapshot_resume_is_bit_identical(engine, tmp_path):
    """k + m steps equal k steps, a snapshot, a fresh workflow from it and m
    more steps, bit for bit: steps, t0 and the second moments are restored."""
    from veles_amd.backends import Device
    from veles_amd.dummy import DummyLauncher
    from veles_amd.prng import random_generator
    from veles_amd.snapshotter import SnapshotterToFile
    from veles_amd.utils.config import root
    engine.clip_gradient_norm = 0.45
    snap = {"prefix": "adam", "directory": str(tmp_path), "interval": 1,
            "time_interval": 0, "compression": "gz"}
    root.common.disable.snapshotting = False
    random_generator.get().seed(11)
    wf = _workflow(_tiny(solvers=("adam",)), snap=snap, epochs=2,
                   class_lengths=(0, 32, 32 * 4))
    wf.initialize(device=Device(backend="cpu"))
    wf.run()
    k = wf.param_store_.steps
    assert k >= 4
    path = [os.path.join(tmp_path, f) for f in sorted(os.listdir(tmp_path))
            if "current" in f][0]
    wf2 = SnapshotterToFile.import_(path)
    wf2.workflow = DummyLauncher()
    wf2.initialize(device=Device(backend="cpu"))
    s1, s2 = wf.param_store_, wf2.param_store_
    s2.finalize()
    assert (s2.steps, s2.t0) == (s1.steps, s1.t0) == (k, 0)
    for name in ("master", "mom", "mom2"):
        assert torch.equal(getattr(s1, name), getattr(s2, name)), name
    for w in (wf, wf2):
        w.decision.max_epochs += 1
        w.decision.complete <<= False
        w.run_steps(3)
    assert s1.steps == s2.steps == k + 3
    for name in ("master", "mom", "mom2"):
        assert torch.equal(getattr(s1, name), getattr(s2, name)), name


@pytest.mark.gpu
def test_eager_and_graph_steps_agree_on_the_gpu(engine, monkeypatch):
    """Adam with clipping, deterministic kernels: 6 eager steps and 6 steps
    through HIP graphs (the table refreshed before every replay) end with
    bit-identical master weights."""
    from veles_amd.backends import Device
    from veles_amd.prng import random_generator
    engine.clip_gradient_norm = 0.45
    ops.set_deterministic(True)
    out = []
    try:
        for graphs in ("0", "1"):
            monkeypatch.setenv("VELES_AMD_GRAPHS", graphs)
            random_generator.get().seed(11)
            wf = _workflow(_tiny(solvers=("adam",)))
            wf.initialize(device=Device(backend="hip"))
            wf.run_steps(6)
            torch.cuda.synchronize()
            st = wf.param_store_
            segs = getattr(wf, "graph_segments_", None) or []
            replays = sum(s.replays for s in segs if s.name == "backward")
            assert (replays > 0) == (graphs == "1"), replays
            assert st.steps == 6 and st.t0 == 0
            norm = st.last_grad_norm()
            assert numpy.isfinite(norm) and norm > 0
            out.append((st.master.cpu().clone(), st.mom.cpu().clone(),
                        st.mom2.cpu().clone(), norm))
    finally:
        ops.set_deterministic(False)
    for a, b in zip(*out):
        assert (a == b) if isinstance(a, float) else torch.equal(a, b)
