"""Recurrent layers on the CPU reference device: ops.lstm_fwd / lstm_bwd
against torch.nn.LSTM / torch.nn.RNN in float64 (the oracle pins the gate
order i, f, g, o and the cell equations independently of this project's
code), the LSTM / RNN units in StandardWorkflow, and the host checks.

Tolerance: the float32 rounding bound of the reference loop, u = 2^-24,
gamma_n = n u / (1 - n u).

Forward, per step: the pre-activation is one sum of I + H + 1 products plus
the propagated error of h_{t-1},
    e_pre = gamma_{I+H+2} (|x_t| |Wx|^T + |b| + |h| |Wh|^T) + e_h |Wh|^T,
a gate errs by its Lipschitz constant (sigmoid 1/4, tanh 1) times e_pre plus
4 u for the function itself, and
    e_c = |c'| e_f + f e_c' + |g| e_i + i e_g + 3 u (|f c'| + |i g|),
    e_h = |tanh c| e_o + o (e_c + 4 u) + 2 u |h|.
Backward: every result is a sum of products of |err|, the gate factors,
|W| and |x| / |h| with non-negative coefficients, so (running error
analysis) it errs by at most gamma_n M', where M' is the same computation on
absolute values and n its longest chain, T (4H + 16) + B T + I + H; the
forward errors of the gate factors enter through M' - M, M' evaluated with
every factor raised by its forward bound.
"""
import numpy
import pytest
import torch

from veles_amd import ops

U = 2.0 ** -24
CELLS = {"lstm": 4, "rnn": 1}
SHAPES = [(1, 1, 1, 1), (3, 5, 6, 7), (4, 9, 8, 16), (2, 16, 3, 33)]
IDS = ["%dx%dx%dx%d" % s for s in SHAPES]


def gamma(n):
    return n * U / (1 - n * U)


def oracle(cell, x, w, b, I, H):
    m = (torch.nn.LSTM if cell == "lstm" else torch.nn.RNN)(
        I, H, batch_first=True).double()
    with torch.no_grad():
        m.weight_ih_l0.copy_(w[:, :I])
        m.weight_hh_l0.copy_(w[:, I:])
        m.bias_ih_l0.copy_(b)
        m.bias_hh_l0.zero_()
    return m


def forward_bound(cell, x, w, b, I, H):
    """float64 model of the loop with the per-step error bounds of the module
    docstring; returns a list of per-step dicts"""
    B, T, _ = x.shape
    wx, wh = w[:, :I], w[:, I:]
    h = torch.zeros(B, H, dtype=torch.float64)
    c, e_h, e_c = h.clone(), h.clone(), h.clone()
    steps = []
    for t in range(T):
        pre = x[:, t] @ wx.t() + b + h @ wh.t()
        e_pre = gamma(I + H + 2) * (x[:, t].abs() @ wx.abs().t() + b.abs() +
                                    h.abs() @ wh.abs().t()) + \
            e_h @ wh.abs().t()
        s = dict(hp=h, e_hp=e_h, cp=c, e_cp=e_c)
        if cell == "rnn":
            h = torch.tanh(pre)
            e_h = e_pre + 4 * U
            s.update(h=h, e_h=e_h)
            steps.append(s)
            continue
        p, e = pre.split(H, 1), e_pre.split(H, 1)
        gi, gf, go = (torch.sigmoid(p[k]) for k in (0, 1, 3))
        gg = torch.tanh(p[2])
        e_i, e_f, e_o = (0.25 * e[k] + 4 * U for k in (0, 1, 3))
        e_g = e[2] + 4 * U
        cn = gf * c + gi * gg
        e_c = c.abs() * e_f + gf * e_c + gg.abs() * e_i + gi * e_g + \
            3 * U * ((gf * c).abs() + (gi * gg).abs())
        c = cn
        tc = torch.tanh(c)
        h = go * tc
        e_h = tc.abs() * e_o + go * (e_c + 4 * U) + 2 * U * h.abs()
        s.update(i=gi, f=gf, g=gg, o=go, e_i=e_i, e_f=e_f, e_g=e_g, e_o=e_o,
                 c=c, e_c=e_c, tc=tc, e_tc=e_c + 4 * U, h=h, e_h=e_h)
        steps.append(s)
    return steps


def backward_magnitude(cell, steps, x, w, err, I, H, raised):
    """the backward on absolute values; ``raised``: every forward quantity
    plus its forward bound"""
    B, T, _ = x.shape
    wh, wx = w[:, I:].abs(), w[:, :I].abs()
    r = 1.0 if raised else 0.0
    dgs = [None] * T
    dc = torch.zeros(B, H, dtype=torch.float64)
    for t in range(T - 1, -1, -1):
        s = steps[t]
        dh = err[:, t].abs()
        if t < T - 1:
            dh = dh + dgs[t + 1] @ wh
        if cell == "rnn":
            # |1 - h^2| and its error 2 |h| e_h
            dgs[t] = dh * ((1 - s["h"] ** 2).abs() +
                           r * 2 * s["h"].abs() * s["e_h"])
            continue
        i, f, g, o = (s[k] + r * s["e_" + k] for k in "ifgo")
        g = s["g"].abs() + r * s["e_g"]
        tc = s["tc"].abs() + r * s["e_tc"]
        cp = s["cp"].abs() + r * s["e_cp"]
        one_tc2 = (1 - s["tc"] ** 2).abs() + r * 2 * s["tc"].abs() * s["e_tc"]
        one_g2 = (1 - s["g"] ** 2).abs() + r * 2 * s["g"].abs() * s["e_g"]

        def dsig(v, e):   # v (1 - v) and its error |1 - 2 v| e
            return v * (1 - v) + r * (1 - 2 * v).abs() * e
        dc = dc + dh * o * one_tc2
        dgs[t] = torch.cat((dc * g * dsig(s["i"], s["e_i"]),
                            dc * cp * dsig(s["f"], s["e_f"]),
                            dc * i * one_g2,
                            dh * tc * dsig(s["o"], s["e_o"])), 1)
        dc = dc * f
    dg = torch.stack(dgs, 1).reshape(B * T, -1)
    hp = torch.stack([s["hp"].abs() + r * s["e_hp"] for s in steps], 1)
    dw = torch.cat((dg.t() @ x.abs().reshape(B * T, I),
                    dg.t() @ hp.reshape(B * T, H)), 1)
    return dw, dg.sum(0), (dg @ wx).reshape(B, T, I)


def operands(cell, shape, seed=0):
    B, T, I, H = shape
    ng = CELLS[cell]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, I, generator=g)
    w = torch.randn(ng * H, I + H, generator=g) / (I + H) ** 0.5
    b = torch.randn(ng * H, generator=g) * 0.5
    return x, w, b


@pytest.mark.parametrize("seq", (False, True))
@pytest.mark.parametrize("cell", sorted(CELLS))
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_forward_and_backward_match_torch(shape, cell, seq):
    B, T, I, H = shape
    ng = CELLS[cell]
    x, w, b = operands(cell, shape)
    x64, w64, b64 = x.double(), w.double(), b.double()
    m = oracle(cell, x64, w64, b64, I, H)
    xd = x64.clone().requires_grad_()
    y, _ = m(xd)
    ref = y if seq else y[:, -1]
    save = {}
    out = ops.lstm_fwd(x, w, b, H, cell=cell, return_sequences=seq, save=save)
    assert out.shape == ref.shape and out.dtype == torch.float32
    steps = forward_bound(cell, x64, w64, b64, I, H)
    e_h = torch.stack([s["e_h"] for s in steps], 1)
    bound = e_h if seq else e_h[:, -1]
    r = ((out.double() - ref.detach()).abs() / bound).max().item()
    print("forward max err / bound %.3f" % r)
    assert r <= 1.0

    g = torch.Generator().manual_seed(7)
    err = torch.randn(ref.shape, generator=g)
    ref.backward(err.double())
    dw = torch.full((ng * H, I + H), 9.0)
    db = torch.full((ng * H,), 9.0)
    ei = ops.lstm_bwd(err, x, w, save, dw, db, cell=cell)
    e_full = torch.zeros(B, T, H, dtype=torch.float64)
    if seq:
        e_full.copy_(err)
    else:
        e_full[:, -1] = err
    m0 = backward_magnitude(cell, steps, x64, w64, e_full, I, H, False)
    m1 = backward_magnitude(cell, steps, x64, w64, e_full, I, H, True)
    n = T * (4 * H + 16) + B * T + I + H
    refs = (torch.cat((m.weight_ih_l0.grad, m.weight_hh_l0.grad), 1),
            m.bias_ih_l0.grad, xd.grad)
    for name, got, want, a, c in zip(("dw", "dbias", "err_input"),
                                     (dw, db, ei), refs, m0, m1):
        bound = gamma(n) * c + (c - a) + 1e-300
        r = ((got.double() - want).abs() / bound).max().item()
        print("%s max err / bound %.3f" % (name, r))
        assert r <= 1.0, name


def test_gradient_modes_agree():
    """accumulate adds to what is there, "overwrite" replaces it"""
    x, w, b = operands("lstm", (3, 5, 6, 7))
    err = torch.randn(3, 7)
    save = {}
    ops.lstm_fwd(x, w, b, 7, save=save)
    dw0, db0 = torch.full((28, 13), 5.0), torch.full((28,), 5.0)
    ops.lstm_bwd(err, x, w, save, dw0, db0, accumulate="overwrite")
    dw1, db1 = torch.zeros(28, 13), torch.zeros(28)
    ops.lstm_bwd(err, x, w, save, dw1, db1, accumulate=True)
    assert torch.equal(dw0, dw1) and torch.equal(db0, db1)
    ops.lstm_bwd(err, x, w, save, dw1, db1, accumulate=True,
                 need_err_input=False)
    torch.testing.assert_close(dw1, 2 * dw0, rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(db1, 2 * db0, rtol=1e-6, atol=1e-7)


def test_save_none_writes_no_gates():
    x, w, b = operands("lstm", (3, 5, 6, 7))
    ws = {}
    y = ops.lstm_fwd(x, w, b, 7, ws=ws)
    save = {}
    assert torch.equal(y, ops.lstm_fwd(x, w, b, 7, save=save))
    assert "gates" in save and "h" in ws
    h = ws["h"]
    ops.lstm_fwd(x, w, b, 7, ws=ws)
    assert ws["h"] is h       # buffers are reused


# (B, I, H, T): H = 7 is off the 8-element grid (on the GPU the scalar kernel
# path, padded pitch != width), H = 8 is on it (the vector path)
CONTRACT = [(3, 5, 7, 2), (2, 8, 8, 2)]


@pytest.mark.parametrize("cell", sorted(CELLS))
@pytest.mark.parametrize("shape", CONTRACT, ids=("H7", "H8"))
def test_save_contract(shape, cell):
    """what fwd + bwd leave in ``save`` under public keys (docs/OPS.md): the
    tools and the tests that launch steps by hand read these.  The CPU loop
    carries dc in a local, so "dc" is a GPU key only."""
    B, I, H, T = shape
    ng = CELLS[cell]
    x, w, b = operands(cell, (B, T, I, H))
    save = {}
    ops.lstm_fwd(x, w, b, H, cell=cell, save=save)
    ops.lstm_bwd(torch.randn(B, H), x, w, save, torch.zeros(ng * H, I + H),
                 torch.zeros(ng * H), cell=cell)
    want = {"h": (B, T, H), "xg": (B, T, ng * H), "dg": (B, T, ng * H)}
    if cell == "lstm":
        want.update(c=(B, T, H), gates=(B, T, 4 * H))
    assert {k for k in save if not k.startswith("_")} == set(want)
    for k, shape in want.items():
        assert tuple(save[k].shape) == shape, k
        assert save[k].dtype == torch.float32, k


@pytest.mark.parametrize("cell", sorted(CELLS))
def test_forward_is_the_default_direction(cell):
    B, T, I, H = 3, 5, 6, 7
    ng = CELLS[cell]
    x, w, b = operands(cell, (B, T, I, H))
    err = torch.randn(B, T, H)
    res = []
    for kw in ({}, {"direction": "forward"}):
        save = {}
        y = ops.lstm_fwd(x, w, b, H, cell=cell, return_sequences=True,
                         save=save, **kw)
        dw, db = torch.zeros(ng * H, I + H), torch.zeros(ng * H)
        ei = ops.lstm_bwd(err, x, w, save, dw, db, cell=cell, **kw)
        res.append((y, ei, dw, db))
    for a, c in zip(*res):
        assert torch.equal(a, c)
    for bad in (lambda: ops.lstm_fwd(x, w, b, H, cell=cell,
                                     direction="backward"),
                lambda: ops.lstm_bwd(err, x, w, save, dw, db, cell=cell,
                                     direction="backward")):
        with pytest.raises(ValueError) as e:
            bad()
        assert all(d in str(e.value) for d in ("forward", "reverse", "both"))


def test_host_checks():
    x, w, b = operands("lstm", (3, 5, 6, 7))
    for bad in (lambda: ops.lstm_fwd(x[0], w, b, 7),
                lambda: ops.lstm_fwd(x, w, b, 8),
                lambda: ops.lstm_fwd(x, w[:, :-1], b, 7),
                lambda: ops.lstm_fwd(x, w, b[:-1], 7),
                lambda: ops.lstm_fwd(x, w, b, 7, cell="gru"),
                lambda: ops.lstm_fwd(x.transpose(0, 1), w, b, 7),
                lambda: ops.lstm_fwd(x, w, b, 7, out=torch.zeros(3, 8))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        ops.lstm_fwd(x.long(), w, b, 7)
    save = {}
    ops.lstm_fwd(x, w, b, 7, save=save)
    dw = torch.zeros(28, 13)
    err = torch.randn(3, 7)
    for bad in (lambda: ops.lstm_bwd(err[:, :-1], x, w, save, dw, None),
                lambda: ops.lstm_bwd(err, x, w, {}, dw, None),
                lambda: ops.lstm_bwd(err, x, w, save, dw[:-1], None),
                lambda: ops.lstm_bwd(err, x, w, save, dw.double(), None),
                lambda: ops.lstm_bwd(err, x, w, save, dw, torch.zeros(27)),
                lambda: ops.lstm_bwd(err, x, w, save, dw, None,
                                     accumulate=False)):
        with pytest.raises(ValueError):
            bad()
    assert not dw.any()


# ------------------------------------------------------------------ units
def _workflow(layers, snap=None, epochs=1, **loader):
    from veles_amd.dummy import DummyLauncher
    from veles_amd.models import StandardWorkflow
    import veles_amd.loader  # noqa: F401
    cfg = {"steps": 6, "features": 8, "class_lengths": (0, 64, 128),
           "minibatch_size": 32, "seed": 3}
    cfg.update(loader)
    return StandardWorkflow(
        DummyLauncher(), loader_name="seq_recall", loader_config=cfg,
        layers=layers, decision_config={"max_epochs": epochs,
                                        "fail_iterations": 100},
        snapshotter_config=snap)


def _layers(kind="lstm", lr=0.1):
    g = {"learning_rate": lr, "gradient_moment": 0.9}
    return [{"type": kind, "->": {"output_sample_shape": 12,
                                  "return_sequences": True}, "<-": dict(g)},
            {"type": kind, "->": {"output_sample_shape": 10}, "<-": dict(g)},
            {"type": "softmax", "->": {"output_sample_shape": 8},
             "<-": dict(g)}]


@pytest.mark.parametrize("kind", ("lstm", "rnn"))
def test_stacked_layers_build_and_train(kind):
    from veles_amd.backends import Device
    from veles_amd.models import LSTM, GDLSTM, LAYER_TYPES
    assert LAYER_TYPES["lstm"] == (LSTM, GDLSTM)
    wf = _workflow(_layers(kind), epochs=2)
    wf.initialize(device=Device(backend="cpu"))
    ng = CELLS[kind]
    f0, f1 = wf.forwards[:2]
    assert f0.weights.mem.shape == (ng * 12, 8 + 12)
    assert f1.weights.mem.shape == (ng * 10, 12 + 10)
    assert tuple(f0.output.shape) == (32, 6, 12)
    assert tuple(f1.output.shape) == (32, 10)
    if kind == "lstm":   # forget-gate bias 1, the rest within the filling
        b = f0.bias.mem
        assert (b[12:24] == 1.0).all()
        assert numpy.abs(numpy.delete(b, range(12, 24))).max() <= 20 ** -0.5
    w0 = [f.weights_master.clone() for f in wf.forwards]
    wf.run()
    assert wf.gds[0].err_input.devmem is None     # need_err_input False
    assert tuple(wf.gds[1].err_input.shape) == (32, 6, 12)
    for f, w in zip(wf.forwards, w0):
        assert torch.isfinite(f.weights_master).all()
        assert not torch.equal(f.weights_master, w)
    h = wf.decision.history
    assert len(h) == 2 and numpy.isfinite(h[-1]["train_loss"])


def test_gradient_modes_give_the_same_step(monkeypatch):
    from veles_amd.backends import Device
    from veles_amd.prng import random_generator
    ws = []
    for ow in ("1", "0"):
        monkeypatch.setenv("VELES_AMD_GRAD_OVERWRITE", ow)
        random_generator.get().seed(5)
        wf = _workflow(_layers())
        wf.initialize(device=Device(backend="cpu"))
        wf.run_steps(2)
        assert wf.param_store_.overwrite == (ow == "1")
        ws.append([f.weights_master.clone() for f in wf.forwards])
    for a, b in zip(*ws):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-7)


def test_snapshot_resume_gives_the_identical_next_step(tmp_path):
    import os
    from veles_amd.backends import Device
    from veles_amd.dummy import DummyLauncher
    from veles_amd.snapshotter import SnapshotterToFile
    from veles_amd.utils.config import root
    snap = {"prefix": "rec", "directory": str(tmp_path), "interval": 1,
            "time_interval": 0, "compression": "gz"}
    root.common.disable.snapshotting = False
    wf = _workflow(_layers(), snap=snap)
    wf.initialize(device=Device(backend="cpu"))
    wf.run()
    path = [os.path.join(tmp_path, f) for f in sorted(os.listdir(tmp_path))
            if "current" in f][0]
    wf2 = SnapshotterToFile.import_(path)
    wf2.workflow = DummyLauncher()
    wf2.initialize(device=Device(backend="cpu"))
    for f, f2 in zip(wf.forwards, wf2.forwards):
        assert torch.equal(f.weights_master, f2.weights_master)
    for w in (wf, wf2):
        w.decision.max_epochs += 1
        w.decision.complete <<= False
        w.run_steps(1)
    for f, f2 in zip(wf.forwards, wf2.forwards):
        assert torch.equal(f.weights_master, f2.weights_master)
        assert torch.equal(f.bias_master, f2.bias_master)


def test_training_trajectory_matches_float64_torch():
    """20 plain SGD steps of seq_recall on the CPU device against the same
    net in torch float64 from the same initial weights and batches.  The
    loss of one step is 1-Lipschitz in the largest logit error times 2, the
    logits err by gamma_{H+2} (|h| |W|^T + |b|) + e_h |W|^T with e_h the
    forward bound of the module docstring; step k is allowed k times that
    (the weights of step k carry the rounding of k - 1 updates)."""
    from veles_amd.backends import Device
    from veles_amd.prng import random_generator
    H, T, I, B, K, lr = 16, 6, 8, 32, 20, 0.5
    g = {"learning_rate": lr, "learning_rate_bias": lr,
         "gradient_moment": 0.0, "gradient_moment_bias": 0.0}
    layers = [{"type": "lstm", "->": {"output_sample_shape": H},
               "<-": dict(g)},
              {"type": "softmax", "->": {"output_sample_shape": 8},
               "<-": dict(g)}]
    random_generator.get().seed(11)
    wf = _workflow(layers, steps=T, class_lengths=(0, 0, B * K),
                   minibatch_size=B)
    wf.decision.max_epochs = None
    wf.initialize(device=Device(backend="cpu"))
    f0, f1 = wf.forwards
    lstm = torch.nn.LSTM(I, H, batch_first=True).double()
    fc = torch.nn.Linear(H, 8).double()
    with torch.no_grad():
        w = torch.from_numpy(f0.weights.mem).double()
        lstm.weight_ih_l0.copy_(w[:, :I])
        lstm.weight_hh_l0.copy_(w[:, I:])
        lstm.bias_ih_l0.copy_(torch.from_numpy(f0.bias.mem))
        lstm.bias_hh_l0.zero_()
        fc.weight.copy_(torch.from_numpy(f1.weights.mem))
        fc.bias.copy_(torch.from_numpy(f1.bias.mem))
    lstm.bias_hh_l0.requires_grad_(False)
    params = [p for p in list(lstm.parameters()) + list(fc.parameters())
              if p.requires_grad]
    worst = 0.0
    for k in range(1, K + 1):
        wf.run_steps(1)
        x = wf.loader.minibatch_data.devmem.double().clone()
        lab = wf.loader.minibatch_labels.devmem.long().clone()
        p = f1.output.devmem.double()
        got = -torch.log(p[torch.arange(B), lab]).mean().item()
        # the float64 net on the same batch, with the bound from its weights
        w64 = torch.cat((lstm.weight_ih_l0, lstm.weight_hh_l0), 1).detach()
        steps = forward_bound("lstm", x, w64, lstm.bias_ih_l0.detach(), I, H)
        h, e_h = steps[-1]["h"], steps[-1]["e_h"]
        wa = fc.weight.detach().abs()
        e_logit = gamma(H + 2) * (h.abs() @ wa.t() + fc.bias.detach().abs()) \
            + e_h @ wa.t()
        bound = k * (2 * e_logit.max().item() + 8 * U)
        y, _ = lstm(x)
        loss = torch.nn.functional.cross_entropy(fc(y[:, -1]), lab)
        r = abs(got - loss.item()) / bound
        worst = max(worst, r)
        print("step %2d loss %.6f / %.6f, difference / bound %.2e" %
              (k, got, loss.item(), r))
        grads = torch.autograd.grad(loss, params)
        with torch.no_grad():
            for q, gq in zip(params, grads):
                q -= lr * gq
    assert worst <= 1.0
