"""GRU layers on the CPU reference device: the float64 formula against
torch.nn.GRUCell, ops.gru_fwd / gru_bwd against torch.nn.GRU in float64 with
autograd, the GRU / GDGRU units in StandardWorkflow, and the host checks.

Bias mapping: bias [4H] = (b_r, b_z, b_n, b_hn); torch's bias_ih = bias[:3H],
bias_hh = (0, 0, bias[3H:]) (torch's b_hr / b_hz only add to b_ir / b_iz).

Tolerance: the float32 rounding bound that tests/test_recurrent.py derives
for the LSTM, with the GRU's K and gate count; u = 2^-24,
gamma_n = n u / (1 - n u).

Forward, per step: r and z have one pre-activation sum of I + H + 1 products,
    e_pre = gamma_{I+H+2} (|x_t| |Wx|^T + |b| + |h| |Wh|^T) + e_h |Wh|^T,
    e_r, e_z = e_pre / 4 + 4 u;
the hidden-side candidate product and the candidate:
    e_hn = gamma_{H+2} (|h| |Whn|^T + |b_hn|) + e_h |Whn|^T
    e_n = gamma_{I+2} (|x_t| |Wxn|^T + |b_n|) + |hn| e_r + (r + e_r) e_hn
          + 3 u (|xg_n| + |r hn|) + 4 u
    e_h' = |n - h| e_z + (1 - z) e_n + z e_h + e_z (e_n + e_h)
           + 4 u (|(1 - z) n| + |z h|).
Backward: every result is a sum of products of |err|, the gate factors, |W|
and |x| / |h| with non-negative coefficients once h_{t-1} - n is replaced by
|h_{t-1}| + |n|, so (running error analysis) it errs by at most gamma_n M',
where M' is the same computation on absolute values and n its longest chain,
T (3H + 16) + B T + I + H; the forward errors of the gate factors enter
through M' - M, M' evaluated with every factor raised by its forward bound.
"""
import numpy
import pytest
import torch

from veles_amd import ops

U = 2.0 ** -24
SHAPES = [(3, 5, 6, 7), (1, 1, 8, 8), (4, 6, 5, 16)]
IDS = ["%dx%dx%dx%d" % s for s in SHAPES]


def gamma(n):
    return n * U / (1 - n * U)


def gru_step(xt, hp, w, b, I, H):
    """the float64 formula of docs/OPS.md "GRU": one step, (h, r, z, n, hn)"""
    wx, wh = w[:, :I], w[:, I:]
    xg = xt @ wx.t() + b[:3 * H]
    hh = hp @ wh.t()
    r = torch.sigmoid(xg[:, :H] + hh[:, :H])
    z = torch.sigmoid(xg[:, H:2 * H] + hh[:, H:2 * H])
    hn = hh[:, 2 * H:] + b[3 * H:]
    n = torch.tanh(xg[:, 2 * H:] + r * hn)
    return (1 - z) * n + z * hp, r, z, n, hn


def torch_biases(b, H):
    bhh = torch.zeros(3 * H, dtype=b.dtype)
    bhh[2 * H:] = b[3 * H:]
    return b[:3 * H].clone(), bhh


def oracle(w, b, I, H):
    m = torch.nn.GRU(I, H, batch_first=True).double()
    bih, bhh = torch_biases(b, H)
    with torch.no_grad():
        m.weight_ih_l0.copy_(w[:, :I])
        m.weight_hh_l0.copy_(w[:, I:])
        m.bias_ih_l0.copy_(bih)
        m.bias_hh_l0.copy_(bhh)
    return m


def operands(shape, seed=0, dtype=torch.float32):
    B, T, I, H = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, I, generator=g)
    w = torch.randn(3 * H, I + H, generator=g) / (I + H) ** 0.5
    b = torch.randn(4 * H, generator=g) * 0.5      # b_hn != 0
    return x.to(dtype), w.to(dtype), b.to(dtype)


def test_formula_matches_torch_grucell():
    for shape in SHAPES:
        B, T, I, H = shape
        x, w, b = operands(shape, seed=1, dtype=torch.float64)
        assert b[3 * H:].abs().min() > 0
        cell = torch.nn.GRUCell(I, H).double()
        bih, bhh = torch_biases(b, H)
        with torch.no_grad():
            cell.weight_ih.copy_(w[:, :I])
            cell.weight_hh.copy_(w[:, I:])
            cell.bias_ih.copy_(bih)
            cell.bias_hh.copy_(bhh)
        h = torch.zeros(B, H, dtype=torch.float64)
        g = torch.Generator().manual_seed(2)
        for t in range(T + 1):
            if t == 1:   # a non-zero, non-trajectory state too
                h = torch.randn(B, H, generator=g).double()
            with torch.no_grad():
                ref = cell(x[:, t % T], h)
            got = gru_step(x[:, t % T], h, w, b, I, H)[0]
            assert (got - ref).abs().max().item() <= 1e-12
            h = got


def forward_bound(x, w, b, I, H):
    """float64 model of the loop with the per-step error bounds of the module
    docstring; returns a list of per-step dicts"""
    B, T, _ = x.shape
    wx, wh = w[:, :I].abs(), w[:, I:].abs()
    h = torch.zeros(B, H, dtype=torch.float64)
    e_h = h.clone()
    steps = []
    for t in range(T):
        xa = x[:, t].abs()
        hn_, r, z, n, hn = gru_step(x[:, t], h, w, b, I, H)
        e_pre = gamma(I + H + 2) * (xa @ wx.t() + b[:3 * H].abs() +
                                    h.abs() @ wh.t()) + e_h @ wh.t()
        e_r = 0.25 * e_pre[:, :H] + 4 * U
        e_z = 0.25 * e_pre[:, H:2 * H] + 4 * U
        e_hn = gamma(H + 2) * (h.abs() @ wh[2 * H:].t() + b[3 * H:].abs()) + \
            e_h @ wh[2 * H:].t()
        xgn = x[:, t] @ w[2 * H:, :I].t() + b[2 * H:3 * H]
        e_n = gamma(I + 2) * (xa @ wx[2 * H:].t() + b[2 * H:3 * H].abs()) + \
            hn.abs() * e_r + (r + e_r) * e_hn + \
            3 * U * (xgn.abs() + (r * hn).abs()) + 4 * U
        e_new = (n - h).abs() * e_z + (1 - z) * e_n + z * e_h + \
            e_z * (e_n + e_h) + 4 * U * (((1 - z) * n).abs() + (z * h).abs())
        steps.append(dict(hp=h, e_hp=e_h, r=r, z=z, n=n, hn=hn, e_r=e_r,
                          e_z=e_z, e_n=e_n, e_hn=e_hn, h=hn_, e_h=e_new))
        h, e_h = hn_, e_new
    return steps


def backward_magnitude(steps, x, w, err, I, H, raised):
    """the backward on absolute values; ``raised``: every forward quantity
    plus its forward bound.  Returns (dw, dbias [4H], err_input)."""
    B, T, _ = x.shape
    wh, wx = w[:, I:].abs(), w[:, :I].abs()
    q = 1.0 if raised else 0.0
    dgx, dgh = [None] * T, [None] * T
    dc = torch.zeros(B, H, dtype=torch.float64)
    for t in range(T - 1, -1, -1):
        s = steps[t]
        dh = err[:, t].abs() + dc
        if t < T - 1:
            dh = dh + dgh[t + 1] @ wh
        r = s["r"] + q * s["e_r"]
        z = s["z"] + q * s["e_z"]
        one_z = (1 - s["z"]) + q * s["e_z"]
        one_n2 = (1 - s["n"] ** 2).abs() + q * 2 * s["n"].abs() * s["e_n"]
        hpn = s["hp"].abs() + s["n"].abs() + q * (s["e_hp"] + s["e_n"])
        hn = s["hn"].abs() + q * s["e_hn"]

        def dsig(v, e):   # v (1 - v) and its error |1 - 2 v| e
            return v * (1 - v) + q * (1 - 2 * v).abs() * e
        dn = dh * one_z * one_n2
        dz = dh * hpn * dsig(s["z"], s["e_z"])
        dr = dn * hn * dsig(s["r"], s["e_r"])
        dgx[t] = torch.cat((dr, dz, dn), 1)
        dgh[t] = torch.cat((dr, dz, dn * r), 1)
        dc = dh * z
    gx = torch.stack(dgx, 1).reshape(B * T, -1)
    gh = torch.stack(dgh, 1).reshape(B * T, -1)
    hp = torch.stack([s["hp"].abs() + q * s["e_hp"] for s in steps], 1)
    dw = torch.cat((gx.t() @ x.abs().reshape(B * T, I),
                    gh.t() @ hp.reshape(B * T, H)), 1)
    db = torch.cat((gx.sum(0), gh[:, 2 * H:].sum(0)))
    return dw, db, (gx @ wx).reshape(B, T, I)


@pytest.mark.parametrize("seq", (False, True))
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_forward_and_backward_match_torch(shape, seq):
    B, T, I, H = shape
    x, w, b = operands(shape)
    x64, w64, b64 = x.double(), w.double(), b.double()
    m = oracle(w64, b64, I, H)
    xd = x64.clone().requires_grad_()
    y, _ = m(xd)
    ref = y if seq else y[:, -1]
    save = {}
    out = ops.gru_fwd(x, w, b, H, return_sequences=seq, save=save)
    assert out.shape == ref.shape and out.dtype == torch.float32
    for k, shape_k in (("h", (B, T, H)), ("hf", (B, T, H)), ("hn", (B, T, H)),
                       ("gates", (B, T, 3 * H)), ("xg", (B, T, 3 * H))):
        assert tuple(save[k].shape) == shape_k, k
    steps = forward_bound(x64, w64, b64, I, H)
    e_h = torch.stack([s["e_h"] for s in steps], 1)
    bound = e_h if seq else e_h[:, -1]
    r = ((out.double() - ref.detach()).abs() / bound).max().item()
    print("forward max err / bound %.3f" % r)
    assert r <= 1.0

    g = torch.Generator().manual_seed(7)
    err = torch.randn(ref.shape, generator=g)
    ref.backward(err.double())
    dw = torch.full((3 * H, I + H), 9.0)
    db = torch.full((4 * H,), 9.0)
    ei = ops.gru_bwd(err, x, w, save, dw, db)
    for k in ("dgx", "dgh"):
        assert tuple(save[k].shape) == (B, T, 3 * H), k
    assert tuple(save["dcarry"].shape) == (T, B, H)
    e_full = torch.zeros(B, T, H, dtype=torch.float64)
    if seq:
        e_full.copy_(err)
    else:
        e_full[:, -1] = err
    m0 = backward_magnitude(steps, x64, w64, e_full, I, H, False)
    m1 = backward_magnitude(steps, x64, w64, e_full, I, H, True)
    n = T * (3 * H + 16) + B * T + I + H
    # torch's b_hr / b_hz gradients equal those of b_ir / b_iz (folded)
    want_db = torch.cat((m.bias_ih_l0.grad, m.bias_hh_l0.grad[2 * H:]))
    refs = (torch.cat((m.weight_ih_l0.grad, m.weight_hh_l0.grad), 1),
            want_db, xd.grad)
    for name, got, want, a, c in zip(("dw", "dbias", "err_input"),
                                     (dw, db, ei), refs, m0, m1):
        bound = gamma(n) * c + (c - a) + 1e-300
        ratio = (got.double() - want).abs() / bound
        if name == "dbias":     # all four blocks, one by one
            for k, blk in zip(("b_r", "b_z", "b_n", "b_hn"),
                              ratio.split(H)):
                print("dbias %s max err / bound %.3f" % (k, blk.max().item()))
                assert blk.max().item() <= 1.0, k
        r = ratio.max().item()
        print("%s max err / bound %.3f" % (name, r))
        assert r <= 1.0, name


def test_gradient_modes_agree():
    """accumulate adds to what is there, "overwrite" replaces it,
    need_err_input=False leaves err_input alone"""
    x, w, b = operands((3, 5, 6, 7))
    err = torch.randn(3, 7)
    save = {}
    ops.gru_fwd(x, w, b, 7, save=save)
    dw0, db0 = torch.full((21, 13), 5.0), torch.full((28,), 5.0)
    ei0 = ops.gru_bwd(err, x, w, save, dw0, db0, accumulate="overwrite")
    dw1, db1 = torch.zeros(21, 13), torch.zeros(28)
    ops.gru_bwd(err, x, w, save, dw1, db1, accumulate=True)
    assert torch.equal(dw0, dw1) and torch.equal(db0, db1)
    assert db0[21:].abs().min() > 0          # b_hn has a gradient
    ei = torch.full((3, 5, 6), 7.0)
    assert ops.gru_bwd(err, x, w, save, dw1, db1, accumulate=True,
                       need_err_input=False, err_input=ei) is None
    assert (ei == 7.0).all()
    torch.testing.assert_close(dw1, 2 * dw0, rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(db1, 2 * db0, rtol=1e-6, atol=1e-7)
    got = ops.gru_bwd(err, x, w, save, dw1, None, err_input=ei)
    assert got is ei and torch.equal(ei, ei0)


def test_save_none_writes_no_gates():
    x, w, b = operands((3, 5, 6, 7))
    ws = {}
    y = ops.gru_fwd(x, w, b, 7, ws=ws)
    save = {}
    assert torch.equal(y, ops.gru_fwd(x, w, b, 7, save=save))
    assert "gates" in save and "hn" in save and "h" in ws
    assert "gates" not in ws and "hn" not in ws and "xg" not in ws
    h = ws["h"]
    ops.gru_fwd(x, w, b, 7, ws=ws)
    assert ws["h"] is h       # buffers are reused
    g = save["gates"]
    ops.gru_fwd(x, w, b, 7, save=save)
    assert save["gates"] is g
    # no bias at all is the zero bias
    assert torch.equal(ops.gru_fwd(x, w, None, 7),
                       ops.gru_fwd(x, w, torch.zeros(28), 7))


# (B, I, H, T): H = 7 is off the 8-element grid (on the GPU the scalar kernel
# path, padded pitch != width), H = 8 is on it (the vector path)
CONTRACT = [(3, 5, 7, 2), (2, 8, 8, 2)]


@pytest.mark.parametrize("shape", CONTRACT, ids=("H7", "H8"))
def test_save_contract(shape):
    """what fwd + bwd leave in ``save`` under public keys (the table of
    docs/OPS.md "GRU"): the tools and the tests that launch steps by hand
    read these"""
    B, I, H, T = shape
    x, w, b = operands((B, T, I, H))
    save = {}
    ops.gru_fwd(x, w, b, H, save=save)
    ops.gru_bwd(torch.randn(B, H), x, w, save, torch.zeros(3 * H, I + H),
                torch.zeros(4 * H))
    want = {"h": (B, T, H), "hf": (B, T, H), "hn": (B, T, H),
            "gates": (B, T, 3 * H), "xg": (B, T, 3 * H),
            "dgx": (B, T, 3 * H), "dgh": (B, T, 3 * H), "dcarry": (T, B, H)}
    assert {k for k in save if not k.startswith("_")} == set(want)
    for k, shape in want.items():
        assert tuple(save[k].shape) == shape, k
        assert save[k].dtype == torch.float32, k


def test_forward_is_the_default_direction():
    B, T, I, H = 3, 5, 6, 7
    x, w, b = operands((B, T, I, H))
    err = torch.randn(B, T, H)
    res = []
    for kw in ({}, {"direction": "forward"}):
        save = {}
        y = ops.gru_fwd(x, w, b, H, return_sequences=True, save=save, **kw)
        dw, db = torch.zeros(3 * H, I + H), torch.zeros(4 * H)
        ei = ops.gru_bwd(err, x, w, save, dw, db, **kw)
        res.append((y, ei, dw, db))
    for a, c in zip(*res):
        assert torch.equal(a, c)
    for bad in (lambda: ops.gru_fwd(x, w, b, H, direction="backward"),
                lambda: ops.gru_bwd(err, x, w, save, dw, db,
                                    direction="backward")):
        with pytest.raises(ValueError) as e:
            bad()
        assert all(d in str(e.value) for d in ("forward", "reverse", "both"))


def test_host_checks():
    x, w, b = operands((3, 5, 6, 7))
    for bad in (lambda: ops.gru_fwd(x[0], w, b, 7),
                lambda: ops.gru_fwd(x, w, b, 8),
                lambda: ops.gru_fwd(x, w[:, :-1], b, 7),
                lambda: ops.gru_fwd(x, w[:-1], b, 7),
                lambda: ops.gru_fwd(x, w, b[:21], 7),       # 3H: no b_hn
                lambda: ops.gru_fwd(x, w, b[:-1], 7),
                lambda: ops.gru_fwd(x, w, b.repeat(2)[::2], 7),
                lambda: ops.gru_fwd(x.transpose(0, 1), w, b, 7),
                lambda: ops.gru_fwd(x[:, :, ::2], w[:, :10], b, 7),
                lambda: ops.gru_fwd(x, w.t().contiguous().t(), b, 7),
                lambda: ops.gru_fwd(x, w, b, 7, out=torch.zeros(3, 8))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        ops.gru_fwd(x.long(), w, b, 7)
    with pytest.raises(TypeError):
        ops.gru_fwd(x, w.long(), b, 7)
    save = {}
    ops.gru_fwd(x, w, b, 7, save=save)
    dw = torch.zeros(21, 13)
    err = torch.randn(3, 7)
    no_hn = {k: v for k, v in save.items() if k != "hn"}
    bad_hf = dict(save, hf=save["hf"].double())
    for bad in (lambda: ops.gru_bwd(err[:, :-1], x, w, save, dw, None),
                lambda: ops.gru_bwd(err, x, w, {}, dw, None),
                lambda: ops.gru_bwd(err, x, w, None, dw, None),
                lambda: ops.gru_bwd(err, x, w, no_hn, dw, None),
                lambda: ops.gru_bwd(err, x, w, bad_hf, dw, None),
                lambda: ops.gru_bwd(err, x, w, save, dw[:-1], None),
                lambda: ops.gru_bwd(err, x, w, save, dw.double(), None),
                lambda: ops.gru_bwd(err, x, w, save, dw, torch.zeros(21)),
                lambda: ops.gru_bwd(err, x, w, save, dw, torch.zeros(27)),
                lambda: ops.gru_bwd(err, x, w[:-1], save, dw, None),
                lambda: ops.gru_bwd(err, x, w, save, dw, None,
                                    err_input=torch.zeros(3, 5, 7)),
                lambda: ops.gru_bwd(err, x, w, save, dw, None,
                                    accumulate=False)):
        with pytest.raises(ValueError):
            bad()
    assert not dw.any()
    # the LSTM entry point still refuses the cell
    with pytest.raises(ValueError):
        ops.lstm_fwd(x, w, b[:21], 7, cell="gru")


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


def _layers(lr=0.1):
    g = {"learning_rate": lr, "gradient_moment": 0.9}
    return [{"type": "gru", "->": {"output_sample_shape": 12,
                                   "return_sequences": True}, "<-": dict(g)},
            {"type": "gru", "->": {"output_sample_shape": 10}, "<-": dict(g)},
            {"type": "softmax", "->": {"output_sample_shape": 8},
             "<-": dict(g)}]


def test_stacked_layers_build_and_train():
    from veles_amd.backends import Device
    from veles_amd.models import GRU, GDGRU, LSTM, LAYER_TYPES
    assert LAYER_TYPES["gru"] == (GRU, GDGRU)
    assert GRU.__id__ != LSTM.__id__ and GRU.MAPPING == "gru"
    wf = _workflow(_layers(), epochs=2)
    wf.initialize(device=Device(backend="cpu"))
    f0, f1 = wf.forwards[:2]
    assert f0.weights.mem.shape == (36, 8 + 12)
    assert f1.weights.mem.shape == (30, 12 + 10)
    assert f0.bias.mem.shape == (48,) and f1.bias.mem.shape == (40,)
    assert tuple(f0.output.shape) == (32, 6, 12)
    assert tuple(f1.output.shape) == (32, 10)
    # all four bias blocks within the uniform filling, none set to a constant
    b = f0.bias.mem
    assert numpy.abs(b).max() <= 20 ** -0.5 and len(set(b.tolist())) > 40
    assert numpy.abs(f0.weights.mem).max() <= 20 ** -0.5
    w0 = [f.weights_master.clone() for f in wf.forwards]
    b0 = f0.bias_master.clone()
    wf.run()
    assert wf.gds[0].err_input.devmem is None     # need_err_input False
    assert tuple(wf.gds[1].err_input.shape) == (32, 6, 12)
    for f, w in zip(wf.forwards, w0):
        assert torch.isfinite(f.weights_master).all()
        assert not torch.equal(f.weights_master, w)
    assert (f0.bias_master[36:] != b0[36:]).any()   # b_hn is trained
    h = wf.decision.history
    assert len(h) == 2 and numpy.isfinite(h[-1]["train_loss"])


def test_testing_mode_keeps_no_gates():
    from veles_amd.backends import Device
    wf = _workflow(_layers())
    wf.initialize(device=Device(backend="cpu"))
    wf.testing = True
    wf.loader.run()
    for f in wf.forwards[:2]:
        f.run()
        for k in ("gates", "hn", "xg"):
            assert k not in f.save_, k
        assert torch.isfinite(f.output.devmem).all()
    wf.testing = False
    wf.forwards[0].run()
    assert "gates" in wf.forwards[0].save_


def test_snapshot_resume_gives_the_identical_next_steps(tmp_path):
    """a snapshot after k steps (one epoch) plus m = 3 more steps equals
    k + m steps, bit for bit"""
    import os
    from veles_amd.backends import Device
    from veles_amd.dummy import DummyLauncher
    from veles_amd.snapshotter import SnapshotterToFile
    from veles_amd.utils.config import root
    snap = {"prefix": "gru", "directory": str(tmp_path), "interval": 1,
            "time_interval": 0, "compression": "gz"}
    before = root.common.disable.snapshotting
    root.common.disable.snapshotting = False
    try:
        wf = _workflow(_layers(), snap=snap)
        wf.initialize(device=Device(backend="cpu"))
        wf.run()
    finally:
        root.common.disable.snapshotting = before
    path = [os.path.join(tmp_path, f) for f in sorted(os.listdir(tmp_path))
            if "current" in f][0]
    wf2 = SnapshotterToFile.import_(path)
    wf2.workflow = DummyLauncher()
    wf2.initialize(device=Device(backend="cpu"))
    for f, f2 in zip(wf.forwards, wf2.forwards):
        assert f2.bias.mem.shape == f.bias.mem.shape
        assert torch.equal(f.weights_master, f2.weights_master)
    for w in (wf, wf2):
        w.decision.max_epochs += 1
        w.decision.complete <<= False
        w.run_steps(3)
    for f, f2 in zip(wf.forwards, wf2.forwards):
        assert torch.equal(f.weights_master, f2.weights_master)
        assert torch.equal(f.bias_master, f2.bias_master)


def test_training_trajectory_matches_float64_torch():
    """20 plain SGD steps of seq_recall on the CPU device against the same
    net in torch float64 from the same initial weights and batches, with the
    loss agreement of the LSTM trajectory test: the loss of one step is
    1-Lipschitz in the largest logit error times 2, the logits err by
    gamma_{H+2} (|h| |W|^T + |b|) + e_h |W|^T with e_h the forward bound of
    the module docstring; step k is allowed k times that."""
    from veles_amd.backends import Device
    from veles_amd.prng import random_generator
    H, T, I, B, K, lr = 16, 6, 8, 32, 20, 0.5
    g = {"learning_rate": lr, "learning_rate_bias": lr,
         "gradient_moment": 0.0, "gradient_moment_bias": 0.0}
    layers = [{"type": "gru", "->": {"output_sample_shape": H},
               "<-": dict(g)},
              {"type": "softmax", "->": {"output_sample_shape": 8},
               "<-": dict(g)}]
    random_generator.get().seed(11)
    wf = _workflow(layers, steps=T, class_lengths=(0, 0, B * K),
                   minibatch_size=B)
    wf.decision.max_epochs = None
    wf.initialize(device=Device(backend="cpu"))
    f0, f1 = wf.forwards
    b0 = torch.from_numpy(f0.bias.mem).double()
    gru = oracle(torch.from_numpy(f0.weights.mem).double(), b0, I, H)
    fc = torch.nn.Linear(H, 8).double()
    with torch.no_grad():
        fc.weight.copy_(torch.from_numpy(f1.weights.mem))
        fc.bias.copy_(torch.from_numpy(f1.bias.mem))
    # b_hr and b_hz stay 0: their gradient is masked out of the update
    mask = torch.zeros(3 * H, dtype=torch.float64)
    mask[2 * H:] = 1
    params = list(gru.parameters()) + list(fc.parameters())
    worst = 0.0
    for k in range(1, K + 1):
        wf.run_steps(1)
        x = wf.loader.minibatch_data.devmem.double().clone()
        lab = wf.loader.minibatch_labels.devmem.long().clone()
        p = f1.output.devmem.double()
        got = -torch.log(p[torch.arange(B), lab]).mean().item()
        w64 = torch.cat((gru.weight_ih_l0, gru.weight_hh_l0), 1).detach()
        b64 = torch.cat((gru.bias_ih_l0, gru.bias_hh_l0[2 * H:])).detach()
        steps = forward_bound(x, w64, b64, I, H)
        h, e_h = steps[-1]["h"], steps[-1]["e_h"]
        wa = fc.weight.detach().abs()
        e_logit = gamma(H + 2) * (h.abs() @ wa.t() + fc.bias.detach().abs()) \
            + e_h @ wa.t()
        bound = k * (2 * e_logit.max().item() + 8 * U)
        y, _ = gru(x)
        loss = torch.nn.functional.cross_entropy(fc(y[:, -1]), lab)
        r = abs(got - loss.item()) / bound
        worst = max(worst, r)
        print("step %2d loss %.6f / %.6f, difference / bound %.2e" %
              (k, got, loss.item(), r))
        grads = torch.autograd.grad(loss, params)
        with torch.no_grad():
            for q, gq in zip(params, grads):
                q -= lr * (gq * mask if q is gru.bias_hh_l0 else gq)
    assert worst <= 1.0
