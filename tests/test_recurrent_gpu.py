"""The fused gfx950 recurrent step kernels (csrc/kernels/recurrent.hip) and
ops.lstm_fwd / lstm_bwd on the GPU.

Step kernels, teacher-forced: every step is checked on its own, from the
GPU's OWN stored h_{t-1}, c_{t-1}, projection and bf16 weights fed to the
float64 torch.nn.LSTMCell / RNNCell, so the bound is local and derivable:

* accumulation: e_acc = (K + 4) 2^-24 (sum|a||b| + |xg|); the bf16 x bf16
  products are exact in f32, K + 4 covers the MFMA chain, the 3 additions of
  the 4 K-split partial sums and the addition of xg (forward K = H,
  backward K = NG*H with |err| in the place of |xg|);
* every transcendental: e_fn, measured in the same GPU run (the ROCm math
  documentation's ulp table is not on the test machine): the cell's device
  sigmoid / tanh against float64 on 2^16 points of [-20, 20], taken TWICE
  because sampling does not reach every input (figures of the development
  run: profiles/recurrent/gpu_tests_figures.txt, 8.9e-8 and 7.4e-8);
* pushed through the cell with the gates' Lipschitz constants (sigmoid 1/4,
  tanh 1) and the partial derivatives of the cell equations, plus 8 f32
  roundings (2^-24 relative) for the few multiply-adds of an output;
* half a bf16 ulp for every bf16 store: 8 significant bits, so at most
  2^-8 relative (named U9 below for "bit 9 onward is rounded off").

Whole layer: the three gradient GEMMs against float64 products of the GPU's
own dG with the tolerance of the existing bf16 GEMM tests (1e-2 of the
largest reference magnitude for a bf16 output, 1e-3 for float32).
"""
import functools
import os

import pytest
import torch

import veles_amd.ops as ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U24, U9 = 2.0 ** -24, 2.0 ** -8

# (B, I, H, T); the tile is 16 hidden units x 32 batch rows, K chunks of 32
# dealt to 4 waves
CASES = [
    (1, 8, 8, 1),       # degenerate: one step, no product
    (3, 8, 16, 2),      # the smallest shape with the recurrent product
    (32, 32, 16, 3),    # exactly one tile
    (31, 32, 16, 3),    # ... and its neighbours: one row short,
    (33, 32, 24, 3),    # one row / one 8-column group over
    (64, 32, 64, 3),    # 2 x 4 whole tiles
    (65, 40, 72, 4),    # partial tiles in both dimensions
    (130, 24, 136, 5),  # several tiles, partial last K chunk (K = 136, 544)
    (32, 16, 264, 3),   # many hidden tiles, K over 256 (every wave loops)
    (17, 5, 20, 3),     # I and H off the 8-grid: the guarded element path
    (33, 8, 64, 3),     # saturated: pre-activations of +-200
]
SAT = len(CASES) - 1
IDS = ["%dx%dx%dx%d" % c for c in CASES]
CELLS = {"lstm": 4, "rnn": 1}


@functools.lru_cache(maxsize=None)
def e_fn():
    """twice the largest error of the device sigmoid / tanh on [-20, 20]"""
    fn = ops._rec_fn("hvk_recurrent_fn")
    x = torch.linspace(-20, 20, 1 << 16, device=DEV)
    out = []
    for kind, ref in ((0, torch.sigmoid), (1, torch.tanh)):
        y = torch.empty_like(x)
        ops._lib.check(fn(kind, x.data_ptr(), y.data_ptr(), x.numel(),
                          ops._s(x)), "hvk_recurrent_fn")
        torch.cuda.synchronize()
        out.append(2 * (y.double() - ref(x.double())).abs().max().item())
    print("e_fn: sigmoid %.3g tanh %.3g (twice the measured maxima)" %
          tuple(out))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def case(i, cell):
    """One forward + backward of case i on the GPU, everything the checks
    need copied to the host once as float64."""
    B, I, H, T = CASES[i]
    ng = CELLS[cell]
    g = torch.Generator().manual_seed(300 + i)
    x = torch.randn(B, T, I, generator=g).to(BF)
    w = (torch.randn(ng * H, I + H, generator=g) / (I + H) ** 0.5).to(BF)
    bias = torch.randn(ng * H, generator=g) * 0.5
    if i == SAT:
        # +-200 through the projection, Wh at normal scale
        bias = torch.where(torch.rand(ng * H, generator=g) < 0.5, -200., 200.)
    err = torch.randn(B, T, H, generator=g).to(BF)
    d = dict(x=x.to(DEV), w=w.to(DEV), bias=bias.to(DEV), err=err.to(DEV),
             B=B, I=I, H=H, T=T, ng=ng, cell=cell)
    d["save"] = save = {}
    d["out"] = ops.lstm_fwd(d["x"], d["w"], d["bias"], H, cell=cell,
                            return_sequences=True, save=save)
    d["dw"] = torch.full((ng * H, I + H), 3.0, device=DEV)
    d["db"] = torch.full((ng * H,), 3.0, device=DEV)
    d["ei"] = ops.lstm_bwd(d["err"], d["x"], d["w"], save, d["dw"], d["db"],
                           cell=cell)
    torch.cuda.synchronize()
    for k in ("h", "c", "gates", "xg", "dg", "dc"):
        if k in save:
            d[k] = save[k].double().cpu()
    d["wh"] = w[:, I:].double()
    d["e64"] = err.double()
    return d


def _ratio(got, ref, bound):
    r = ((got - ref).abs() / bound).max().item()
    assert r == r, "NaN"
    return r


@pytest.mark.parametrize("cell", sorted(CELLS))
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_forward_steps(i, cell):
    d = case(i, cell)
    B, H, T, ng = d["B"], d["H"], d["T"], d["ng"]
    es, et = e_fn()
    if ng == 4:
        ref = torch.nn.LSTMCell(4 * H, H).double()
    else:
        ref = torch.nn.RNNCell(H, H, nonlinearity="tanh").double()
    with torch.no_grad():
        ref.weight_ih.copy_(torch.eye(ng * H, dtype=torch.float64))
        ref.weight_hh.copy_(d["wh"])
        ref.bias_ih.zero_()
        ref.bias_hh.zero_()
    worst = {}
    zero = torch.zeros(B, H, dtype=torch.float64)
    for t in range(T):
        hp = d["h"][:, t - 1] if t else zero
        xg = d["xg"][:, t]
        e_pre = (H + 4) * U24 * (hp.abs() @ d["wh"].abs().t() + xg.abs())
        pre = xg + hp @ d["wh"].t()
        with torch.no_grad():
            if ng == 4:
                cp = d["c"][:, t - 1] if t else zero
                h64, c64 = ref(xg, (hp, cp))
            else:
                h64 = ref(xg, hp)
        if ng == 1:
            e_h = e_pre + et + 8 * U24
            worst["h"] = max(worst.get("h", 0), _ratio(
                d["h"][:, t], h64, e_h + U9 * h64.abs()))
            continue
        p = pre.split(H, 1)
        e = e_pre.split(H, 1)
        gi, gf, go = (torch.sigmoid(p[k]) for k in (0, 1, 3))
        gg = torch.tanh(p[2])
        e_i, e_f, e_o = (0.25 * e[k] + es + 8 * U24 for k in (0, 1, 3))
        e_g = e[2] + et + 8 * U24
        g64 = torch.cat((gi, gf, gg, go), 1)
        e_gate = torch.cat((e_i, e_f, e_g, e_o), 1)
        worst["gates"] = max(worst.get("gates", 0), _ratio(
            d["gates"][:, t], g64, e_gate + U9 * g64.abs()))
        e_c = cp.abs() * e_f + gg.abs() * e_i + gi * e_g + \
            8 * U24 * ((gf * cp).abs() + (gi * gg).abs())
        worst["c"] = max(worst.get("c", 0), _ratio(d["c"][:, t], c64, e_c))
        tc = torch.tanh(c64)
        e_h = tc.abs() * e_o + go * (e_c + et) + 8 * U24 * h64.abs()
        worst["h"] = max(worst.get("h", 0), _ratio(
            d["h"][:, t], h64, e_h + U9 * h64.abs()))
    print("fwd %s %s max err / bound:" % (cell, IDS[i]),
          " ".join("%s %.3f" % kv for kv in sorted(worst.items())))
    assert max(worst.values()) <= 1.0, worst
    if i == SAT:
        for k in ("h", "c", "gates"):
            if k in d:
                assert torch.isfinite(d[k]).all(), k
        if ng == 4:
            gt = d["gates"].reshape(B, T, 4, H)
            sig = gt[:, :, (0, 1, 3)]
            assert ((sig == 0) | (sig == 1)).all()
            assert (gt[:, :, 2].abs() == 1).all()
        else:
            assert (d["h"].abs() == 1).all()


@pytest.mark.parametrize("cell", sorted(CELLS))
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_backward_steps(i, cell):
    d = case(i, cell)
    B, H, T, ng = d["B"], d["H"], d["T"], d["ng"]
    es, et = e_fn()
    del es
    worst = {}
    zero = torch.zeros(B, H, dtype=torch.float64)
    dg = d["dg"]
    assert torch.isfinite(dg).all()
    for t in range(T - 1, -1, -1):
        last = t == T - 1
        e_t = d["e64"][:, t]
        if last:
            dh, e_dh = e_t, 4 * U24 * e_t.abs()
        else:
            dh = e_t + dg[:, t + 1] @ d["wh"]
            e_dh = (ng * H + 4) * U24 * (
                dg[:, t + 1].abs() @ d["wh"].abs() + e_t.abs())
        if ng == 1:
            ht = d["h"][:, t]
            ref = dh * (1 - ht * ht)
            bound = e_dh * (1 - ht * ht).abs() + 8 * U24 * ref.abs() + \
                U9 * ref.abs()
            worst["dg"] = max(worst.get("dg", 0),
                              _ratio(dg[:, t], ref, bound + 1e-45))
            continue
        gi, gf, gg, go = d["gates"][:, t].split(H, 1)
        cp = d["c"][:, t - 1] if t else zero
        tc = torch.tanh(d["c"][:, t])
        dci = zero if last else d["dc"][t + 1]
        s = go * (1 - tc * tc)
        dcr = dci + dh * s
        e_dcr = e_dh * s.abs() + (dh * go).abs() * 2 * tc.abs() * et + \
            8 * U24 * (dci.abs() + (dh * s).abs())
        fo = tc * go * (1 - go)
        parts = ((dcr, e_dcr, gg * gi * (1 - gi)),
                 (dcr, e_dcr, cp * gf * (1 - gf)),
                 (dcr, e_dcr, gi * (1 - gg * gg)),
                 (dh, e_dh + dh.abs() * et / (tc.abs() + 1e-300), fo))
        ref = torch.cat([a * f for a, _, f in parts], 1)
        bound = torch.cat([ea * f.abs() for _, ea, f in parts], 1) + \
            (8 * U24 + U9) * ref.abs()
        worst["dg"] = max(worst.get("dg", 0),
                          _ratio(dg[:, t], ref, bound + 1e-45))
        rdc = dcr * gf
        worst["dc"] = max(worst.get("dc", 0), _ratio(
            d["dc"][t], rdc, e_dcr * gf + 8 * U24 * rdc.abs() + 1e-45))
    print("bwd %s %s max err / bound:" % (cell, IDS[i]),
          " ".join("%s %.3f" % kv for kv in sorted(worst.items())))
    assert max(worst.values()) <= 1.0, worst


def _close(got, ref, tol):
    err = (got.double().cpu() - ref).abs().max().item()
    mag = ref.abs().max().item() + 1e-6
    print("   max err %.3g of scale %.3g (tolerance %g)" % (err, mag, tol))
    assert err <= tol * mag, "max err %g vs scale %g" % (err, mag)


@pytest.mark.parametrize("cell", sorted(CELLS))
@pytest.mark.parametrize("i", (3, 6, 7, 9), ids=[IDS[k] for k in (3, 6, 7, 9)])
def test_gradient_gemms(i, cell):
    """dw (both column slices), dbias and err_input from the GPU's own dG"""
    d = case(i, cell)
    B, T, I, H = d["B"], d["T"], d["I"], d["H"]
    dg = d["dg"].reshape(B * T, -1)
    x = d["x"].double().cpu().reshape(B * T, I)
    hp = torch.zeros(B, T, H, dtype=torch.float64)
    hp[:, 1:] = d["h"][:, :-1]
    w = d["w"].double().cpu()
    _close(d["dw"][:, :I], dg.t() @ x, 1e-3)
    _close(d["dw"][:, I:], dg.t() @ hp.reshape(B * T, H), 1e-3)
    _close(d["db"], dg.sum(0), 1e-3)
    _close(d["ei"].reshape(B * T, I), dg @ w[:, :I], 1e-2)


def _run(d, x=None, last_only=False):
    ng, I, H = d["ng"], d["I"], d["H"]
    x = d["x"] if x is None else x
    save = {}
    y = ops.lstm_fwd(x, d["w"], d["bias"], H, cell=d["cell"],
                     return_sequences=not last_only, save=save)
    dw = torch.zeros(ng * H, I + H, device=DEV)
    db = torch.zeros(ng * H, device=DEV)
    err = d["err"][:, -1] if last_only else d["err"]
    ei = ops.lstm_bwd(err, x, d["w"], save, dw, db, cell=d["cell"])
    torch.cuda.synchronize()
    return [t.clone() for t in (y, save["h"], save["dg"], dw, db, ei)]


@pytest.mark.parametrize("cell", sorted(CELLS))
def test_bit_identity(cell):
    d = case(6, cell)
    a, b = _run(d), _run(d)
    for u, v in zip(a[:3], b[:3]):      # step kernels: always
        assert torch.equal(u, v)
    ops.set_deterministic(True)
    try:
        a, b = _run(d), _run(d)
    finally:
        ops.set_deterministic(False)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


# (B, I, H, T): H = 7 is off the 8-element grid (scalar kernel path, padded
# pitch != width), H = 8 is on it (vector path)
CONTRACT = [(3, 5, 7, 2), (2, 8, 8, 2)]


@pytest.mark.parametrize("cell", sorted(CELLS))
@pytest.mark.parametrize("shape", CONTRACT, ids=("H7", "H8"))
def test_save_contract(shape, cell):
    """what fwd + bwd leave in ``save`` (docs/OPS.md): the public keys with
    their shapes and dtypes, and the padded buffers behind them"""
    B, I, H, T = shape
    ng = CELLS[cell]
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, T, I, generator=g).to(BF).to(DEV)
    w = (torch.randn(ng * H, I + H, generator=g) / (I + H) ** 0.5).to(BF) \
        .to(DEV)
    b = torch.randn(ng * H, generator=g).to(DEV)
    err = torch.randn(B, H, generator=g).to(BF).to(DEV)
    save = {}
    ops.lstm_fwd(x, w, b, H, cell=cell, save=save)
    ops.lstm_bwd(err, x, w, save, torch.zeros(ng * H, I + H, device=DEV),
                 torch.zeros(ng * H, device=DEV), cell=cell)
    torch.cuda.synchronize()
    f32 = torch.float32
    want = {"h": ((B, T, H), BF), "xg": ((B, T, ng * H), f32),
            "dg": ((B, T, ng * H), BF)}
    pads = ["_xg", "_dg"]
    if cell == "lstm":
        want.update(c=((B, T, H), f32), gates=((B, T, 4 * H), BF),
                    dc=((T, B, H), f32))
        pads.append("_gates")
    assert {k for k in save if not k.startswith("_")} == set(want)
    for k, (shape, dt) in want.items():
        assert tuple(save[k].shape) == shape and save[k].dtype == dt, k
    P = -(-ng * H // 8) * 8
    for k in pads:
        assert tuple(save[k].shape) == (B, T, P), k
    for k in ("xg", "dg") + (("gates",) if cell == "lstm" else ()):
        assert save[k].data_ptr() == save["_" + k].data_ptr(), k
        assert save[k].stride() == (T * P, P, 1), k


@pytest.mark.parametrize("last_only", (False, True))
def test_strided_input(last_only):
    """a [B][T][.] view with a padded pitch gives the bits of a contiguous
    copy"""
    d = case(6, "lstm")
    B, T, I = d["B"], d["T"], d["I"]
    buf = torch.zeros(B, T, I + 24, dtype=BF, device=DEV)
    xs = buf[:, :, :I]
    xs.copy_(d["x"])
    assert not xs.is_contiguous()
    ops.set_deterministic(True)
    try:
        a, b = _run(d, last_only=last_only), _run(d, xs, last_only=last_only)
    finally:
        ops.set_deterministic(False)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_graph_capture():
    """T-step forward + backward captured once on the current stream (a
    linear chain), replayed twice after the operands changed"""
    d = case(6, "lstm")
    ng, I, H = d["ng"], d["I"], d["H"]
    x, w, bias, err = (d[k].clone() for k in ("x", "w", "bias", "err"))
    dw = torch.zeros(ng * H, I + H, device=DEV)
    db = torch.zeros(ng * H, device=DEV)
    save = {}
    ops.set_deterministic(True)
    try:
        def step():
            y = ops.lstm_fwd(x, w, bias, H, return_sequences=True, save=save)
            ei = ops.lstm_bwd(err, x, w, save, dw, db)
            return y, ei
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            step()       # warm-up: every buffer of ``save`` exists now
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y, ei = step()
        for k in (1, 2):
            g = torch.Generator().manual_seed(900 + k)
            x.copy_(torch.randn(x.shape, generator=g).to(BF))
            err.copy_(torch.randn(err.shape, generator=g).to(BF))
            w.copy_((torch.randn(w.shape, generator=g) / (I + H) ** 0.5)
                    .to(BF))
            graph.replay()
            torch.cuda.synchronize()
            got = [t.clone() for t in (y, save["dg"], dw, db, ei)]
            e = dict(d, x=x, w=w, bias=bias, err=err)
            ref = _run(e)
            for u, v in zip(got, [ref[0]] + ref[2:]):
                assert torch.equal(u, v)
    finally:
        ops.set_deterministic(False)


def test_host_checks_raise_before_any_launch():
    d = case(1, "lstm")
    x, w, b, H = d["x"], d["w"], d["bias"], d["H"]
    with pytest.raises(TypeError):
        ops.lstm_fwd(x.float(), w, b, H)
    with pytest.raises(TypeError):
        ops.lstm_fwd(x, w, b.to(BF), H)
    with pytest.raises(ValueError):
        ops.lstm_fwd(x, w[:-1], b, H)
    with pytest.raises(ValueError):
        ops.lstm_fwd(x, w, b, H, cell="gru")
    with pytest.raises(ValueError):
        ops.lstm_fwd(x.transpose(0, 1), w, b, H)
    with pytest.raises(ValueError):
        ops.lstm_fwd(x, w.t().contiguous().t(), b, H)
    with pytest.raises(ValueError):
        ops.lstm_fwd(x, w, b.cpu(), H)
    save = dict(d["save"])
    dw = torch.zeros_like(d["dw"])
    with pytest.raises(ValueError):
        ops.lstm_bwd(d["err"][:, :, :-1], x, w, save, dw, None)
    with pytest.raises(TypeError):
        ops.lstm_bwd(d["err"].float(), x, w, save, dw, None)
    with pytest.raises(ValueError):
        ops.lstm_bwd(d["err"], x, w, save, dw.to(BF), None)
    with pytest.raises(ValueError):
        ops.lstm_bwd(d["err"], x, w, {}, dw, None)
    torch.cuda.synchronize()
    assert not dw.any()


# validation errors of seeds 1 .. 5 on the CPU device after the sample's 25
# epochs (tests/test_recurrent_sample.py): 0, 0, 0, 0, 0 of 256
CPU_SEED_ERRORS = (0, 0, 0, 0, 0)


def test_sample_trains_on_the_gpu(tmp_path):
    import json
    import subprocess
    import sys
    res = tmp_path / "results.json"
    r = subprocess.run(
        [sys.executable, "-m", "veles_amd", "samples/seq_recall.py", "-",
         "-r", "1", "--result-file", str(res),
         "root.common.disable.snapshotting=True"], cwd=REPO,
        env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True,
        timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "<CpuDevice>" not in r.stdout + r.stderr
    h = json.loads(res.read_text())["Epoch history"]
    assert len(h) == 25
    n_valid = 256
    errors = [round(e["validation_err_pt"] * n_valid / 100.0) for e in h]
    print("validation errors per epoch:", errors)
    assert errors[-1] <= max(CPU_SEED_ERRORS) + 0.01 * n_valid, errors
