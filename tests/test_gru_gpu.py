"""The fused gfx950 GRU step kernels (csrc/kernels/recurrent.hip) and
ops.gru_fwd / gru_bwd on the GPU.

Step kernels, teacher-forced: every step is checked on its own, from the
GPU's OWN stored tensors (h, hf, hn, gates, xg, dgx, dgh, dcarry and the bf16
weights) fed to the float64 formula of docs/OPS.md "GRU" (pinned to
torch.nn.GRUCell by tests/test_gru.py), so the bound is local and derivable.
Every element of every step is compared.

* accumulation: e_acc = (K + 4) 2^-24 (sum|a||b| + |addend|); the bf16 x
  bf16 products are exact in f32, K + 4 covers the MFMA chain, the 3
  additions of the 4 K-split partial sums and the additions of the addends
  (forward K = H with xg or b_hn, backward K = 3H with err and dcarry);
* every transcendental: e_fn, measured in the same GPU run through the
  existing hvk_recurrent_fn (the cell's device sigmoid / tanh against
  float64 on 2^16 points of [-20, 20]), taken TWICE because sampling does
  not reach every input;
* pushed through the cell with the Lipschitz constants (sigmoid 1/4, tanh
  1) and the partial derivatives of the GRU equations:
      e_r, e_z = e_acc / 4 + e_sigmoid + 8 u
      e_n = |hn| e_r + r e_hn + e_r e_hn + 4 u (|xg_n| + |r hn|)
            + e_tanh + 8 u
      e_h = |n - h_prev| e_z + (1 - z) e_n + e_z e_n
            + 8 u (|(1 - z) n| + |z h_prev|)
  with u = 2^-24 for the few multiply-adds of an output;
* the backward has no transcendental and reads its gate factors exactly as
  stored, so a gradient errs by e_dh times its factor plus 8 u relative;
* half a bf16 ulp, 2^-8 relative (U9), for every bf16 store (h, gates, dgx,
  dgh) and none for the float32 stores (hf, hn, dcarry);
* TINY: the kernels flush denormals (below 2^-126) to zero.

Whole layer: the gradient GEMMs and the b_hn sums against float64 products
of the GPU's own dGx / dGh with the tolerance of the existing bf16 GEMM
tests (1e-2 of the largest reference magnitude for a bf16 output, 1e-3 for
float32).  Figures of the development run: profiles/gru/gpu_tests_figures.txt.
"""
import functools

import pytest
import torch

import veles_amd.ops as ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
U24, U9 = 2.0 ** -24, 2.0 ** -8
TINY = 8 * 2.0 ** -126

# (B, I, H, T), the list of tests/test_recurrent_gpu.py; the tile is 16
# hidden units x 32 batch rows, K chunks of 32 dealt to 4 waves
CASES = [
    (1, 8, 8, 1),       # degenerate: one step, no product
    (3, 8, 16, 2),      # the smallest shape with the recurrent product
    (32, 32, 16, 3),    # exactly one tile
    (31, 32, 16, 3),    # ... and its neighbours: one row short,
    (33, 32, 24, 3),    # one row / one 8-column group over
    (64, 32, 64, 3),    # 2 x 4 whole tiles
    (65, 40, 72, 4),    # partial tiles in both dimensions
    (130, 24, 136, 5),  # several tiles, partial last K chunk (K = 136, 408)
    (32, 16, 264, 3),   # many hidden tiles, K over 256 (every wave loops)
    (17, 5, 20, 3),     # I and H off the 8-grid: the guarded element path
    (33, 8, 64, 3),     # saturated: projection biases of +-200
]
SAT = len(CASES) - 1
IDS = ["%dx%dx%dx%d" % c for c in CASES]
ALL = range(len(CASES))


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
def case(i):
    """One forward + backward of case i on the GPU, everything the checks
    need copied to the host once as float64."""
    B, I, H, T = CASES[i]
    g = torch.Generator().manual_seed(500 + i)
    x = torch.randn(B, T, I, generator=g).to(BF)
    w = (torch.randn(3 * H, I + H, generator=g) / (I + H) ** 0.5).to(BF)
    bias = torch.randn(4 * H, generator=g) * 0.5
    if i == SAT:
        # +-200 through the projection; b_hn and Wh at normal scale
        bias[:3 * H] = torch.where(torch.rand(3 * H, generator=g) < 0.5,
                                   -200., 200.)
    err = torch.randn(B, T, H, generator=g).to(BF)
    d = dict(x=x.to(DEV), w=w.to(DEV), bias=bias.to(DEV), err=err.to(DEV),
             B=B, I=I, H=H, T=T)
    d["save"] = save = {}
    d["out"] = ops.gru_fwd(d["x"], d["w"], d["bias"], H,
                           return_sequences=True, save=save)
    d["dw"] = torch.full((3 * H, I + H), 3.0, device=DEV)
    d["db"] = torch.full((4 * H,), 3.0, device=DEV)
    d["ei"] = ops.gru_bwd(d["err"], d["x"], d["w"], save, d["dw"], d["db"])
    torch.cuda.synchronize()
    for k in ("h", "hf", "hn", "gates", "xg", "dgx", "dgh", "dcarry"):
        d[k] = save[k].double().cpu()
    d["wh"] = w[:, I:].double()
    d["bhn"] = bias[3 * H:].double()
    d["e64"] = err.double()
    return d


def _ratio(got, ref, bound):
    r = ((got - ref).abs() / (bound + TINY)).max().item()
    assert r == r, "NaN"
    return r


def _up(worst, key, r):
    worst[key] = max(worst.get(key, 0.0), r)


@pytest.mark.parametrize("i", ALL, ids=IDS)
def test_forward_steps(i):
    d = case(i)
    B, H, T = d["B"], d["H"], d["T"]
    es, et = e_fn()
    wh, wa = d["wh"], d["wh"].abs()
    assert d["out"].data_ptr() == d["save"]["h"].data_ptr()
    for k in ("h", "hf", "hn", "gates"):
        assert torch.isfinite(d[k]).all(), k
    worst = {}
    zero = torch.zeros(B, H, dtype=torch.float64)
    for t in range(T):
        hp = d["h"][:, t - 1] if t else zero        # the MFMA operand
        hfp = d["hf"][:, t - 1] if t else zero      # the carry
        xg = d["xg"][:, t].split(H, 1)
        s = (hp @ wh.t()).split(H, 1)
        sa = (hp.abs() @ wa.t()).split(H, 1)
        acc = (H + 4) * U24
        r = torch.sigmoid(xg[0] + s[0])
        z = torch.sigmoid(xg[1] + s[1])
        e_r = 0.25 * acc * (sa[0] + xg[0].abs()) + es + 8 * U24
        e_z = 0.25 * acc * (sa[1] + xg[1].abs()) + es + 8 * U24
        hn = s[2] + d["bhn"]
        e_hn = acc * (sa[2] + d["bhn"].abs())
        n = torch.tanh(xg[2] + r * hn)
        e_n = hn.abs() * e_r + r * e_hn + e_r * e_hn + \
            4 * U24 * (xg[2].abs() + (r * hn).abs()) + et + 8 * U24
        h = (1 - z) * n + z * hfp
        e_h = (n - hfp).abs() * e_z + (1 - z) * e_n + e_z * e_n + \
            8 * U24 * (((1 - z) * n).abs() + (z * hfp).abs())
        g64 = torch.cat((r, z, n), 1)
        e_g = torch.cat((e_r, e_z, e_n), 1)
        _up(worst, "gates", _ratio(d["gates"][:, t], g64,
                                   e_g + U9 * g64.abs()))
        _up(worst, "hn", _ratio(d["hn"][:, t], hn, e_hn))
        _up(worst, "hf", _ratio(d["hf"][:, t], h, e_h))
        _up(worst, "h", _ratio(d["h"][:, t], h, e_h + U9 * h.abs()))
        # the bf16 h is the rounded float32 h, not a second computation
        assert torch.equal(d["h"][:, t], d["hf"][:, t].float().to(BF).double())
    print("fwd gru %s max err / bound:" % IDS[i],
          " ".join("%s %.3f" % kv for kv in sorted(worst.items())))
    assert max(worst.values()) <= 1.0, worst
    if i == SAT:
        gt = d["gates"].reshape(B, T, 3, H)
        sig = gt[:, :, :2]
        assert ((sig == 0) | (sig == 1)).all()
        assert (gt[:, :, 2].abs() == 1).all()
        z1 = gt[:, :, 1] == 1
        assert z1.any() and (~z1).any()
        for k in ("hf", "h"):
            prev = torch.cat((torch.zeros(B, 1, H, dtype=torch.float64),
                              d[k][:, :-1]), 1)
            assert torch.equal(d[k][z1], prev[z1]), k
            # and z = 0 takes the candidate exactly
            assert torch.equal(d[k][~z1], gt[:, :, 2][~z1]), k


@pytest.mark.parametrize("i", ALL, ids=IDS)
def test_backward_steps(i):
    d = case(i)
    B, H, T = d["B"], d["H"], d["T"]
    wh, wa = d["wh"], d["wh"].abs()
    dgx, dgh, dc = d["dgx"], d["dgh"], d["dcarry"]
    for k in ("dgx", "dgh", "dcarry"):
        assert torch.isfinite(d[k]).all(), k
    worst = {}
    zero = torch.zeros(B, H, dtype=torch.float64)
    for t in range(T - 1, -1, -1):
        last = t == T - 1
        e_t = d["e64"][:, t]
        if last:
            dh, e_dh = e_t, 4 * U24 * e_t.abs()
        else:
            dh = e_t + dgh[:, t + 1] @ wh + dc[t + 1]
            e_dh = (3 * H + 4) * U24 * (dgh[:, t + 1].abs() @ wa +
                                        e_t.abs() + dc[t + 1].abs())
        r, z, n = d["gates"][:, t].split(H, 1)
        hn = d["hn"][:, t]
        hfp = d["hf"][:, t - 1] if t else zero
        f_n = (1 - z) * (1 - n * n)
        f_z = (hfp - n) * z * (1 - z)
        f_r = f_n * hn * r * (1 - r)
        f_x = torch.cat((f_r, f_z, f_n), 1)
        f_h = torch.cat((f_r, f_z, f_n * r), 1)
        dh3, e3 = dh.repeat(1, 3), e_dh.repeat(1, 3)
        for key, got, f in (("dgx", dgx[:, t], f_x), ("dgh", dgh[:, t], f_h)):
            ref = dh3 * f
            _up(worst, key, _ratio(got, ref, e3 * f.abs() +
                                   (8 * U24 + U9) * ref.abs()))
        ref = dh * z
        _up(worst, "dcarry", _ratio(dc[t], ref,
                                    e_dh * z + 8 * U24 * ref.abs()))
    print("bwd gru %s max err / bound:" % IDS[i],
          " ".join("%s %.3f" % kv for kv in sorted(worst.items())))
    assert max(worst.values()) <= 1.0, worst


def _close(what, got, ref, tol):
    err = (got.double().cpu() - ref).abs().max().item()
    mag = ref.abs().max().item() + 1e-6
    print("   %s max err %.3g of scale %.3g (tolerance %g)" %
          (what, err, mag, tol))
    assert err <= tol * mag, "%s: max err %g vs scale %g" % (what, err, mag)


@pytest.mark.parametrize("i", ALL, ids=IDS)
def test_gradient_gemms(i):
    """dw (both column slices), all four dbias blocks and err_input from the
    GPU's own dGx / dGh"""
    d = case(i)
    B, T, I, H = d["B"], d["T"], d["I"], d["H"]
    gx = d["dgx"].reshape(B * T, -1)
    gh = d["dgh"].reshape(B * T, -1)
    x = d["x"].double().cpu().reshape(B * T, I)
    hp = torch.zeros(B, T, H, dtype=torch.float64)
    hp[:, 1:] = d["h"][:, :-1]
    w = d["w"].double().cpu()
    _close("dw[:, :I]", d["dw"][:, :I], gx.t() @ x, 1e-3)
    _close("dw[:, I:]", d["dw"][:, I:], gh.t() @ hp.reshape(B * T, H), 1e-3)
    _close("dbias[:3H]", d["db"][:3 * H], gx.sum(0), 1e-3)
    _close("dbias[3H:]", d["db"][3 * H:], gh[:, 2 * H:].sum(0), 1e-3)
    _close("err_input", d["ei"].reshape(B * T, I), gx @ w[:, :I], 1e-2)


def _run(d, x=None, last_only=False, save=None):
    I, H = d["I"], d["H"]
    x = d["x"] if x is None else x
    save = {} if save is None else save
    y = ops.gru_fwd(x, d["w"], d["bias"], H, return_sequences=not last_only,
                    save=save)
    dw = torch.zeros(3 * H, I + H, device=DEV)
    db = torch.zeros(4 * H, device=DEV)
    err = d["err"][:, -1] if last_only else d["err"]
    ei = ops.gru_bwd(err, x, d["w"], save, dw, db)
    torch.cuda.synchronize()
    return [t.clone() for t in (y, save["h"], save["hf"], save["hn"],
                                save["dgx"], save["dgh"], save["dcarry"],
                                dw, db, ei)]


N_STEP = 7      # the outputs of _run that the step kernels alone write


def test_bit_identity_and_buffer_reuse():
    d = case(6)
    save = {}
    a = _run(d, save=save)
    ptrs = {k: v.data_ptr() for k, v in save.items()}
    b = _run(d, save=save)
    assert ptrs == {k: v.data_ptr() for k, v in save.items()}
    for u, v in zip(a[:N_STEP], b[:N_STEP]):      # step kernels: always
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


@pytest.mark.parametrize("shape", CONTRACT, ids=("H7", "H8"))
def test_save_contract(shape):
    """what fwd + bwd leave in ``save`` (the table of docs/OPS.md "GRU"): the
    public keys with their shapes and dtypes, and the padded buffers behind
    them"""
    B, I, H, T = shape
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, T, I, generator=g).to(BF).to(DEV)
    w = (torch.randn(3 * H, I + H, generator=g) / (I + H) ** 0.5).to(BF) \
        .to(DEV)
    b = torch.randn(4 * H, generator=g).to(DEV)
    err = torch.randn(B, H, generator=g).to(BF).to(DEV)
    save = {}
    ops.gru_fwd(x, w, b, H, save=save)
    ops.gru_bwd(err, x, w, save, torch.zeros(3 * H, I + H, device=DEV),
                torch.zeros(4 * H, device=DEV))
    torch.cuda.synchronize()
    f32 = torch.float32
    want = {"h": ((B, T, H), BF), "hf": ((B, T, H), f32),
            "hn": ((B, T, H), f32), "gates": ((B, T, 3 * H), BF),
            "xg": ((B, T, 3 * H), f32), "dgx": ((B, T, 3 * H), BF),
            "dgh": ((B, T, 3 * H), BF), "dcarry": ((T, B, H), f32)}
    assert {k for k in save if not k.startswith("_")} == set(want)
    for k, (shape, dt) in want.items():
        assert tuple(save[k].shape) == shape and save[k].dtype == dt, k
    P = -(-3 * H // 8) * 8
    for k in ("xg", "gates", "dgx", "dgh"):
        assert tuple(save["_" + k].shape) == (B, T, P), k
        assert save[k].data_ptr() == save["_" + k].data_ptr(), k
        assert save[k].stride() == (T * P, P, 1), k


def test_save_none_stores_no_gates_and_last_step_output():
    d = case(6)
    ws = {}
    y = ops.gru_fwd(d["x"], d["w"], d["bias"], d["H"], ws=ws)
    torch.cuda.synchronize()
    assert "gates" not in ws and "_gates" not in ws and "xg" not in ws
    assert torch.equal(y, d["out"][:, -1])
    out = torch.empty_like(y)
    assert ops.gru_fwd(d["x"], d["w"], d["bias"], d["H"], ws=ws,
                       out=out) is out
    assert torch.equal(out, y)
    with pytest.raises(ValueError):
        ops.gru_bwd(d["err"], d["x"], d["w"], ws, torch.zeros_like(d["dw"]),
                    None)


@pytest.mark.parametrize("last_only", (False, True))
def test_strided_input(last_only):
    """a [B][T][.] view with a padded pitch gives the bits of a contiguous
    copy"""
    d = case(6)
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
    d = case(6)
    I, H = d["I"], d["H"]
    x, w, bias, err = (d[k].clone() for k in ("x", "w", "bias", "err"))
    dw = torch.zeros(3 * H, I + H, device=DEV)
    db = torch.zeros(4 * H, device=DEV)
    ei = torch.empty(d["B"], d["T"], I, dtype=BF, device=DEV)
    save = {}
    ops.set_deterministic(True)
    try:
        def step():
            y = ops.gru_fwd(x, w, bias, H, return_sequences=True, save=save)
            ops.gru_bwd(err, x, w, save, dw, db, err_input=ei)
            return y
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            step()       # warm-up: every buffer of ``save`` exists now
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = step()
        for k in (1, 2):
            g = torch.Generator().manual_seed(900 + k)
            x.copy_(torch.randn(x.shape, generator=g).to(BF))
            err.copy_(torch.randn(err.shape, generator=g).to(BF))
            w.copy_((torch.randn(w.shape, generator=g) / (I + H) ** 0.5)
                    .to(BF))
            bias.copy_(torch.randn(bias.shape, generator=g) * 0.5)
            graph.replay()
            torch.cuda.synchronize()
            got = [t.clone() for t in (
                y, save["h"], save["hf"], save["hn"], save["dgx"],
                save["dgh"], save["dcarry"], dw, db, ei)]
            ref = _run(dict(d, x=x, w=w, bias=bias, err=err))
            for u, v in zip(got, ref):
                assert torch.equal(u, v)
    finally:
        ops.set_deterministic(False)


def test_host_checks_raise_before_any_launch():
    d = case(1)
    x, w, b, H = d["x"], d["w"], d["bias"], d["H"]
    with pytest.raises(TypeError):
        ops.gru_fwd(x.float(), w, b, H)
    with pytest.raises(TypeError):
        ops.gru_fwd(x, w, b.to(BF), H)
    with pytest.raises(ValueError):
        ops.gru_fwd(x, w[:-1], b, H)
    with pytest.raises(ValueError):
        ops.gru_fwd(x, w, b[:3 * H], H)
    with pytest.raises(ValueError):
        ops.gru_fwd(x.transpose(0, 1), w, b, H)
    with pytest.raises(ValueError):
        ops.gru_fwd(x, w.t().contiguous().t(), b, H)
    with pytest.raises(ValueError):
        ops.gru_fwd(x, w, b.cpu(), H)
    with pytest.raises(ValueError):
        ops.lstm_fwd(x, w, b[:3 * H], H, cell="gru")
    save = dict(d["save"])
    dw = torch.zeros_like(d["dw"])
    with pytest.raises(ValueError):
        ops.gru_bwd(d["err"][:, :, :-1], x, w, save, dw, None)
    with pytest.raises(TypeError):
        ops.gru_bwd(d["err"].float(), x, w, save, dw, None)
    with pytest.raises(ValueError):
        ops.gru_bwd(d["err"], x, w, save, dw.to(BF), None)
    with pytest.raises(ValueError):
        ops.gru_bwd(d["err"], x, w, save, dw, d["db"][:3 * H])
    with pytest.raises(ValueError):
        ops.gru_bwd(d["err"], x, w, {}, dw, None)
    with pytest.raises(ValueError):    # gates that are not gru_fwd's buffer
        ops.gru_bwd(d["err"], x, w, dict(save, gates=save["gates"].clone()),
                    dw, None)
    torch.cuda.synchronize()
    assert not dw.any()


def test_kernel_entry_points_refuse_bad_arguments():
    """unsupported arguments return -1 without a launch"""
    fwd, bwd = ops._rec_fn("hvk_gru_step_fwd"), ops._rec_fn("hvk_gru_step_bwd")
    d = case(1)
    B, H = d["B"], d["H"]
    sv = d["save"]
    xg, h, hf, hn = (sv[k].data_ptr() for k in ("_xg", "h", "hf", "hn"))
    s = ops._s(d["x"])
    P = sv["_xg"].shape[2]
    T = d["T"]

    def f(B_=B, H_=H, xg_=xg, ld_xg=T * P, ld_h=T * H, h_=h):
        return fwd(B_, H_, None, 0, None, 0, xg_, ld_xg, None, 0, hf, T * H,
                   hn, T * H, h_, ld_h, None, 0, None, s)
    assert f(B_=0) == -1 and f(H_=0) == -1 and f(xg_=None) == -1
    assert f(h_=None) == -1 and f(ld_xg=3 * H - 1) == -1
    assert f(ld_h=H - 1) == -1
    g, dgx, dgh, dc = (sv[k].data_ptr() for k in
                       ("_gates", "_dgx", "_dgh", "dcarry"))

    def b(g_=g, ld_g=T * P, dc_=dc, ld_dgx=T * P, dgn=None):
        return bwd(B, H, dgn, T * P, None, P, None, 0, g_, ld_g, hn, T * H,
                   None, 0, None, 0, dc_, H, dgx, ld_dgx, dgh, T * P, s)
    assert b(g_=None) == -1 and b(ld_g=3 * H - 1) == -1
    assert b(dc_=None) == -1 and b(ld_dgx=1) == -1
    assert b(dgn=dgh) == -1          # a product without WhT
    torch.cuda.synchronize()


def test_gru_layer_trains_on_the_gpu():
    """gru -> gru -> softmax on the GPU device, 60 SGD steps of seq_recall:
    the loss starts at chance (ln 8 = 2.08) and falls"""
    from veles_amd.backends import Device
    from veles_amd.dummy import DummyLauncher
    from veles_amd.models import StandardWorkflow
    from veles_amd.prng import random_generator
    from veles_amd.utils.config import root
    import veles_amd.loader  # noqa: F401
    root.common.disable.snapshotting = True
    random_generator.get().seed(4)
    B, K = 64, 60
    g = {"learning_rate": 1.0, "learning_rate_bias": 1.0,
         "gradient_moment": 0.9, "gradient_moment_bias": 0.9}
    layers = [{"type": "gru", "->": {"output_sample_shape": 24,
                                     "return_sequences": True},
               "<-": dict(g)},
              {"type": "gru", "->": {"output_sample_shape": 16},
               "<-": dict(g)},
              {"type": "softmax", "->": {"output_sample_shape": 8},
               "<-": dict(g)}]
    wf = StandardWorkflow(
        DummyLauncher(), loader_name="seq_recall",
        loader_config={"steps": 4, "features": 8,
                       "class_lengths": (0, 0, B * K), "minibatch_size": B,
                       "seed": 3},
        layers=layers, decision_config={"max_epochs": None,
                                        "fail_iterations": 100})
    wf.initialize(device=Device(backend="hip"))
    assert wf.forwards[0].weights_lp.is_cuda
    loss = []
    for _ in range(K):
        wf.run_steps(1)
        lab = wf.loader.minibatch_labels.devmem.long()
        p = wf.forwards[-1].output.devmem.double()
        loss.append(-torch.log(p[torch.arange(B, device=DEV), lab])
                    .mean().item())
    for f in wf.forwards:
        assert torch.isfinite(f.weights_master).all()
        assert torch.isfinite(f.bias_master).all()
    assert wf.forwards[0].save_["gates"].dtype == BF
    print("loss every 5th step:", " ".join("%.3f" % v for v in loss[::5]))
    first, last = sum(loss[:5]) / 5, sum(loss[-5:]) / 5
    assert abs(first - 2.08) < 0.2 and last < first, (first, last)
