"""Reverse and bidirectional recurrent layers on the GPU: the paired step
launches (hvk_lstm_step_fwd2 / _bwd2, hvk_gru_step_fwd2 / _bwd2) behind
``direction="both"`` and the one-direction kernels walked backwards behind
``direction="reverse"``.

Primary check, tolerance-free: per direction a paired launch must do exactly
what a one-direction launch does.  tests/test_recurrent_gpu.py and
tests/test_gru_gpu.py hold the one-direction kernels to float64 at these
tile edges; here every direction of the op is re-run as a host-side chain of
the one-direction entry points over T steps, from the op's own projection
(``xg`` slice) and weights into fresh contiguous buffers, and every tensor
the step kernels write must equal the op's direction slice bit for bit.  That
carries the float64 result over to the paired launch, the blockIdx.z
argument select and the [B][T][2H] pitches.

The gradient GEMMs are compared with float64 products of the GPU's own dG
and h (tolerance of the one-direction files' test_gradient_gemms: 1e-3 of
the largest reference magnitude for float32 outputs, 1e-2 for bf16), with
Hprev shifted per direction: h^f_{t-1} forward, h^r_{t+1} reverse.
"""
import functools

import pytest
import torch

import veles_amd.ops as ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
NG = {"lstm": 4, "rnn": 1, "gru": 3}
BB = {"lstm": 4, "rnn": 1, "gru": 4}
CELLS = ("lstm", "rnn", "gru")

# (B, I, H, T); the tile is 16 hidden units x 32 batch rows
CASES = [
    (1, 8, 8, 1),       # one step: both directions meet at the only t
    (3, 8, 16, 2),      # the smallest shape with the recurrent product
    (33, 32, 24, 3),    # odd T: both directions write the middle step in one
                        # launch; partial tiles; reverse half 48 B in (vector)
    (65, 40, 72, 4),    # partial tiles both ways, even T
    (17, 5, 20, 3),     # reverse half off the 16-B grid: element path
    (32, 16, 264, 3),   # K over 256
]
IDS = ["%dx%dx%dx%d" % c for c in CASES]
ALL = range(len(CASES))
MID = 2                 # the case of the single-shape tests
DIRS = {"forward": ((0, False),), "reverse": ((0, True),),
        "both": ((0, False), (1, True))}


def r8(n):
    return -(-n // 8) * 8


def fwd_op(cell, x, w, b, H, **kw):
    if cell == "gru":
        return ops.gru_fwd(x, w, b, H, **kw)
    return ops.lstm_fwd(x, w, b, H, cell=cell, **kw)


def bwd_op(cell, err, x, w, save, dw, db, **kw):
    if cell == "gru":
        return ops.gru_bwd(err, x, w, save, dw, db, **kw)
    return ops.lstm_bwd(err, x, w, save, dw, db, cell=cell, **kw)


def step_keys(cell):
    """the save tensors the step kernels alone write"""
    return {"lstm": ("h", "c", "gates", "dg", "dc"),
            "rnn": ("h", "dg"),
            "gru": ("h", "hf", "hn", "gates", "dgx", "dgh", "dcarry")}[cell]


def operands(cell, i, D=2, seed=700):
    B, I, H, T = CASES[i]
    g = torch.Generator().manual_seed(seed + i)
    x = torch.randn(B, T, I, generator=g).to(BF)
    w = (torch.randn(D * NG[cell] * H, I + H, generator=g) /
         (I + H) ** 0.5).to(BF)
    bias = torch.randn(D * BB[cell] * H, generator=g) * 0.5
    err = torch.randn(B, T, D * H, generator=g).to(BF)
    return x.to(DEV), w.to(DEV), bias.to(DEV), err.to(DEV)


def run(cell, x, w, bias, err, H, direction="both", save=None):
    """forward + backward; (y, the step kernels' tensors ..., dw, db, ei)"""
    D = len(DIRS[direction])
    I = x.shape[2]
    save = {} if save is None else save
    y = fwd_op(cell, x, w, bias, H, return_sequences=err.dim() == 3,
               save=save, direction=direction)
    dw = torch.full((D * NG[cell] * H, I + H), 3.0, device=DEV)
    db = torch.full((D * BB[cell] * H,), 3.0, device=DEV)
    ei = bwd_op(cell, err, x, w, save, dw, db, direction=direction)
    torch.cuda.synchronize()
    return [t.clone() for t in [y] + [save[k] for k in step_keys(cell)] +
            [dw, db, ei]]


@functools.lru_cache(maxsize=None)
def case(cell, i, direction="both"):
    B, I, H, T = CASES[i]
    D = len(DIRS[direction])
    x, w, bias, err = operands(cell, i, D)
    d = dict(x=x, w=w, bias=bias, err=err, B=B, I=I, H=H, T=T, D=D)
    d["save"] = save = {}
    d["out"] = fwd_op(cell, x, w, bias, H, return_sequences=True, save=save,
                      direction=direction)
    d["dw"] = torch.full((D * NG[cell] * H, I + H), 3.0, device=DEV)
    d["db"] = torch.full((D * BB[cell] * H,), 3.0, device=DEV)
    d["ei"] = bwd_op(cell, err, x, w, save, d["dw"], d["db"],
                     direction=direction)
    torch.cuda.synchronize()
    return d


# ---------------------------------------------- chains of one-direction steps
def _chk(rc, name):
    assert rc == 0, "%s returned %d" % (name, rc)


def chain(cell, d, di, rev):
    """Direction ``di`` of case ``d`` through the one-direction entry points,
    T forward and T backward launches into fresh buffers; returns the dict
    of what the step kernels wrote, [B][T][.] (dc / dcarry: [T][B][H])."""
    B, I, H, T, D = d["B"], d["I"], d["H"], d["T"], d["D"]
    sv, w, err = d["save"], d["w"], d["err"]
    ng = NG[cell]
    gh = ng * H
    P, PW = r8(gh), sv["_xg"].shape[2]
    s = ops._s(d["x"])
    z = lambda *shape, dt=BF: torch.zeros(*shape, dtype=dt, device=DEV)  # noqa
    f32 = torch.float32
    h, dc = z(B, T, H), z(T, B, H, dt=f32)
    pxg = sv["_xg"].data_ptr() + 4 * di * gh
    pw, ldw = w.data_ptr() + 2 * (I + di * gh * w.stride(0)), w.stride(0)
    pwt = sv["_wht"].data_ptr() + 2 * di * H * P
    pe, lde = err.data_ptr() + 2 * di * H, err.stride(0)
    ph, pdc = h.data_ptr(), dc.data_ptr()
    order = range(T - 1, -1, -1) if rev else range(T)
    if cell == "gru":
        fwd = ops._rec_fn("hvk_gru_step_fwd")
        bwd = ops._rec_fn("hvk_gru_step_bwd")
        hf, hn = z(B, T, H, dt=f32), z(B, T, H, dt=f32)
        g, dgx, dgh = z(B, T, P), z(B, T, P), z(B, T, P)
        phf, phn, pg = hf.data_ptr(), hn.data_ptr(), g.data_ptr()
        pdx, pdh = dgx.data_ptr(), dgh.data_ptr()
        pb = d["bias"].data_ptr() + 4 * (di * 4 * H + gh)
        prev = None
        for t in order:
            _chk(fwd(B, H, None if prev is None else ph + 2 * prev * H, T * H,
                     pw, ldw, pxg + 4 * t * PW, T * PW,
                     None if prev is None else phf + 4 * prev * H, T * H,
                     phf + 4 * t * H, T * H, phn + 4 * t * H, T * H,
                     ph + 2 * t * H, T * H, pg + 2 * t * P, T * P, pb, s),
                 "gru fwd")
            prev = t
        nxt = None
        for k, t in enumerate(reversed(order)):
            tp = (t + 1 if rev else t - 1) if k < T - 1 else None
            _chk(bwd(B, H, None if nxt is None else pdh + 2 * nxt * P, T * P,
                     pwt, P, pe + 2 * t * err.stride(1), lde,
                     pg + 2 * t * P, T * P, phn + 4 * t * H, T * H,
                     None if tp is None else phf + 4 * tp * H, T * H,
                     None if nxt is None else pdc + 4 * nxt * B * H, H,
                     pdc + 4 * t * B * H, H, pdx + 2 * t * P, T * P,
                     pdh + 2 * t * P, T * P, s), "gru bwd")
            nxt = t
        torch.cuda.synchronize()
        return dict(h=h, hf=hf, hn=hn, gates=g[:, :, :gh],
                    dgx=dgx[:, :, :gh], dgh=dgh[:, :, :gh], dcarry=dc)
    fwd = ops._rec_fn("hvk_lstm_step_fwd")
    bwd = ops._rec_fn("hvk_lstm_step_bwd")
    lstm = cell == "lstm"
    code = 0 if lstm else 1
    c, g, dg = z(B, T, H, dt=f32), z(B, T, P), z(B, T, P)
    pc, pg, pdg = c.data_ptr(), g.data_ptr(), dg.data_ptr()
    prev = None
    for t in order:
        _chk(fwd(code, B, H, None if prev is None else ph + 2 * prev * H,
                 T * H, pw, ldw, pxg + 4 * t * PW, T * PW,
                 None if prev is None or not lstm else pc + 4 * prev * H,
                 T * H, pc + 4 * t * H if lstm else None, T * H,
                 ph + 2 * t * H, T * H, pg + 2 * t * P if lstm else None,
                 T * P, s), "lstm fwd")
        prev = t
    nxt = None
    for k, t in enumerate(reversed(order)):
        tp = (t + 1 if rev else t - 1) if k < T - 1 else None
        _chk(bwd(code, B, H, None if nxt is None else pdg + 2 * nxt * P,
                 T * P, pwt, P, pe + 2 * t * err.stride(1), lde,
                 pg + 2 * t * P if lstm else ph + 2 * t * H,
                 T * P if lstm else T * H,
                 None if tp is None or not lstm else pc + 4 * tp * H, T * H,
                 pc + 4 * t * H if lstm else None, T * H,
                 None if nxt is None or not lstm else pdc + 4 * nxt * B * H,
                 H, pdc + 4 * t * B * H if lstm else None, H,
                 pdg + 2 * t * P, T * P, s), "lstm bwd")
        nxt = t
    torch.cuda.synchronize()
    out = dict(h=h, dg=dg[:, :, :gh])
    if lstm:
        out.update(c=c, gates=g[:, :, :gh], dc=dc)
    return out


def _slice(cell, key, t, di, H):
    wide = key in ("gates", "dg", "dgx", "dgh", "xg")
    W = NG[cell] * H if wide else H
    return t[..., di * W:(di + 1) * W]


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("i", ALL, ids=IDS)
def test_paired_launches_equal_the_one_direction_chain(i, cell):
    d = case(cell, i)
    for di, rev in DIRS["both"]:
        ref = chain(cell, d, di, rev)
        assert set(ref) == set(step_keys(cell))
        for k, want in ref.items():
            got = _slice(cell, k, d["save"][k], di, d["H"])
            assert got.shape == want.shape, (k, got.shape, want.shape)
            assert torch.equal(got, want), "direction %d: %s" % (di, k)
    assert d["out"].data_ptr() == d["save"]["h"].data_ptr()


def _close(what, got, ref, tol):
    err = (got.double().cpu() - ref).abs().max().item()
    mag = ref.abs().max().item() + 1e-6
    print("   %s max err %.3g of scale %.3g (tolerance %g)" %
          (what, err, mag, tol))
    assert err <= tol * mag, "%s: max err %g vs scale %g" % (what, err, mag)


def gemm_checks(cell, d, direction):
    """dw (both column slices), dbias and err_input from the GPU's own dG"""
    B, T, I, H = d["B"], d["T"], d["I"], d["H"]
    gh, bb = NG[cell] * H, BB[cell] * H
    sv = d["save"]
    x = d["x"].double().cpu().reshape(B * T, I)
    w = d["w"].double().cpu()
    hall = sv["h"].double().cpu()
    kx, kh = ("dgx", "dgh") if cell == "gru" else ("dg", "dg")
    gx_all = sv[kx].double().cpu().reshape(B * T, -1)
    gh_all = sv[kh].double().cpu().reshape(B * T, -1)
    dw, db = d["dw"], d["db"]
    for di, rev in DIRS[direction]:
        gx = gx_all[:, di * gh:(di + 1) * gh]
        ghd = gh_all[:, di * gh:(di + 1) * gh]
        hd = hall[:, :, di * H:(di + 1) * H]
        hp = torch.zeros(B, T, H, dtype=torch.float64)
        if rev:
            hp[:, :-1] = hd[:, 1:]       # h^r_{t+1}, zero at t = T-1
        else:
            hp[:, 1:] = hd[:, :-1]       # h^f_{t-1}, zero at t = 0
        rows = slice(di * gh, (di + 1) * gh)
        tag = "direction %d " % di
        _close(tag + "dw[:, :I]", dw[rows, :I], gx.t() @ x, 1e-3)
        _close(tag + "dw[:, I:]", dw[rows, I:],
               ghd.t() @ hp.reshape(B * T, H), 1e-3)
        if cell == "gru":
            _close(tag + "dbias[:3H]", db[di * bb:di * bb + gh], gx.sum(0),
                   1e-3)
            _close(tag + "dbias[3H:]", db[di * bb + gh:(di + 1) * bb],
                   ghd[:, 2 * H:].sum(0), 1e-3)
        else:
            _close(tag + "dbias", db[rows], gx.sum(0), 1e-3)
    _close("err_input", d["ei"].reshape(B * T, I), gx_all @ w[:, :I], 1e-2)


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("i", ALL, ids=IDS)
def test_gradient_gemms(i, cell):
    gemm_checks(cell, case(cell, i), "both")


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("i", ALL, ids=IDS)
def test_reverse_is_forward_on_the_flipped_input(i, cell):
    """direction="reverse" against the one-direction op on the time-flipped
    input and error, flipped back: the same bits from the step kernels, and
    its gradient GEMMs against float64"""
    d = case(cell, i, "reverse")
    H = d["H"]
    xf = d["x"].flip(1).contiguous()
    ef = d["err"].flip(1).contiguous()
    ref = run(cell, xf, d["w"], d["bias"], ef, H, direction="forward")
    keys = ("y",) + step_keys(cell)
    assert torch.equal(d["out"], ref[0].flip(1))
    for k, want in zip(keys[1:], ref[1:]):
        time_axis = 0 if k in ("dc", "dcarry") else 1
        assert torch.equal(d["save"][k], want.flip(time_axis)), k
    gemm_checks(cell, d, "reverse")
    # last-step mode: h^r_0 out, the error enters at t = 0
    y = fwd_op(cell, d["x"], d["w"], d["bias"], H, direction="reverse")
    torch.cuda.synchronize()
    assert torch.equal(y, d["save"]["h"][:, 0])


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("i", (0, MID, 4), ids=[IDS[0], IDS[MID], IDS[4]])
def test_last_step_mode(i, cell):
    """err [B][2H] gives the dG of [B][T][2H] that is zero except
    [:, T-1, :H] and [:, 0, H:]; out is [h^f_{T-1} | h^r_0]"""
    B, I, H, T = CASES[i]
    x, w, bias, err = operands(cell, i)
    e_last = torch.cat((err[:, T - 1, :H], err[:, 0, H:]), 1).contiguous()
    e_full = torch.zeros_like(err)
    e_full[:, T - 1, :H] = err[:, T - 1, :H]
    e_full[:, 0, H:] = err[:, 0, H:]
    a = run(cell, x, w, bias, e_last, H)
    b = run(cell, x, w, bias, e_full, H)
    h = b[1]
    assert a[0].shape == (B, 2 * H)
    assert torch.equal(a[0], torch.cat((h[:, T - 1, :H], h[:, 0, H:]), 1))
    for k, u, v in zip(step_keys(cell), a[1:], b[1:]):
        assert torch.equal(u, v), k
    out = torch.empty(B, 2 * H, dtype=BF, device=DEV)
    assert fwd_op(cell, x, w, bias, H, direction="both", out=out) is out
    torch.cuda.synchronize()
    assert torch.equal(out, a[0])


@pytest.mark.parametrize("cell", CELLS)
def test_bit_reproducible_and_buffers_reused(cell):
    B, I, H, T = CASES[MID]
    x, w, bias, err = operands(cell, MID)
    ops.set_deterministic(True)
    try:
        save = {}
        a = run(cell, x, w, bias, err, H, save=save)
        ptrs = {k: v.data_ptr() for k, v in save.items()}
        b = run(cell, x, w, bias, err, H, save=save)
        assert ptrs == {k: v.data_ptr() for k, v in save.items()}
    finally:
        ops.set_deterministic(False)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize("cell", CELLS)
def test_chain_of_single_launches_gives_the_same_bits(cell):
    """the A/B switch of the benchmark: 2T one-direction launches over the
    same buffers"""
    B, I, H, T = CASES[MID]
    x, w, bias, err = operands(cell, MID)
    a = run(cell, x, w, bias, err, H)
    old = ops.set_birecurrent_paired(False)
    try:
        b = run(cell, x, w, bias, err, H)
    finally:
        ops.set_birecurrent_paired(old)
    n = 1 + len(step_keys(cell))
    for u, v in zip(a[:n], b[:n]):
        assert torch.equal(u, v)


@pytest.mark.parametrize("cell", CELLS)
def test_strided_input(cell):
    """a [B][T][.] view with a padded pitch gives the bits of a contiguous
    copy"""
    B, I, H, T = CASES[MID]
    x, w, bias, err = operands(cell, MID)
    buf = torch.zeros(B, T, I + 24, dtype=BF, device=DEV)
    xs = buf[:, :, :I]
    xs.copy_(x)
    assert not xs.is_contiguous()
    ops.set_deterministic(True)
    try:
        a = run(cell, x, w, bias, err, H)
        b = run(cell, xs, w, bias, err, H)
    finally:
        ops.set_deterministic(False)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize("cell", CELLS)
def test_graph_capture(cell):
    """forward + backward captured once on the current stream (a linear
    chain) and replayed once after the operands changed: eager's bits"""
    B, I, H, T = CASES[MID]
    x, w, bias, err = operands(cell, MID)
    dw = torch.zeros(2 * NG[cell] * H, I + H, device=DEV)
    db = torch.zeros(2 * BB[cell] * H, device=DEV)
    ei = torch.empty(B, T, I, dtype=BF, device=DEV)
    save = {}
    ops.set_deterministic(True)
    try:
        def step():
            y = fwd_op(cell, x, w, bias, H, return_sequences=True, save=save,
                       direction="both")
            bwd_op(cell, err, x, w, save, dw, db, err_input=ei,
                   direction="both")
            return y
        step()           # warm-up: every buffer of ``save`` exists now
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = step()
        g = torch.Generator().manual_seed(901)
        x.copy_(torch.randn(x.shape, generator=g).to(BF))
        err.copy_(torch.randn(err.shape, generator=g).to(BF))
        w.copy_((torch.randn(w.shape, generator=g) / (I + H) ** 0.5).to(BF))
        bias.copy_(torch.randn(bias.shape, generator=g) * 0.5)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in [y] + [save[k] for k in step_keys(cell)] +
               [dw, db, ei]]
        ref = run(cell, x, w, bias, err, H)
        for u, v in zip(got, ref):
            assert torch.equal(u, v)
    finally:
        ops.set_deterministic(False)


def test_host_checks_raise_before_any_launch():
    for cell in CELLS:
        d = case(cell, 1)
        x, w, b, H, err = d["x"], d["w"], d["bias"], d["H"], d["err"]
        both = dict(direction="both")
        gh = NG[cell] * H
        with pytest.raises(TypeError):
            fwd_op(cell, x.float(), w, b, H, **both)
        with pytest.raises(TypeError):
            fwd_op(cell, x, w, b.to(BF), H, **both)
        for bad in (lambda: fwd_op(cell, x, w[:gh], b, H, **both),
                    lambda: fwd_op(cell, x, w, b[:BB[cell] * H], H, **both),
                    lambda: fwd_op(cell, x, w, b, H, direction="backward"),
                    lambda: fwd_op(cell, x, w, b, H),
                    lambda: fwd_op(cell, x, w, b.cpu(), H, **both),
                    lambda: fwd_op(cell, x.transpose(0, 1), w, b, H, **both),
                    lambda: fwd_op(cell, x, w, b, H,
                                   out=torch.empty(d["B"], H, dtype=BF,
                                                   device=DEV), **both)):
            with pytest.raises(ValueError):
                bad()
        save = dict(d["save"])
        dw = torch.zeros_like(d["dw"])
        with pytest.raises(TypeError):
            bwd_op(cell, err.float(), x, w, save, dw, None, **both)
        for bad in (lambda: bwd_op(cell, err[:, :, :H], x, w, save, dw, None,
                                   **both),
                    lambda: bwd_op(cell, err, x, w, save, dw[:gh], None,
                                   **both),
                    lambda: bwd_op(cell, err, x, w, save, dw.to(BF), None,
                                   **both),
                    lambda: bwd_op(cell, err, x, w, save, dw,
                                   d["db"][:BB[cell] * H], **both),
                    lambda: bwd_op(cell, err, x, w, {}, dw, None, **both),
                    lambda: bwd_op(cell, err, x, w, save, dw, None,
                                   direction="up")):
            with pytest.raises(ValueError):
                bad()
        if cell != "rnn":    # gates that are not the forward's buffer
            with pytest.raises(ValueError):
                bwd_op(cell, err, x, w,
                       dict(save, gates=save["gates"].clone()), dw, None,
                       **both)
        torch.cuda.synchronize()
        assert not dw.any()


def test_paired_entry_points_refuse_bad_arguments():
    """a bad argument in EITHER direction returns -1 without a launch"""
    s = None
    # ---- LSTM / RNN
    d = case("lstm", 1)
    B, H, T = d["B"], d["H"], d["T"]
    sv = d["save"]
    s = ops._s(d["x"])
    PW = sv["_xg"].shape[2]
    xg, h, c = (sv[k].data_ptr() for k in ("_xg", "h", "c"))
    ldh = 2 * T * H
    fwd2 = ops._rec_fn("hvk_lstm_step_fwd2")

    def fdir(o, xg_=xg, h_=h, ld_xg=T * PW, ld_h=ldh, c_=c, hp=None):
        return (hp, ldh, None, 0, None if xg_ is None else xg_ + 16 * o * H,
                ld_xg, None, 0, c_, ldh, h_, ld_h, None, 0)

    def f(cell=0, B_=B, H_=H, k0=None, k1=None):
        return fwd2(cell, B_, H_, *(fdir(0, **(k0 or {})) +
                                    fdir(1, **(k1 or {})) + (s,)))
    assert f(cell=2) == -1 and f(B_=0) == -1 and f(H_=0) == -1
    for k in ("k0", "k1"):       # each direction is validated on its own
        assert f(**{k: dict(xg_=None)}) == -1
        assert f(**{k: dict(h_=None)}) == -1
        assert f(**{k: dict(c_=None)}) == -1
        assert f(**{k: dict(ld_xg=4 * H - 1)}) == -1
        assert f(**{k: dict(ld_h=H - 1)}) == -1
        assert f(**{k: dict(hp=h)}) == -1        # a product without Wh
    g, dg, dc = (sv[k].data_ptr() for k in ("_gates", "_dg", "dc"))
    bwd2 = ops._rec_fn("hvk_lstm_step_bwd2")

    def bdir(o, g_=g, ld_g=T * PW, dc_=dc, ld_dg=T * PW, dgn=None, c_=c):
        return (dgn, T * PW, None, 0, None, 0, g_, ld_g, None, 0, c_, ldh,
                None, 0, dc_, 2 * H, dg, ld_dg)

    def b(cell=0, k0=None, k1=None):
        return bwd2(cell, B, H, *(bdir(0, **(k0 or {})) +
                                  bdir(1, **(k1 or {})) + (s,)))
    assert b(cell=-1) == -1
    for k in ("k0", "k1"):
        assert b(**{k: dict(g_=None)}) == -1
        assert b(**{k: dict(ld_g=4 * H - 1)}) == -1
        assert b(**{k: dict(dc_=None)}) == -1
        assert b(**{k: dict(c_=None)}) == -1
        assert b(**{k: dict(ld_dg=1)}) == -1
        assert b(**{k: dict(dgn=dg)}) == -1      # a product without WhT
    # ---- GRU
    d = case("gru", 1)
    sv = d["save"]
    PW = sv["_xg"].shape[2]
    xg, h, hf, hn = (sv[k].data_ptr() for k in ("_xg", "h", "hf", "hn"))
    gfwd2 = ops._rec_fn("hvk_gru_step_fwd2")

    def gfdir(xg_=xg, h_=h, hf_=hf, ld_xg=T * PW, ld_h=ldh, hp=None):
        return (hp, ldh, None, 0, xg_, ld_xg, None, 0, hf_, ldh, hn, ldh, h_,
                ld_h, None, 0, None)

    def gf(B_=B, H_=H, k0=None, k1=None):
        return gfwd2(B_, H_, *(gfdir(**(k0 or {})) + gfdir(**(k1 or {})) +
                               (s,)))
    assert gf(B_=0) == -1 and gf(H_=0) == -1
    for k in ("k0", "k1"):
        assert gf(**{k: dict(xg_=None)}) == -1
        assert gf(**{k: dict(h_=None)}) == -1
        assert gf(**{k: dict(hf_=None)}) == -1
        assert gf(**{k: dict(ld_xg=3 * H - 1)}) == -1
        assert gf(**{k: dict(ld_h=H - 1)}) == -1
        assert gf(**{k: dict(hp=h)}) == -1
    g, dgx, dgh, dc = (sv[k].data_ptr() for k in
                       ("_gates", "_dgx", "_dgh", "dcarry"))
    gbwd2 = ops._rec_fn("hvk_gru_step_bwd2")

    def gbdir(g_=g, ld_g=T * PW, dc_=dc, ld_dgx=T * PW, dgn=None):
        return (dgn, T * PW, None, 0, None, 0, g_, ld_g, hn, ldh, None, 0,
                None, 0, dc_, 2 * H, dgx, ld_dgx, dgh, T * PW)

    def gb(k0=None, k1=None):
        return gbwd2(B, H, *(gbdir(**(k0 or {})) + gbdir(**(k1 or {})) +
                             (s,)))
    for k in ("k0", "k1"):
        assert gb(**{k: dict(g_=None)}) == -1
        assert gb(**{k: dict(ld_g=3 * H - 1)}) == -1
        assert gb(**{k: dict(dc_=None)}) == -1
        assert gb(**{k: dict(ld_dgx=1)}) == -1
        assert gb(**{k: dict(dgn=dgh)}) == -1
    torch.cuda.synchronize()


def test_bidirectional_sample_layers_train_on_the_gpu():
    """the layers of samples/seq_recall_bi_config.py (a bidirectional LSTM of
    16 units per direction, last states -> softmax) on the GPU device, 60 SGD
    steps of seq_recall: the loss starts at chance (ln 8 = 2.08) and falls"""
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
    layers = [{"type": "lstm", "->": {"output_sample_shape": 16,
                                      "return_sequences": False,
                                      "bidirectional": True}, "<-": dict(g)},
              {"type": "softmax", "->": {"output_sample_shape": 8},
               "<-": dict(g)}]
    wf = StandardWorkflow(
        DummyLauncher(), loader_name="seq_recall",
        loader_config={"steps": 8, "features": 8, "n_markers": 8,
                       "noise": 0.4, "class_lengths": (0, 0, B * K),
                       "minibatch_size": B, "seed": 1},
        layers=layers, decision_config={"max_epochs": None,
                                        "fail_iterations": 100})
    wf.initialize(device=Device(backend="hip"))
    f0 = wf.forwards[0]
    assert f0.weights_lp.is_cuda and f0.direction == "both"
    assert tuple(f0.output.shape) == (B, 32)
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
    assert tuple(f0.save_["h"].shape) == (B, 8, 32)
    print("loss every 5th step:", " ".join("%.3f" % v for v in loss[::5]))
    first, last = sum(loss[:5]) / 5, sum(loss[-5:]) / 5
    assert abs(first - 2.08) < 0.2 and last < first, (first, last)
