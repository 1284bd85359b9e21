"""Restricted Boltzmann machines on the CPU device: the ops against a float64
numpy model that follows docs/OPS.md "Restricted Boltzmann machines"
literally (its own hash32), the trainer teacher-forced against that model
step by step, the chain variants, snapshot / resume and rbm_to_all2all.

Bounds.  The float32 path computes a pre-activation a = sum_k x_k w_k + b of
K + 1 terms in some order: |a32 - a64| <= (K + 1) 2^-24 (sum |x_k w_k| + |b|)
to first order.  The logistic function has slope <= 1/4, and exp, the
addition and the division each contribute at most 2^-24 relative to a result
p <= 1, one more for the float32 inputs of the model being exact but the
operations not, so

    |p32 - p64| <= 1/4 (K + 1) 2^-24 (sum |x w| + |b|) + 4 2^-24  =: band.

A sample u < p can differ from the model's only where |u - p64| <= band.
The statistic sums 2n products in float32: |g32 - g64| <= |scale| (2n + 1)
2^-24 sum_b (|h0 v0| + |hk vk|) plus 2^-24 |g| for the scaling.
"""
import pickle

import numpy
import pytest
import torch

from veles_amd import ops

EPS = 2.0 ** -24
M32 = 0xFFFFFFFF


# ------------------------------------------------------------ float64 model
def model_hash32(i, seed):
    x = (i.astype(numpy.uint64) ^ numpy.uint64((seed * 0x9E3779B9) & M32))
    x ^= x >> numpy.uint64(16)
    x = (x * numpy.uint64(0x7feb352d)) & numpy.uint64(M32)
    x ^= x >> numpy.uint64(15)
    x = (x * numpy.uint64(0x846ca68b)) & numpy.uint64(M32)
    x ^= x >> numpy.uint64(16)
    return x


def model_uniforms(rows, N, seed, base):
    i = (numpy.arange(rows * N, dtype=numpy.uint64) +
         numpy.uint64(base & M32)) & numpy.uint64(M32)
    u = (model_hash32(i, seed & M32) >> numpy.uint64(8)).astype(
        numpy.float64) / 16777216.0
    return u.reshape(rows, N)


def model_seed_advance(seed):
    i = numpy.array([(seed + 1) & M32], numpy.uint64)
    return int(model_hash32(i, 0x2545F491)[0])


def model_probs(x, w, bias, transposed):
    """(p, band) of one sampling call in float64."""
    m = w if transposed else w.T
    a = x @ m + bias[None, :]
    mag = numpy.abs(x) @ numpy.abs(m) + numpy.abs(bias)[None, :]
    p = 1.0 / (1.0 + numpy.exp(-a))
    band = 0.25 * (x.shape[1] + 1) * EPS * mag + 4 * EPS
    return p, band


def model_grad(v0, h0, vk, hk, scale):
    gw = scale * (h0.T @ v0 - hk.T @ vk)
    ghb = scale * (h0 - hk).sum(0)
    gvb = scale * (v0 - vk).sum(0)
    n = len(v0)
    mag = numpy.abs(h0).T @ numpy.abs(v0) + numpy.abs(hk).T @ numpy.abs(vk)
    bw = abs(scale) * (2 * n + 1) * EPS * mag + EPS * numpy.abs(gw)
    bh = abs(scale) * (2 * n + 1) * EPS * (numpy.abs(h0) +
                                            numpy.abs(hk)).sum(0) + \
        EPS * numpy.abs(ghb)
    bv = abs(scale) * (2 * n + 1) * EPS * (numpy.abs(v0) +
                                            numpy.abs(vk)).sum(0) + \
        EPS * numpy.abs(gvb)
    return (gw, ghb, gvb), (bw, bh, bv)


def f64(t):
    return t.detach().double().cpu().numpy()


def check_call(x, w, bias, transposed, n, seed, base, probs, sample):
    """One sampling call against the model; returns (elements inside the
    undecided band, elements, worst probability error / band)."""
    p, band = model_probs(f64(x)[:n], f64(w), f64(bias), transposed)
    worst = 0.0
    if probs is not None:
        err = numpy.abs(f64(probs)[:n] - p)
        assert (err <= band).all(), (err / band).max()
        worst = float((err / band).max())
    inside = 0
    if sample is not None:
        u = model_uniforms(n, p.shape[1], seed, base)
        s = f64(sample)[:n]
        assert ((s == 0) | (s == 1)).all()
        decided = numpy.abs(u - p) > band
        assert (s[decided] == (u < p)[decided]).all()
        inside = int((~decided).sum())
    return inside, p.size, worst


# ---------------------------------------------------------------------- ops
def _operands(rows, V, H, seed, wscale=1.0):
    g = torch.Generator().manual_seed(seed)
    v = (torch.rand(rows, V, generator=g) < 0.5).float()
    h = (torch.rand(rows, H, generator=g) < 0.5).float()
    w = (torch.rand(H, V, generator=g) * 2 - 1) * wscale
    hb = torch.rand(H, generator=g) - 0.5
    vb = torch.rand(V, generator=g) - 0.5
    return v, h, w, hb, vb


SHAPES = [(1, 1, 1), (30, 16, 16), (100, 37, 50), (33, 130, 7)]


@pytest.mark.parametrize("rows,V,H", SHAPES)
@pytest.mark.parametrize("transposed", [False, True])
def test_sample_against_the_model(rows, V, H, transposed):
    v, h, w, hb, vb = _operands(rows, V, H, 3)
    x, bias, U = (h, vb, V) if transposed else (v, hb, H)
    probs, sample = torch.zeros(rows, U), torch.zeros(rows, U)
    seed, base = 0x9ABCDEF1, 12345
    got = ops.rbm_sample(x, w, bias, transposed=transposed, probs=probs,
                         sample=sample, seed=seed, base=base)
    assert got[0] is probs and got[1] is sample
    inside, total, _ = check_call(x, w, bias, transposed, rows, seed, base,
                                  probs, sample)
    assert inside <= 1e-3 * total + 1
    # the uniforms are the documented ones, also across the 2^32 wrap
    u = ops.rbm_uniforms(rows, U, seed, base=M32 - 5).double().numpy()
    assert (u == model_uniforms(rows, U, seed, M32 - 5)).all()
    # the device seed gives the same draws as the host seed
    sd = torch.tensor([seed - (1 << 32)], dtype=torch.int32)
    s2 = torch.zeros(rows, U)
    ops.rbm_sample(x, w, bias, transposed=transposed, sample=s2, seed_dev=sd,
                   base=base)
    assert torch.equal(s2, sample)


def test_saturated_probabilities_never_and_always_fire():
    v, h, w, hb, vb = _operands(40, 12, 9, 5)
    hb[:4], hb[4:] = -200.0, 200.0
    probs, sample = torch.zeros(40, 9), torch.zeros(40, 9)
    ops.rbm_sample(v, w, hb, probs=probs, sample=sample, seed=7)
    assert (probs[:, :4] == 0).all() and (sample[:, :4] == 0).all()
    assert (probs[:, 4:] == 1).all() and (sample[:, 4:] == 1).all()


@pytest.mark.parametrize("rows,V,H", SHAPES)
def test_grad_against_the_model(rows, V, H):
    v0, _, w, hb, vb = _operands(rows, V, H, 11)
    vk = _operands(rows, V, H, 12)[0]
    h0 = torch.sigmoid(v0 @ w.t() + hb)
    hk = torch.sigmoid(vk @ w.t() + hb)
    total = ops.rbm_layout(V, H)[2]
    grad = torch.full((total,), float("nan"))
    assert ops.rbm_grad(v0, h0, vk, hk, grad) is grad
    off_hb, off_vb, _ = ops.rbm_layout(V, H)
    assert off_hb % 16 == 0 and off_vb % 16 == 0 and total % 16 == 0
    (gw, ghb, gvb), (bw, bh, bv) = model_grad(f64(v0), f64(h0), f64(vk),
                                              f64(hk), -1.0 / rows)
    g = f64(grad)
    assert (numpy.abs(g[:H * V].reshape(H, V) - gw) <= bw).all()
    assert (numpy.abs(g[off_hb:off_hb + H] - ghb) <= bh).all()
    assert (numpy.abs(g[off_vb:off_vb + V] - gvb) <= bv).all()
    # overwritten everywhere: the padding between the segments is zero
    pad = numpy.ones(total, bool)
    pad[:H * V] = pad[off_hb:off_hb + H] = pad[off_vb:off_vb + V] = False
    assert (g[pad] == 0).all()
    g2 = torch.zeros(total)
    ops.rbm_grad(v0, h0, vk, hk, g2, scale=0.5)
    assert torch.allclose(g2, grad * (0.5 * -rows), rtol=1e-5, atol=1e-6)


def test_short_minibatch_reads_and_writes_only_the_valid_rows():
    rows, n, V, H = 48, 29, 21, 13
    v, h, w, hb, vb = _operands(rows, V, H, 17)
    nan = float("nan")
    for transposed in (False, True):
        x, bias, U = (h, vb, V) if transposed else (v, hb, H)
        stale = x.clone()
        stale[n:] = nan
        p1, s1 = torch.full((rows, U), 7.0), torch.full((rows, U), 7.0)
        p2, s2 = torch.zeros(n, U), torch.zeros(n, U)
        ops.rbm_sample(stale, w, bias, transposed=transposed, n=n, probs=p1,
                       sample=s1, seed=3, base=rows * U)
        ops.rbm_sample(x[:n].contiguous(), w, bias, transposed=transposed,
                       probs=p2, sample=s2, seed=3, base=rows * U)
        assert torch.equal(p1[:n], p2) and torch.equal(s1[:n], s2)
        assert (p1[n:] == 7).all() and (s1[n:] == 7).all()
    h0 = torch.sigmoid(v @ w.t() + hb)
    hk = torch.rand(rows, H)
    vk = _operands(rows, V, H, 18)[0]
    total = ops.rbm_layout(V, H)[2]
    g1, g2 = torch.zeros(total), torch.zeros(total)
    bad = [t.clone() for t in (v, h0, vk, hk)]
    for t in bad:
        t[n:] = nan
    ops.rbm_grad(*bad, g1, n=n)
    ops.rbm_grad(*[t[:n].contiguous() for t in (v, h0, vk, hk)], g2)
    assert torch.isfinite(g1).all() and torch.equal(g1, g2)


def test_host_checks():
    rows, V, H = 16, 12, 8
    v, h, w, hb, vb = _operands(rows, V, H, 19)
    p, s = torch.zeros(rows, H), torch.zeros(rows, H)
    ok = dict(probs=p, sample=s)
    with pytest.raises(ValueError):
        ops.rbm_sample(v, w, hb)                       # no output wanted
    with pytest.raises(ValueError):
        ops.rbm_sample(v[:, :11].contiguous(), w, hb, **ok)
    with pytest.raises(ValueError):
        ops.rbm_sample(h, w, hb, **ok)                 # wrong direction
    with pytest.raises(ValueError):
        ops.rbm_sample(v, w, vb, **ok)                 # the other bias
    with pytest.raises(ValueError):
        ops.rbm_sample(v, w.t(), hb, **ok)             # rows not contiguous
    with pytest.raises(ValueError):
        ops.rbm_sample(v, w, hb, probs=torch.zeros(rows, H + 1))
    with pytest.raises(ValueError):
        ops.rbm_sample(v, w, hb, sample=torch.zeros(rows - 1, H))
    with pytest.raises(ValueError):
        ops.rbm_sample(v, w, hb, n=0, **ok)
    with pytest.raises(ValueError):
        ops.rbm_sample(v, w, hb, n=rows + 1, **ok)
    with pytest.raises(ValueError):
        ops.rbm_sample(v, w, hb, base=-1, **ok)
    with pytest.raises(ValueError):
        ops.rbm_sample(v, w, hb, seed_dev=torch.zeros(1), **ok)
    with pytest.raises(ValueError):
        ops.rbm_sample(v.view(rows, 3, 4), w, hb, **ok)
    with pytest.raises(TypeError):
        ops.rbm_sample(v.int(), w, hb, **ok)
    with pytest.raises(TypeError):
        ops.rbm_sample(v, w, hb, probs=p.long())
    assert (p == 0).all() and (s == 0).all()           # before any work
    total = ops.rbm_layout(V, H)[2]
    g = torch.full((total,), 5.0)
    h0 = torch.rand(rows, H)
    with pytest.raises(ValueError):
        ops.rbm_grad(v, h0, v, h0, g[:-1])
    with pytest.raises(ValueError):
        ops.rbm_grad(v, h0, v[:, :11].contiguous(), h0, g)
    with pytest.raises(ValueError):
        ops.rbm_grad(v, h0, v, h0[:15], g)
    with pytest.raises(ValueError):
        ops.rbm_grad(v, h0, v, h0, g, n=17)
    with pytest.raises(ValueError):
        ops.rbm_grad(v, h0, v, h0, g, splits=-1)
    with pytest.raises(TypeError):
        ops.rbm_grad(v, h0, v, h0, g.double())
    with pytest.raises(TypeError):
        ops.rbm_grad(v, h0, v, h0, None)
    assert (g == 5).all()


# -------------------------------------------------------------------- units
def make_workflow(epochs=1, minibatch=30, backend="cpu", copies=1, seed=77,
                  decision=None, **trainer):
    from veles_amd.backends import Device
    from veles_amd.dummy import DummyLauncher
    from veles_amd.models import RBMWorkflow
    from veles_amd.prng import random_generator
    import veles_amd.loader  # noqa: F401
    random_generator.get().seed(seed)
    trainer.setdefault("hidden", 16)
    dc = {"max_epochs": epochs}
    dc.update(decision or {})
    wf = RBMWorkflow(
        DummyLauncher(), loader_name="bars_stripes",
        loader_config={"minibatch_size": minibatch, "copies": copies},
        trainer_config=trainer, decision_config=dc)
    wf.initialize(device=Device(backend=backend))
    return wf


class Recorder(object):
    """Records every ops.rbm_sample call of a step: the arguments and copies
    of what it wrote."""

    def __init__(self, monkeypatch):
        self.calls = []
        self.real = ops.rbm_sample
        monkeypatch.setattr(ops, "rbm_sample", self)

    def __call__(self, x, w, bias, **kw):
        sd = kw.get("seed_dev")
        seed = None if sd is None else int(sd[0]) & M32
        r = self.real(x, w, bias, **kw)
        self.calls.append(dict(
            x=x.clone(), transposed=kw.get("transposed", False), n=kw["n"],
            base=kw.get("base", 0), seed=seed,
            probs=None if kw.get("probs") is None else kw["probs"].clone(),
            sample=None if kw.get("sample") is None
            else kw["sample"].clone()))
        return r


def teacher_forced_steps(tr, steps, rec, data):
    """Run ``steps`` CD steps of the trainer ``tr`` on ``data``; before each
    the float64 model starts from the unit's parameters, checks every
    sampling call (its input must be what the spec feeds it, its output the
    model's off the undecided band), computes the update from the unit's own
    samples and compares the parameters after the step."""
    rows, n = data.shape[0], data.shape[0]
    V, H, k = tr.visible, tr.hidden, tr.cd_k
    off_hb, off_vb, total = ops.rbm_layout(V, H)
    worst_in = 0.0
    for step in range(steps):
        p0, m0 = f64(tr.params.devmem), f64(tr.moment.devmem)
        w, hb, vb = tr.weights.clone(), tr.hbias.clone(), tr.vbias.clone()
        seed = int(tr.seed_dev[0]) & M32
        chained = tr.persistent and tr.chain_valid
        chain0 = tr.chain.devmem.clone()
        t0 = tr.time
        del rec.calls[:]
        tr.step(data, n)
        calls = rec.calls
        draws = 1 + k * (1 if tr.sample_visible else 0) + (k - 1) + \
            (1 if tr.persistent else 0)
        assert len(calls) == 1 + 2 * k
        assert sum(c["sample"] is not None for c in calls) == draws
        base, pband = 0, 0.0
        prev, plist = None, []
        for i, c in enumerate(calls):
            hid = i % 2 == 0          # v -> h calls alternate with h -> v
            assert c["transposed"] == (not hid) and c["n"] == n
            assert c["seed"] == seed
            if i == 0:
                want = data
            elif i == 1 and chained:
                want = chain0
            else:
                want = prev
            assert torch.equal(c["x"], want), i
            if c["sample"] is not None:
                assert c["base"] == base, (i, c["base"], base)
            inside, cnt, _ = check_call(
                c["x"], w, hb if hid else vb, not hid, n, seed, c["base"],
                c["probs"], c["sample"])
            assert inside <= 1e-3 * cnt
            worst_in = max(worst_in, inside / cnt)
            p, band = model_probs(f64(c["x"]), f64(w),
                                  f64(hb if hid else vb), not hid)
            plist.append(p)
            pband = max(pband, float(band.max()))
            if c["sample"] is not None:
                base += rows * (H if hid else V)
            # what the next call reads: the draw, or the probabilities
            if hid:
                prev = c["sample"]
            else:
                prev = c["sample"] if tr.sample_visible else c["probs"]
        if tr.persistent:
            assert torch.equal(tr.chain.devmem, calls[-1]["sample"])
        vk = f64(calls[-1]["x"])
        (gw, ghb, gvb), _ = model_grad(f64(data), plist[0], vk, plist[-1],
                                       -1.0 / n)
        g = numpy.zeros(total)
        g[:H * V] = gw.ravel()
        g[off_hb:off_hb + H] = ghb
        g[off_vb:off_vb + V] = gvb
        lr = numpy.zeros(total)
        mo = numpy.zeros(total)
        for b, e, l, d, l1, m in tr.segs_:
            assert d == 0
            lr[b:e], mo[b:e] = l, m
        m1 = mo * m0 - lr * g
        p1 = p0 + m1
        # each probability is within pband of the model's, the states are
        # shared: the statistic moves by <= 2 pband, plus its float32 sum;
        # then the float32 roundings of the moment and the parameter
        tol = lr * (2 * pband + (2 * n + 1) * EPS * 2) + \
            2 * EPS * (numpy.abs(m1) + numpy.abs(p1))
        assert (numpy.abs(f64(tr.moment.devmem) - m1) <= tol).all()
        assert (numpy.abs(f64(tr.params.devmem) - p1) <= tol).all()
        assert int(tr.seed_dev[0]) & M32 == model_seed_advance(seed)
        assert tr.time == t0 + 1
    return worst_in


def _data(wf):
    return torch.from_numpy(wf.loader.original_data.mem.copy())


def test_trainer_teacher_forced(monkeypatch):
    wf = make_workflow()
    tr = wf.trainer
    assert tr.cd_k == 1 and tr.learning_rate == 0.1 and \
        tr.gradient_moment == 0.5 and tr.weights_decay == 0 and \
        tr.sample_visible and not tr.persistent
    w = f64(tr.weights)
    assert tuple(w.shape) == (16, 16) and numpy.abs(w).max() <= 0.05 and \
        numpy.abs(w).max() > 0.04
    assert (tr.hbias == 0).all() and (tr.vbias == 0).all()
    rec = Recorder(monkeypatch)
    teacher_forced_steps(tr, 100, rec, _data(wf))
    assert tr.time == 100


@pytest.mark.parametrize("variant", [
    {"cd_k": 3}, {"persistent": True}, {"sample_visible": False},
    {"cd_k": 2, "persistent": True, "sample_visible": False}])
def test_chain_variants(monkeypatch, variant):
    wf = make_workflow(**variant)
    rec = Recorder(monkeypatch)
    teacher_forced_steps(wf.trainer, 20, rec, _data(wf))


def test_short_minibatch_does_not_shift_the_draws(monkeypatch):
    """rows = 12 over 30 samples: the last minibatch has 6 valid rows; the
    bases still advance by rows * N."""
    wf = make_workflow(minibatch=12, cd_k=2)
    rec = Recorder(monkeypatch)
    wf.run()
    calls = [c for c in rec.calls if c["seed"] is not None]   # the trainer's
    assert len(rec.calls) == len(calls) + 3                   # + the forward
    assert [c["n"] for c in calls[::5]] == [12, 12, 6]
    for i in range(0, 15, 5):
        assert [c["base"] for c in calls[i:i + 4]] == \
            [0, 12 * 16, 2 * 12 * 16, 3 * 12 * 16]
    assert wf.trainer.time == 3


def state_of(wf):
    tr = wf.trainer
    return (tr.params.devmem.clone(), tr.moment.devmem.clone(),
            int(tr.seed_dev[0]), tr.chain.devmem.clone(), tr.chain_valid,
            tr.time)


def test_exact_resume():
    from veles_amd.backends import Device
    from veles_amd.dummy import DummyLauncher
    kw = dict(minibatch=12, persistent=True, cd_k=2)
    wf = make_workflow(epochs=5, **kw)
    wf.run()
    ref = state_of(wf)
    hist = list(wf.decision.history)
    wf = make_workflow(epochs=2, **kw)
    wf.run()
    blob = pickle.dumps(wf, protocol=pickle.HIGHEST_PROTOCOL)
    del wf
    wf2 = pickle.loads(blob)
    wf2.workflow = DummyLauncher()
    wf2.decision.max_epochs = 5
    wf2.decision.complete <<= False
    wf2.initialize(device=Device(backend="cpu"))
    assert wf2.trainer.time == 6 and wf2.trainer.chain_valid
    wf2.run()
    got = state_of(wf2)
    assert got[5] == ref[5] == 15 and got[2] == ref[2] and got[4] and ref[4]
    for a, b in zip(got[:4:3] + got[1:2], ref[:4:3] + ref[1:2]):
        assert torch.equal(a, b)
    assert wf2.decision.history == hist


def test_decision_metrics_and_exact_likelihood():
    from veles_amd.models import rbm_log_likelihood
    wf = make_workflow(epochs=3, decision={"exact_likelihood": True})
    wf.run()
    res = wf.decision.get_metric_values()
    assert res["epochs"] == 3 and len(res["log_likelihood_history"]) == 3
    assert 0 < res["reconstruction_rmse"] < 1
    tr = wf.trainer
    # brute force over the 2^16 states, written independently
    w, hb, vb = f64(tr.weights), f64(tr.hbias), f64(tr.vbias)
    states = ((numpy.arange(1 << 16)[:, None] >> numpy.arange(16)) & 1) \
        .astype(numpy.float64)

    def logp_unnorm(v):
        return v @ vb + numpy.log1p(numpy.exp(v @ w.T + hb)).sum(1)
    log_z = numpy.log(numpy.exp(logp_unnorm(states)).sum())
    data = wf.loader.original_data.mem.astype(numpy.float64)
    ll = (logp_unnorm(data) - log_z).mean()
    assert abs(res["log_likelihood"] - ll) < 1e-9
    assert abs(rbm_log_likelihood(numpy.zeros((16, 16)), numpy.zeros(16),
                                  numpy.zeros(16), data) +
               16 * numpy.log(2)) < 1e-12


def test_rbm_to_all2all():
    from veles_amd.dummy import DummyWorkflow
    from veles_amd.memory import Array
    from veles_amd.models import All2AllSigmoid, rbm_to_all2all
    wf = make_workflow(epochs=20)
    wf.run()
    tr = wf.trainer
    assert wf.forward.output.devmem.shape == (30, 16)
    x = _data(wf)
    unit = All2AllSigmoid(DummyWorkflow(), output_sample_shape=16)
    unit.input = Array(x.numpy())
    rbm_to_all2all(tr, unit)
    unit.initialize()
    unit.input.initialize(unit.device)
    unit.run()
    ref = torch.zeros(30, 16)
    ops.rbm_sample(x, tr.weights, tr.hbias, probs=ref)
    assert torch.equal(unit.weights_master.view(16, 16), tr.weights)
    assert (unit.output.devmem - ref).abs().max() <= 4 * 2.0 ** -24
    # the forward unit gives the same output
    from veles_amd.models import RBMForward
    fw = RBMForward(DummyWorkflow())
    fw.trainer, fw.input, fw.minibatch_size = tr, Array(x.numpy()), 30
    fw.initialize()
    fw.input.initialize(fw.device)
    fw.run()
    assert torch.equal(fw.output.devmem, ref)
    # after initialisation the copy goes into the registered parameters
    tr.params.devmem[:256] += 0.25
    rbm_to_all2all(tr, unit)
    assert torch.equal(unit.weights_master.view(16, 16), tr.weights)
    with pytest.raises(ValueError):
        rbm_to_all2all(tr, All2AllSigmoid(DummyWorkflow(),
                                          output_sample_shape=15))


def test_multi_rank_is_refused(monkeypatch):
    import veles_amd.parallel as par
    wf = make_workflow()

    class TwoRanks(object):
        world_size, rank = 2, 0
    monkeypatch.setattr(par, "find_dp", lambda wf: TwoRanks())
    with pytest.raises(NotImplementedError, match="one rank"):
        wf.initialize()
