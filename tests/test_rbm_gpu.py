"""The fused gfx950 RBM kernels (csrc/kernels/rbm.hip) against a float64
model of docs/OPS.md "Restricted Boltzmann machines", computed from the
GPU's own stored bf16 tensors; a CD-1 step captured in a graph; one
end-to-end run of RBMWorkflow on the GPU.

Probability bound.  bf16 x bf16 products are exact in f32, so the
pre-activation errs only by its f32 accumulation: a wave adds at most
ceil(K / 128) MFMA results of 32 products each into its accumulator, the
four waves' partial sums meet in three additions, the bias is one more.
That chain is shorter than the K sequential fmaf of the Kohonen kernels,
whose measured figure 1.5e-7 sum |a b| (K <= 1024) therefore bounds it.  The
logistic function has slope <= 1/4; 1 / (1 + __expf(-a)) measured 0.89e-7
absolute (1.78e-7 is twice that, profiles/recurrent/gpu_tests_figures.txt),
covered by 3e-7.  With the 3x margin and the bf16 rounding of the stored
value

    |P - p64| <= 3 (1/4 1.5e-7 (sum |x w| + |b|) + 3e-7) + half ulp_bf16(p)

and a sample can differ from u < p64 only where |u - p64| is within the
first term (the draw compares the f32 p before the bf16 rounding).
Statistic bound: the same chain figure, 3 x 1.5e-7 |scale| sum_b (|h0 v0| +
|hk vk|), plus 2^-23 |g| for the slice sum's scaling and final rounding.
"""
import numpy
import pytest
import torch

import veles_amd.ops as ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
M32 = 0xFFFFFFFF
NAN = float("nan")

# (rows, n, V, H)
CASES = [(1, 1, 1, 1), (30, 30, 16, 16), (100, 77, 37, 50),
         (128, 128, 784, 136), (257, 257, 130, 1032), (64, 64, 1000, 8)]
IDS = ["x".join(map(str, c)) for c in CASES]
SAT = 5


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


def f64(t):
    return t.detach().double().cpu().numpy()


def half_ulp_bf16(p):
    """Half the spacing of bfloat16 (8 significant bits) at p > 0."""
    return numpy.ldexp(1.0, numpy.floor(numpy.log2(numpy.maximum(
        p, 1e-300))).astype(int) - 8)


def operands(i):
    """bf16 operands of case i on the GPU; rows past n are NaN."""
    rows, n, V, H = CASES[i]
    g = torch.Generator().manual_seed(100 + i)
    v = (torch.rand(rows, V, generator=g) < 0.5).float()
    h = (torch.rand(rows, H, generator=g) < 0.5).float()
    if i == SAT:
        # pre-activations near +-30 in both directions: about V / 2 inputs
        # are on, so +-60 / V per weight; the visible side through its bias.
        # Units 6 and 7 / the first 16 pixels are pushed to +-200, where the
        # f32 sigmoid is exactly 0 / 1
        sign = torch.tensor([1., -1.] * (H // 2)).view(H, 1)
        w = sign * (60.0 / V) * (0.9 + 0.2 * torch.rand(H, V, generator=g))
        hb = torch.zeros(H)
        hb[6], hb[7] = 200.0, -200.0
        vb = 30.0 * torch.tensor([1., -1.] * (V // 2))
        vb[:16] *= 200.0 / 30.0
    else:
        w = (torch.rand(H, V, generator=g) * 2 - 1) * (2.0 / V ** 0.5)
        hb = torch.rand(H, generator=g) - 0.5
        vb = torch.rand(V, generator=g) - 0.5
    v[n:], h[n:] = NAN, NAN
    return (v.to(DEV, BF), h.to(DEV, BF), w.to(DEV, BF), hb.to(DEV),
            vb.to(DEV))


def check_sample(x, w, bias, transposed, n, seed, base, probs, sample):
    """(worst probability error / bound, share of elements in the undecided
    band) of one call against the float64 model."""
    m = f64(w) if transposed else f64(w).T
    xs, b = f64(x)[:n], f64(bias)
    p = 1.0 / (1.0 + numpy.exp(-(xs @ m + b[None, :])))
    band = 3 * (0.25 * 1.5e-7 * (numpy.abs(xs) @ numpy.abs(m) +
                                 numpy.abs(b)[None, :]) + 3e-7)
    bound = band + half_ulp_bf16(p + band)
    err = numpy.abs(f64(probs)[:n] - p)
    worst = float((err / bound).max())
    assert worst <= 1.0, worst
    u = model_uniforms(n, p.shape[1], seed, base)
    s = f64(sample)[:n]
    assert ((s == 0) | (s == 1)).all()
    decided = numpy.abs(u - p) > band
    assert (s[decided] == (u < p)[decided]).all()
    inside = float((~decided).mean())
    assert (~decided).sum() <= max(1e-3 * p.size, 0)
    return worst, inside, p


@pytest.mark.parametrize("transposed", [False, True], ids=["vh", "hv"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_sample(i, transposed):
    rows, n, V, H = CASES[i]
    v, h, w, hb, vb = operands(i)
    x, bias, U = (h, vb, V) if transposed else (v, hb, H)
    seed = 0x9E3779B1 + i
    worst = inside = 0.0
    for base in (0, M32 - 7 * U - 3):      # the second wraps past 2^32
        probs = torch.full((rows, U), 7.0, device=DEV, dtype=BF)
        sample = torch.full((rows, U), 7.0, device=DEV, dtype=BF)
        ops.rbm_sample(x, w, bias, transposed=transposed, n=n, probs=probs,
                       sample=sample, seed=seed, base=base)
        torch.cuda.synchronize()
        a, b, p = check_sample(x, w, bias, transposed, n, seed, base, probs,
                               sample)
        worst, inside = max(worst, a), max(inside, b)
        assert (probs[n:] == 7).all() and (sample[n:] == 7).all()
        if i == SAT:
            # exactly 0 / 1 where the f32 sigmoid saturates
            on = bias > 100
            off = bias < -100
            assert on.any() and off.any()
            assert (probs[:n][:, on] == 1).all()
            assert (sample[:n][:, on] == 1).all()
            assert (probs[:n][:, off] == 0).all()
            assert (sample[:n][:, off] == 0).all()
            mid = p[:, (~(on | off)).cpu().numpy()]
            assert numpy.abs(numpy.log(mid / (1 - mid))).min() > 20
    # the same draws from the device seed; either output alone
    sd = torch.tensor([seed - (1 << 32) if seed >= 1 << 31 else seed],
                      dtype=torch.int32, device=DEV)
    s2 = torch.full((rows, U), 7.0, device=DEV, dtype=BF)
    p2 = torch.full((rows, U), 7.0, device=DEV, dtype=BF)
    ops.rbm_sample(x, w, bias, transposed=transposed, n=n, sample=s2,
                   seed_dev=sd, base=base)
    ops.rbm_sample(x, w, bias, transposed=transposed, n=n, probs=p2)
    assert torch.equal(s2, sample) and torch.equal(p2, probs)
    # a view with a row pitch off the 16-B grid takes the element path and
    # gives the same result
    xp = torch.full((rows, x.shape[1] + 3), NAN, device=DEV, dtype=BF)
    xv = xp[:, 1:1 + x.shape[1]]
    xv.copy_(x)
    s3 = torch.full((rows, U + 1), 7.0, device=DEV, dtype=BF)
    ops.rbm_sample(xv, w, bias, transposed=transposed, n=n,
                   sample=s3[:, :U], seed=seed, base=base)
    assert torch.equal(s3[:, :U], sample) and (s3[:, U] == 7).all()
    print("sample %s %s: max err / bound %.3f, undecided share %.2e" % (
        IDS[i], "h->v" if transposed else "v->h", worst, inside))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_grad(i):
    rows, n, V, H = CASES[i]
    v0, _, w, hb, vb = operands(i)
    g = torch.Generator().manual_seed(200 + i)
    vk = (torch.rand(rows, V, generator=g) < 0.5).float()
    h0 = torch.rand(rows, H, generator=g)
    hk = torch.rand(rows, H, generator=g)
    for t in (vk, h0, hk):
        t[n:] = NAN
    vk, h0, hk = (t.to(DEV, BF) for t in (vk, h0, hk))
    off_hb, off_vb, total = ops.rbm_layout(V, H)
    scale = -1.0 / n
    a0, b0, ak, bk = (f64(t)[:n] for t in (h0, v0, hk, vk))
    ref = numpy.zeros(total)
    mag = numpy.zeros(total)
    ref[:H * V] = (scale * (a0.T @ b0 - ak.T @ bk)).ravel()
    mag[:H * V] = (a0.T @ b0 + ak.T @ bk).ravel()       # all >= 0
    ref[off_hb:off_hb + H] = scale * (a0 - ak).sum(0)
    mag[off_hb:off_hb + H] = (a0 + ak).sum(0)
    ref[off_vb:off_vb + V] = scale * (b0 - bk).sum(0)
    mag[off_vb:off_vb + V] = (b0 + bk).sum(0)
    bound = 3 * 1.5e-7 * abs(scale) * mag + 2.0 ** -23 * numpy.abs(ref) + \
        1e-45
    worst = 0.0
    for splits in (0, 1, 2, 3, 5):
        grad = torch.full((total,), NAN, device=DEV)
        ops.rbm_grad(v0, h0, vk, hk, grad, n=n, splits=splits)
        again = torch.full((total,), NAN, device=DEV)
        ops.rbm_grad(v0, h0, vk, hk, again, n=n, splits=splits)
        torch.cuda.synchronize()
        assert torch.isfinite(grad).all()      # overwritten, NaN rows unread
        assert torch.equal(grad, again)
        err = numpy.abs(f64(grad) - ref)
        r = float((err / bound).max())
        assert r <= 1.0, (splits, r)
        worst = max(worst, r)
    print("grad %s: max err / bound %.3f" % (IDS[i], worst))


def test_unsupported_arguments_return_minus_one():
    from veles_amd.ops import _lib
    v, h, w, hb, vb = operands(1)
    p = torch.zeros(30, 16, device=DEV, dtype=BF)
    fn = _lib.lib().hvk_rbm_sample
    s = ops._s(v)
    args = [0, 30, 16, 16, v.data_ptr(), 16, w.data_ptr(), 16, hb.data_ptr(),
            p.data_ptr(), 16, None, 0, 1, None, 0, s]
    for k, bad in ((1, 0), (2, 0), (0, 2), (5, 15), (7, 15), (10, 15),
                   (9, None), (4, None), (8, None)):
        a = list(args)
        a[k] = bad
        assert fn(*a) == -1, k
    g = torch.zeros(ops.rbm_layout(16, 16)[2], device=DEV)
    fg = _lib.lib().hvk_rbm_grad
    ok = [30, 16, 16, v.data_ptr(), 16, p.data_ptr(), 16, v.data_ptr(), 16,
          p.data_ptr(), 16, g.data_ptr(), 1.0, None, 1, s]
    for k, bad in ((0, 0), (1, 0), (4, 15), (6, 15), (11, None), (14, -1),
                   (14, 2)):          # 2 slices without a workspace
        a = list(ok)
        a[k] = bad
        assert fg(*a) == -1, k
    torch.cuda.synchronize()
    assert not p.any() and not g.any()
    with pytest.raises(TypeError):
        ops.rbm_sample(v.float(), w, hb, probs=p)
    with pytest.raises(TypeError):
        ops.rbm_sample(v, w, hb.to(BF), probs=p)
    with pytest.raises(ValueError):
        ops.rbm_sample(v, w, hb.cpu(), probs=p)


def make_workflow(epochs=1, **trainer):
    from veles_amd.backends import Device
    from veles_amd.dummy import DummyLauncher
    from veles_amd.models import RBMWorkflow
    from veles_amd.prng import random_generator
    import veles_amd.loader  # noqa: F401
    random_generator.get().seed(1)
    trainer.setdefault("hidden", 16)
    wf = RBMWorkflow(
        DummyLauncher(), loader_name="bars_stripes",
        loader_config={"minibatch_size": 30}, trainer_config=trainer,
        decision_config={"max_epochs": epochs, "exact_likelihood": True,
                         "likelihood_interval": 100})
    wf.initialize(device=Device(backend="hip"))
    return wf


def test_captured_step():
    """One CD-1 step captured with torch.cuda.graph and replayed three times
    equals three eager steps from the same state, bit for bit; the seed
    advances on the device."""
    wf = make_workflow()
    tr = wf.trainer
    data = torch.from_numpy(wf.loader.original_data.mem).to(DEV, BF)

    def state():
        torch.cuda.synchronize()
        return [t.clone() for t in (tr.params.devmem, tr.moment.devmem,
                                    tr.params_lp_, tr.seed_dev)]

    def restore(st):
        for t, s in zip((tr.params.devmem, tr.moment.devmem, tr.params_lp_,
                         tr.seed_dev), st):
            t.copy_(s)
    tr.step(data, 30)            # every buffer and cached table exists now
    start = state()
    for _ in range(3):
        tr.step(data, 30)
    eager = state()
    assert not torch.equal(eager[0], start[0])
    restore(start)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        tr.step(data, 30)
    torch.cuda.current_stream().wait_stream(s)
    restore(start)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tr.step(data, 30)
    restore(start)
    for _ in range(3):
        graph.replay()
    got = state()
    for a, b in zip(got, eager):
        assert torch.equal(a, b)
    seed = int(start[3][0]) & M32
    for _ in range(3):
        seed = ops.seed_advance_ref(seed)
    assert int(got[3][0]) & M32 == seed


def test_workflow_trains_on_the_gpu():
    """The sample's configuration on the GPU: the same criterion as
    tests/test_rbm_sample.py (first epoch <= -10.5, last >= -6.0)."""
    wf = make_workflow(epochs=2000)
    assert wf.trainer.params.devmem.is_cuda
    wf.run()
    hist = wf.decision.get_metric_values()["log_likelihood_history"]
    print("workflow on the GPU: log-likelihood %.4f -> %.4f" % (
        hist[0][1], hist[-1][1]))
    assert hist[0][0] == 0 and hist[-1][0] == 1999
    assert hist[0][1] <= -10.5, hist
    assert hist[-1][1] >= -6.0, hist
