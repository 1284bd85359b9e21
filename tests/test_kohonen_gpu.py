"""The fused gfx950 Kohonen kernels (csrc/kernels/kohonen.hip) against a
float64 model of docs/OPS.md "Kohonen maps", and one end-to-end run of
KohonenWorkflow on the GPU against the CPU device.

Winner bound: the f32 MFMA chain errs by <= 1.5e-7 * sum|a b| at K <= 1024;
that enters the dot product (times 2), |W|^2 and both candidates of a
comparison, about 6e-7 of (|x|^2 + max|W|^2), taken with a 3x margin: 2e-6.
Update bound: the same chain error plus __expf at about 2 ulp, with a 10x
margin: 4e-6 * gmult * sum_b G (|x| + |W|) + 2^-23 |W|."""
import functools
import os

import numpy
import pytest
import torch

import veles_amd.ops as ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, sx, sy, D, scale, offset): the smallest shapes that reach every tile
# edge of the 128 x 128 x 32 kernels
CASES = [
    (1, 1, 1, 1, 1.0, 0.0),        # degenerate sizes
    (64, 8, 8, 2, 1.0, 0.0),       # the demo shape
    (100, 5, 7, 3, 1.0, 0.0),      # partial tiles, rows off the 16-B grid
    (257, 16, 16, 37, 1.0, 0.0),   # several sample / neuron tiles, odd D
    (130, 12, 11, 784, 1.0, 0.0),  # many K tiles, NN = 132 crosses 128
    (64, 4, 4, 1000, 1.0, 10.0),   # cancellation in the expansion
    (300, 33, 3, 129, 100.0, 0.0),  # large magnitudes
]
IDS = ["%dx%dx%dx%d" % c[:4] for c in CASES]
DTYPES = [torch.float32, torch.bfloat16]


@functools.lru_cache(maxsize=None)
def case(i, dtype):
    """Device operands and the float64 reference of case i, built once."""
    B, sx, sy, D, scale, offset = CASES[i]
    g = torch.Generator().manual_seed(100 + i)
    x = (torch.randn(B, D, generator=g) * scale + offset).to(dtype)
    w = (torch.rand(sx * sy, D, generator=g) * 2 - 1) * scale + offset
    coords = ops.kohonen_coords(sx, sy)
    x64, w64 = x.double().numpy(), w.double().numpy()
    # float64 distances through the exact expansion (x64, w64 are exact)
    d = (x64 ** 2).sum(1)[:, None] + (w64 ** 2).sum(1)[None, :] - \
        2.0 * (x64 @ w64.T)
    d = numpy.maximum(d, 0.0)
    bound = 2e-6 * ((x64 ** 2).sum(1) + (w64 ** 2).sum(1).max())
    return dict(x=x.to(DEV), w=w.to(DEV), coords=coords.to(DEV), x64=x64,
                w64=w64, c64=coords.double().numpy(), d=d, bound=bound,
                NN=sx * sy, B=B, D=D)


def _argmin(c, splits=0, w=None, **kw):
    a = ops.kohonen_argmin(c["x"], c["w"] if w is None else w,
                           splits=splits, **kw)
    torch.cuda.synchronize()
    return a.cpu().long().numpy()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_winners(i, dtype):
    c = case(i, dtype)
    B, NN, d = c["B"], c["NN"], c["d"]
    qerr = torch.full((B,), -1.0, device=DEV)
    hist = torch.full((NN,), 2, dtype=torch.int32, device=DEV)
    a = _argmin(c, qerr=qerr, winners=hist)
    assert a.min() >= 0 and a.max() < NN
    gap = d[numpy.arange(B), a] - d.min(1)
    print("winners %s %s: max gap / bound %.3g, wrong %d of %d" % (
        IDS[i], dtype, (gap / c["bound"]).max(),
        int((a != d.argmin(1)).sum()), B))
    assert (gap <= c["bound"]).all()
    q = qerr.cpu().double().numpy()
    print("qerr %s %s: max err / bound %.3g" % (
        IDS[i], dtype, (numpy.abs(q - d.min(1)) / c["bound"]).max()))
    assert (numpy.abs(q - d.min(1)) <= c["bound"]).all()
    assert (hist.cpu().numpy() == 2 + numpy.bincount(a, minlength=NN)).all()
    for splits in (1, 2, 3):
        assert (_argmin(c, splits) == a).all(), splits


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_ties_go_to_the_lowest_index(dtype):
    c = case(3, dtype)            # 16 x 16 neurons: two neuron tiles
    x = c["x"].clone()
    for n in (3, 120):            # n + 17 in the same / in the next tile
        w = c["w"].clone()
        w[n + 17] = w[n]
        # samples that sit on the doubled row itself
        x[:5] = w[n].to(x.dtype)
        cc = dict(c, x=x)
        for splits in (0, 1, 2):
            a = _argmin(cc, splits, w=w)
            assert not (a == n + 17).any(), (n, splits)
            if dtype == torch.float32:
                assert (a[:5] == n).all(), (n, splits)
    for splits in (0, 1, 2):
        a = _argmin(c, splits, w=torch.zeros_like(c["w"]))
        assert (a == 0).all()


def _model_update(c, a, sigma, gradient):
    """Float64 model (element-wise bound alongside)."""
    x64, w64, c64, B = c["x64"], c["w64"], c["c64"], c["B"]
    G = numpy.exp(-((c64[None] - c64[a][:, None]) ** 2).sum(2) /
                  (2.0 * sigma * sigma))               # [B][NN]
    r = G.sum(0)[:, None]
    gm = gradient / B
    ref = w64 + gm * (G.T @ x64 - r * w64)
    bound = 4e-6 * gm * (G.T @ numpy.abs(x64) + r * numpy.abs(w64)) + \
        2.0 ** -23 * numpy.abs(w64)
    return ref, bound


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_update(i, dtype):
    c = case(i, dtype)
    a_dev = ops.kohonen_argmin(c["x"], c["w"])
    torch.cuda.synchronize()
    a = a_dev.cpu().long().numpy()
    worst = 0.0
    for sigma in (0.05, 0.5, 2.84):
        ref, bound = _model_update(c, a, sigma, 0.1)
        for splits in (0, 1, 2, 5):
            w = c["w"].clone()
            ops.kohonen_update(c["x"], w, c["coords"], a_dev, sigma, 0.1,
                               splits=splits)
            again = c["w"].clone()
            ops.kohonen_update(c["x"], again, c["coords"], a_dev, sigma, 0.1,
                               splits=splits)
            torch.cuda.synchronize()
            assert torch.equal(w, again), (sigma, splits)
            err = numpy.abs(w.cpu().double().numpy() - ref)
            ratio = float((err / bound).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (sigma, splits, ratio)
    print("update %s %s: max err / bound %.3g" % (IDS[i], dtype, worst))


def test_out_of_range_winners_are_clamped():
    c = case(2, torch.float32)
    NN = c["NN"]
    a = ops.kohonen_argmin(c["x"], c["w"]).clone()
    bad = a.clone()
    a[0], bad[0] = 0, -1
    a[1], bad[1] = NN - 1, NN
    a[2], bad[2] = NN - 1, 2 ** 31 - 1
    a[3], bad[3] = 0, -2 ** 31
    for splits in (1, 2):
        w1, w2 = c["w"].clone(), c["w"].clone()
        ops.kohonen_update(c["x"], w1, c["coords"], bad, 0.5, 0.1,
                           splits=splits)
        ops.kohonen_update(c["x"], w2, c["coords"], a, 0.5, 0.1,
                           splits=splits)
        torch.cuda.synchronize()
        assert torch.equal(w1, w2)


def test_valid_rows_only():
    c = case(2, torch.float32)
    n = 77
    stale = c["x"].clone()
    stale[n:] = 1e30
    a1 = ops.kohonen_argmin(stale, c["w"], n=n)
    a2 = ops.kohonen_argmin(c["x"][:n].contiguous(), c["w"])
    assert torch.equal(a1, a2)
    w1, w2 = c["w"].clone(), c["w"].clone()
    ops.kohonen_update(stale, w1, c["coords"], a1, 0.5, 0.1, n=n)
    ops.kohonen_update(c["x"][:n].contiguous(), w2, c["coords"], a2, 0.5,
                       0.1)
    torch.cuda.synchronize()
    assert torch.isfinite(w1).all() and torch.equal(w1, w2)


def test_host_checks_raise_before_any_launch():
    c = case(2, torch.float32)
    x, w, coords = c["x"], c["w"], c["coords"]
    a = ops.kohonen_argmin(x, w)
    for bad_w in (w.t().contiguous().t(), w.bfloat16()):
        with pytest.raises(ValueError):
            ops.kohonen_argmin(x, bad_w)
        with pytest.raises(ValueError):
            ops.kohonen_update(x, bad_w, coords, a, 0.5, 0.1)
    with pytest.raises(ValueError):
        ops.kohonen_argmin(x[:, :2].contiguous(), w)       # D mismatch
    with pytest.raises(ValueError):
        ops.kohonen_update(x[:, :2].contiguous(), w, coords, a, 0.5, 0.1)
    with pytest.raises(ValueError):
        ops.kohonen_argmin(x.cpu(), w)
    with pytest.raises(ValueError):
        ops.kohonen_update(x, w, coords, a.long(), 0.5, 0.1)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- end to end
def _workflow(sample, backend, epochs=2):
    from veles_amd.backends import Device
    from veles_amd.dummy import DummyLauncher
    from veles_amd.models import KohonenWorkflow
    from veles_amd.prng import random_generator
    assert sample.GaussianClustersLoader.MAPPING == "gaussian_clusters"
    random_generator.get().seed(77)
    wf = KohonenWorkflow(
        DummyLauncher(), loader_name="gaussian_clusters",
        loader_config={"n_train": 400, "seed": 0, "minibatch_size": 20},
        trainer_config={"shape": (8, 8), "gradient_decay": (0.5, 0.02),
                        "radius_decay": (1.0, 0.1)},
        forward_config={"total": True},
        decision_config={"max_epochs": epochs})
    wf.initialize(device=Device(backend=backend))
    return wf


def test_workflow_matches_the_cpu_device():
    from veles_amd.utils.import_file import import_file
    sample = import_file(os.path.join(REPO, "samples", "kohonen.py"))
    cpu = _workflow(sample, "cpu")
    ld, tr = cpu.loader, cpu.trainer
    w = tr.weights.mem.astype(numpy.float64)
    order = []
    tr.before_run_ = [lambda: order.append(
        ld.minibatch_indices.mem[:ld.minibatch_size].copy())]
    cpu.run()
    # the float64 model on the same minibatch order: every sample's winner
    # is decided by more than the winner bound, so both devices must agree
    data = ld.original_data.mem.astype(numpy.float64)
    c64 = tr.coords.mem.astype(numpy.float64)
    sigma0 = 1.42 * (c64.max() - c64.min())
    assert len(order) == 40
    for t, idx in enumerate(order):
        x = data[idx]
        d = ((x[:, None, :] - w[None, :, :]) ** 2).sum(2)
        two = numpy.sort(d, axis=1)[:, :2]
        bound = 2e-6 * ((x ** 2).sum(1) + (w ** 2).sum(1).max())
        assert (two[:, 1] - two[:, 0] > bound).all(), t
        a = d.argmin(1)
        sigma, grad = sigma0 / (1 + 0.1 * t), 0.5 / (1 + 0.02 * t)
        G = numpy.exp(-((c64[None] - c64[a][:, None]) ** 2).sum(2) /
                      (2 * sigma * sigma))
        w = w + grad / len(x) * (G.T @ x - G.sum(0)[:, None] * w)

    gpu = _workflow(sample, "hip")
    assert gpu.trainer.weights.devmem.is_cuda
    assert gpu.loader.minibatch_data.devmem.dtype == torch.float32
    gpu.run()
    torch.cuda.synchronize()
    wc = cpu.trainer.weights.devmem.numpy().astype(numpy.float64)
    wg = gpu.trainer.weights.devmem.cpu().numpy().astype(numpy.float64)
    scale = numpy.abs(wc).max()
    assert numpy.abs(wc - w).max() <= 1e-4 * scale
    assert numpy.abs(wg - wc).max() <= 1e-4 * scale
    assert gpu.trainer.time == cpu.trainer.time == 40
    for e in range(2):
        assert (gpu.decision.epoch_winners[e] ==
                cpu.decision.epoch_winners[e]).all()
    assert (gpu.forward.total.devmem.cpu().numpy() ==
            cpu.forward.total.devmem.numpy()).all()
    assert abs(gpu.decision.history[-1] - cpu.decision.history[-1]) <= \
        1e-4 * cpu.decision.history[0]
