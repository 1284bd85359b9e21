"""Kohonen maps on the CPU device: the ops against a float64 numpy model
that follows docs/OPS.md "Kohonen maps" literally (a per-sample loop), the
trainer against that model fed the same minibatch order, snapshot / resume,
and the forward, validator and plotter units."""
import os
import pickle

import numpy
import pytest
import torch

from veles_amd import ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------ float64 model
def model_winners(x, w):
    """a_b = argmin_n |x_b - W[n]|^2, the first of equal minima."""
    return numpy.array([int(numpy.argmin(((xb[None, :] - w) ** 2).sum(1)))
                        for xb in x], numpy.int64)


def model_step(x, w, coords, sigma, gradient):
    """One training step; returns (new weights, winners)."""
    B = len(x)
    a = model_winners(x, w)
    dw = numpy.zeros_like(w)
    for b in range(B):
        g = numpy.exp(-((coords - coords[a[b]][None, :]) ** 2).sum(1) /
                      (2.0 * sigma * sigma))
        dw += g[:, None] * (x[b][None, :] - w)
    return w + (gradient / B) * dw, a


def model_coords(sx, sy):
    h = 2.0 / max(sx - 1, sy - 1, 1)
    return numpy.array([[(x - (sx - 1) / 2.0) * h, (y - (sy - 1) / 2.0) * h]
                        for y in range(sy) for x in range(sx)])


def _operands(B, sx, sy, D, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, D, generator=g)
    w = torch.rand(sx * sy, D, generator=g) * 2 - 1
    return x, w, ops.kohonen_coords(sx, sy)


SHAPES = [(1, 1, 1, 1), (64, 8, 8, 2), (37, 5, 4, 3), (50, 7, 3, 19)]


# ---------------------------------------------------------------------- ops
def test_coords_follow_the_spec():
    for sx, sy in ((1, 1), (8, 8), (5, 7), (33, 3)):
        c = ops.kohonen_coords(sx, sy).double().numpy()
        assert numpy.abs(c - model_coords(sx, sy)).max() < 1e-7
    c = ops.kohonen_coords(33, 3)
    assert float(c[:, 0].min()) == -1.0 and float(c[:, 0].max()) == 1.0


@pytest.mark.parametrize("B,sx,sy,D", SHAPES)
def test_argmin_against_the_model(B, sx, sy, D):
    x, w, _ = _operands(B, sx, sy, D, 3)
    NN = sx * sy
    qerr = torch.zeros(B)
    winners = torch.ones(NN, dtype=torch.int32)
    got = ops.kohonen_argmin(x, w, qerr=qerr, winners=winners)
    assert got.dtype == torch.int32 and tuple(got.shape) == (B,)
    x64, w64 = x.double().numpy(), w.double().numpy()
    d = ((x64[:, None, :] - w64[None, :, :]) ** 2).sum(2)
    ref = model_winners(x64, w64)
    # float32 expansion |W|^2 - 2 x.W: a different winner only within its
    # rounding error (a few 2^-24 of the magnitudes summed)
    bound = 2e-6 * ((x64 ** 2).sum(1) + (w64 ** 2).sum(1).max())
    g = got.long().numpy()
    assert (d[numpy.arange(B), g] - d.min(1) <= bound).all()
    assert (g == ref).all()   # and on this data the same winner outright
    assert (numpy.abs(qerr.double().numpy() - d.min(1)) <= bound).all()
    assert (winners.numpy() == 1 + numpy.bincount(ref, minlength=NN)).all()


def test_argmin_ties_go_to_the_lowest_index():
    x, w, _ = _operands(40, 6, 5, 4, 5)
    w[20] = w[3]
    a = ops.kohonen_argmin(x, w)
    assert not (a == 20).any() and (a == 3).any()
    assert (ops.kohonen_argmin(x, torch.zeros_like(w)) == 0).all()


@pytest.mark.parametrize("B,sx,sy,D", SHAPES)
@pytest.mark.parametrize("sigma", [0.05, 0.5, 2.84])
def test_update_against_the_model(B, sx, sy, D, sigma):
    x, w, coords = _operands(B, sx, sy, D, 7)
    a = ops.kohonen_argmin(x, w)
    w0 = w.clone()
    ops.kohonen_update(x, w, coords, a, sigma, 0.1)
    x64, w64 = x.double().numpy(), w0.double().numpy()
    c64 = coords.double().numpy()
    ref, am = model_step(x64, w64, c64, sigma, 0.1)
    assert (am == a.long().numpy()).all()
    G = numpy.exp(-((c64[None] - c64[am][:, None]) ** 2).sum(2) /
                  (2 * sigma * sigma))               # [B][NN]
    mag = G.T @ numpy.abs(x64) + G.sum(0)[:, None] * numpy.abs(w64)
    bound = 4e-6 * (0.1 / B) * mag + 2.0 ** -23 * numpy.abs(w64)
    assert (numpy.abs(w.double().numpy() - ref) <= bound).all()


def test_only_the_valid_rows_are_read():
    x, w, coords = _operands(48, 6, 4, 5, 11)
    n = 29
    stale = x.clone()
    stale[n:] = 1e30
    q1, q2 = torch.zeros(48), torch.zeros(48)
    h1 = torch.zeros(24, dtype=torch.int32)
    h2 = torch.zeros(24, dtype=torch.int32)
    a1 = ops.kohonen_argmin(stale, w, n=n, qerr=q1, winners=h1)
    a2 = ops.kohonen_argmin(x[:n].contiguous(), w, qerr=q2, winners=h2)
    assert tuple(a1.shape) == (n,) and torch.equal(a1, a2)
    assert torch.equal(q1[:n], q2[:n]) and torch.equal(h1, h2)
    w1, w2 = w.clone(), w.clone()
    ops.kohonen_update(stale, w1, coords, a1, 0.5, 0.1, n=n)
    ops.kohonen_update(x[:n].contiguous(), w2, coords, a2, 0.5, 0.1)
    assert torch.isfinite(w1).all() and torch.equal(w1, w2)


def test_out_of_range_winners_are_clamped():
    x, w, coords = _operands(16, 4, 4, 3, 13)
    a = ops.kohonen_argmin(x, w).clone()
    bad = a.clone()
    a[0], bad[0] = 0, -1
    a[1], bad[1] = 15, 16
    w1, w2 = w.clone(), w.clone()
    ops.kohonen_update(x, w1, coords, bad, 0.5, 0.1)
    ops.kohonen_update(x, w2, coords, a, 0.5, 0.1)
    assert torch.equal(w1, w2)


def test_host_checks():
    x, w, coords = _operands(16, 4, 4, 6, 17)
    a = ops.kohonen_argmin(x, w)
    with pytest.raises(ValueError):
        ops.kohonen_argmin(x, w.t().contiguous().t())      # non-contiguous
    with pytest.raises(ValueError):
        ops.kohonen_argmin(x, w.bfloat16())
    with pytest.raises(ValueError):
        ops.kohonen_argmin(x[:, :5].contiguous(), w)       # D mismatch
    with pytest.raises(ValueError):
        ops.kohonen_argmin(x, w, n=17)
    with pytest.raises(ValueError):
        ops.kohonen_argmin(x, w, argmin=torch.zeros(16, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.kohonen_update(x, w, coords[:15], a, 0.5, 0.1)
    with pytest.raises(ValueError):
        ops.kohonen_update(x, w, coords, a, 0.0, 0.1)


# -------------------------------------------------------------------- units
@pytest.fixture(scope="module")
def sample():
    from veles_amd.utils.import_file import import_file
    return import_file(os.path.join(REPO, "samples", "kohonen.py"))


def make_workflow(sample, n_train=400, minibatch=20, shape=(8, 8), epochs=6,
                  backend="cpu", seed=0, total=True, plotters=False,
                  plot_dir=None):
    from veles_amd.backends import Device
    from veles_amd.dummy import DummyLauncher
    from veles_amd.models import KohonenWorkflow
    from veles_amd.prng import random_generator
    assert sample.GaussianClustersLoader.MAPPING == "gaussian_clusters"
    random_generator.get().seed(77)
    wf = KohonenWorkflow(
        DummyLauncher(), loader_name="gaussian_clusters",
        loader_config={"n_train": n_train, "seed": seed,
                       "minibatch_size": minibatch},
        trainer_config={"shape": shape, "gradient_decay": (0.5, 0.02),
                        "radius_decay": (1.0, 0.1)},
        forward_config={"total": total},
        decision_config={"max_epochs": epochs}, plotters=plotters)
    if plot_dir is not None:
        for p in wf.plotters:
            p.directory = str(plot_dir)
            p.redraw_threshold = 0.0
    wf.initialize(device=Device(backend=backend))
    return wf


def state_of(wf):
    tr = wf.trainer
    if tr.weights.devmem.is_cuda:
        torch.cuda.synchronize()
    return (tr.weights.devmem.detach().cpu().numpy().copy(),
            tr.winners.devmem.detach().cpu().numpy().copy(), tr.time)


def test_trainer_matches_the_model(sample):
    wf = make_workflow(sample, n_train=90, minibatch=40, shape=(5, 4),
                       epochs=3)
    tr, ld = wf.trainer, wf.loader
    w = tr.weights.mem.astype(numpy.float64)
    order = []
    tr.before_run_ = [lambda: order.append(
        ld.minibatch_indices.mem[:ld.minibatch_size].copy())]
    wf.run()
    assert [len(o) for o in order] == [40, 40, 10] * 3
    data = ld.original_data.mem.astype(numpy.float64)
    coords = model_coords(5, 4)
    sigma0 = 1.42 * (coords.max() - coords.min())
    hist = []
    for t, idx in enumerate(order):
        w, a = model_step(data[idx], w, coords,
                          sigma0 / (1 + 0.1 * t), 0.5 / (1 + 0.02 * t))
        hist.append(a)
    got_w, got_winners, got_t = state_of(wf)
    assert got_t == 9
    assert numpy.abs(got_w - w).max() <= 1e-4 * numpy.abs(w).max()
    # the decision moved every epoch's histogram into its history
    assert (got_winners == 0).all()
    for e in range(3):
        ref = numpy.bincount(numpy.concatenate(hist[3 * e:3 * e + 3]),
                             minlength=20)
        assert (wf.decision.epoch_winners[e] == ref).all()
    res = wf.decision.get_metric_values()
    assert res["epochs"] == 3 and len(
        res["quantization_error_history"]) == 3


def test_snapshot_resume_is_bit_equal(sample):
    from veles_amd.backends import Device
    from veles_amd.dummy import DummyLauncher
    wf = make_workflow(sample, n_train=90, minibatch=40, shape=(5, 4),
                       epochs=4)
    wf.run()
    ref = state_of(wf)
    hist = list(wf.decision.history)
    wf = make_workflow(sample, n_train=90, minibatch=40, shape=(5, 4),
                       epochs=2)
    wf.run()
    blob = pickle.dumps(wf, protocol=pickle.HIGHEST_PROTOCOL)
    del wf
    wf2 = pickle.loads(blob)
    wf2.workflow = DummyLauncher()
    wf2.decision.max_epochs = 4
    wf2.decision.complete <<= False
    wf2.initialize(device=Device(backend="cpu"))
    assert wf2.trainer.time == 6
    wf2.run()
    got = state_of(wf2)
    assert got[2] == ref[2] == 12
    assert (got[0] == ref[0]).all() and (got[1] == ref[1]).all()
    assert wf2.decision.history == hist


def test_forward_total_validator_and_plotters(sample, tmp_path):
    from veles_amd.models import KohonenValidator
    from veles_amd.utils.config import root
    old = root.common.disable.plotting
    root.common.disable.plotting = False
    try:
        wf = make_workflow(sample, plotters=True, plot_dir=tmp_path)
        wf.run()
    finally:
        root.common.disable.plotting = old
    total = wf.forward.total.devmem.numpy()
    # every sample exactly once per epoch: no gaps, and the histogram of
    # the scattered winners is the epoch's winners histogram
    assert total.shape == (400,) and (total >= 0).all()
    assert (numpy.bincount(total, minlength=64) ==
            wf.decision.epoch_winners[-1]).all()
    assert wf.forward.output.devmem is wf.trainer.argmins.devmem
    val = KohonenValidator(wf)
    val.link_attrs(wf.forward, "total")
    val.link_attrs(wf.trainer, "shape")
    val.loader = wf.loader
    val.initialize()
    val.run()
    assert val.fitness == 1.0
    assert val.result.shape == (64,) and set(val.result) <= {-1, 0, 1, 2, 3}
    assert len(wf.plotters) == 3
    for p in wf.plotters:
        assert p.files, p.name
        for f in p.files:
            assert os.path.getsize(f) > 0


def test_forward_without_a_trainer_runs_the_search(sample):
    from veles_amd.dummy import DummyWorkflow
    from veles_amd.memory import Array
    from veles_amd.models import KohonenForward
    x, w, _ = _operands(12, 3, 3, 4, 19)
    fw = KohonenForward(DummyWorkflow())
    fw.input, fw.weights = Array(x.numpy()), Array(w.numpy())
    fw.minibatch_size = 9
    fw.initialize()
    fw.input.initialize(fw.device)
    fw.weights.initialize(fw.device)
    fw.run()
    assert torch.equal(fw.output.devmem[:9],
                       ops.kohonen_argmin(x[:9].contiguous(), w))


def test_multi_rank_is_refused(sample, monkeypatch):
    import veles_amd.parallel as par
    wf = make_workflow(sample, epochs=1)

    class TwoRanks(object):
        world_size, rank = 2, 0
    monkeypatch.setattr(par, "find_dp", lambda wf: TwoRanks())
    with pytest.raises(NotImplementedError, match="one rank"):
        wf.initialize()
