"""Batch normalisation under synchronous data parallelism on the CPU (gloo,
world_size 2): dgamma and dbeta are all-reduced with the other gradients, so
gamma and beta stay equal across the ranks; the statistics are each rank's
own (plain batch normalisation, not SyncBN), so the running statistics are
those of the rank's shard and differ between the ranks."""
import os
import socket

import numpy
import torch.multiprocessing as mp

MOM = 0.25


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _train(rank, world, port, out, steps):
    import torch
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world),
                       "LOCAL_RANK": str(rank), "MASTER_ADDR": "127.0.0.1",
                       "MASTER_PORT": str(port)})
    torch.set_num_threads(1)
    from veles_amd import ops
    from veles_amd.backends import Device
    from veles_amd.dummy import DummyLauncher
    from veles_amd.models import StandardWorkflow
    from veles_amd.parallel.dp import DataParallel
    import veles_amd.loader  # noqa: F401
    dp = DataParallel(backend="gloo")
    la = DummyLauncher()
    la.dp_ = dp
    g = {"learning_rate": 0.02, "gradient_moment": 0.9}
    layers = [{"type": "all2all", "->": {"output_sample_shape": 24},
               "<-": dict(g)},
              {"type": "batch_norm_tanh", "->": {"momentum": MOM},
               "<-": dict(g)},
              {"type": "softmax", "->": {"output_sample_shape": 10},
               "<-": dict(g)}]
    wf = StandardWorkflow(
        la, loader_name="synthetic_images",
        loader_config={"dataset": "mnist", "class_lengths": (0, 0, 400),
                       "minibatch_size": 40,
                       "normalization_type": "mean_disp"},
        layers=layers,
        decision_config={"max_epochs": None, "fail_iterations": None})
    wf.initialize(device=Device(backend="cpu"))
    bn = wf.forwards[1]
    seen = []
    real = ops.batchnorm_fwd

    def spy(x, *a, **kw):
        seen.append(x.double().reshape(-1, x.shape[-1]).clone())
        return real(x, *a, **kw)
    ops.batchnorm_fwd = spy
    wf.run_steps(steps)
    ops.batchnorm_fwd = real
    # the running statistics of this rank, replayed from the shards it saw
    rm = torch.zeros(24, dtype=torch.float64)
    rv = torch.ones(24, dtype=torch.float64)
    for x in seen:
        rm = (1 - MOM) * rm + MOM * x.mean(0)
        rv = (1 - MOM) * rv + MOM * x.var(0, unbiased=True)
    got_rm, got_rv = (t.double() for t in bn.running_stats())
    assert len(seen) == steps
    assert torch.allclose(got_rm, rm, rtol=1e-4, atol=1e-5)
    assert torch.allclose(got_rv, rv, rtol=1e-4, atol=1e-5)
    numpy.savez(out % rank, gamma=bn.weights_master.numpy().copy(),
                beta=bn.bias_master.numpy().copy(),
                rm=got_rm.numpy(), rv=got_rv.numpy(),
                rows=numpy.array([x.shape[0] for x in seen]))
    dp.shutdown()


def test_two_ranks_share_gamma_and_beta_and_keep_their_own_statistics(
        tmp_path):
    steps = 4
    out = str(tmp_path / "w%d.npz")
    port = _free_port()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_train, args=(r, 2, port, out, steps))
             for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
        assert p.exitcode == 0
    w0, w1 = numpy.load(out % 0), numpy.load(out % 1)
    numpy.testing.assert_array_equal(w0["gamma"], w1["gamma"])
    numpy.testing.assert_array_equal(w0["beta"], w1["beta"])
    assert (w0["gamma"] != 1).any() and (w0["beta"] != 0).any()
    # each rank normalised its own half of the 40-sample minibatch
    assert (w0["rows"] == 20).all() and (w1["rows"] == 20).all()
    assert not numpy.allclose(w0["rm"], w1["rm"], rtol=1e-3, atol=1e-4)
    assert not numpy.allclose(w0["rv"], w1["rv"], rtol=1e-3, atol=1e-4)
