"""Adam with clipping by the global gradient norm under synchronous data
parallelism on the CPU (gloo, world_size 2): the norm is taken of the whole
gradient buffer after every bucket's all-reduce, so both ranks clip by the
same coefficient and end with bit-identical weights."""
import os
import socket

import numpy
import torch.multiprocessing as mp

CLIP = 0.3


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
    from veles_amd.utils.config import root
    root.common.engine.clip_gradient_norm = CLIP
    root.common.engine.dp.bucket_mb = 0.02       # several buckets
    from veles_amd.backends import Device
    from veles_amd.dummy import DummyLauncher
    from veles_amd.models import StandardWorkflow
    from veles_amd.parallel.dp import DataParallel
    import veles_amd.loader  # noqa: F401
    dp = DataParallel(backend="gloo")
    la = DummyLauncher()
    la.dp_ = dp
    g = {"solvers": ("adam",), "learning_rate": 1e-2}
    layers = [{"type": "all2all_tanh", "->": {"output_sample_shape": 100},
               "<-": dict(g)},
              {"type": "softmax", "->": {"output_sample_shape": 10},
               "<-": dict(g)}]
    wf = StandardWorkflow(
        la, loader_name="synthetic_images",
        loader_config={"dataset": "mnist", "class_lengths": (0, 100, 400),
                       "minibatch_size": 40,
                       "normalization_type": "mean_disp"},
        layers=layers,
        decision_config={"max_epochs": None, "fail_iterations": None})
    wf.initialize(device=Device(backend="cpu"))
    st = wf.param_store_
    norms = []
    for _ in range(steps):
        wf.run_steps(1)
        norms.append(st.last_grad_norm())
    assert len(st.buckets) >= 2, len(st.buckets)
    assert st._solver_segs is not None and st.t0 == 0 and st.steps == steps
    w = [f.weights_master.cpu().numpy().copy() for f in wf.forwards
         if getattr(f, "_pw_", None) is not None]
    numpy.savez(out % rank, numpy.array(norms, numpy.float64), *w)
    dp.shutdown()


def test_adam_with_clipping_on_two_ranks(tmp_path):
    steps = 5
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
    assert len(w0.files) == 3
    for k in w0.files:
        numpy.testing.assert_array_equal(w0[k], w1[k])
    norms = w0[w0.files[0]]
    print("pre-clip gradient norms:", norms)
    assert numpy.isfinite(norms).all() and (norms > 0).all()
    assert (norms > CLIP).any(), "no step clipped: %s" % norms
