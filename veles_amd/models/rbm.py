"""Restricted Boltzmann machines (reference algorithm list
docs/source/manualrst_veles_algorithms.rst "Restricted Boltzmann machine").
The Znicz sources are absent from the reference snapshot; the semantics are
this project's (docs/OPS.md "Restricted Boltzmann machines", parity
unpinned): Bernoulli-Bernoulli units trained by contrastive divergence.

Visible size V (the flattened sample), hidden size H, ``weights`` [H][V]
(the [out][in] convention: an All2AllSigmoid takes them as they are),
``hbias`` [H], ``vbias`` [V].  One CD-k step on the n valid rows of a
minibatch buffer of ``rows`` rows (rows past n are neither read nor written):

    ph0 = sigmoid(v0.W^T + hbias), h0 ~ Bern(ph0)
    for s = 1 .. k:  pv_s = sigmoid(h_{s-1}.W + vbias), v_s ~ Bern(pv_s)
                     (v_s = pv_s with sample_visible=False)
                     ph_s = sigmoid(v_s.W^T + hbias), h_s ~ Bern(ph_s), s < k
    g_W  = -(ph0^T.v0 - ph_k^T.v_k) / n
    g_hb = -sum_b (ph0 - ph_k) / n,  g_vb = -sum_b (v0 - v_k) / n
    one ops.sgd_update over the flat buffer (three segments)
    ops.seed_advance(seed_dev); time += 1

Every draw is ``u < p`` with the counter-based uniforms of ops.rbm_uniforms:
within a step ``base`` starts at 0 and advances by rows * N after every call
that draws, so a short last minibatch does not shift later draws.
``persistent=True`` (PCD) starts the negative chain from the hidden states
drawn at the end of the previous step (h_k ~ Bern(ph_k), one more draw)
instead of from h0; the first step starts from h0.  The hot steps are
``ops.rbm_sample`` and ``ops.rbm_grad`` (fused gfx950 kernels on the GPU, the
float32 reference on the CPU device).
"""
from __future__ import annotations

import numpy

from veles_amd.accelerated_units import AcceleratedUnit, AcceleratedWorkflow
from veles_amd.loader.base import TRAIN, VALID, UserLoaderRegistry
from veles_amd.memory import Array
from veles_amd.models.decision import DecisionBase
from veles_amd.models.nn_units import fill_weights
from veles_amd.plumbing import Repeater
from veles_amd.prng import device_seed, random_generator
from veles_amd import ops

__all__ = ["RBMTrainer", "RBMForward", "RBMDecision", "RBMWorkflow",
           "rbm_to_all2all", "rbm_log_likelihood"]


def _sync(t):
    """Host reads outside a workflow run are ordered against the current
    stream only; the step ran on the workflow's compute stream."""
    if t is not None and getattr(t, "is_cuda", False):
        import torch
        torch.cuda.synchronize(t.device)


def _hidden(kwargs):
    h = kwargs.get("hidden", kwargs.get("output_sample_shape", 16))
    if not isinstance(h, int):
        h = int(numpy.prod(tuple(h)))
    return int(h)


class RBMTrainer(AcceleratedUnit):
    """One CD-k step per TRAIN minibatch (module docstring); on the other
    minibatches only ph0, h0 and the reconstruction pv_1 are computed (for
    the decision), nothing is updated and the seed does not advance.

    kwargs: ``hidden`` (H), ``cd_k`` (1), ``learning_rate`` (0.1),
    ``gradient_moment`` (0.5), ``weights_decay`` (0), ``l1_vs_l2`` (0), the
    ``_bias`` variants of these four (default: the same values),
    ``sample_visible`` (True), ``persistent`` (False), ``weights_filling`` /
    ``weights_stddev`` (uniform +-0.05 from the project PRNG; biases start at
    zero).

    Creates the flat float32 ``params`` / ``moment`` / ``grad`` buffers in
    the layout of ops.rbm_layout ([W | hbias | vbias], segments on 16-element
    boundaries) with a bfloat16 copy of ``params`` on the GPU that the fused
    update rewrites; ``weights`` / ``hbias`` / ``vbias`` are views of
    ``params``.  Parameters, moment, the device seed, the PCD chain and
    ``time`` are pickled: k steps, snapshot, restore and m more steps equal
    k + m steps."""

    MAPPING = "rbm_trainer"

    def __init__(self, workflow, **kwargs):
        kwargs.setdefault("view_group", "TRAINER")
        super().__init__(workflow, **kwargs)
        self.hidden = _hidden(kwargs)
        self.cd_k = int(kwargs.get("cd_k", 1))
        self.learning_rate = float(kwargs.get("learning_rate", 0.1))
        self.gradient_moment = float(kwargs.get("gradient_moment", 0.5))
        self.weights_decay = float(kwargs.get("weights_decay", 0.0))
        self.l1_vs_l2 = float(kwargs.get("l1_vs_l2", 0.0))
        self.learning_rate_bias = float(kwargs.get("learning_rate_bias",
                                                   self.learning_rate))
        self.gradient_moment_bias = float(kwargs.get("gradient_moment_bias",
                                                     self.gradient_moment))
        self.weights_decay_bias = float(kwargs.get("weights_decay_bias",
                                                   self.weights_decay))
        self.l1_vs_l2_bias = float(kwargs.get("l1_vs_l2_bias",
                                              self.l1_vs_l2))
        self.sample_visible = bool(kwargs.get("sample_visible", True))
        self.persistent = bool(kwargs.get("persistent", False))
        self.weights_filling = kwargs.get("weights_filling", "uniform")
        self.weights_stddev = kwargs.get("weights_stddev", 0.05)
        self.rand = kwargs.get("rand", random_generator.get())
        if self.hidden < 1 or self.cd_k < 1:
            raise ValueError("RBMTrainer: hidden %d, cd_k %d" %
                             (self.hidden, self.cd_k))
        self.params = Array()
        self.moment = Array()
        self.chain = Array()          # PCD: h_k of the previous step
        self.chain_valid = False
        self.visible = 0
        self.time = 0
        self.seed = None
        self.seed_dev_saved = None
        self.minibatch_class = TRAIN
        self.demand("input", "minibatch_size")

    def init_unpickled(self):
        super().init_unpickled()
        self.seed_dev_ = None
        self.params_lp_ = None
        self.grad_ = None
        self.bufs_ = None
        self.segs_ = None
        self.table_ = None

    def __getstate__(self):
        _sync(self.params.devmem)
        device_seed.save(self)
        return super().__getstate__()

    # -- parameters ---------------------------------------------------------
    @property
    def layout(self):
        return ops.rbm_layout(self.visible, self.hidden)

    @property
    def weights(self):
        H, V = self.hidden, self.visible
        return self.params.devmem[:H * V].view(H, V)

    @property
    def hbias(self):
        o = self.layout[0]
        return self.params.devmem[o:o + self.hidden]

    @property
    def vbias(self):
        o = self.layout[1]
        return self.params.devmem[o:o + self.visible]

    @property
    def weights_lp(self):
        """The weights in the compute dtype (the bfloat16 copy on the GPU)."""
        if self.params_lp_ is None:
            return self.weights
        H, V = self.hidden, self.visible
        return self.params_lp_[:H * V].view(H, V)

    @property
    def seed_dev(self):
        return device_seed.get(self, self.torch_device, self._draw_seed)

    def _draw_seed(self):
        self.seed = int(self.rand.randint(0, 2 ** 31 - 1))
        return self.seed

    def refresh_lp(self):
        """Re-derive the bfloat16 copy after ``params`` was written from
        outside a step."""
        if self.params_lp_ is not None:
            self.params_lp_.copy_(self.params.devmem)

    def initialize(self, device=None, **kwargs):
        import torch
        super().initialize(device=device, **kwargs)
        rows = int(self.input.shape[0])
        V = int(numpy.prod(self.input.shape[1:]))
        H = self.hidden
        self.visible = V
        off_hb, off_vb, total = ops.rbm_layout(V, H)
        if self.params.mem is None or self.params.mem.shape != (total,):
            p = numpy.zeros(total, numpy.float32)
            w = numpy.zeros((H, V), numpy.float32)
            fill_weights(w, self.weights_filling, self.weights_stddev,
                         self.rand)
            p[:H * V] = w.ravel()
            self.params.reset(p)
            self.moment.reset(numpy.zeros(total, numpy.float32))
            self.chain_valid = False
        if self.chain.mem is None or self.chain.mem.shape != (rows, H):
            self.chain.reset(numpy.zeros((rows, H), numpy.float32))
            self.chain_valid = False
        dt = self.compute_dtype if self.is_gpu else torch.float32
        self.chain.initialize(self.device, device_dtype=dt)
        self.init_vectors(self.params, self.moment)
        dev = self.torch_device
        self.grad_ = torch.zeros(total, dtype=torch.float32, device=dev)
        self.params_lp_ = self.params.devmem.to(dt) if self.is_gpu else None

        def buf(n):
            return torch.zeros(rows, n, dtype=dt, device=dev)
        self.bufs_ = {"ph0": buf(H), "h": buf(H), "phk": buf(H),
                      "pv1": buf(V), "v": buf(V)}
        if self.cd_k > 1:
            self.bufs_["pv"] = buf(V)
        self.segs_ = [
            (0, H * V, self.learning_rate, self.weights_decay,
             self.l1_vs_l2, self.gradient_moment),
            (off_hb, off_hb + H, self.learning_rate_bias,
             self.weights_decay_bias, self.l1_vs_l2_bias,
             self.gradient_moment_bias),
            (off_vb, off_vb + V, self.learning_rate_bias,
             self.weights_decay_bias, self.l1_vs_l2_bias,
             self.gradient_moment_bias)]
        # created (or restored) before the first step
        device_seed.get(self, self.torch_device, self._draw_seed)

    # the buffers of the last step, for the decision and the tests
    @property
    def ph0(self):
        return self.bufs_["ph0"]

    @property
    def pv1(self):
        return self.bufs_["pv1"]

    def visible_input(self):
        x = self.input.devmem
        x = x.view(x.shape[0], -1)
        want = self.bufs_["v"].dtype
        return x if x.dtype == want else x.to(want)

    def run(self):
        n = int(self.minibatch_size)
        if n <= 0:
            return
        self.step(self.visible_input(), n, self.minibatch_class == TRAIN)

    def step(self, v0, n, train=True):
        """One CD-k step on the first ``n`` rows of ``v0`` (module
        docstring); ``train=False`` stops after pv_1."""
        b = self.bufs_
        rows = v0.shape[0]
        H, V = self.hidden, self.visible
        w, hb, vb = self.weights_lp, self.hbias, self.vbias
        sd = self.seed_dev
        k = self.cd_k
        h = b["h"]
        ops.rbm_sample(v0, w, hb, n=n, probs=b["ph0"], sample=h, seed_dev=sd,
                       base=0)
        base = rows * H
        hprev = h
        if train and self.persistent and self.chain_valid:
            hprev = self.chain.devmem
        vk = phk = None
        for s in range(1, k + 1):
            pv = b["pv1"] if s == 1 else b["pv"]
            if self.sample_visible:
                ops.rbm_sample(hprev, w, vb, transposed=True, n=n, probs=pv,
                               sample=b["v"], seed_dev=sd, base=base)
                base += rows * V
                vk = b["v"]
            else:
                ops.rbm_sample(hprev, w, vb, transposed=True, n=n, probs=pv,
                               seed_dev=sd)
                vk = pv
            if not train:
                return
            last = s == k
            hs = None if last else h
            if last and self.persistent:
                hs = self.chain.devmem
            phk = b["phk"]
            ops.rbm_sample(vk, w, hb, n=n, probs=phk, sample=hs, seed_dev=sd,
                           base=base)
            if hs is not None:
                base += rows * H
            hprev = h
        ops.rbm_grad(v0, b["ph0"], vk, phk, self.grad_, n=n)
        ops.sgd_update(self.params.devmem, self.grad_, self.moment.devmem,
                       self.segs_, w_lp=self.params_lp_)
        ops.seed_advance(sd)
        if self.persistent:
            self.chain_valid = True
        self.time += 1


class RBMForward(AcceleratedUnit):
    """``output`` = ph = sigmoid(v.W^T + hbias) of the minibatch, from a
    trainer's parameters (link ``weights`` = the trainer's ``weights_lp`` and
    ``hbias``, or set ``trainer``)."""

    MAPPING = "rbm_forward"

    def __init__(self, workflow, **kwargs):
        kwargs.setdefault("view_group", "WORKER")
        super().__init__(workflow, **kwargs)
        self.output = Array(shallow_pickle=True)
        self.trainer = None
        self.demand("input", "minibatch_size")

    def initialize(self, device=None, **kwargs):
        import torch
        super().initialize(device=device, **kwargs)
        if self.trainer is None:
            raise AttributeError("%s: trainer is not set" % self)
        rows = int(self.input.shape[0])
        dt = self.compute_dtype if self.is_gpu else torch.float32
        self.output.devmem = torch.zeros(rows, self.trainer.hidden, dtype=dt,
                                         device=self.torch_device)

    def run(self):
        n = int(self.minibatch_size)
        if n <= 0:
            return
        tr = self.trainer
        x = self.input.devmem
        x = x.view(x.shape[0], -1)
        y = self.output.devmem
        if x.dtype != y.dtype:
            x = x.to(y.dtype)
        ops.rbm_sample(x, tr.weights_lp, tr.hbias, n=n, probs=y)


def rbm_log_likelihood(weights, hbias, vbias, data):
    """The exact mean log-likelihood of the rows of ``data`` ([N][V], 0 / 1)
    under the RBM, by enumerating the 2^V visible states in float64 on the
    host (V <= 20):  log p(v) = v.vbias + sum_j softplus(v.W_j + hbias_j)
    - log Z."""
    w = numpy.asarray(weights, numpy.float64)
    hb = numpy.asarray(hbias, numpy.float64)
    vb = numpy.asarray(vbias, numpy.float64)
    V = w.shape[1]
    if V > 20:
        raise ValueError("rbm_log_likelihood: V = %d > 20" % V)

    def neg_free_energy(v):
        return v @ vb + numpy.logaddexp(0.0, v @ w.T + hb).sum(1)
    m = -numpy.inf
    parts = []
    bits = numpy.arange(V)
    for lo in range(0, 1 << V, 1 << 14):
        idx = numpy.arange(lo, min(lo + (1 << 14), 1 << V))
        a = neg_free_energy(((idx[:, None] >> bits) & 1).astype(
            numpy.float64))
        parts.append(a)
        m = max(m, float(a.max()))
    log_z = m + numpy.log(sum(float(numpy.exp(a - m).sum()) for a in parts))
    d = numpy.asarray(data, numpy.float64).reshape(len(data), -1)
    return float((neg_free_energy(d) - log_z).mean())


class RBMDecision(DecisionBase):
    """Per epoch and class (TRAIN, VALID): the reconstruction RMSE of v0
    against pv_1 (``ops.mse`` on the trainer's buffers, summed on the
    device and read once per epoch); with ``exact_likelihood=True`` and
    V <= 20 also the exact mean log-likelihood of the TRAIN samples under
    the parameters at the epoch's end (:func:`rbm_log_likelihood`), at
    every ``likelihood_interval``-th epoch (1) counted from the first, and
    at the last one.  ``complete`` at ``max_epochs``.  Results:
    ``reconstruction_rmse``, ``reconstruction_rmse_history`` ([train, valid]
    per epoch), ``log_likelihood``, ``log_likelihood_history`` ([epoch,
    value] pairs), ``epochs``."""

    MAPPING = "decision_rbm"

    def __init__(self, workflow, **kwargs):
        kwargs.setdefault("fail_iterations", None)
        super().__init__(workflow, **kwargs)
        self.exact_likelihood = bool(kwargs.get("exact_likelihood", False))
        self.likelihood_interval = max(
            1, int(kwargs.get("likelihood_interval", 1)))
        self.rmse = [None, None, None]
        self.history = []
        self.log_likelihood = None
        self.ll_history = []
        self.trainer = None
        self.loader = None

    def init_unpickled(self):
        super().init_unpickled()
        self.metrics_ = None

    def run(self):
        import torch
        n = int(self.minibatch_size)
        mc = self.minibatch_class
        tr = self.trainer
        if n > 0 and mc in (TRAIN, VALID):
            if self.metrics_ is None:
                self.metrics_ = torch.zeros(
                    3, 3, dtype=torch.float32, device=tr.pv1.device)
            ops.mse(tr.pv1, tr.visible_input(), metrics=self.metrics_[mc],
                    valid_rows=n)
        super().run()

    def on_epoch_ended(self):
        tr = self.trainer
        if self.metrics_ is not None:
            m = self.metrics_.detach().cpu().numpy().astype(numpy.float64)
            self.metrics_.zero_()
            for c in (TRAIN, VALID):
                # mean over the samples of the per-sample mean square
                self.rmse[c] = float(numpy.sqrt(m[c][0] / m[c][2])) \
                    if m[c][2] > 0 else None
        self.history.append([self.rmse[TRAIN], self.rmse[VALID]])
        msg = ""
        e = self.epoch_number
        last = self.max_epochs is not None and e + 1 >= self.max_epochs
        if self.exact_likelihood and (
                e % self.likelihood_interval == 0 or last):
            if tr.visible > 20:
                raise ValueError("%s: exact_likelihood needs V <= 20, got %d"
                                 % (self, tr.visible))
            ld = self.loader
            rows = ld.class_rows(TRAIN)
            data = ld.original_data.mem[numpy.sort(rows)]
            _sync(tr.params.devmem)
            self.log_likelihood = rbm_log_likelihood(
                tr.weights.detach().cpu().numpy(),
                tr.hbias.detach().cpu().numpy(),
                tr.vbias.detach().cpu().numpy(), data)
            self.ll_history.append([e, self.log_likelihood])
            msg = " log-likelihood %.4f" % self.log_likelihood
        self.improved <<= True
        self.snapshot_suffix = "rmse_%.6f" % (self.rmse[TRAIN] or 0.0)
        self.info("Epoch %d: reconstruction rmse train %s valid %s%s",
                  self.epoch_number, self.rmse[TRAIN], self.rmse[VALID], msg)
        self.increment_epoch()

    def get_metric_names(self):
        return {"reconstruction_rmse", "reconstruction_rmse_history",
                "log_likelihood", "log_likelihood_history", "epochs"}

    def get_metric_values(self):
        return {"reconstruction_rmse": self.rmse[TRAIN],
                "reconstruction_rmse_history": list(self.history),
                "log_likelihood": self.log_likelihood,
                "log_likelihood_history": list(self.ll_history),
                "epochs": len(self.history)}


class RBMWorkflow(AcceleratedWorkflow):
    """repeater -> loader -> trainer -> forward -> decision -> [snapshotter]
    -> repeater / end point, wired and gated as KohonenWorkflow.  kwargs:
    ``loader_name``, ``loader_config``, ``trainer_config``,
    ``decision_config``, ``snapshotter_config`` (None: no snapshots).

    The loop runs eager on one rank: no HIP-graph segments are attached
    (a step of the ops captures in a graph, tests/test_rbm_gpu.py), and
    training over a data-parallel group of more than one rank is not
    supported."""

    def __init__(self, workflow, **kwargs):
        super().__init__(workflow, **kwargs)
        self.loader_name = kwargs.get("loader_name")
        self.loader_config = dict(kwargs.get("loader_config") or {})
        self.trainer_config = dict(kwargs.get("trainer_config") or {})
        self.decision_config = dict(kwargs.get("decision_config") or {})
        self.snapshotter_config = kwargs.get("snapshotter_config")
        self.snapshotter = None
        self.create_workflow()

    def create_workflow(self):
        self.repeater = Repeater(self)
        self.repeater.link_from(self.start_point)

        cls = UserLoaderRegistry.loaders.get(self.loader_name)
        if cls is None:
            raise ValueError("Unknown loader %r (known: %s)" % (
                self.loader_name, sorted(UserLoaderRegistry.loaders)))
        self.loader = ld = cls(self, **self.loader_config)
        ld.link_from(self.repeater)

        self.trainer = tr = RBMTrainer(self, **self.trainer_config)
        tr.link_from(ld)
        tr.link_attrs(ld, ("input", "minibatch_data"), "minibatch_size",
                      "minibatch_class")

        self.forward = fw = RBMForward(self)
        fw.trainer = tr
        fw.link_from(tr)
        fw.link_attrs(ld, ("input", "minibatch_data"), "minibatch_size")

        self.decision = dc = RBMDecision(self, **self.decision_config)
        dc.trainer = tr
        dc.loader = ld
        dc.link_from(fw)
        dc.link_attrs(ld, "minibatch_class", "last_minibatch",
                      "class_lengths", "epoch_ended", "minibatch_size")
        dc.link_attrs(ld, "epoch_number", two_way=True)
        last = dc

        if self.snapshotter_config is not None:
            from veles_amd.snapshotter import SnapshotterRegistry, \
                SnapshotterToFile
            cfg = dict(self.snapshotter_config)
            kind = cfg.pop("kind", "file")
            scls = SnapshotterRegistry.snapshotters.get(kind,
                                                        SnapshotterToFile)
            self.snapshotter = sn = scls(self, **cfg)
            sn.link_from(last)
            sn.link_attrs(dc, ("suffix", "snapshot_suffix"))
            sn.gate_skip = ~dc.epoch_ended_flag
            last = sn

        self.repeater.link_from(last)
        self.repeater.gate_block = dc.complete | dc.steps_complete
        self.end_point.link_from(last)
        self.end_point.gate_block = ~dc.complete

    def initialize(self, **kwargs):
        from veles_amd.parallel import find_dp
        dp = find_dp(self)
        if dp is not None and dp.world_size > 1:
            raise NotImplementedError(
                "RBMWorkflow trains on one rank: the data-parallel group "
                "has %d (multi-rank RBM training is not implemented)" %
                dp.world_size)
        return super().initialize(**kwargs)


def rbm_to_all2all(trainer, unit):
    """Copy ``weights`` [H][V] and ``hbias`` of a trained RBM into the
    All2AllSigmoid ``unit`` (H outputs, V inputs): greedy pre-training of a
    layer, and export through the existing All2All path.  Before the unit is
    initialised the copies become its initial parameters; afterwards they
    are written into its registered parameters."""
    _sync(trainer.params.devmem)
    w = trainer.weights.detach().float().cpu().numpy().copy()
    hb = trainer.hbias.detach().float().cpu().numpy().copy()
    if getattr(unit, "weights_transposed", False):
        raise ValueError("rbm_to_all2all: %s has transposed weights" % unit)
    if unit.neurons_number != w.shape[0]:
        raise ValueError("rbm_to_all2all: %s has %d outputs, the RBM %d "
                         "hidden units" % (unit, unit.neurons_number,
                                           w.shape[0]))
    pw, pb = unit._pw_, unit._pb_
    if pw is not None and tuple(pw.host.shape) != w.shape:
        raise ValueError("rbm_to_all2all: %s weights %s, the RBM's %s" %
                         (unit, tuple(pw.host.shape), w.shape))
    unit.weights.reset(w)
    if unit.include_bias:
        unit.bias.reset(hb)
    if pw is None:
        return unit
    import torch
    for p, arr, v in ((pw, unit.weights, w), (pb, unit.bias, hb)):
        if p is None:
            continue
        p.host = arr.mem
        if p.master is not None:
            t = torch.from_numpy(v).to(p.master.device)
            p.master.copy_(t.view(p.master.shape))
            if p.lp is not None and p.lp is not p.master:
                p.lp.copy_(t.view(p.lp.shape))
    return unit
