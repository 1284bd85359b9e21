"""Kohonen maps (self-organising maps; reference algorithm list
docs/source/manualrst_veles_algorithms.rst "Kohonen maps": forward, trainer
and decision units, plotters, the DemoKohonen sample).  The Znicz sources
are absent from the reference snapshot; the semantics are this project's
(docs/OPS.md "Kohonen maps", parity unpinned).

A map of ``shape = (sx, sy)`` has ``NN = sx * sy`` neurons; neuron
``n = y * sx + x`` has float32 weights ``W[n]`` and a grid position
``coords[n]``.  One training step on a minibatch of B valid rows:

    a_b   = argmin_n |x_b - W[n]|^2                    (ties: lowest n)
    G     = exp(-|coords[n] - coords[a_b]|^2 / (2 sigma^2))
    W[n] += (gradient_decay(t) / B) * sum_b G[b][n] (x_b - W[n])
    winners[a_b] += 1 ; t += 1

with ``sigma = radius_decay(t) * 1.42 * (max(coords) - min(coords))``.  The
two hot steps are ``ops.kohonen_argmin`` and ``ops.kohonen_update`` (fused
gfx950 kernels on the GPU, the float32 reference on the CPU device).  This is
the one algorithm family here that is not gradient descent: it reuses the
loaders, the decision / snapshot / plotting layers, but no GD unit.
"""
from __future__ import annotations

import numpy

from veles_amd.accelerated_units import AcceleratedUnit, AcceleratedWorkflow
from veles_amd.loader.base import TRAIN, UserLoaderRegistry
from veles_amd.memory import Array
from veles_amd.models.decision import DecisionBase
from veles_amd.models.nn_units import fill_weights
from veles_amd.plumbing import Repeater
from veles_amd.prng import random_generator
from veles_amd.units import Unit
from veles_amd.workflow import IResultProvider
from veles_amd import ops

__all__ = ["HyperbolicDecay", "KohonenTrainer", "KohonenForward",
           "KohonenDecision", "KohonenValidator", "KohonenWorkflow"]


class HyperbolicDecay(object):
    """t -> a / (1 + b t): a picklable schedule (a lambda in a unit would
    keep the workflow out of snapshots)."""

    def __init__(self, a, b):
        self.a, self.b = float(a), float(b)

    def __call__(self, t):
        return self.a / (1.0 + self.b * t)

    def __repr__(self):
        return "HyperbolicDecay(%g, %g)" % (self.a, self.b)


def _decay(v, default):
    """A schedule from a callable or an ``(a, b)`` pair (config files)."""
    if v is None:
        return HyperbolicDecay(*default)
    if callable(v):
        return v
    a, b = v
    return HyperbolicDecay(a, b)


def _sync(t):
    """Host reads outside a workflow run are ordered against the current
    stream only; the step ran on the workflow's compute stream."""
    if t is not None and getattr(t, "is_cuda", False):
        import torch
        torch.cuda.synchronize(t.device)


class KohonenTrainer(AcceleratedUnit):
    """One training step per TRAIN minibatch (module docstring).  kwargs:
    ``shape`` (sx, sy); ``weights_filling`` / ``weights_stddev`` (initial
    weights from the project PRNG); ``gradient_decay`` / ``radius_decay``:
    callables of the step number t, or (a, b) for a / (1 + b t) - plain
    floats evaluated on the host once per step and passed by value.

    Creates ``weights`` [NN][D], ``coords`` [NN][2] (``coords.reset(...)``
    before ``initialize`` installs another grid, e.g. a hexagonal one: the
    kernels only read it), ``winners`` [NN], ``argmins``
    and ``qerr`` per minibatch row, and ``time``.  Weights, winners and time
    are pickled: a k-epoch run, snapshot, restore and m more epochs equal a
    k + m epoch run."""

    MAPPING = "kohonen_trainer"

    def __init__(self, workflow, **kwargs):
        kwargs.setdefault("view_group", "TRAINER")
        super().__init__(workflow, **kwargs)
        shape = kwargs.get("shape", (8, 8))
        self.shape = (int(shape[0]), int(shape[1]))
        self.weights_filling = kwargs.get("weights_filling", "uniform")
        self.weights_stddev = kwargs.get("weights_stddev", 0.05)
        self.gradient_decay = _decay(kwargs.get("gradient_decay"),
                                     (0.1, 0.05))
        self.radius_decay = _decay(kwargs.get("radius_decay"), (1.0, 0.05))
        self.rand = kwargs.get("rand", random_generator.get())
        self.weights = Array()
        self.coords = Array()
        self.winners = Array()
        self.argmins = Array(shallow_pickle=True)
        self.qerr = Array(shallow_pickle=True)
        self.time = 0
        self.minibatch_class = TRAIN
        self.demand("input", "minibatch_size")

    @property
    def neurons_number(self):
        return self.shape[0] * self.shape[1]

    @property
    def sigma0(self):
        """1.42 x the extent of the grid over both axes (1.42 for a map of
        one neuron, where every gravity is 1 whatever sigma)."""
        c = self.coords.to_numpy()
        ext = float(c.max() - c.min())
        return 1.42 * ext if ext > 0 else 1.42

    def __getstate__(self):
        _sync(self.weights.devmem)
        return super().__getstate__()

    def initialize(self, device=None, **kwargs):
        super().initialize(device=device, **kwargs)
        sx, sy = self.shape
        if sx < 1 or sy < 1:
            raise ValueError("KohonenTrainer: shape %s" % (self.shape,))
        NN = self.neurons_number
        rows = int(self.input.shape[0])
        D = int(numpy.prod(self.input.shape[1:]))
        if self.weights.mem is None or self.weights.mem.shape != (NN, D):
            w = numpy.zeros((NN, D), numpy.float32)
            fill_weights(w, self.weights_filling, self.weights_stddev,
                         self.rand)
            self.weights.reset(w)
        if self.coords.mem is None or self.coords.mem.shape != (NN, 2):
            self.coords.reset(ops.kohonen_coords(sx, sy).numpy())
        if self.winners.mem is None or self.winners.mem.shape != (NN,):
            self.winners.reset(numpy.zeros(NN, numpy.int32))
        self.argmins.reset(numpy.zeros(rows, numpy.int32))
        self.qerr.reset(numpy.zeros(rows, numpy.float32))
        self.init_vectors(self.weights, self.coords, self.winners,
                          self.argmins, self.qerr)
        self.sigma0_ = self.sigma0

    def run(self):
        n = int(self.minibatch_size)
        if n <= 0:
            return
        x = self.input.devmem
        w = self.weights.devmem
        a = self.argmins.devmem
        train = self.minibatch_class == TRAIN
        ops.kohonen_argmin(x, w, n=n, argmin=a, qerr=self.qerr.devmem,
                           winners=self.winners.devmem if train else None)
        if not train:
            return
        t = self.time
        ops.kohonen_update(x, w, self.coords.devmem, a,
                           float(self.radius_decay(t)) * self.sigma0_,
                           float(self.gradient_decay(t)), n=n)
        self.time = t + 1


class KohonenForward(AcceleratedUnit):
    """``output``: the winner of every minibatch row.  Linked to a trainer's
    ``argmins`` it reuses them (the winners under the weights the step
    started from); otherwise it needs ``weights`` and runs the winner search
    itself.  ``total=True``: the winners are also scattered to
    ``total[minibatch_indices[i]]``, which therefore holds every sample's
    winner after an epoch (``total_samples`` rows, -1 before)."""

    MAPPING = "kohonen_forward"

    def __init__(self, workflow, **kwargs):
        kwargs.setdefault("view_group", "WORKER")
        super().__init__(workflow, **kwargs)
        self.with_total = bool(kwargs.get("total", False))
        self.output = Array(shallow_pickle=True)
        self.total = Array()
        self.argmins = None
        self.weights = None
        self.minibatch_indices = None
        self.total_samples = 0
        self.demand("input", "minibatch_size")
        if self.with_total:
            self.demand("minibatch_indices", "total_samples")

    def initialize(self, device=None, **kwargs):
        super().initialize(device=device, **kwargs)
        if self.argmins is None and self.weights is None:
            raise AttributeError("%s: link argmins (a trainer's) or weights"
                                 % self)
        rows = int(self.input.shape[0])
        if self.argmins is None:
            self.output.reset(numpy.zeros(rows, numpy.int32))
            self.init_vectors(self.output)
        if self.with_total:
            n = int(self.total_samples)
            if self.total.mem is None or self.total.mem.shape != (n,):
                self.total.reset(numpy.full(n, -1, numpy.int32))
            self.init_vectors(self.total)

    def run(self):
        n = int(self.minibatch_size)
        if n <= 0:
            return
        if self.argmins is not None:
            if self.output.devmem is not self.argmins.devmem:
                self.output.devmem = self.argmins.devmem
        else:
            ops.kohonen_argmin(self.input.devmem, self.weights.devmem, n=n,
                               argmin=self.output.devmem)
        if self.with_total:
            idx = self.minibatch_indices.devmem[:n].long()
            self.total.devmem.index_copy_(0, idx, self.output.devmem[:n])


class KohonenDecision(DecisionBase):
    """Per epoch: the mean quantisation error of the TRAIN minibatches and a
    copy of ``winners`` (then reset for the next epoch); ``complete`` at
    ``max_epochs``.  Results: ``quantization_error`` (last epoch),
    ``quantization_error_history`` and ``epochs``."""

    MAPPING = "decision_kohonen"

    def __init__(self, workflow, **kwargs):
        kwargs.setdefault("fail_iterations", None)
        super().__init__(workflow, **kwargs)
        self.quantization_error = None
        self.history = []
        self.winners_history_limit = int(kwargs.get("winners_history_limit",
                                                    16))
        self.epoch_winners = []
        self.last_winners = Array()
        self._qsum = 0.0
        self._qcount = 0
        self.demand("winners", "qerr")

    def init_unpickled(self):
        super().init_unpickled()
        self.qacc_ = None

    def run(self):
        n = int(self.minibatch_size)
        if self.minibatch_class == TRAIN and n > 0:
            # summed on the device; read once per epoch
            s = self.qerr.devmem[:n].sum(dtype=_f64())
            self.qacc_ = s if self.qacc_ is None else self.qacc_ + s
            self._qcount += n
        super().run()

    def on_epoch_ended(self):
        if self.qacc_ is not None:
            self._qsum += float(self.qacc_.item())
            self.qacc_ = None
        q = self._qsum / max(self._qcount, 1)
        self._qsum, self._qcount = 0.0, 0
        self.quantization_error = q
        self.history.append(q)
        self.improved <<= True
        w = self.winners.devmem
        last = w.detach().cpu().numpy().copy()
        self.last_winners.reset(last)
        self.epoch_winners.append(last)
        del self.epoch_winners[:-self.winners_history_limit]
        w.zero_()
        self.snapshot_suffix = "qerr_%.6f" % q
        self.info("Epoch %d: quantization error %.6f", self.epoch_number, q)
        self.increment_epoch()

    def get_metric_names(self):
        return {"quantization_error", "quantization_error_history", "epochs"}

    def get_metric_values(self):
        return {"quantization_error": self.quantization_error,
                "quantization_error_history": list(self.history),
                "epochs": len(self.history)}


def _f64():
    import torch
    return torch.float64


class KohonenValidator(Unit, IResultProvider):
    """From ``total`` (every sample's winner, KohonenForward(total=True))
    and the samples' ``labels``: ``result`` = the majority label of every
    neuron (-1 where no sample won) and ``fitness`` = the share of labelled
    samples whose winner's majority label is their own.  The labels are
    ``labels`` (one per sample, in dataset order) or, with ``loader`` set,
    that loader's ``original_labels`` at run time."""

    MAPPING = "kohonen_validator"

    def __init__(self, workflow, **kwargs):
        kwargs.setdefault("view_group", "EVALUATOR")
        super().__init__(workflow, **kwargs)
        self.result = None
        self.fitness = 0.0
        self.labels = None
        self.loader = None
        self.demand("total", "shape")

    def initialize(self, **kwargs):
        pass

    def run(self):
        tot = self.total
        tot = tot.devmem.detach().cpu().numpy() if getattr(
            tot, "devmem", None) is not None else numpy.asarray(
                getattr(tot, "mem", tot))
        labels = self.labels if self.loader is None else \
            self.loader.original_labels
        labels = numpy.asarray(labels).astype(numpy.int64).reshape(-1)
        NN = int(self.shape[0]) * int(self.shape[1])
        ok = (tot >= 0) & (tot < NN) & (labels[:len(tot)] >= 0)
        win, lab = tot[ok].astype(numpy.int64), labels[:len(tot)][ok]
        ncls = int(lab.max()) + 1 if lab.size else 1
        votes = numpy.zeros((NN, ncls), numpy.int64)
        numpy.add.at(votes, (win, lab), 1)
        res = votes.argmax(1).astype(numpy.int32)
        res[votes.sum(1) == 0] = -1
        self.result = res
        self.fitness = float((res[win] == lab).mean()) if lab.size else 0.0

    def get_metric_names(self):
        return {"kohonen_fitness"}

    def get_metric_values(self):
        return {"kohonen_fitness": self.fitness}


class KohonenWorkflow(AcceleratedWorkflow):
    """repeater -> loader -> trainer -> forward -> decision -> [snapshotter,
    plotters] -> repeater / end point, gated as StandardWorkflow's loop.
    kwargs: ``loader_name``, ``loader_config``, ``trainer_config``,
    ``forward_config``, ``decision_config``, ``snapshotter_config`` (None:
    no snapshots), ``plotters`` (the three Kohonen plotters at epoch ends).

    The loop runs eager: no HIP-graph segments are attached, the per-step
    scalars (gradient, sigma, valid rows) are kernel arguments.  Training
    over a data-parallel group of more than one rank is not supported."""

    def __init__(self, workflow, **kwargs):
        super().__init__(workflow, **kwargs)
        self.loader_name = kwargs.get("loader_name")
        self.loader_config = dict(kwargs.get("loader_config") or {})
        self.trainer_config = dict(kwargs.get("trainer_config") or {})
        self.forward_config = dict(kwargs.get("forward_config") or {})
        self.decision_config = dict(kwargs.get("decision_config") or {})
        self.snapshotter_config = kwargs.get("snapshotter_config")
        self.with_plotters = bool(kwargs.get("plotters", False))
        self.snapshotter = None
        self.plotters = []
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

        self.trainer = tr = KohonenTrainer(self, **self.trainer_config)
        tr.link_from(ld)
        tr.link_attrs(ld, ("input", "minibatch_data"), "minibatch_size",
                      "minibatch_class")

        self.forward = fw = KohonenForward(self, **self.forward_config)
        fw.link_from(tr)
        fw.link_attrs(ld, ("input", "minibatch_data"), "minibatch_size",
                      "minibatch_indices", "total_samples")
        fw.link_attrs(tr, "weights", "argmins")

        self.decision = dc = KohonenDecision(self, **self.decision_config)
        dc.link_from(fw)
        dc.link_attrs(ld, "minibatch_class", "last_minibatch",
                      "class_lengths", "epoch_ended", "minibatch_size")
        dc.link_attrs(ld, "epoch_number", two_way=True)
        dc.link_attrs(tr, "winners", "qerr")
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

        if self.with_plotters:
            from veles_amd.plotting_units import (
                KohonenHits, KohonenInputMaps, KohonenNeighborMap)
            hits = KohonenHits(self, name="kohonen hits",
                               shape=tr.shape)
            hits.link_attrs(dc, ("input", "last_winners"))
            umat = KohonenNeighborMap(self, name="kohonen neighbor map",
                                      shape=tr.shape)
            umat.link_attrs(tr, ("input", "weights"))
            maps = KohonenInputMaps(self, name="kohonen input maps",
                                    shape=tr.shape)
            maps.link_attrs(tr, ("input", "weights"))
            for p in (hits, umat, maps):
                p.gate_skip = ~dc.epoch_ended_flag
                p.link_from(last)
                last = p
                self.plotters.append(p)

        self.repeater.link_from(last)
        self.repeater.gate_block = dc.complete | dc.steps_complete
        self.end_point.link_from(last)
        self.end_point.gate_block = ~dc.complete

    def initialize(self, **kwargs):
        from veles_amd.parallel import find_dp
        dp = find_dp(self)
        if dp is not None and dp.world_size > 1:
            raise NotImplementedError(
                "KohonenWorkflow trains on one rank: the data-parallel group "
                "has %d (multi-rank Kohonen training is not implemented)" %
                dp.world_size)
        return super().initialize(**kwargs)
