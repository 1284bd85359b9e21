"""Batch normalisation (``batch_norm*`` layer types; docs/OPS.md §Batch
normalisation).  This project's semantics, pinned to ``torch.nn.BatchNorm2d``
/ ``BatchNorm1d``: the last axis of the input is the channel axis, every
other axis is a row.

Training minibatches: y = act(gamma (x - mean) invstd + beta) with the rows'
mean and biased variance, and the running statistics move by ``momentum``
towards the mean and the unbiased variance.  Validation / test minibatches,
``forward_mode`` and a ``testing`` workflow normalise with the running
statistics and leave them alone (the rule of ``DropoutForward.run``).

gamma is ``weights`` [C] (constant 1), beta is ``bias`` (constant 0): both
live in the flat parameter store like any layer's, so the solvers, the LR
adjuster and the data-parallel all-reduce apply unchanged; the kernels read
the float32 masters.  The running statistics are float32 device tensors that
only the kernels write, so a captured step replays them; they are read back
into the pickled ``running_mean`` / ``running_var`` for a snapshot.

Data parallel: every rank normalises with the statistics of its own shard
(plain batch normalisation, not SyncBN) and keeps its own running
statistics; dgamma / dbeta are all-reduced with the other gradients.

float8 workflows: the layer takes and produces bf16; an fp8 consumer above
it quantises its input itself.
"""
from __future__ import annotations

import numpy

from veles_amd.memory import Array
from veles_amd.models.nn_units import (
    Forward, GradientDescentBase, _sync_device)
from veles_amd import ops

__all__ = ["BatchNorm", "BatchNormTanh", "BatchNormRELU",
           "BatchNormStrictRELU", "BatchNormSigmoid", "GDBatchNorm",
           "GDBatchNormTanh", "GDBatchNormRELU", "GDBatchNormStrictRELU",
           "GDBatchNormSigmoid"]


class BatchNorm(Forward):
    MAPPING = "batch_norm"
    ACTIVATION = 0

    def __init__(self, workflow, **kwargs):
        kwargs.setdefault("weights_filling", "constant")
        kwargs.setdefault("weights_stddev", 1.0)
        kwargs.setdefault("bias_filling", "constant")
        kwargs.setdefault("bias_stddev", 0.0)
        super().__init__(workflow, **kwargs)
        self.eps = float(kwargs.get("eps", 1e-5))
        self.momentum = float(kwargs.get("momentum", 0.1))
        self.running_mean = Array()
        self.running_var = Array()
        self.forward_mode = False

    def init_unpickled(self):
        super().init_unpickled()
        self.rm_ = self.rv_ = self.x_ = None
        self.save_ = {}
        self.ws_ = {}
        self.trained_ = False

    def initialize(self, device=None, **kwargs):
        super().initialize(device=device, **kwargs)
        if not self.include_bias:
            raise ValueError("%s: batch normalisation has a bias (beta)" %
                             self.name)
        C = int(self.input.shape[-1])
        self.register_params((C,), C)
        for arr, v in ((self.running_mean, 0.0), (self.running_var, 1.0)):
            if arr.mem is None or arr.mem.shape != (C,):
                arr.reset(numpy.full(C, v, numpy.float32))
        self.rm_ = self.rv_ = None
        x = self.input.devmem
        self.alloc_output(tuple(self.input.shape),
                          x.dtype if x is not None else None)

    def running_stats(self):
        """The float32 [C] device tensors (running_mean, running_var)"""
        import torch
        if self.rm_ is None or self.rm_.device != self.torch_device:
            self.rm_, self.rv_ = (
                torch.from_numpy(numpy.array(a.mem, numpy.float32)).to(
                    self.torch_device)
                for a in (self.running_mean, self.running_var))
        return self.rm_, self.rv_

    def sync_running_to_host(self):
        if self.rm_ is None:
            return
        _sync_device(self.rm_)
        self.running_mean.reset(self.rm_.detach().cpu().numpy().copy())
        self.running_var.reset(self.rv_.detach().cpu().numpy().copy())

    def __getstate__(self):
        self.sync_running_to_host()
        return super().__getstate__()

    def training(self):
        """The rule of DropoutForward.run"""
        train = not self.forward_mode and not bool(
            getattr(self.workflow, "testing", False))
        mc = getattr(self, "minibatch_class", None)
        if mc is not None and mc != 2:
            train = False
        return train

    def run(self):
        import torch
        x = self.input.devmem
        want = torch.bfloat16 if x.is_cuda else torch.float32
        if x.dtype != want:
            x = x.to(want)
        self.x_ = x
        self.ensure_params()
        rm, rv = self.running_stats()
        y = self.alloc_output(tuple(x.shape), want)
        self.trained_ = self.training()
        ops.batchnorm_fwd(x, self.weights_master, self.bias_master, rm, rv,
                          training=self.trained_, eps=self.eps,
                          momentum=self.momentum, act=self.activation,
                          save=self.save_, out=y, ws=self.ws_)

    def package_export(self):
        self.sync_params_to_host()
        self.sync_running_to_host()
        return {"weights": self.weights.mem, "bias": self.bias.mem,
                "running_mean": self.running_mean.mem,
                "running_var": self.running_var.mem, "eps": self.eps,
                "activation_mode": self.activation_mode}


class BatchNormTanh(BatchNorm):
    MAPPING = "batch_norm_tanh"
    ACTIVATION = 1


class BatchNormRELU(BatchNorm):
    MAPPING = "batch_norm_relu"
    ACTIVATION = 2


class BatchNormStrictRELU(BatchNorm):
    MAPPING = "batch_norm_str"
    ACTIVATION = 3


class BatchNormSigmoid(BatchNorm):
    MAPPING = "batch_norm_sigmoid"
    ACTIVATION = 4


class GDBatchNorm(GradientDescentBase):
    MAPPING = "batch_norm"
    OVERWRITES_GRADS = True  # see ParameterStore.overwrite

    def initialize(self, device=None, **kwargs):
        super().initialize(device=device, **kwargs)
        fwd = self.forward
        if fwd is None:
            raise AttributeError("%s: forward_unit is not set" % self)
        self.attach_params(fwd)

    def init_unpickled(self):
        super().init_unpickled()
        self.ws_ = {}

    def run(self):
        fwd = self.forward
        fwd.ensure_params()
        if not fwd.trained_:
            raise RuntimeError("%s: the forward pass of this minibatch used "
                               "the running statistics" % self.name)
        x = fwd.x_
        err = self.err_output.devmem
        if err.dtype != x.dtype:
            err = err.to(x.dtype)
        if err.shape != x.shape:
            err = err.reshape(x.shape)
        act = fwd.activation if self.own_derivative else 0
        aux, aux_act = self.aux_tensor()
        if aux is not None and aux.shape != x.shape:
            aux = aux.reshape(x.shape)
        ei = self.alloc_err_input(tuple(x.shape), x.dtype) \
            if self.need_err_input else None
        pw, pb = fwd._pw_, fwd._pb_
        ops.batchnorm_bwd(
            err, x, fwd.output.devmem if act else None, fwd.weights_master,
            fwd.save_, pw.grad, pb.grad, act=act,
            accumulate="overwrite" if self.store_.overwrite else True,
            aux=aux, aux_act=aux_act, out=ei, ws=self.ws_,
            need_dx=self.need_err_input)
        self.report_gradients()


class GDBatchNormTanh(GDBatchNorm):
    MAPPING = "batch_norm_tanh"


class GDBatchNormRELU(GDBatchNorm):
    MAPPING = "batch_norm_relu"


class GDBatchNormStrictRELU(GDBatchNorm):
    MAPPING = "batch_norm_str"


class GDBatchNormSigmoid(GDBatchNorm):
    MAPPING = "batch_norm_sigmoid"
