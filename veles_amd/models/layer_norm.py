"""Layer normalisation (``layer_norm`` layer type; docs/OPS.md §Layer
normalisation and residual connections).  This project's semantics, pinned
to ``torch.nn.LayerNorm(C, eps=1e-5, elementwise_affine=True)``: the last
axis of the input has the C features, every other axis is a row, and every
row is normalised with its own mean and biased variance, in training and in
evaluation alike: there are no running statistics and no train / evaluate
switch.

``residual="<name of an earlier skip layer>"`` makes the layer "add & norm":
y = LayerNorm(x + skip tensor).  The sum is taken in float32 inside the
kernel and is not stored; the backward adds the two again.  The gradient of
the skip branch is this layer's err_input itself (``GDSkip`` adds it to its
own err_output), not a copy.

gamma is ``weights`` [C] (constant 1), beta is ``bias`` (constant 0): both
live in the flat parameter store like any layer's, so the solvers, the LR
adjuster, snapshots and the data-parallel all-reduce apply unchanged; the
kernels read the float32 masters.

There are no activation variants, and the derivative of the layer below is
never fused into this layer's err_input (``GDLayerNorm`` is not in
``_FUSABLE``): with a residual that tensor doubles as the skip gradient.

float8 workflows: the layer takes and produces bf16, as ``batch_norm``.
"""
from __future__ import annotations

from veles_amd.models.nn_units import (
    Forward, GradientDescentBase, _compute_dtype)
from veles_amd import ops

__all__ = ["LayerNorm", "GDLayerNorm"]


class LayerNorm(Forward):
    MAPPING = "layer_norm"

    def __init__(self, workflow, **kwargs):
        kwargs.setdefault("weights_filling", "constant")
        kwargs.setdefault("weights_stddev", 1.0)
        kwargs.setdefault("bias_filling", "constant")
        kwargs.setdefault("bias_stddev", 0.0)
        super().__init__(workflow, **kwargs)
        self.eps = float(kwargs.get("eps", 1e-5))
        self.residual = kwargs.get("residual", None)
        self.skip_unit = None      # set by StandardWorkflow.link_forwards

    def init_unpickled(self):
        super().init_unpickled()
        self.x_ = self.r_ = None
        self.save_ = {}

    def initialize(self, device=None, **kwargs):
        super().initialize(device=device, **kwargs)
        if not self.include_bias:
            raise ValueError("%s: layer normalisation has a bias (beta)" %
                             self.name)
        if self.residual is not None and self.skip_unit is None:
            raise ValueError("%s: residual=%r is not linked to a skip layer"
                             % (self.name, self.residual))
        shape = tuple(self.input.shape)
        if self.skip_unit is not None and \
                tuple(self.skip_unit.output.shape) != shape:
            raise ValueError(
                "%s: the skip tensor of %s is %s, the input is %s" % (
                    self.name, self.skip_unit.name,
                    tuple(self.skip_unit.output.shape), shape))
        C = int(shape[-1])
        self.register_params((C,), C)
        x = self.input.devmem
        self.alloc_output(shape, _compute_dtype(x) if x is not None
                          else None)

    def run(self):
        x = self.input.devmem
        want = _compute_dtype(x)
        if x.dtype != want:
            x = x.to(want)
        r = None
        if self.skip_unit is not None:
            r = self.skip_unit.output.devmem
            if r.dtype != want:
                r = r.to(want)
        self.x_, self.r_ = x, r
        self.ensure_params()
        y = self.alloc_output(tuple(x.shape), want)
        ops.layernorm_fwd(x, self.weights_master, self.bias_master,
                          residual=r, eps=self.eps, save=self.save_, out=y)

    def package_export(self):
        self.sync_params_to_host()
        return {"weights": self.weights.mem, "bias": self.bias.mem,
                "eps": self.eps, "residual": self.residual}


class GDLayerNorm(GradientDescentBase):
    MAPPING = "layer_norm"
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

    def skip_gradient(self):
        """ds: the gradient of the skip tensor (this unit's err_input)"""
        return self.err_input.devmem

    def run(self):
        fwd = self.forward
        fwd.ensure_params()
        x = fwd.x_
        err = self.err_output.devmem
        if err.dtype != x.dtype:
            err = err.to(x.dtype)
        if err.shape != x.shape:
            err = err.reshape(x.shape)
        ei = self.alloc_err_input(tuple(x.shape), x.dtype) \
            if self.need_err_input else None
        pw, pb = fwd._pw_, fwd._pb_
        ops.layernorm_bwd(
            err, x, fwd.weights_master, fwd.save_, pw.grad, pb.grad,
            residual=fwd.r_,
            accumulate="overwrite" if self.store_.overwrite else True,
            out=ei, ws=self.ws_, need_dx=self.need_err_input)
        self.report_gradients()
