"""Position-wise feed-forward layer (``ffn`` layer type; docs/OPS.md
"Position-wise feed-forward").  Znicz has no such layer, so the semantics are
this project's own, pinned to float64 ``torch.nn.Sequential(Linear(I, F),
GELU(), Linear(F, E))``: the ``linear1`` / ``linear2`` of
``TransformerEncoderLayer``.

The last axis of the input has the I features, every other axis is a row
((T, I) samples of a sequence, or (I,)):

    u = x W1^T + b1        W1 [F][I]
    h = a(u)               "gelu" (default), "gelu_tanh" or "str"
    y = h W2^T + b2        W2 [E][F]

E = ``output_sample_shape`` (default I), F = ``hidden`` (default 4 E).  The
one ``weights`` parameter is 1-D, W1 then W2 (F*I + E*F values), the one
``bias`` is [F + E] = (b1, b2): both live in the flat parameter store, so
the solvers, the LR adjuster, snapshots and the data-parallel all-reduce
apply unchanged.  W1 is filled uniformly with fan-in I, W2 with fan-in F; the
biases start at 0.

GELU's derivative needs the pre-activation, which the ``all2all_*`` /
``aux_act`` plumbing (derivatives of the layer's OUTPUT) cannot express: the
layer keeps u and h itself (``ops.ffn_fwd`` / ``ops.ffn_bwd``).  Its own
output is linear, so nothing is fused into the layer above; the derivative of
the layer below rides the err_input GEMM (``GDFeedForward`` is in
``_FUSABLE``).
"""
from __future__ import annotations

import numpy

from veles_amd.models.nn_units import (
    Forward, GradientDescentBase, _compute_dtype, fill_weights)
from veles_amd import ops

__all__ = ["FeedForward", "GDFeedForward"]


class FeedForward(Forward):
    __id__ = "3f9a6c2e-71d4-4b8a-a5e3-0c2d9f4b7e61"
    MAPPING = "ffn"

    def __init__(self, workflow, **kwargs):
        super().__init__(workflow, **kwargs)
        oss = kwargs.get("output_sample_shape", kwargs.get("output_shape"))
        if oss is not None and not isinstance(oss, int):
            oss = tuple(oss)
            if len(oss) != 1:
                raise ValueError("%s: output_sample_shape must be E, got %s"
                                 % (self.name, oss))
            oss = oss[0]
        self.width = None if oss is None else int(oss)
        hidden = kwargs.get("hidden", None)
        self.hidden = None if hidden is None else int(hidden)
        for what, v in (("output_sample_shape", self.width),
                        ("hidden", self.hidden)):
            if v is not None and v < 1:
                raise ValueError("%s: %s must be positive, got %d" %
                                 (self.name, what, v))
        self.act = kwargs.get("activation", "gelu")
        ops.ffn_act_code(self.act)
        if self.weights_transposed:
            raise ValueError("%s: weights_transposed is not supported" %
                             self.name)

    def init_unpickled(self):
        super().init_unpickled()
        self.save_ = {}
        self.x_ = None

    @property
    def neurons_number(self):
        return self.width

    def split(self, flat):
        """(W1 [F][I], W2 [E][F]) views of a flat weights-like tensor"""
        n = self.hidden * self.n_in
        return (flat[:n].view(self.hidden, self.n_in),
                flat[n:].view(self.width, self.hidden))

    def initialize(self, device=None, **kwargs):
        super().initialize(device=device, **kwargs)
        shape = tuple(self.input.shape)
        if len(shape) < 2:
            raise ValueError("%s: input samples must have a feature axis, "
                             "got %s" % (self.name, shape))
        n_in = int(shape[-1])
        if self.width is None:
            self.width = n_in
        if self.hidden is None:
            self.hidden = 4 * self.width
        self.n_in = n_in
        E, Fh = self.width, self.hidden
        n = Fh * n_in
        wshape = (n + E * Fh,)
        # created here, weights before bias as register_params would: the
        # two blocks have a fan-in each, and the biases start at 0
        if self.weights.mem is None or self.weights.mem.shape != wshape:
            w = numpy.zeros(wshape, numpy.float32)
            for part, fan_in in ((w[:n], n_in), (w[n:], Fh)):
                fill_weights(part, self.weights_filling,
                             1.0 / numpy.sqrt(fan_in)
                             if self.weights_stddev is None
                             else self.weights_stddev, self.rand)
            self.weights.reset(w)
        if self.include_bias and (self.bias.mem is None or
                                  self.bias.mem.shape != (Fh + E,)):
            self.bias.reset(numpy.zeros(Fh + E, numpy.float32))
        self.register_params(wshape, n_in, bias_len=Fh + E)
        self.save_ = {}
        x = self.input.devmem
        self.alloc_output(shape[:-1] + (E,), _compute_dtype(x)
                          if x is not None else None)

    @property
    def output_sample_shape(self):
        return tuple(self.input.shape)[1:-1] + (self.width,)

    def run(self):
        x = self.input.devmem
        w = self.weights_lp
        if x.dtype != w.dtype:
            x = x.to(w.dtype)
        if not x.is_contiguous():
            x = x.contiguous()
        self.x_ = x
        w1, w2 = self.split(w)
        testing = bool(getattr(self.workflow, "testing", False))
        y = self.alloc_output(tuple(x.shape[:-1]) + (self.width,), w.dtype)
        ops.ffn_fwd(x, w1, w2, self.bias_master, self.act,
                    save=None if testing else self.save_, ws=self.save_,
                    out=y)

    def package_export(self):
        d = super().package_export()
        d.update(hidden=self.hidden, activation=self.act)
        return d


class GDFeedForward(GradientDescentBase):
    MAPPING = "ffn"
    OVERWRITES_GRADS = True  # see ParameterStore.overwrite

    def initialize(self, device=None, **kwargs):
        super().initialize(device=device, **kwargs)
        fwd = self.forward
        if fwd is None:
            raise AttributeError("%s: forward_unit is not set" % self)
        self.attach_params(fwd)

    def run(self):
        fwd = self.forward
        fwd.ensure_params()
        w = fwd.weights_lp
        x = fwd.x_
        err = self.err_output.devmem
        if err.dtype != w.dtype:
            err = err.to(w.dtype)
        err = err.reshape(tuple(x.shape[:-1]) + (fwd.width,))
        if not err.is_contiguous():
            err = err.contiguous()
        pw, pb = fwd._pw_, fwd._pb_
        w1, w2 = fwd.split(w)
        dw1, dw2 = fwd.split(pw.grad)
        # the step's only contribution: write, not read-modify-write
        mode = "overwrite" if self.store_.overwrite else True
        aux, aux_act = self.aux_tensor()
        ei = self.alloc_err_input(x.shape, w.dtype) \
            if self.need_err_input else None
        ops.ffn_bwd(err, x, w1, w2, fwd.save_, dw1, dw2,
                    None if pb is None else pb.grad, fwd.act,
                    accumulate=mode, need_err_input=self.need_err_input,
                    err_input=ei, aux=aux, aux_act=aux_act)
        self.report_gradients()
