"""Multi-head scaled dot-product self-attention (``attention`` layer type;
docs/OPS.md "Attention").  Znicz has no such layer, so the semantics are this
project's own, pinned to ``torch.nn.MultiheadAttention(E, NH, bias=True,
dropout=0, batch_first=True)`` applied to (x, x, x), with a causal
``attn_mask`` when ``causal`` is set (parity unpinned).

Input samples are (T, I), batch-major [B][T][I] as for the recurrent layers;
the output is (T, E) with E = ``output_sample_shape``, NH = ``heads`` and
D = E / NH in (32, 64, 128):

    qkv = x W_in^T + b_in       W_in [3E][I], rows q, k, v, head-major blocks
    S = q k^T / sqrt(D) per (batch, head); causal: key j visible iff j <= i
    o = softmax_j(S) v,  y = o W_o^T + b_o       W_o [E][E]

The one ``weights`` parameter is 1-D, W_in then W_o (3E*I + E*E values), the
one ``bias`` is [4E] = (b_q, b_k, b_v, b_o): with I = E they are torch's
``in_proj_weight`` / ``out_proj.weight`` and ``in_proj_bias`` /
``out_proj.bias`` back to back.  W_in is filled uniformly with fan-in I, W_o
with fan-in E; the biases start at 0.  The forward is two GEMMs around the
fused attention kernel (``ops.mha_fwd``), the backward five GEMMs around the
three backward kernels (``ops.mha_bwd``).
"""
from __future__ import annotations

import numpy

from veles_amd.models.nn_units import (
    Forward, GradientDescentBase, fill_weights)
from veles_amd import ops

__all__ = ["Attention", "GDAttention"]


class Attention(Forward):
    __id__ = "b8e4c1d7-52a9-4f3e-9d06-7a1c3e5f8b24"
    MAPPING = "attention"

    def __init__(self, workflow, **kwargs):
        super().__init__(workflow, **kwargs)
        oss = kwargs.get("output_sample_shape", kwargs.get("output_shape", 64))
        if not isinstance(oss, int):
            oss = tuple(oss)
            if len(oss) != 1:
                raise ValueError("%s: output_sample_shape must be E, got %s"
                                 % (self.name, oss))
            oss = oss[0]
        self.width = int(oss)
        self.heads = int(kwargs.get("heads", 1))
        self.causal = bool(kwargs.get("causal", False))
        if self.weights_transposed:
            raise ValueError("%s: weights_transposed is not supported" %
                             self.name)

    def init_unpickled(self):
        super().init_unpickled()
        self.save_ = {}

    @property
    def neurons_number(self):
        return self.width

    @property
    def output_sample_shape(self):
        return (self.steps, self.width)

    def split(self, flat, n_in):
        """(W_in [3E][I], W_o [E][E]) views of a flat weights-like tensor"""
        E = self.width
        n = 3 * E * n_in
        return flat[:n].view(3 * E, n_in), flat[n:].view(E, E)

    def initialize(self, device=None, **kwargs):
        super().initialize(device=device, **kwargs)
        shape = tuple(self.input.shape)
        if len(shape) != 3:
            raise ValueError("%s: input samples must be (T, I), got %s" %
                             (self.name, shape[1:]))
        B, self.steps, n_in = shape
        E = self.width
        ops.attn_head_dim(E, self.heads, self.name)
        self.n_in = n_in
        n = 3 * E * n_in
        wshape = (n + E * E,)
        # created here, weights before bias as register_params would: the
        # two blocks have a fan-in each, and the biases start at 0
        if self.weights.mem is None or self.weights.mem.shape != wshape:
            w = numpy.zeros(wshape, numpy.float32)
            for part, fan_in in ((w[:n], n_in), (w[n:], E)):
                fill_weights(part, self.weights_filling,
                             1.0 / numpy.sqrt(fan_in)
                             if self.weights_stddev is None
                             else self.weights_stddev, self.rand)
            self.weights.reset(w)
        if self.include_bias and (self.bias.mem is None or
                                  self.bias.mem.shape != (4 * E,)):
            self.bias.reset(numpy.zeros(4 * E, numpy.float32))
        self.register_params(wshape, n_in, bias_len=4 * E)
        self.save_ = {}
        self.alloc_output((B,) + self.output_sample_shape)

    def run(self):
        x = self.input.devmem
        w = self.weights_lp
        if x.dtype != w.dtype:
            x = x.to(w.dtype)
        w_in, w_out = self.split(w, self.n_in)
        testing = bool(getattr(self.workflow, "testing", False))
        y = self.alloc_output((x.shape[0],) + self.output_sample_shape,
                              w.dtype)
        ops.mha_fwd(x, w_in, w_out, self.bias_master, self.heads,
                    causal=self.causal, save=None if testing else self.save_,
                    ws=self.save_, out=y)


class GDAttention(GradientDescentBase):
    MAPPING = "attention"
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
        x = self.input.devmem
        if x.dtype != w.dtype:
            x = x.to(w.dtype)
        B, T = x.shape[0], x.shape[1]
        err = self.err_output.devmem
        if err.dtype != w.dtype:
            err = err.to(w.dtype)
        err = err.reshape(B, T, fwd.width)
        if not err.is_contiguous():
            err = err.contiguous()
        pw, pb = fwd._pw_, fwd._pb_
        w_in, w_out = fwd.split(w, fwd.n_in)
        dw_in, dw_out = fwd.split(pw.grad, fwd.n_in)
        # the step's only contribution: write, not read-modify-write
        mode = "overwrite" if self.store_.overwrite else True
        aux, aux_act = self.aux_tensor()
        ei = self.alloc_err_input(x.shape, w.dtype) \
            if self.need_err_input else None
        ops.mha_bwd(err, x, w_in, w_out, fwd.save_, dw_in, dw_out,
                    None if pb is None else pb.grad, fwd.heads,
                    causal=fwd.causal, accumulate=mode,
                    need_err_input=self.need_err_input, err_input=ei,
                    aux=aux, aux_act=aux_act)
        self.report_gradients()
