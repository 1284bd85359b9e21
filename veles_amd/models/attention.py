"""Multi-head scaled dot-product self-attention (``attention`` layer type;
docs/OPS.md "Attention").  Znicz has no such layer, so the semantics are this
project's own, pinned to ``torch.nn.MultiheadAttention(E, NH, bias=True,
dropout=p, batch_first=True)`` applied to (x, x, x), with a causal
``attn_mask`` when ``causal`` is set (parity unpinned); p = ``dropout``
(default 0) drops attention weights on TRAIN minibatches with this project's
counter-based mask, not torch's generator.

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

Dropout: o = (P o M / (1 - p)) v inside the fused kernels (P never exists in
memory, so no ``dropout`` layer can reach it).  As for ``DropoutForward`` the
seed lives on the device and is advanced once per forward (a captured step
draws a fresh mask every replay), a snapshot resumes the mask stream exactly,
and rank r of a data-parallel run draws the rows of samples r B .. r B + B - 1
of the global minibatch.  Identity when the workflow is testing and on
non-TRAIN minibatches.

Grouped-query heads: ``kv_heads`` = KVH (default ``heads``; it must divide
``heads``; 1 is multi-query attention) projects KVH key / value heads, and
query head h reads K/V head h // (NH / KVH).  W_in is then [E + 2 KVH D][I],
rows q (E), k (KVH D), v (KVH D), ``weights`` has (E + 2 KVH D) I + E E
values and ``bias`` is [E + 2 KVH D + E]; fan-ins and fills are unchanged.
"""
from __future__ import annotations

import numpy

from veles_amd.models.nn_units import (
    Forward, GradientDescentBase, fill_weights)
from veles_amd.prng import device_seed
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
        kvh = kwargs.get("kv_heads")
        self.kv_heads = self.heads if kvh is None else int(kvh)
        self.causal = bool(kwargs.get("causal", False))
        self.dropout = float(kwargs.get("dropout", 0.0))
        if not 0.0 <= self.dropout < 1.0:
            raise ValueError("%s: dropout must be in [0, 1), got %s" %
                             (self.name, self.dropout))
        self.seed = 0
        self.seed_dev_saved = None
        if self.weights_transposed:
            raise ValueError("%s: weights_transposed is not supported" %
                             self.name)

    def init_unpickled(self):
        super().init_unpickled()
        self.save_ = {}
        self.seed_dev_ = None
        self.drop_ = {}

    def __getstate__(self):
        device_seed.save(self)   # exact resume of the device mask stream
        return super().__getstate__()

    def _draw_seed(self):
        self.seed = int(self.rand.randint(0, 2 ** 31 - 1))
        return self.seed

    def drop_args(self, x, testing):
        """The dropout arguments of this minibatch's ``ops.mha_fwd`` and
        ``ops.mha_bwd``: none unless training on a TRAIN minibatch (the rule
        of ``DropoutForward.run``).  Draws or advances the seed."""
        mc = getattr(self, "minibatch_class", None)
        if testing or self.dropout <= 0 or (mc is not None and mc != 2):
            return {}
        ld = getattr(self.workflow, "loader", None)
        rank = int(getattr(ld, "rank", 0) or 0) if ld is not None else 0
        kw = {"dropout": self.dropout, "base_row": rank * x.shape[0]}
        if x.is_cuda:
            sd = device_seed.get(self, x.device, self._draw_seed)
            ops.seed_advance(sd)
            kw["seed_dev"] = sd
        else:
            kw["seed"] = self._draw_seed()
        return kw

    @property
    def neurons_number(self):
        return self.width

    @property
    def output_sample_shape(self):
        return (self.steps, self.width)

    @property
    def qkv_width(self):
        """rows of W_in: E + 2 KVH D (3E without ``kv_heads``)"""
        return self.width + 2 * self.kv_heads * (self.width // self.heads)

    def split(self, flat, n_in):
        """(W_in [E + 2 KVH D][I], W_o [E][E]) views of a flat weights-like
        tensor"""
        E, W = self.width, self.qkv_width
        n = W * n_in
        return flat[:n].view(W, n_in), flat[n:].view(E, E)

    def initialize(self, device=None, **kwargs):
        super().initialize(device=device, **kwargs)
        shape = tuple(self.input.shape)
        if len(shape) != 3:
            raise ValueError("%s: input samples must be (T, I), got %s" %
                             (self.name, shape[1:]))
        B, self.steps, n_in = shape
        E = self.width
        ops.attn_head_dim(E, self.heads, self.name)
        ops.attn_kv_heads(self.heads, self.kv_heads, self.name)
        self.n_in = n_in
        W = self.qkv_width
        n = W * n_in
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
                                  self.bias.mem.shape != (W + E,)):
            self.bias.reset(numpy.zeros(W + E, numpy.float32))
        self.register_params(wshape, n_in, bias_len=W + E)
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
        self.drop_ = self.drop_args(x, testing)
        ops.mha_fwd(x, w_in, w_out, self.bias_master, self.heads,
                    causal=self.causal, save=None if testing else self.save_,
                    ws=self.save_, out=y, kv_heads=self.kv_heads,
                    **self.drop_)


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
                    aux=aux, aux_act=aux_act, kv_heads=fwd.kv_heads,
                    **fwd.drop_)
        self.report_gradients()
