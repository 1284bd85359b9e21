"""Recurrent layers: LSTM and plain tanh RNN (docs/OPS.md "Recurrent layers").

The Znicz recurrent units are absent from the reference snapshot, so the
semantics are this project's own, pinned to torch.nn.LSTM / torch.nn.RNN
(parity unpinned): gate order i, f, g, o, plain sigmoid / tanh,

    c_t = f c_{t-1} + i g,  h_t = o tanh(c_t)        (LSTM)
    h_t = tanh(x_t.Wx^T + b + h_{t-1}.Wh^T)          (RNN)

h and c start at zero at every minibatch.  Input samples are (T, I); the
output is h_T (H,) or, with ``return_sequences``, every h_t (T, H).  The one
``weights`` parameter is [NG*H][I+H] = [Wx | Wh] (NG = 4 / 1), the one
``bias`` [NG*H]; weights and bias are filled uniformly with fan-in I + H,
the forget-gate bias is 1.  The forward is one GEMM for the input projection
plus T fused step kernels (``ops.lstm_fwd``), the backward T step kernels
plus three GEMMs (``ops.lstm_bwd``).

GRU (pinned to torch.nn.GRU, parity unpinned): gate order r, z, n,

    r, z = sigmoid(x_t.Wx^T + b + h_{t-1}.Wh^T)
    hn = h_{t-1}.Whn^T + b_hn,  n = tanh(x_t.Wxn^T + b_n + r hn)
    h_t = (1 - z) n + z h_{t-1}

``weights`` [3H][I+H], ``bias`` [4H] = (b_r, b_z, b_n, b_hn), all filled
uniformly with fan-in I + H; no forget bias (``ops.gru_fwd`` / ``gru_bwd``).

``bidirectional`` (D = 2 directions) adds a reverse chain h^r_t =
cell(x_t, h^r_{t+1}) with parameters of its own: ``weights``
[D*NG*H][I+H] and ``bias`` are direction-major, each block the one-direction
layout; the output is (T, 2H) = [h^f_t | h^r_t] or (2H,) =
[h^f_{T-1} | h^r_0] (torch's ``output`` / ``h_n``).  ``reverse`` runs the
reverse chain alone (docs/OPS.md "Bidirectional").
"""
from __future__ import annotations

import numpy

from veles_amd.models.nn_units import (
    Forward, GradientDescentBase, fill_weights)
from veles_amd import ops

__all__ = ["LSTM", "RNN", "GRU", "GDLSTM", "GDRNN", "GDGRU"]


class LSTM(Forward):
    __id__ = "7d0f1c5e-3b7a-4a57-9c1d-2f8e6a4b9d31"
    MAPPING = "lstm"
    CELL = "lstm"
    GATES = 4
    BIAS_BLOCKS = 4   # bias length in units of H

    def __init__(self, workflow, **kwargs):
        super().__init__(workflow, **kwargs)
        oss = kwargs.get("output_sample_shape", kwargs.get("output_shape", 10))
        if not isinstance(oss, int):
            oss = tuple(oss)
            if len(oss) != 1:
                raise ValueError("%s: output_sample_shape must be H, got %s"
                                 % (self.name, oss))
            oss = oss[0]
        self.hidden = int(oss)
        self.return_sequences = bool(kwargs.get("return_sequences", False))
        self.forget_bias = float(kwargs.get("forget_bias", 1.0))
        self.bidirectional = bool(kwargs.get("bidirectional", False))
        self.reverse = bool(kwargs.get("reverse", False))
        if self.bidirectional and self.reverse:
            raise ValueError("%s: bidirectional and reverse exclude each "
                             "other" % self.name)
        if self.weights_transposed:
            raise ValueError("%s: weights_transposed is not supported" %
                             self.name)

    def init_unpickled(self):
        super().init_unpickled()
        self.save_ = {}

    @property
    def direction(self):
        """the ops' ``direction``; a layer pickled before the attributes
        existed runs forward-only"""
        if getattr(self, "bidirectional", False):
            return "both"
        return "reverse" if getattr(self, "reverse", False) else "forward"

    @property
    def directions(self):
        return 2 if self.direction == "both" else 1

    @property
    def neurons_number(self):
        return self.directions * self.hidden

    @property
    def output_sample_shape(self):
        width = self.directions * self.hidden
        return (self.steps, width) if self.return_sequences else (width,)

    def initialize(self, device=None, **kwargs):
        super().initialize(device=device, **kwargs)
        shape = tuple(self.input.shape)
        if len(shape) != 3:
            raise ValueError("%s: input samples must be (T, I), got %s" %
                             (self.name, shape[1:]))
        B, self.steps, n_in = shape
        H, ng, D = self.hidden, self.GATES, self.directions
        fan_in = n_in + H
        wshape = (D * ng * H, fan_in)
        # created here, weights before bias as register_params would, so that
        # the forget gate's bias can start at forget_bias
        std = 1.0 / numpy.sqrt(fan_in)
        if self.weights.mem is None or self.weights.mem.shape != wshape:
            w = numpy.zeros(wshape, numpy.float32)
            fill_weights(w, self.weights_filling,
                         std if self.weights_stddev is None
                         else self.weights_stddev, self.rand)
            self.weights.reset(w)
        nb = D * self.BIAS_BLOCKS * H
        if self.include_bias and (self.bias.mem is None or
                                  self.bias.mem.shape != (nb,)):
            b = numpy.zeros(nb, numpy.float32)
            fill_weights(b, self.bias_filling,
                         std if self.bias_stddev is None
                         else self.bias_stddev, self.rand)
            if ng == 4:
                for d in range(D):
                    b[(4 * d + 1) * H:(4 * d + 2) * H] = self.forget_bias
            self.bias.reset(b)
        self.register_params(wshape, fan_in, bias_len=nb)
        self.save_ = {}
        y = self.alloc_output((B,) + self.output_sample_shape)
        if self.return_sequences:
            self.save_["h"] = y   # the output is the kernels' h buffer

    def run(self):
        x = self.input.devmem
        w = self.weights_lp
        if x.dtype != w.dtype:
            x = x.to(w.dtype)
        B = x.shape[0]
        seq = self.return_sequences
        testing = bool(getattr(self.workflow, "testing", False))
        out = None if seq else self.alloc_output(
            (B, self.directions * self.hidden))
        y = self.forward_op(x, w, return_sequences=seq,
                            save=None if testing else self.save_,
                            ws=self.save_, out=out)
        if seq:
            self.output.devmem = y

    def forward_op(self, x, w, **kwargs):
        return ops.lstm_fwd(x, w, self.bias_master, self.hidden,
                            cell=self.CELL, direction=self.direction,
                            **kwargs)


class RNN(LSTM):
    __id__ = "e4a2b8c6-91d3-4f0e-8b75-6c3d1a9f2e48"
    MAPPING = "rnn"
    CELL = "rnn"
    GATES = 1
    BIAS_BLOCKS = 1


class GRU(LSTM):
    __id__ = "3c9e5b2a-6f14-4d8b-a7e0-8b1d4f6c2a95"
    MAPPING = "gru"
    CELL = "gru"
    GATES = 3
    BIAS_BLOCKS = 4   # (b_r, b_z, b_n, b_hn)

    def forward_op(self, x, w, **kwargs):
        return ops.gru_fwd(x, w, self.bias_master, self.hidden,
                           direction=self.direction, **kwargs)


class GDLSTM(GradientDescentBase):
    MAPPING = "lstm"
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
        width = fwd.directions * fwd.hidden
        err = err.reshape((B, T, width) if fwd.return_sequences
                          else (B, width))
        pw, pb = fwd._pw_, fwd._pb_
        # the step's only contribution: write, not read-modify-write
        mode = "overwrite" if self.store_.overwrite else True
        ei = self.alloc_err_input(x.shape, w.dtype) \
            if self.need_err_input else None
        self.backward_op(err, x, w, fwd, pw.grad,
                         None if pb is None else pb.grad, mode, ei)
        self.report_gradients()

    def backward_op(self, err, x, w, fwd, dw, dbias, mode, ei):
        ops.lstm_bwd(err, x, w, fwd.save_, dw, dbias, cell=fwd.CELL,
                     accumulate=mode, need_err_input=self.need_err_input,
                     err_input=ei, direction=fwd.direction)


class GDRNN(GDLSTM):
    MAPPING = "rnn"


class GDGRU(GDLSTM):
    MAPPING = "gru"

    def backward_op(self, err, x, w, fwd, dw, dbias, mode, ei):
        ops.gru_bwd(err, x, w, fwd.save_, dw, dbias, accumulate=mode,
                    need_err_input=self.need_err_input, err_input=ei,
                    direction=fwd.direction)
