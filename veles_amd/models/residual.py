"""Residual connections in a ``layers`` list (docs/OPS.md §Layer
normalisation and residual connections).

``skip`` marks a tensor: its forward is the identity without a copy
(``output`` is the input's tensor), and later layers add that tensor back:
``residual`` (y = x + skip tensor, the pre-LN form ``skip, layer_norm,
attention, residual``) or ``layer_norm`` with ``residual="<name>"`` ("add &
norm").  Both name the skip layer with the kwarg ``residual``.

Backward: the unit chain stays linear (so a step still captures in a HIP
graph); the skip branch's gradient does not travel along a second chain but
is picked up by ``GDSkip``, which runs after every consumer's GD unit:
err_input = err_output + the sum of each consumer's skip gradient, in layer
order, with ``ops.add``.  ``GDResidual`` passes err_output on as err_input
without a copy, and that same tensor is its skip gradient.  The derivative
of the layer below is never fused into any of these tensors (the units are
not in ``_FUSABLE``): they are shared with the skip branch.
"""
from __future__ import annotations

from veles_amd.accelerated_units import AcceleratedUnit
from veles_amd.memory import Array
from veles_amd.models.nn_units import GradientDescentBase, _compute_dtype
from veles_amd import ops

__all__ = ["Skip", "GDSkip", "Residual", "GDResidual"]


def _compute(t):
    want = _compute_dtype(t)
    return t if t.dtype == want else t.to(want)


class _Passive(AcceleratedUnit):
    """A forward unit without parameters"""
    hide_from_registry = True

    def __init__(self, workflow, **kwargs):
        kwargs.setdefault("view_group", "WORKER")
        super().__init__(workflow, **kwargs)
        self.output = Array(shallow_pickle=True)
        self.demand("input")

    @property
    def activation(self):
        return 0


class Skip(_Passive):
    MAPPING = "skip"

    def __init__(self, workflow, **kwargs):
        super().__init__(workflow, **kwargs)
        self.consumers = []        # forward units that add this tensor back

    def initialize(self, device=None, **kwargs):
        super().initialize(device=device, **kwargs)
        import torch
        x = self.input.devmem
        self.output.devmem = x if x is not None else torch.zeros(
            tuple(self.input.shape), dtype=self.compute_dtype,
            device=self.torch_device)

    def run(self):
        self.output.devmem = self.input.devmem

    def package_export(self):
        return {}


class GDSkip(GradientDescentBase):
    MAPPING = "skip"

    def __init__(self, workflow, **kwargs):
        super().__init__(workflow, **kwargs)
        self.consumer_gds = []     # set by StandardWorkflow.link_gds

    def run(self):
        if not self.need_err_input:
            return
        err = _compute(self.err_output.devmem)
        shape = tuple(self.input.shape)
        if tuple(err.shape) != shape:
            err = err.reshape(shape)
        ei = self.alloc_err_input(shape, err.dtype)
        acc = err
        for gd in self.consumer_gds:
            ds = _compute(gd.skip_gradient())
            if tuple(ds.shape) != shape:
                ds = ds.reshape(shape)
            ops.add(acc, ds, out=ei)
            acc = ei


class Residual(_Passive):
    MAPPING = "residual"

    def __init__(self, workflow, **kwargs):
        super().__init__(workflow, **kwargs)
        self.residual = kwargs.get("residual", None)
        self.skip_unit = None      # set by StandardWorkflow.link_forwards

    def initialize(self, device=None, **kwargs):
        super().initialize(device=device, **kwargs)
        import torch
        if self.skip_unit is None:
            raise ValueError("%s: residual=%r is not linked to a skip layer"
                             % (self.name, self.residual))
        shape = tuple(self.input.shape)
        if tuple(self.skip_unit.output.shape) != shape:
            raise ValueError(
                "%s: the skip tensor of %s is %s, the input is %s" % (
                    self.name, self.skip_unit.name,
                    tuple(self.skip_unit.output.shape), shape))
        x = self.input.devmem
        dt = self.compute_dtype if x is None else _compute_dtype(x)
        y = self.output.devmem
        if y is None or tuple(y.shape) != shape or y.dtype != dt:
            self.output.devmem = torch.zeros(shape, dtype=dt,
                                             device=self.torch_device)

    def run(self):
        import torch
        x = _compute(self.input.devmem)
        r = _compute(self.skip_unit.output.devmem)
        y = self.output.devmem
        if y is None or y.shape != x.shape or y.dtype != x.dtype or \
                y.device != x.device:
            self.output.devmem = y = torch.empty_like(x)
        ops.add(x, r, out=y)

    def package_export(self):
        return {"residual": self.residual}


class GDResidual(GradientDescentBase):
    MAPPING = "residual"

    def skip_gradient(self):
        """the gradient of the skip tensor: err_output itself"""
        return self.err_output.devmem

    def run(self):
        self.err_input.devmem = self.err_output.devmem
