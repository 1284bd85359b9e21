"""Bars and stripes: the classic toy distribution of the restricted Boltzmann
machine sample (samples/rbm.py), generated in-process.

An image of side ``s`` is either ``s`` rows each entirely 0 or 1 (bars) or
``s`` columns each entirely 0 or 1 (stripes).  The all-0 and the all-1 image
are both, so there are 2 * 2^s - 2 distinct patterns (30 of 16 pixels at the
default side 4).  The training set is these patterns in lexicographic order,
repeated ``copies`` times; there are no labels.
"""
from __future__ import annotations

import itertools

import numpy

from veles_amd.loader.base import TEST, TRAIN, VALID
from veles_amd.loader.fullbatch import FullBatchLoader

__all__ = ["BarsStripesLoader", "bars_and_stripes"]


def bars_and_stripes(side=4):
    """The distinct patterns, float32 [2 * 2^side - 2][side * side], sorted."""
    side = int(side)
    if side < 1 or side > 16:
        raise ValueError("bars_and_stripes: side %d" % side)
    pats = set()
    for bits in itertools.product((0, 1), repeat=side):
        a = numpy.tile(numpy.array(bits)[:, None], (1, side))
        pats.add(tuple(a.ravel()))
        pats.add(tuple(a.T.ravel()))
    return numpy.array(sorted(pats), dtype=numpy.float32)


class BarsStripesLoader(FullBatchLoader):
    """kwargs: ``side`` (4), ``copies`` (1); all samples are TRAIN."""

    MAPPING = "bars_stripes"

    def __init__(self, workflow, **kwargs):
        kwargs.setdefault("normalization_type", "none")
        super().__init__(workflow, **kwargs)
        self.side = int(kwargs.get("side", 4))
        self.copies = int(kwargs.get("copies", 1))
        if self.copies < 1:
            raise ValueError("bars_stripes: copies %d" % self.copies)

    def load_data(self):
        pats = bars_and_stripes(self.side)
        data = numpy.tile(pats, (self.copies, 1))
        self.class_lengths[TEST] = self.class_lengths[VALID] = 0
        self.class_lengths[TRAIN] = len(data)
        self.original_labels = []
        self.original_data.reset(data)
