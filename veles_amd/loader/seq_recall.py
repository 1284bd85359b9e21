"""Sequence recall: the synthetic task of the recurrent sample
(samples/seq_recall.py), generated in-process.

A sample is a (T, I) sequence: step 0 carries one of ``n_markers`` marker
tokens (a one-hot vector over the first ``n_markers`` of the I features), the
T - 1 steps after it are Gaussian noise (standard deviation ``noise``) on all
features.  The label is the marker: the network has to carry it across the
noise to the last step.
"""
from __future__ import annotations

import numpy

from veles_amd.loader.fullbatch import FullBatchLoader

__all__ = ["SeqRecallLoader"]


class SeqRecallLoader(FullBatchLoader):
    """kwargs: ``steps`` (T), ``features`` (I >= n_markers), ``n_markers``,
    ``noise``, ``class_lengths`` = (test, validation, train), ``seed``."""

    MAPPING = "seq_recall"

    def __init__(self, workflow, **kwargs):
        kwargs.setdefault("normalization_type", "none")
        super().__init__(workflow, **kwargs)
        self.steps = int(kwargs.get("steps", 12))
        self.n_markers = int(kwargs.get("n_markers", 8))
        self.features = int(kwargs.get("features", self.n_markers))
        self.noise = float(kwargs.get("noise", 0.5))
        self.requested_lengths = list(kwargs.get("class_lengths",
                                                 (0, 256, 1024)))
        self.seed = int(kwargs.get("seed", 1))
        if self.steps < 1 or self.features < self.n_markers or \
                self.n_markers < 2:
            raise ValueError("seq_recall: steps %d, features %d, markers %d" %
                             (self.steps, self.features, self.n_markers))

    def load_data(self):
        self.class_lengths = [int(x) for x in self.requested_lengths]
        n = sum(self.class_lengths)
        rs = numpy.random.RandomState(self.seed)
        labels = rs.randint(0, self.n_markers, n).astype(numpy.int32)
        data = rs.normal(0.0, self.noise, (n, self.steps, self.features))
        data[:, 0] = 0.0
        data[numpy.arange(n), 0, labels] = 1.0
        self.original_labels = labels
        self.original_data.reset(data.astype(numpy.float32))
        self.labels_mapping = {i: i for i in range(self.n_markers)}
        self.reversed_labels_mapping = list(range(self.n_markers))
