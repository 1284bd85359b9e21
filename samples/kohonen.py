"""Kohonen map demo (the reference's DemoKohonen): an 8 x 8 map trained on
400 two-dimensional points drawn from 4 Gaussian clusters.
``python -m veles_amd samples/kohonen.py -`` (CPU: -a cpu)."""
import numpy

from veles_amd.loader.base import TEST, TRAIN, VALID
from veles_amd.loader.fullbatch import FullBatchLoader
from veles_amd.models import KohonenWorkflow
from veles_amd.utils.config import root, fix_contents

CENTRES = ((-.6, -.6), (.6, -.5), (-.5, .6), (.55, .55))


class GaussianClustersLoader(FullBatchLoader):
    """``n_train`` float32 points around CENTRES (standard deviation
    ``stddev``), generated from ``seed``; the cluster ids are the labels.
    Served as float32 on every device: a bf16 minibatch would move the
    points by up to 2e-3, a quarter of a map cell at 6 epochs."""

    MAPPING = "gaussian_clusters"

    def __init__(self, workflow, **kwargs):
        super().__init__(workflow, **kwargs)
        self.n_train = int(kwargs.get("n_train", 400))
        self.stddev = float(kwargs.get("stddev", 0.08))
        self.seed = int(kwargs.get("seed", 0))

    def _torch_dtype_for_minibatch(self):
        import torch
        return torch.float32

    def load_data(self):
        rs = numpy.random.RandomState(self.seed)
        labels = (numpy.arange(self.n_train) % len(CENTRES)).astype(
            numpy.int32)
        data = numpy.asarray(CENTRES, numpy.float64)[labels] + \
            rs.normal(0.0, self.stddev, (self.n_train, 2))
        self.class_lengths[TEST] = self.class_lengths[VALID] = 0
        self.class_lengths[TRAIN] = self.n_train
        self.original_labels = labels
        self.original_data.reset(data.astype(numpy.float32))
        self.labels_mapping = {i: i for i in range(len(CENTRES))}
        self.reversed_labels_mapping = list(range(len(CENTRES)))


def run(load, main):
    cfg = fix_contents(root.kohonen)
    load(KohonenWorkflow, loader_name=cfg["loader_name"],
         loader_config=cfg["loader"], trainer_config=cfg["trainer"],
         forward_config=cfg.get("forward"), decision_config=cfg["decision"],
         snapshotter_config=cfg.get("snapshotter"),
         plotters=cfg.get("plotters", False))
    main()
