"""Restricted Boltzmann machine demo: 16 hidden units trained by CD-1 on the
30 bars-and-stripes patterns of 4 x 4 pixels, full batch, with the exact
log-likelihood (2^16 visible states enumerated on the host) logged at the
first, every 100th and the last epoch.  ``python -m veles_amd samples/rbm.py -`` (CPU: -a cpu)."""
from veles_amd.models import RBMWorkflow
from veles_amd.utils.config import root, fix_contents


def run(load, main):
    cfg = fix_contents(root.rbm)
    load(RBMWorkflow, loader_name=cfg["loader_name"],
         loader_config=cfg["loader"], trainer_config=cfg["trainer"],
         decision_config=cfg["decision"],
         snapshotter_config=cfg.get("snapshotter"))
    main()
