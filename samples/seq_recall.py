"""Sequence recall with an LSTM: one of 8 marker tokens at step 0, T - 1 noise
steps after it, the label is the marker (veles_amd/loader/seq_recall.py; no
dataset).  (T, 8) -> lstm(32) -> softmax(8).
``python -m veles_amd samples/seq_recall.py -`` (CPU: -a cpu)."""
from veles_amd.models import StandardWorkflow
from veles_amd.utils.config import root, fix_contents
import veles_amd.loader  # noqa: F401


def run(load, main):
    cfg = fix_contents(root.seq_recall)
    load(StandardWorkflow, loader_name=cfg["loader_name"],
         loader_config=cfg["loader"], layers=cfg["layers"],
         decision_config=cfg["decision"],
         snapshotter_config=cfg.get("snapshotter"))
    main()
