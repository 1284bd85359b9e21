"""The sequence-recall sample with a GRU in the LSTM's place
(samples/seq_recall.py with samples/seq_recall_gru_config.py) trains through
the CLI on the CPU device: after the configured 15 epochs no validation
sample of 256 is misclassified.

The epoch count was measured, not fixed in advance: seeds 1 .. 5 (``-r``) ran
60 epochs on the CPU device and reach zero validation errors for good at
epochs 9, 11, 12, 10 and 11 (they stay there through epoch 60), so all five
are at zero from epoch 12; rounded up to a multiple of 5 that is 15, and
epochs 16 .. 20 keep zero errors for every seed.  Validation errors after
epoch 15, seeds 1 .. 5: 0, 0, 0, 0, 0."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_SEED_ERRORS = (0, 0, 0, 0, 0)
EPOCHS = 15


def cli(*args, timeout=600):
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-m", "veles_amd"] + list(args),
                       cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout + r.stderr


@pytest.mark.parametrize("seed", (1, 2, 3, 4, 5))
def test_gru_sample_trains_on_cpu(tmp_path, seed):
    res = tmp_path / "results.json"
    out = cli("samples/seq_recall.py", "samples/seq_recall_gru_config.py",
              "-a", "cpu", "-r", str(seed), "--result-file", str(res),
              "root.common.disable.snapshotting=True")
    assert "Workflow wall time" in out
    h = json.loads(res.read_text())["Epoch history"]
    assert len(h) == EPOCHS
    errors = [round(e["validation_err_pt"] * 256 / 100.0) for e in h]
    assert errors[0] > 128, errors        # it starts near chance (7/8)
    assert errors[-1] == CPU_SEED_ERRORS[seed - 1], errors
