"""The RBM sample (samples/rbm.py) trains through the CLI on the CPU device:
16 hidden units, CD-1, the 30 bars-and-stripes patterns as one full batch,
2000 epochs, the exact log-likelihood from the decision unit.

An untrained model gives -16 ln 2 = -11.09 nats per pattern, a uniform
distribution over the 30 patterns would give -3.40.  A float64 numpy model
of exactly this configuration ends between -4.69 and -4.96 over five seeds.
Measured here, seeds 1 .. 5 (``-r``), first epoch: -11.101, -11.106,
-11.101, -11.101, -11.099; last epoch: -5.230, -5.032, -4.670, -4.969,
-4.913.  The bounds are the issue's: first <= -10.5, last >= -6.0."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cli(*args, timeout=600):
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-m", "veles_amd"] + list(args),
                       cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout + r.stderr


@pytest.mark.parametrize("seed", (1, 2, 3, 4, 5))
def test_sample_trains_on_cpu(tmp_path, seed):
    res = tmp_path / "results.json"
    out = cli("samples/rbm.py", "-", "-a", "cpu", "-r", str(seed),
              "--result-file", str(res),
              "root.common.disable.snapshotting=True")
    assert "Workflow wall time" in out
    r = json.loads(res.read_text())
    hist = r["log_likelihood_history"]
    assert r["epochs"] == 2000
    assert hist[0][0] == 0 and hist[-1][0] == 1999
    assert r["log_likelihood"] == hist[-1][1]
    print("seed %d: log-likelihood %.4f -> %.4f" % (seed, hist[0][1],
                                                    hist[-1][1]))
    assert hist[0][1] <= -10.5, hist
    assert hist[-1][1] >= -6.0, hist
