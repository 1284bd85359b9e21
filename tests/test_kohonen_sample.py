"""The Kohonen sample (samples/kohonen.py) trains through the CLI on the CPU
device and its quantisation error falls by more than 10x in 6 epochs (the
float64 model of this configuration gives 55x - 75x over seeds 0-2)."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cli(*args, timeout=600):
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-m", "veles_amd"] + list(args),
                       cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout + r.stderr


def test_sample_trains_on_cpu(tmp_path):
    res = tmp_path / "results.json"
    out = cli("samples/kohonen.py", "-", "-a", "cpu", "--result-file",
              str(res), "root.common.disable.snapshotting=True")
    assert "Workflow wall time" in out
    r = json.loads(res.read_text())
    hist = r["quantization_error_history"]
    assert r["epochs"] == 6 and len(hist) == 6
    assert r["quantization_error"] == hist[-1]
    assert 0 < hist[-1] <= hist[0] / 10, hist
