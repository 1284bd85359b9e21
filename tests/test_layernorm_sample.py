"""The sequence-recall sample with a post-LN attention block
(samples/seq_recall.py with samples/seq_recall_block_config.py: (T, 8) ->
attention(64, 2 heads) -> skip "x" -> attention(64, 2 heads) ->
layer_norm(residual="x") -> softmax(8), Adam) trains through the CLI on the
CPU device.

The epoch count was measured, not fixed in advance: seeds 1 .. 5 (``-r``) ran
60 epochs on the CPU device.  The validation errors (of 256; chance is 224)
start at 216, 230, 223, 217 and 223, first fall below 20 at epochs 10, 9, 8,
8 and 7 and settle by epoch 20: over epochs 20 .. 60 they stay within
6 .. 8, 8 .. 10, 6 .. 7, 7 .. 8 and 1 .. 4 (seed 5 keeps creeping down, one
sample every few epochs).  The configured count is 20, as for the attention
sample.  Validation errors after epoch 20, seeds 1 .. 5: 8, 10, 7, 7, 4; each
seed is held to its measured plateau widened by 2 samples either way, since
a count on a plateau, unlike a zero, moves by a sample with the summation
order of the host's BLAS."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_SEED_ERRORS = (8, 10, 7, 7, 4)
CPU_SEED_PLATEAU = ((6, 8), (8, 10), (6, 7), (7, 8), (1, 4))
EPOCHS = 20


def cli(*args, timeout=600):
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-m", "veles_amd"] + list(args),
                       cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout + r.stderr


@pytest.mark.parametrize("seed", (1, 2, 3, 4, 5))
def test_block_sample_trains_on_cpu(tmp_path, seed):
    res = tmp_path / "results.json"
    out = cli("samples/seq_recall.py", "samples/seq_recall_block_config.py",
              "-a", "cpu", "-r", str(seed), "--result-file", str(res),
              "root.common.disable.snapshotting=True")
    assert "Workflow wall time" in out
    h = json.loads(res.read_text())["Epoch history"]
    assert len(h) == EPOCHS
    errors = [round(e["validation_err_pt"] * 256 / 100.0) for e in h]
    print(seed, errors, "measured", CPU_SEED_ERRORS[seed - 1])
    assert errors[0] > 128, errors        # it starts near chance (7/8)
    lo, hi = CPU_SEED_PLATEAU[seed - 1]
    assert lo - 2 <= errors[-1] <= hi + 2, errors
