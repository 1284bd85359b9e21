"""The sequence-recall sample with a full post-LN encoder block
(samples/seq_recall.py with samples/seq_recall_encoder_config.py: (T, 8) ->
attention(64, 2 heads) -> skip "a" -> attention(64, 2 heads) ->
layer_norm(residual="a") -> skip "b" -> ffn(64, hidden 256) ->
layer_norm(residual="b") -> softmax(8), Adam) trains through the CLI on the
CPU device.

The epoch count was measured, not fixed in advance: seeds 1 .. 5 (``-r``) ran
44 epochs on the CPU device.  The validation errors (of 256; chance is 224)
start at 231, 223, 238, 206 and 205 and first fall below 20 at epochs 10, 9,
13, 13 and 10.  After 20 epochs seed 4 is still moving (8, then 12 .. 15 over
the next four epochs), so the configured count is 30, where every seed has
settled: over epochs 30 .. 44 the errors stay within 3 .. 3, 6 .. 8, 3 .. 3,
7 .. 9 and 2 .. 2.  Validation errors after epoch 30, seeds 1 .. 5: 3, 6, 3,
9, 2; each seed is held to its measured plateau widened by 2 samples either
way, since a count on a plateau, unlike a zero, moves by a sample with the
summation order of the host's BLAS."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_SEED_ERRORS = (3, 6, 3, 9, 2)
CPU_SEED_PLATEAU = ((3, 3), (6, 8), (3, 3), (7, 9), (2, 2))
EPOCHS = 30


def cli(*args, timeout=900):
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-m", "veles_amd"] + list(args),
                       cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout + r.stderr


@pytest.mark.parametrize("seed", (1, 2, 3, 4, 5))
def test_encoder_sample_trains_on_cpu(tmp_path, seed):
    res = tmp_path / "results.json"
    out = cli("samples/seq_recall.py", "samples/seq_recall_encoder_config.py",
              "-a", "cpu", "-r", str(seed), "--result-file", str(res),
              "root.common.disable.snapshotting=True")
    assert "Workflow wall time" in out
    h = json.loads(res.read_text())["Epoch history"]
    assert len(h) == EPOCHS
    errors = [round(e["validation_err_pt"] * 256 / 100.0) for e in h]
    print(seed, errors, "measured", CPU_SEED_ERRORS[seed - 1])
    assert errors[0] > 128, errors        # it starts near chance (7/8)
    lo, hi = CPU_SEED_PLATEAU[seed - 1]
    assert max(lo - 2, 0) <= errors[-1] <= hi + 2, errors
