"""samples/seq_recall.py with a post-LN attention block: (T, 8) ->
attention(E = 64, heads = 2) -> skip "x" -> attention(64, heads = 2) ->
layer_norm(residual = "x") -> softmax(8), trained with Adam:
``python -m veles_amd samples/seq_recall.py samples/seq_recall_block_config.py``

The second attention layer sits on a residual path: the ``skip`` layer marks
its input, and ``layer_norm`` with ``residual="x"`` normalises the sum of
that tensor and the attention output ("add & norm").  As with
samples/seq_recall_attn_config.py the task does not need the block; the
sample shows the wiring of ``skip`` / ``layer_norm`` and that the stack
trains.
"""
_gd = {"solvers": ("adam",), "learning_rate": 1e-2, "learning_rate_bias": 1e-2}

root.seq_recall.update({  # noqa: F821 (root is injected)
    "loader_name": "seq_recall",
    "loader": {"steps": 8, "features": 8, "n_markers": 8, "noise": 0.4,
               "class_lengths": (0, 256, 1024), "minibatch_size": 64,
               "seed": 1},
    "decision": {"max_epochs": 20, "fail_iterations": 100},
    "snapshotter": {"prefix": "seq_recall_block", "interval": 1,
                    "time_interval": 0},
})
root.seq_recall.layers = [  # noqa: F821
    {"type": "attention", "->": {"output_sample_shape": 64, "heads": 2},
     "<-": dict(_gd)},
    {"type": "skip", "name": "x"},
    {"type": "attention", "->": {"output_sample_shape": 64, "heads": 2},
     "<-": dict(_gd)},
    {"type": "layer_norm", "->": {"residual": "x"}, "<-": dict(_gd)},
    {"type": "softmax", "->": {"output_sample_shape": 8}, "<-": dict(_gd)}]
