"""samples/seq_recall.py with a self-attention layer in the LSTM's place:
(T, 8) -> attention(E = 64, heads = 2) -> softmax(8), trained with Adam:
``python -m veles_amd samples/seq_recall.py samples/seq_recall_attn_config.py``

The task does not need attention: the marker sits at step 0 and the softmax
layer sees every step of the attention output, so a linear read-out of step 0
would do.  The sample shows the wiring of the ``attention`` layer type and
that the layer trains.
"""
_gd = {"solvers": ("adam",), "learning_rate": 1e-2, "learning_rate_bias": 1e-2}

root.seq_recall.update({  # noqa: F821 (root is injected)
    "loader_name": "seq_recall",
    "loader": {"steps": 8, "features": 8, "n_markers": 8, "noise": 0.4,
               "class_lengths": (0, 256, 1024), "minibatch_size": 64,
               "seed": 1},
    "decision": {"max_epochs": 20, "fail_iterations": 100},
    "snapshotter": {"prefix": "seq_recall_attn", "interval": 1,
                    "time_interval": 0},
})
root.seq_recall.layers = [  # noqa: F821
    {"type": "attention", "->": {"output_sample_shape": 64, "heads": 2},
     "<-": dict(_gd)},
    {"type": "softmax", "->": {"output_sample_shape": 8}, "<-": dict(_gd)}]
