"""samples/seq_recall.py with a full post-LN transformer encoder block:
(T, 8) -> attention(E = 64, heads = 2) -> skip "a" -> attention(64, heads =
2) -> layer_norm(residual = "a") -> skip "b" -> ffn(64, hidden 256, GELU) ->
layer_norm(residual = "b") -> softmax(8), trained with Adam:
``python -m veles_amd samples/seq_recall.py samples/seq_recall_encoder_config.py``

The first attention layer lifts the 8 input features to the block's width;
the rest is the encoder layer of "Attention is all you need" with its two
sublayers, self-attention and the position-wise feed-forward layer, each on
a residual path followed by a layer normalisation ("add & norm").  As with
samples/seq_recall_block_config.py the task does not need the block; the
sample shows the wiring of ``ffn`` with ``skip`` / ``layer_norm`` and that
the stack trains.
"""
_gd = {"solvers": ("adam",), "learning_rate": 1e-2, "learning_rate_bias": 1e-2}

root.seq_recall.update({  # noqa: F821 (root is injected)
    "loader_name": "seq_recall",
    "loader": {"steps": 8, "features": 8, "n_markers": 8, "noise": 0.4,
               "class_lengths": (0, 256, 1024), "minibatch_size": 64,
               "seed": 1},
    "decision": {"max_epochs": 30, "fail_iterations": 100},
    "snapshotter": {"prefix": "seq_recall_encoder", "interval": 1,
                    "time_interval": 0},
})
root.seq_recall.layers = [  # noqa: F821
    {"type": "attention", "->": {"output_sample_shape": 64, "heads": 2},
     "<-": dict(_gd)},
    {"type": "skip", "name": "a"},
    {"type": "attention", "->": {"output_sample_shape": 64, "heads": 2},
     "<-": dict(_gd)},
    {"type": "layer_norm", "->": {"residual": "a"}, "<-": dict(_gd)},
    {"type": "skip", "name": "b"},
    {"type": "ffn", "->": {"output_sample_shape": 64, "hidden": 256,
                           "activation": "gelu"}, "<-": dict(_gd)},
    {"type": "layer_norm", "->": {"residual": "b"}, "<-": dict(_gd)},
    {"type": "softmax", "->": {"output_sample_shape": 8}, "<-": dict(_gd)}]
