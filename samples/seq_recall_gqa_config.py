"""samples/seq_recall_encoder_config.py with grouped-query heads: both
attention layers have ``"heads": 2, "kv_heads": 1``, so the two query heads of
a layer share one key / value head (multi-query attention, the smallest
group):
``python -m veles_amd samples/seq_recall.py samples/seq_recall_gqa_config.py``

W_in of a layer has E + 2 KVH D = 128 rows instead of 3E = 192 (docs/OPS.md
"Attention", "Grouped-query heads").  The rest of the block, the loader, the
solver and the epoch count are those of the encoder sample.
"""
_gd = {"solvers": ("adam",), "learning_rate": 1e-2, "learning_rate_bias": 1e-2}
_att = {"output_sample_shape": 64, "heads": 2, "kv_heads": 1}

root.seq_recall.update({  # noqa: F821 (root is injected)
    "loader_name": "seq_recall",
    "loader": {"steps": 8, "features": 8, "n_markers": 8, "noise": 0.4,
               "class_lengths": (0, 256, 1024), "minibatch_size": 64,
               "seed": 1},
    "decision": {"max_epochs": 30, "fail_iterations": 100},
    "snapshotter": {"prefix": "seq_recall_gqa", "interval": 1,
                    "time_interval": 0},
})
root.seq_recall.layers = [  # noqa: F821
    {"type": "attention", "->": dict(_att), "<-": dict(_gd)},
    {"type": "skip", "name": "a"},
    {"type": "attention", "->": dict(_att), "<-": dict(_gd)},
    {"type": "layer_norm", "->": {"residual": "a"}, "<-": dict(_gd)},
    {"type": "skip", "name": "b"},
    {"type": "ffn", "->": {"output_sample_shape": 64, "hidden": 256,
                           "activation": "gelu"}, "<-": dict(_gd)},
    {"type": "layer_norm", "->": {"residual": "b"}, "<-": dict(_gd)},
    {"type": "softmax", "->": {"output_sample_shape": 8}, "<-": dict(_gd)}]
