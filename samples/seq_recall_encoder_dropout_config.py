"""samples/seq_recall_encoder_config.py with dropout 0.1 on the attention
weights of both attention layers (torch's ``MultiheadAttention(dropout=0.1)``):
``python -m veles_amd samples/seq_recall.py
samples/seq_recall_encoder_dropout_config.py``

The dropout runs inside the fused attention kernels on TRAIN minibatches only
(docs/OPS.md "Attention"); validation and testing see the plain softmax.  The
rest of the block, the loader and the solver are those of the encoder sample;
the epoch count is 45 instead of 30: the dropout noise at this learning rate
keeps the validation error moving for longer (docs/OPS.md "Attention" has the
measured errors per seed).
"""
_gd = {"solvers": ("adam",), "learning_rate": 1e-2, "learning_rate_bias": 1e-2}
_att = {"output_sample_shape": 64, "heads": 2, "dropout": 0.1}

root.seq_recall.update({  # noqa: F821 (root is injected)
    "loader_name": "seq_recall",
    "loader": {"steps": 8, "features": 8, "n_markers": 8, "noise": 0.4,
               "class_lengths": (0, 256, 1024), "minibatch_size": 64,
               "seed": 1},
    "decision": {"max_epochs": 45, "fail_iterations": 100},
    "snapshotter": {"prefix": "seq_recall_encoder_dropout", "interval": 1,
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
