"""samples/seq_recall.py trained with Adam and clipping by the global gradient
norm instead of momentum SGD with a learning rate of 1:
``python -m veles_amd samples/seq_recall.py samples/seq_recall_adam_config.py``
"""
_gd = {"solvers": ("adam",), "learning_rate": 1e-2, "learning_rate_bias": 1e-2}

root.common.engine.clip_gradient_norm = 1.0  # noqa: F821 (root is injected)
root.seq_recall.update({  # noqa: F821
    "loader_name": "seq_recall",
    "loader": {"steps": 8, "features": 8, "n_markers": 8, "noise": 0.4,
               "class_lengths": (0, 256, 1024), "minibatch_size": 64,
               "seed": 1},
    "decision": {"max_epochs": 25, "fail_iterations": 100},
    "snapshotter": {"prefix": "seq_recall_adam", "interval": 1,
                    "time_interval": 0},
})
root.seq_recall.layers = [  # noqa: F821
    {"type": "lstm", "->": {"output_sample_shape": 32,
                            "return_sequences": False}, "<-": dict(_gd)},
    {"type": "softmax", "->": {"output_sample_shape": 8}, "<-": dict(_gd)}]
