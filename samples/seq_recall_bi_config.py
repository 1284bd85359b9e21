_gd = {"learning_rate": 1.0, "learning_rate_bias": 1.0,
       "gradient_moment": 0.9, "gradient_moment_bias": 0.9}

# the sequence-recall sample with a bidirectional LSTM (16 units per
# direction, so the softmax still sees 32 features):
# python -m veles_amd samples/seq_recall.py samples/seq_recall_bi_config.py
root.seq_recall.update({  # noqa: F821 (root is injected)
    "loader_name": "seq_recall",
    "loader": {"steps": 8, "features": 8, "n_markers": 8, "noise": 0.4,
               "class_lengths": (0, 256, 1024), "minibatch_size": 64,
               "seed": 1},
    "decision": {"max_epochs": 6, "fail_iterations": 100},
    "snapshotter": {"prefix": "seq_recall_bi", "interval": 1,
                    "time_interval": 0},
})
root.seq_recall.layers = [  # noqa: F821
    {"type": "lstm", "->": {"output_sample_shape": 16,
                            "return_sequences": False,
                            "bidirectional": True}, "<-": dict(_gd)},
    {"type": "softmax", "->": {"output_sample_shape": 8}, "<-": dict(_gd)}]
