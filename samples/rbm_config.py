root.rbm.update({  # noqa: F821 (root is injected)
    "loader_name": "bars_stripes",
    "loader": {"side": 4, "copies": 1, "minibatch_size": 30},
    "trainer": {"hidden": 16, "cd_k": 1, "learning_rate": 0.1,
                "gradient_moment": 0.5, "weights_decay": 0.0,
                "weights_stddev": 0.05, "sample_visible": True,
                "persistent": False},
    "decision": {"max_epochs": 2000, "exact_likelihood": True,
                 "likelihood_interval": 100},
    "snapshotter": {"prefix": "rbm", "interval": 500, "time_interval": 0},
})
