root.kohonen.update({  # noqa: F821 (root is injected)
    "loader_name": "gaussian_clusters",
    "loader": {"n_train": 400, "stddev": 0.08, "seed": 0,
               "minibatch_size": 20},
    # schedules as (a, b): a / (1 + b t), t = the training step
    "trainer": {"shape": (8, 8), "weights_filling": "uniform",
                "weights_stddev": 0.05, "gradient_decay": (0.5, 0.02),
                "radius_decay": (1.0, 0.1)},
    "forward": {"total": True},
    "decision": {"max_epochs": 6},
    "snapshotter": {"prefix": "kohonen", "interval": 1, "time_interval": 0},
    "plotters": True,
})
