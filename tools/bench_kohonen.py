"""HIP-event timing of the two Kohonen kernels (ops.kohonen_argmin /
ops.kohonen_update) against the fp32 torch composition on the same device,
in one process, interleaved, after a warm-up: the median and minimum of
``--rounds`` rounds per arm.

The comparison is what a user would write with torch calls:
  winners  (w2 - 2 * x @ w.T).argmin(1)       with w2 = (w * w).sum(1)
  update   G = K[a]; w += gm * (G.T @ x - G.sum(0)[:, None] * w)
           with K = exp(-cdist(coords)^2 / (2 sigma^2)) prepared outside the
           timed region (it depends only on sigma).
Shapes (B, sx x sy, D): 4096, 32 x 32, 784 and 4096, 8 x 8, 2.

usage: python tools/bench_kohonen.py [--rounds 7] [--reps 20] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(
    __file__))))

import torch  # noqa: E402

from veles_amd import ops  # noqa: E402

SHAPES = [(4096, 32, 32, 784), (4096, 8, 8, 2)]


def timeit(fn, reps):
    a, b = torch.cuda.Event(True), torch.cuda.Event(True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps * 1e3   # microseconds per call


def bench_shape(B, sx, sy, D, rounds, reps, sigma=0.5, gradient=0.1):
    dev = "cuda"
    NN = sx * sy
    g = torch.Generator().manual_seed(B + NN + D)
    x = torch.randn(B, D, generator=g).to(dev)
    w0 = (torch.rand(NN, D, generator=g) * 2 - 1).to(dev)
    coords = ops.kohonen_coords(sx, sy, dev)
    a_out = torch.empty(B, dtype=torch.int32, device=dev)
    qerr = torch.empty(B, device=dev)
    w_hip, w_torch = w0.clone(), w0.clone()
    d = coords[:, None, :] - coords[None, :, :]
    K = torch.exp(-(d * d).sum(2) / (2 * sigma * sigma))
    gm = gradient / B

    def argmin_hip():
        ops.kohonen_argmin(x, w_hip, argmin=a_out, qerr=qerr)

    def argmin_torch():
        w2 = (w_torch * w_torch).sum(1)
        return (w2 - 2.0 * (x @ w_torch.t())).argmin(1)

    a_ref = argmin_torch()
    argmin_hip()
    torch.cuda.synchronize()
    agree = float((a_out.long() == a_ref).float().mean())
    a_long = a_ref.clone()

    def update_hip():
        ops.kohonen_update(x, w_hip, coords, a_out, sigma, gradient)

    def update_torch():
        G = K[a_long]
        w_torch.add_(G.t() @ x - G.sum(0)[:, None] * w_torch, alpha=gm)

    # one step of each from the same weights: the results must agree
    update_hip()
    update_torch()
    torch.cuda.synchronize()
    diff = float((w_hip - w_torch).abs().max())

    arms = {"argmin_hip": argmin_hip, "argmin_torch": argmin_torch,
            "update_hip": update_hip, "update_torch": update_torch}
    for fn in arms.values():          # warm-up of every arm
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():    # interleaved
            ts[k].append(timeit(fn, reps))
    res = {"shape": [B, sx, sy, D], "winners_agree": agree,
           "update_max_abs_diff": diff}
    for k, v in ts.items():
        v = sorted(v)
        res[k + "_us"] = {"median": round(v[len(v) // 2], 2),
                          "min": round(v[0], 2), "max": round(v[-1], 2)}
    flop_a = 2.0 * B * NN * D
    res["argmin_hip_TFLOPs"] = round(
        flop_a / res["argmin_hip_us"]["median"] / 1e6, 2)
    res["update_hip_TFLOPs"] = round(
        flop_a / res["update_hip_us"]["median"] / 1e6, 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kohonen needs the GPU")
    if args.rounds < 5:
        raise SystemExit("at least 5 rounds")
    out = []
    for shape in SHAPES:
        r = bench_shape(*shape, rounds=args.rounds, reps=args.reps)
        print(json.dumps(r), flush=True)
        out.append(r)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
