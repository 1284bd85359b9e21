"""Times the batch-normalisation kernels on one GPU at four layer shapes
([rows][channels], bf16): AlexNet-scale conv outputs [3072*27*27][256], a
VGG-scale [512*56*56][256] and [512*14*14][512], and an FC [3072][4096].

    (a) this project's kernels, whole passes and single kernels:
          training forward   hvk_bn_stats + hvk_bn_apply        6 B / element
          backward           hvk_bn_bwd (linear, no aux)        10 B / element
          inference          hvk_bn_fold + hvk_bn_apply         4 B / element
          statistics only    hvk_bn_stats                       2 B / element
          apply only         hvk_bn_apply                       4 B / element
          backward sums only hvk_bn_bwd without dx              4 B / element
    (b) torch.nn.functional.batch_norm, bf16 channels-last, float32 gamma /
        beta, backward through autograd (bytes: the same minimum as (a))
    (c) a bf16 copy_ of the same tensor, the streaming yardstick: 4 B /
        element like the forward apply

One process, the variants interleaved in every round, the first round
untimed, median and min - max over the rounds; a round times ``--calls``
back-to-back calls of a variant between two device events.  TB/s is the
minimum traffic of the pass over its median time.

    python tools/bench_batchnorm.py [--rounds 7] [--calls 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from veles_amd import ops  # noqa: E402

SHAPES = [(3072, 27, 27, 256), (512, 56, 56, 256), (512, 14, 14, 512),
          (3072, 4096)]


def variants(shape, dev):
    C = shape[-1]
    P = 1
    for d in shape[:-1]:
        P *= d
    gen = torch.Generator(device=dev).manual_seed(1)
    x = (0.5 + torch.randn(P, C, device=dev, generator=gen)).bfloat16()
    err = (0.1 * torch.randn(P, C, device=dev, generator=gen)).bfloat16()
    y, dx = torch.empty_like(x), torch.empty_like(x)
    g = torch.rand(C, device=dev, generator=gen) + 0.5
    b = torch.randn(C, device=dev, generator=gen)
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    save, ws = {}, {}
    lib = ops._lib.lib()
    p = ops._p
    ops.batchnorm_fwd(x, g, b, rm, rv, save=save, out=y, ws=ws)
    ops.batchnorm_bwd(err, x, None, g, save, dg, db, out=dx, ws=ws)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def stats():
        rc = lib.hvk_bn_stats(p(x), C, P, C, 1, p(g), p(b), p(rm), p(rv), 1e-5,
                              0.1, p(save["mean"]), p(save["invstd"]),
                              p(save["table"]), p(ws["stats"]), stream)
        assert rc == 0, rc

    def apply():
        rc = lib.hvk_bn_apply(p(x), C, p(y), C, P, C, p(save["table"]), 3,
                              stream)
        assert rc == 0, rc

    def sums():
        ops.batchnorm_bwd(err, x, None, g, save, dg, db, ws=ws,
                          need_dx=False)

    # torch: the same memory, viewed as NCHW with channels-last strides
    if len(shape) == 4:
        tx = x.view(shape).permute(0, 3, 1, 2)
        terr = err.view(shape).permute(0, 3, 1, 2)
    else:
        tx, terr = x, err
    tx = tx.detach().requires_grad_(True)
    tg, tb = g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    trm, trv = rm.clone(), rv.clone()
    ty = F.batch_norm(tx, trm, trv, tg, tb, True, 0.1, 1e-5)

    def t_fwd():
        with torch.no_grad():
            F.batch_norm(tx, trm, trv, tg, tb, True, 0.1, 1e-5)

    def t_bwd():
        torch.autograd.grad(ty, (tx, tg, tb), terr, retain_graph=True)

    def t_inf():
        with torch.no_grad():
            F.batch_norm(tx, trm, trv, tg, tb, False, 0.1, 1e-5)

    return P * C, [
        ("a training forward", 6, lambda: ops.batchnorm_fwd(
            x, g, b, rm, rv, act=3, save=save, out=y, ws=ws)),
        ("b torch training forward", 6, t_fwd),
        ("a backward", 10, lambda: ops.batchnorm_bwd(
            err, x, None, g, save, dg, db, out=dx, ws=ws)),
        ("b torch backward", 10, t_bwd),
        ("a inference", 4, lambda: ops.batchnorm_fwd(
            x, g, b, rm, rv, training=False, act=3, save=save, out=y,
            ws=ws)),
        ("b torch inference", 4, t_inf),
        ("a hvk_bn_stats", 2, stats),
        ("a hvk_bn_apply", 4, apply),
        ("a hvk_bn_bwd sums", 4, sums),
        ("c bf16 copy_", 4, lambda: y.copy_(x)),
    ]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_batchnorm needs the GPU")
    ops.require_library()
    dev = torch.device("cuda", 0)
    lines, rows = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("%d rounds x %d calls per variant, first round untimed; project "
        "yardsticks: hvk_sgd4 5.3 TB/s, LRN backward 4.9 TB/s" % (
            a.rounds, a.calls))
    for shape in SHAPES:
        n, vs = variants(shape, dev)
        times = {name: [] for name, _, _ in vs}
        for rnd in range(a.rounds + 1):
            for name, _, fn in vs:
                fn()
                t0, t1 = (torch.cuda.Event(enable_timing=True) for _ in "01")
                t0.record()
                for _ in range(a.calls):
                    fn()
                t1.record()
                t1.synchronize()
                if rnd:
                    times[name].append(t0.elapsed_time(t1) * 1e3 / a.calls)
        say("shape %s: %d elements" % ("x".join(map(str, shape)), n))
        say("  %-26s %6s %10s %10s %10s %8s" % (
            "variant", "B/el", "median us", "min us", "max us", "TB/s"))
        for name, bpe, _ in vs:
            t = times[name]
            row = {"shape": list(shape), "variant": name,
                   "bytes_per_element": bpe,
                   "median_us": statistics.median(t), "min_us": min(t),
                   "max_us": max(t), "rounds_us": t,
                   "tb_per_s": bpe * n / statistics.median(t) / 1e6}
            rows.append(row)
            say("  %-26s %6d %10.1f %10.1f %10.1f %8.2f" % (
                name, bpe, row["median_us"], row["min_us"], row["max_us"],
                row["tb_per_s"]))
        del vs
        torch.cuda.empty_cache()
    print(json.dumps({"bench": "batchnorm", "rows": rows}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
