"""Times the layer-normalisation kernels on one GPU at five [rows][features]
bf16 shapes a user would run: [64*512][1024], [16*2048][4096],
[256*128][256], [8*2048][8192] and [3072][4096].

    (a) this project's kernels (minimum traffic per element):
          forward                 hvk_ln_fwd             4 B (x; y)
          backward                hvk_ln_bwd             6 B (err, x; dx)
          forward with residual   hvk_ln_fwd             6 B (x, r; y)
          backward with residual  hvk_ln_bwd             8 B (err, x, r; dx)
        and the backward again with the column sums (dgamma, dbeta) forced
        into the dx kernel ("fused": the traffic above) and into a read pass
        of their own ("separate": 4 B more, 6 B more with a residual), the
        A/B behind ln_cols_fused of csrc/kernels/layernorm.hip
    (b) torch.nn.functional.layer_norm, bf16 (gamma and beta too: torch
        takes no float32 ones with a bf16 input), backward through
        autograd, with a separate bf16 x + r for the residual rows
        (TB/s over the same minimum as (a))
    (c) a bf16 copy_ of the same tensor, the streaming yardstick: 4 B /
        element like the forward

One process, the variants interleaved in every round, the first round
untimed, median and min - max over the rounds; a round times ``--calls``
back-to-back calls of a variant between two device events.  TB/s is the
minimum traffic of the pass over its median time.

Per shape the tool prints whether (a) forward + backward is faster than (b):
only when its median (of the per-round sums) is below (b)'s by more than
the two round-to-round spreads (max - min) added together.

    python tools/bench_layernorm.py [--rounds 7] [--calls 20] [--out FILE]
                                    [--ab-out FILE]
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

SHAPES = [(64 * 512, 1024), (16 * 2048, 4096), (256 * 128, 256),
          (8 * 2048, 8192), (3072, 4096)]
FWD, BWD, FWD_R, BWD_R, COPY = 4, 6, 6, 8, 4


def variants(shape, dev):
    P, C = shape
    gen = torch.Generator(device=dev).manual_seed(1)
    x = (0.5 + torch.randn(P, C, device=dev, generator=gen)).bfloat16()
    r = (0.5 * torch.randn(P, C, device=dev, generator=gen)).bfloat16()
    err = (0.1 * torch.randn(P, C, device=dev, generator=gen)).bfloat16()
    y, dx = torch.empty_like(x), torch.empty_like(x)
    g = torch.rand(C, device=dev, generator=gen) + 0.5
    b = torch.randn(C, device=dev, generator=gen)
    dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    save, save_r, ws = {}, {}, {}
    colsum = ops._lib.lib().hvk_ln_colsum
    ops.layernorm_fwd(x, g, b, save=save, out=y)
    ops.layernorm_fwd(x, g, b, residual=r, save=save_r, out=y)
    ops.layernorm_bwd(err, x, g, save, dg, db, out=dx, ws=ws)

    def bwd(residual):
        def run():
            ops.layernorm_bwd(err, x, g, save_r if residual else save, dg, db,
                              residual=r if residual else None, out=dx,
                              ws=ws)
        return run

    tx = x.detach().requires_grad_(True)
    tr = r.detach().requires_grad_(True)
    # torch's bf16 layer_norm wants gamma and beta in bf16 too
    tg = g.bfloat16().requires_grad_(True)
    tb = b.bfloat16().requires_grad_(True)
    ty = F.layer_norm(tx, (C,), tg, tb, 1e-5)
    ty_r = F.layer_norm(tx + tr, (C,), tg, tb, 1e-5)

    def t_fwd():
        with torch.no_grad():
            F.layer_norm(tx, (C,), tg, tb, 1e-5)

    def t_fwd_r():
        with torch.no_grad():
            F.layer_norm(tx + tr, (C,), tg, tb, 1e-5)

    def t_bwd():
        torch.autograd.grad(ty, (tx, tg, tb), err, retain_graph=True)

    def t_bwd_r():
        torch.autograd.grad(ty_r, (tx, tr, tg, tb), err, retain_graph=True)

    # (name, bytes per element, call, hvk_ln_colsum mode of the round: set
    # before and reset after the timed calls, never inside them)
    return P * C, colsum, [
        ("a forward", FWD, lambda: ops.layernorm_fwd(
            x, g, b, save=save, out=y), -1),
        ("b torch forward", FWD, t_fwd, -1),
        ("a backward", BWD, bwd(False), -1),
        ("b torch backward", BWD, t_bwd, -1),
        ("a forward residual", FWD_R, lambda: ops.layernorm_fwd(
            x, g, b, residual=r, save=save_r, out=y), -1),
        ("b torch forward residual", FWD_R, t_fwd_r, -1),
        ("a backward residual", BWD_R, bwd(True), -1),
        ("b torch backward residual", BWD_R, t_bwd_r, -1),
        ("a backward fused", BWD, bwd(False), 1),
        ("a backward separate", BWD, bwd(False), 0),
        ("a backward residual fused", BWD_R, bwd(True), 1),
        ("a backward residual separate", BWD_R, bwd(True), 0),
        ("a add", 6, lambda: ops.add(x, r, out=y), -1),
        ("c bf16 copy_", COPY, lambda: y.copy_(x), -1),
    ]


def spread(t):
    return max(t) - min(t)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ab-out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_layernorm needs the GPU")
    ops.require_library()
    dev = torch.device("cuda", 0)
    lines, ab, rows = [], [], []

    def say(s, to=None):
        print(s, flush=True)
        (lines if to is None else to).append(s)
    say("%d rounds x %d calls per variant, first round untimed" % (
        a.rounds, a.calls))
    say("column sums of the backward inside the dx kernel (fused) or in a "
        "read pass of their own (separate): %d rounds x %d calls, "
        "interleaved, same process" % (a.rounds, a.calls), ab)
    for shape in SHAPES:
        n, colsum, vs = variants(shape, dev)
        times = {name: [] for name, _, _, _ in vs}
        for rnd in range(a.rounds + 1):
            for name, _, fn, mode in vs:
                colsum(mode)
                fn()
                t0, t1 = (torch.cuda.Event(enable_timing=True) for _ in "01")
                t0.record()
                for _ in range(a.calls):
                    fn()
                t1.record()
                t1.synchronize()
                colsum(-1)
                if rnd:
                    times[name].append(t0.elapsed_time(t1) * 1e3 / a.calls)
        head = "shape %s: %d elements" % ("x".join(map(str, shape)), n)
        cols = "  %-30s %5s %10s %10s %10s %7s" % (
            "variant", "B/el", "median us", "min us", "max us", "TB/s")
        say(head)
        say(cols)
        say(head, ab)
        say(cols, ab)
        for name, bpe, _, _ in vs:
            t = times[name]
            row = {"shape": list(shape), "variant": name,
                   "bytes_per_element": bpe,
                   "median_us": statistics.median(t), "min_us": min(t),
                   "max_us": max(t), "rounds_us": t,
                   "tb_per_s": bpe * n / statistics.median(t) / 1e6}
            rows.append(row)
            is_ab = name.endswith(("fused", "separate"))
            say("  %-30s %5d %10.1f %10.1f %10.1f %7.2f" % (
                name, bpe, row["median_us"], row["min_us"], row["max_us"],
                row["tb_per_s"]), ab if is_ab else None)
        for tag in ("", " residual"):
            ta = [f + w for f, w in zip(times["a forward" + tag],
                                        times["a backward" + tag])]
            tb = [f + w for f, w in zip(times["b torch forward" + tag],
                                        times["b torch backward" + tag])]
            ma, mb = statistics.median(ta), statistics.median(tb)
            margin = spread(ta) + spread(tb)
            verdict = "faster" if ma + margin < mb else (
                "slower" if mb + margin < ma else "within the spreads")
            say("  forward + backward%s: (a) %.1f us (spread %.1f), (b) %.1f "
                "us (spread %.1f): (a) is %s (%.2fx)" % (
                    tag, ma, spread(ta), mb, spread(tb), verdict, mb / ma))
        copy = statistics.median(times["c bf16 copy_"])
        say("  (a) forward runs at %.2f of the copy_'s TB/s, backward at %.2f"
            % (FWD * copy / (COPY * statistics.median(times["a forward"])),
               BWD * copy / (COPY * statistics.median(times["a backward"]))))
        for tag in ("", " residual"):
            f = statistics.median(times["a backward%s fused" % tag])
            s = statistics.median(times["a backward%s separate" % tag])
            margin = spread(times["a backward%s fused" % tag]) + \
                spread(times["a backward%s separate" % tag])
            say("  backward%s: fused %.1f us, separate %.1f us: %s" % (
                tag, f, s, "fused wins" if f + margin < s else
                "separate wins" if s + margin < f else
                "within the spreads"), ab)
        del vs
        torch.cuda.empty_cache()
    print(json.dumps({"bench": "layernorm", "rows": rows}))
    for path, text in ((a.out, lines), (a.ab_out, ab)):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
