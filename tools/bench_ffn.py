"""Times the position-wise feed-forward layer on one GPU at the shapes P x I
-> F (-> E = I) 32768 x 1024 -> 4096, 8192 x 512 -> 2048, 65536 x 256 ->
1024 and the latency-bound 256 x 64 -> 256, all bf16.

    (a) ops.ffn_fwd + ops.ffn_bwd: two GEMMs and hvk_ffn_act_fwd forward;
        three GEMMs (+ one transpose_colsum) and hvk_ffn_act_bwd backward
    (b) torch Linear - GELU - Linear in bf16, backward through autograd
    (c) the two activation kernels alone over [P][F], in TB/s of their
        minimum traffic (forward 4 B / element: u; h.  backward with du^T 8 B:
        dh, u; du, du^T.  backward without 6 B) against a bf16 copy_ (4 B)
    (d) du^T by the tile path of hvk_ffn_act_bwd (8 B / element) against the
        plain backward followed by ops.transpose_colsum (6 + 4 B)

One process, the variants interleaved in every round, the first round
untimed, median and min - max over the rounds; a round times ``--calls``
back-to-back calls of a variant between two device events.

    python tools/bench_ffn.py [--rounds 7] [--calls 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from veles_amd import ops  # noqa: E402

SHAPES = [(32768, 1024, 4096), (8192, 512, 2048), (65536, 256, 1024),
          (256, 64, 256)]
ACT = "gelu"


def variants(shape, dev):
    P, I, F_ = shape
    E = I
    gen = torch.Generator(device=dev).manual_seed(1)

    def r(*s):
        return torch.randn(*s, device=dev, generator=gen)
    x = r(P, I).bfloat16()
    w1 = (r(F_, I) / I ** 0.5).bfloat16()
    w2 = (r(E, F_) / F_ ** 0.5).bfloat16()
    bias = 0.1 * r(F_ + E)
    err = (0.1 * r(P, E)).bfloat16()
    y, ei = torch.empty(P, E, dtype=x.dtype, device=dev), torch.empty_like(x)
    dw1 = torch.empty(F_, I, device=dev)
    dw2 = torch.empty(E, F_, device=dev)
    db = torch.empty(F_ + E, device=dev)
    save = {}

    def fwd():
        ops.ffn_fwd(x, w1, w2, bias, ACT, save=save, out=y)

    def bwd():
        ops.ffn_bwd(err, x, w1, w2, save, dw1, dw2, db, ACT, err_input=ei)
    fwd()
    bwd()

    net = torch.nn.Sequential(
        torch.nn.Linear(I, F_), torch.nn.GELU(), torch.nn.Linear(F_, E)
    ).to(dev).bfloat16()
    tx = x.detach().requires_grad_(True)
    ty = net(tx)
    params = [tx] + list(net.parameters())

    def t_fwd():
        with torch.no_grad():
            net(tx)

    def t_bwd():
        torch.autograd.grad(ty, params, err, retain_graph=True)

    u = (2 * r(P, F_)).bfloat16()
    dh = r(P, F_).bfloat16()
    h, du = torch.empty_like(u), torch.empty_like(u)
    dut = torch.empty(F_, P, dtype=u.dtype, device=dev)
    db1 = torch.empty(F_, device=dev)
    ws_t, ws_r = {}, {}
    tws = torch.empty(P // 64 * F_, device=dev)

    def act_tile():
        ops.ffn_act_bwd(dh, u, ACT, out=du, out_t=dut, db1=db1, ws=ws_t)

    def act_plain():
        ops.ffn_act_bwd(dh, u, ACT, out=du, db1=db1, ws=ws_r)

    def act_plain_t():
        ops.ffn_act_bwd(dh, u, ACT, out=du, ws=ws_r)
        ops.transpose_colsum(du, out=dut, colsum=db1, ws=tws)

    # (name, bytes per element of [P][F] or None, call)
    return P * F_, [
        ("a ffn_fwd", None, fwd),
        ("b torch forward", None, t_fwd),
        ("a ffn_bwd", None, bwd),
        ("b torch backward", None, t_bwd),
        ("c act forward", 4, lambda: ops.ffn_act_fwd(u, ACT, out=h)),
        ("c act backward (row path)", 6, act_plain),
        ("d act backward tile (du, du^T)", 8, act_tile),
        ("d act backward + transpose_colsum", 10, act_plain_t),
        ("c bf16 copy_", 4, lambda: h.copy_(u)),
    ]


def spread(t):
    return max(t) - min(t)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_ffn needs the GPU")
    ops.require_library()
    dev = torch.device("cuda", 0)
    lines, rows = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("%d rounds x %d calls per variant, first round untimed; activation "
        "%s" % (a.rounds, a.calls, ACT))
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
        say("shape P x I -> F %s: %d hidden elements" % (
            " x ".join(map(str, shape)), n))
        say("  %-36s %5s %10s %10s %10s %7s" % (
            "variant", "B/el", "median us", "min us", "max us", "TB/s"))
        med = {}
        for name, bpe, _ in vs:
            t = times[name]
            med[name] = statistics.median(t)
            row = {"shape": list(shape), "variant": name,
                   "bytes_per_element": bpe, "median_us": med[name],
                   "min_us": min(t), "max_us": max(t), "rounds_us": t,
                   "tb_per_s": None if bpe is None else
                   bpe * n / med[name] / 1e6}
            rows.append(row)
            say("  %-36s %5s %10.1f %10.1f %10.1f %7s" % (
                name, "-" if bpe is None else bpe, med[name], min(t), max(t),
                "-" if bpe is None else "%.2f" % row["tb_per_s"]))
        ta = [f + w for f, w in zip(times["a ffn_fwd"], times["a ffn_bwd"])]
        tb = [f + w for f, w in zip(times["b torch forward"],
                                    times["b torch backward"])]
        ma, mb = statistics.median(ta), statistics.median(tb)
        margin = spread(ta) + spread(tb)
        verdict = "faster" if ma + margin < mb else (
            "slower" if mb + margin < ma else "within the spreads")
        say("  forward + backward: (a) %.1f us (spread %.1f), (b) %.1f us "
            "(spread %.1f): (a) is %s (%.2fx)" % (
                ma, spread(ta), mb, spread(tb), verdict, mb / ma))
        acts = med["c act forward"] + med["d act backward tile (du, du^T)"]
        say("  the two activation passes are %.1f us, %.2f of (a)" % (
            acts, acts / ma))
        copy = med["c bf16 copy_"]
        say("  act forward runs at %.2f of the copy_'s TB/s, the row-path "
            "backward at %.2f, the tile backward at %.2f" % (
                copy / med["c act forward"],
                6 * copy / (4 * med["c act backward (row path)"]),
                8 * copy / (4 * med["d act backward tile (du, du^T)"])))
        k1, k2 = ("d act backward tile (du, du^T)",
                  "d act backward + transpose_colsum")
        margin = spread(times[k1]) + spread(times[k2])
        say("  du^T: tile %.1f us, backward + transpose_colsum %.1f us: %s" % (
            med[k1], med[k2], "tile wins" if med[k1] + margin < med[k2] else
            "transpose_colsum wins" if med[k2] + margin < med[k1] else
            "within the spreads"))
        del vs
        torch.cuda.empty_cache()
    print(json.dumps({"bench": "ffn", "rows": rows}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
