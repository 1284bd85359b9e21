#!/usr/bin/env python
"""Same-process A/B of the bidirectional recurrent layer (docs/OPS.md
"Bidirectional"), the method of tools/bench_recurrent.py:

  a   paired    ops.lstm_fwd / lstm_bwd (gru_fwd / gru_bwd) with
                direction="both": T paired step launches per pass
  b   composed  what a user could build before: two one-direction op calls,
                on x and on the time-flipped x, plus the flip and concat
                copies (forward: flip x, flip back, concat; backward: split
                and flip err, flip and add err_input)
  b'  chain     the buffers and GEMMs of (a), but 2T one-direction launches
                through the existing entry points
                (ops.set_birecurrent_paired(False)): isolates the paired launch
  c   torch     torch.nn.LSTM / GRU(bidirectional=True) in bfloat16

for the forward and for forward + backward, each timed eager and as a
replayed graph.  One process, variants interleaved round by round (each
round starts one variant further on), the first round untimed; median,
minimum and the interquartile range (the same-process spread) are reported.  ``--only b`` runs variant (b) alone, e.g. on another
library through HVK_LIBRARY (it uses no entry point the parent lacks).

    python tools/bench_birecurrent.py [--cell lstm|gru] [--rounds 20]
                                      [--limit 30] [--only a,b,b',c]
                                      [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_recurrent import SHAPES, DEV, BF, graphed, timed  # noqa: E402
from veles_amd import ops  # noqa: E402

NG = {"lstm": 4, "gru": 3}
TORCH = {"lstm": torch.nn.LSTM, "gru": torch.nn.GRU}


def variants(cell, B, T, I, H):
    ng = NG[cell] * H
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, T, I, generator=g).to(BF).to(DEV)
    w = (torch.randn(2 * ng, I + H, generator=g) / (I + H) ** 0.5).to(BF) \
        .to(DEV)
    bias = torch.zeros(8 * H, device=DEV)
    err = torch.randn(B, T, 2 * H, generator=g).to(BF).to(DEV)
    dw = torch.zeros(2 * ng, I + H, device=DEV)
    db = torch.zeros(8 * H, device=DEV)
    ei = torch.empty(B, T, I, dtype=BF, device=DEV)
    if cell == "gru":
        fwd, bwd = ops.gru_fwd, ops.gru_bwd
    else:
        fwd, bwd = ops.lstm_fwd, ops.lstm_bwd
    sa, sc, sf, sr = {}, {}, {}, {}
    eif, eir = torch.empty_like(ei), torch.empty_like(ei)
    ref = TORCH[cell](I, H, batch_first=True, bidirectional=True).to(DEV) \
        .to(BF)
    xr = x.clone().requires_grad_()
    params = [xr] + list(ref.parameters())

    def a_f(save=sa):
        fwd(x, w, bias, H, return_sequences=True, save=save,
            direction="both")

    def a_fb(save=sa):
        a_f(save)
        bwd(err, x, w, save, dw, db, err_input=ei, direction="both")

    def chain(fn):
        def run():
            old = ops.set_birecurrent_paired(False)
            try:
                fn(sc)
            finally:
                ops.set_birecurrent_paired(old)
        return run

    def b_f():
        xf = x.flip(1)
        yf = fwd(x, w[:ng], bias[:4 * H], H, return_sequences=True, save=sf)
        yr = fwd(xf, w[ng:], bias[4 * H:], H, return_sequences=True, save=sr)
        return xf, torch.cat((yf, yr.flip(1)), 2)

    def b_fb():
        xf, _ = b_f()
        ef = err[:, :, :H].contiguous()
        er = err[:, :, H:].flip(1)
        bwd(ef, x, w[:ng], sf, dw[:ng], db[:4 * H], err_input=eif)
        bwd(er, xf, w[ng:], sr, dw[ng:], db[4 * H:], err_input=eir)
        return eif + eir.flip(1)

    def c_f():
        with torch.no_grad():
            ref(x)

    def c_fb():
        y, _ = ref(xr)
        torch.autograd.grad(y, params, err)

    return {"a paired fwd": a_f, "b composed fwd": b_f,
            "b' chain fwd": chain(a_f), "c torch fwd": c_f,
            "a paired fwd+bwd": a_fb, "b composed fwd+bwd": b_fb,
            "b' chain fwd+bwd": chain(a_fb), "c torch fwd+bwd": c_fb}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--limit", type=float, default=30.0)
    ap.add_argument("--out")
    ap.add_argument("--cell", choices=("lstm", "gru"), default="lstm")
    ap.add_argument("--only", default="a,b,b',c")
    args = ap.parse_args()
    ops.require_library()
    only = set(args.only.split(","))
    lines = ["cell %s bidirectional, library %s" %
             (args.cell, os.environ.get("HVK_LIBRARY", "(the tree's)")),
             "device %s, %d rounds after one untimed, time limit %g s per "
             "variant; microseconds, median (minimum) [interquartile range]"
             % (torch.cuda.get_device_name(0), args.rounds, args.limit)]
    for shape in SHAPES:
        runs = {}
        for name, fn in variants(args.cell, *shape).items():
            if name.split()[0] not in only:
                continue
            runs[name + " eager"] = fn
            try:
                runs[name + " graph"] = graphed(fn)
            except Exception as e:  # noqa: BLE001 - reported, not hidden
                torch.cuda.synchronize()
                lines.append("  %s graph: capture failed (%s)" %
                             (name, str(e).splitlines()[0][:80]))
        times = {k: [] for k in runs}
        spent = {k: 0.0 for k in runs}
        order = list(runs.items())
        for r in range(args.rounds + 1):
            # interleaved; every round starts one variant further on, so that
            # no variant is always the one that follows the slowest
            for k, fn in order[r % len(order):] + order[:r % len(order)]:
                if spent[k] > args.limit:
                    continue
                t0 = time.time()
                us = timed(fn)
                spent[k] += time.time() - t0
                if r:
                    times[k].append(us)
        lines.append("B%d T%d I%d H%d" % shape)
        for k in runs:
            v = sorted(times[k])
            if len(v) < 4:
                lines.append("  %-28s too few timed rounds (%d)" % (k, len(v)))
                continue
            q = statistics.quantiles(v, n=4)
            lines.append("  %-28s %9.1f (%9.1f) [%7.1f]  n=%d" % (
                k, statistics.median(v), v[0], q[2] - q[0], len(v)))
        print("\n".join(lines[-len(runs) - 1:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
