#!/usr/bin/env python
"""Same-process A/B of the recurrent layer (docs/OPS.md "Recurrent layers"):

  a  fused     ops.lstm_fwd / ops.lstm_bwd (one step kernel per time step)
  b  unfused   the same layer composed from existing ops: the projection
               GEMM, then per step ops.gemm into a float32 buffer plus torch
               pointwise ops (backward: per step ops.gemm plus pointwise,
               the same three gradient GEMMs)
  c  torch     torch.nn.LSTM in bfloat16 on the same device

for the forward and for forward + backward, each timed eager and as a
replayed graph.  All variants live in one process and are interleaved round
by round; the first round is not timed; medians and minima are reported.  A
variant stops being timed once it has used its time limit.

``--cell gru`` runs the same three variants of the GRU layer (ops.gru_fwd /
ops.gru_bwd, the composition from existing ops, torch.nn.GRU); the default
is the LSTM run.

    python tools/bench_recurrent.py [--cell lstm|gru] [--rounds 20]
                                    [--limit 60] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from veles_amd import ops  # noqa: E402

SHAPES = [(256, 64, 512, 512), (64, 128, 1024, 1024), (32, 32, 128, 128)]
DEV = "cuda"
BF = torch.bfloat16


class Unfused(object):
    """variant b: what a user could build before the step kernels"""

    def __init__(self, B, T, I, H):
        self.s = (B, T, I, H)
        self.xg = torch.empty(B, T, 4 * H, device=DEV)
        self.pre = torch.empty(B, 4 * H, device=DEV)
        self.h = torch.zeros(B, T, H, dtype=BF, device=DEV)
        self.c = torch.zeros(B, T, H, device=DEV)
        self.g = torch.zeros(B, T, 4 * H, dtype=BF, device=DEV)
        self.dg = torch.zeros(B, T, 4 * H, dtype=BF, device=DEV)
        self.dh = torch.empty(B, H, device=DEV)
        self.hp = torch.zeros(B, T, H, dtype=BF, device=DEV)

    def fwd(self, x, w, bias):
        B, T, I, H = self.s
        ops.gemm(x.view(B * T, I), w[:, :I], trans_b=True, bias=bias,
                 out=self.xg.view(B * T, 4 * H))
        wh = w[:, I:]
        for t in range(T):
            pre = self.xg[:, t]
            if t:
                ops.gemm(self.h[:, t - 1], wh, trans_b=True, out=self.pre)
                pre = pre + self.pre
            i, f, g, o = pre.split(H, 1)
            i, f, g, o = i.sigmoid(), f.sigmoid(), g.tanh(), o.sigmoid()
            c = i * g if not t else f * self.c[:, t - 1] + i * g
            self.c[:, t] = c
            self.h[:, t] = o * c.tanh()
            self.g[:, t] = torch.cat((i, f, g, o), 1)
        return self.h

    def bwd(self, err, x, w, dw, db):
        B, T, I, H = self.s
        wh = w[:, I:]
        dc = torch.zeros(B, H, device=DEV)
        for t in range(T - 1, -1, -1):
            dh = err[:, t].float()
            if t < T - 1:
                ops.gemm(self.dg[:, t + 1], wh, out=self.dh)
                dh = dh + self.dh
            i, f, g, o = self.g[:, t].float().split(H, 1)
            tc = self.c[:, t].tanh()
            dc = dc + dh * o * (1 - tc * tc)
            cp = self.c[:, t - 1] if t else torch.zeros_like(dc)
            self.dg[:, t] = torch.cat((dc * g * i * (1 - i),
                                       dc * cp * f * (1 - f),
                                       dc * i * (1 - g * g),
                                       dh * tc * o * (1 - o)), 1)
            dc = dc * f
        dg2 = self.dg.view(B * T, 4 * H)
        self.hp[:, 1:].copy_(self.h[:, :T - 1])
        ops.gemm(dg2, x.view(B * T, I), trans_a=True, out=dw[:, :I],
                 accumulate="overwrite", bias_grad=db)
        ops.gemm(dg2, self.hp.view(B * T, H), trans_a=True, out=dw[:, I:],
                 accumulate="overwrite")
        return ops.gemm(dg2, w[:, :I])


class UnfusedGRU(object):
    """variant b of the GRU: gate order r, z, n; bias (b_r, b_z, b_n, b_hn)"""

    def __init__(self, B, T, I, H):
        self.s = (B, T, I, H)
        self.xg = torch.empty(B, T, 3 * H, device=DEV)
        self.pre = torch.empty(B, 3 * H, device=DEV)
        self.h = torch.zeros(B, T, H, dtype=BF, device=DEV)
        self.hf = torch.zeros(B, T, H, device=DEV)
        self.hn = torch.zeros(B, T, H, device=DEV)
        self.g = torch.zeros(B, T, 3 * H, dtype=BF, device=DEV)
        self.dgx = torch.zeros(B, T, 3 * H, dtype=BF, device=DEV)
        self.dgh = torch.zeros(B, T, 3 * H, dtype=BF, device=DEV)
        self.dh = torch.empty(B, H, device=DEV)
        self.hp = torch.zeros(B, T, H, dtype=BF, device=DEV)

    def fwd(self, x, w, bias):
        B, T, I, H = self.s
        ops.gemm(x.view(B * T, I), w[:, :I], trans_b=True, bias=bias[:3 * H],
                 out=self.xg.view(B * T, 3 * H))
        wh, bhn = w[:, I:], bias[3 * H:]
        for t in range(T):
            xr, xz, xn = self.xg[:, t].split(H, 1)
            if t:
                ops.gemm(self.h[:, t - 1], wh, trans_b=True, out=self.pre)
                hr, hz, hn = self.pre.split(H, 1)
                r, z, hn = (xr + hr).sigmoid(), (xz + hz).sigmoid(), hn + bhn
            else:
                r, z, hn = xr.sigmoid(), xz.sigmoid(), bhn.expand(B, H)
            n = (xn + r * hn).tanh()
            h = (1 - z) * n
            if t:
                h = h + z * self.hf[:, t - 1]
            self.hf[:, t] = h
            self.hn[:, t] = hn
            self.h[:, t] = h
            self.g[:, t] = torch.cat((r, z, n), 1)
        return self.h

    def bwd(self, err, x, w, dw, db):
        B, T, I, H = self.s
        wh = w[:, I:]
        dc = torch.zeros(B, H, device=DEV)
        for t in range(T - 1, -1, -1):
            dh = err[:, t].float() + dc
            if t < T - 1:
                ops.gemm(self.dgh[:, t + 1], wh, out=self.dh)
                dh = dh + self.dh
            r, z, n = self.g[:, t].float().split(H, 1)
            dn = dh * (1 - z) * (1 - n * n)
            hp = self.hf[:, t - 1] if t else torch.zeros_like(dc)
            dz = dh * (hp - n) * z * (1 - z)
            dr = dn * self.hn[:, t] * r * (1 - r)
            self.dgx[:, t] = torch.cat((dr, dz, dn), 1)
            self.dgh[:, t] = torch.cat((dr, dz, dn * r), 1)
            dc = dh * z
        gx = self.dgx.view(B * T, 3 * H)
        gh = self.dgh.view(B * T, 3 * H)
        self.hp[:, 1:].copy_(self.h[:, :T - 1])
        ops.gemm(gx, x.view(B * T, I), trans_a=True, out=dw[:, :I],
                 accumulate="overwrite", bias_grad=db[:3 * H])
        ops.gemm(gh, self.hp.view(B * T, H), trans_a=True, out=dw[:, I:],
                 accumulate="overwrite")
        ops.col_sum(gh[:, 2 * H:].contiguous(), out=db[3 * H:])
        return ops.gemm(gx, w[:, :I])


def variants_gru(B, T, I, H):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, T, I, generator=g).to(BF).to(DEV)
    w = (torch.randn(3 * H, I + H, generator=g) / (I + H) ** 0.5).to(BF) \
        .to(DEV)
    bias = torch.zeros(4 * H, device=DEV)
    err = torch.randn(B, T, H, generator=g).to(BF).to(DEV)
    dw = torch.zeros(3 * H, I + H, device=DEV)
    db = torch.zeros(4 * H, device=DEV)
    save, ei = {}, torch.empty(B, T, I, dtype=BF, device=DEV)
    un = UnfusedGRU(B, T, I, H)
    ref = torch.nn.GRU(I, H, batch_first=True).to(DEV).to(BF)
    xr = x.clone().requires_grad_()
    params = [xr] + list(ref.parameters())

    def a_f():
        ops.gru_fwd(x, w, bias, H, return_sequences=True, save=save)

    def a_fb():
        a_f()
        ops.gru_bwd(err, x, w, save, dw, db, err_input=ei)

    def b_f():
        un.fwd(x, w, bias)

    def b_fb():
        un.fwd(x, w, bias)
        un.bwd(err, x, w, dw, db)

    def c_f():
        with torch.no_grad():
            ref(x)

    def c_fb():
        y, _ = ref(xr)
        torch.autograd.grad(y, params, err)

    return {"a fused fwd": a_f, "b unfused fwd": b_f, "c torch fwd": c_f,
            "a fused fwd+bwd": a_fb, "b unfused fwd+bwd": b_fb,
            "c torch fwd+bwd": c_fb}


def variants(B, T, I, H):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, T, I, generator=g).to(BF).to(DEV)
    w = (torch.randn(4 * H, I + H, generator=g) / (I + H) ** 0.5).to(BF) \
        .to(DEV)
    bias = torch.zeros(4 * H, device=DEV)
    err = torch.randn(B, T, H, generator=g).to(BF).to(DEV)
    dw = torch.zeros(4 * H, I + H, device=DEV)
    db = torch.zeros(4 * H, device=DEV)
    save, ei = {}, torch.empty(B, T, I, dtype=BF, device=DEV)
    un = Unfused(B, T, I, H)
    ref = torch.nn.LSTM(I, H, batch_first=True).to(DEV).to(BF)
    xr = x.clone().requires_grad_()
    params = [xr] + list(ref.parameters())

    def a_f():
        ops.lstm_fwd(x, w, bias, H, return_sequences=True, save=save)

    def a_fb():
        a_f()
        ops.lstm_bwd(err, x, w, save, dw, db, err_input=ei)

    def b_f():
        un.fwd(x, w, bias)

    def b_fb():
        un.fwd(x, w, bias)
        un.bwd(err, x, w, dw, db)

    def c_f():
        with torch.no_grad():
            ref(x)

    def c_fb():
        y, _ = ref(xr)
        torch.autograd.grad(y, params, err)

    return {"a fused fwd": a_f, "b unfused fwd": b_f, "c torch fwd": c_f,
            "a fused fwd+bwd": a_fb, "b unfused fwd+bwd": b_fb,
            "c torch fwd+bwd": c_fb}


def graphed(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), \
        torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3   # microseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--limit", type=float, default=60.0)
    ap.add_argument("--out")
    ap.add_argument("--cell", choices=("lstm", "gru"), default="lstm")
    args = ap.parse_args()
    ops.require_library()
    make = variants_gru if args.cell == "gru" else variants
    lines = ["cell %s" % args.cell,
             "device %s, %d rounds after one untimed, time limit %g s per "
             "variant; microseconds, median (minimum)" %
             (torch.cuda.get_device_name(0), args.rounds, args.limit)]
    for shape in SHAPES:
        runs = {}
        for name, fn in make(*shape).items():
            runs[name + " eager"] = fn
            try:
                runs[name + " graph"] = graphed(fn)
            except Exception as e:  # noqa: BLE001 - reported, not hidden
                torch.cuda.synchronize()
                lines.append("  %s graph: capture failed (%s)" %
                             (name, str(e).splitlines()[0][:80]))
        times = {k: [] for k in runs}
        spent = {k: 0.0 for k in runs}
        for r in range(args.rounds + 1):
            for k, fn in runs.items():      # interleaved
                if spent[k] > args.limit:
                    continue
                t0 = time.time()
                us = timed(fn)
                spent[k] += time.time() - t0
                if r:
                    times[k].append(us)
        lines.append("B%d T%d I%d H%d" % shape)
        for k in runs:
            v = times[k]
            lines.append("  %-26s %9.1f (%9.1f)  n=%d" % (
                k, statistics.median(v), min(v), len(v)) if v else
                "  %-26s no timed round" % k)
        print("\n".join(lines[-len(runs) - 1:]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
