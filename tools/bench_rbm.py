#!/usr/bin/env python
"""Same-process A/B of one whole CD-1 step of a restricted Boltzmann machine
(docs/OPS.md "Restricted Boltzmann machines"):

  a  fused     3 x ops.rbm_sample, ops.rbm_grad, ops.sgd_update,
               ops.seed_advance
  b  composed  the same step from the ops that existed before: ops.gemm with
               the sigmoid epilogue, a torch compare against torch.rand for
               every draw, two ops.gemm for the statistics (the negative one
               accumulating) plus torch column sums, ops.sgd_update
  c  torch     plain torch in bfloat16 (matmul, sigmoid, rand, SGD with
               momentum as tensor expressions)

each timed eager and as a replayed graph.  All variants live in one process
and are interleaved round by round; the first round is not timed; medians
and minima are reported.  A variant stops being timed once it has used its
time limit.  The draws of b and c come from torch's generator, so the arms
agree in distribution, not bit for bit.

    python tools/bench_rbm.py [--rounds 30] [--limit 30] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from veles_amd import ops  # noqa: E402

SHAPES = [(30, 16, 16), (128, 784, 1024), (4096, 784, 1024),
          (1024, 4096, 4096)]
DEV = "cuda"
BF = torch.bfloat16
LR, MOM = 0.1, 0.5


def variants(B, V, H):
    g = torch.Generator().manual_seed(0)
    v0 = (torch.rand(B, V, generator=g) < 0.5).to(BF).to(DEV)
    w0 = ((torch.rand(H, V, generator=g) * 2 - 1) * 0.05)
    off_hb, off_vb, total = ops.rbm_layout(V, H)
    segs = [(0, H * V, LR, 0.0, 0.0, MOM), (off_hb, off_hb + H, LR, 0.0, 0.0,
                                            MOM),
            (off_vb, off_vb + V, LR, 0.0, 0.0, MOM)]

    def flat():
        p = torch.zeros(total, device=DEV)
        p[:H * V] = w0.to(DEV).view(-1)
        return p, torch.zeros(total, device=DEV), \
            torch.zeros(total, device=DEV), p.to(BF)

    def bufs():
        return [torch.zeros(B, n, dtype=BF, device=DEV)
                for n in (H, H, H, V, V)]

    # ---- a: the fused ops
    pa, ma, ga, la = flat()
    ph0, h0, phk, pv, v1 = bufs()
    sd = torch.tensor([1234], dtype=torch.int32, device=DEV)
    wa, hba, vba = la[:H * V].view(H, V), pa[off_hb:off_hb + H], \
        pa[off_vb:off_vb + V]

    def a():
        ops.rbm_sample(v0, wa, hba, probs=ph0, sample=h0, seed_dev=sd)
        ops.rbm_sample(h0, wa, vba, transposed=True, probs=pv, sample=v1,
                       seed_dev=sd, base=B * H)
        ops.rbm_sample(v1, wa, hba, probs=phk, seed_dev=sd)
        ops.rbm_grad(v0, ph0, v1, phk, ga)
        ops.sgd_update(pa, ga, ma, segs, w_lp=la)
        ops.seed_advance(sd)

    # ---- b: composed from the ops that existed before
    pb, mb, gb, lb = flat()
    qh0, g0, qhk, qv, g1 = bufs()
    wb, hbb, vbb = lb[:H * V].view(H, V), pb[off_hb:off_hb + H], \
        pb[off_vb:off_vb + V]
    gw = gb[:H * V].view(H, V)

    def b():
        ops.gemm(v0, wb, trans_b=True, bias=hbb, act="sigmoid", out=qh0)
        g0.copy_(torch.rand(B, H, device=DEV) < qh0)
        ops.gemm(g0, wb, bias=vbb, act="sigmoid", out=qv)
        g1.copy_(torch.rand(B, V, device=DEV) < qv)
        ops.gemm(g1, wb, trans_b=True, bias=hbb, act="sigmoid", out=qhk)
        ops.gemm(qh0, v0, trans_a=True, out=gw, alpha=-1.0 / B,
                 accumulate="overwrite")
        ops.gemm(qhk, g1, trans_a=True, out=gw, alpha=1.0 / B,
                 accumulate=True)
        gb[off_hb:off_hb + H] = (qhk.float() - qh0.float()).sum(0) / B
        gb[off_vb:off_vb + V] = (g1.float() - v0.float()).sum(0) / B
        ops.sgd_update(pb, gb, mb, segs, w_lp=lb)

    # ---- c: plain torch
    wc = w0.to(DEV).to(BF)
    hbc, vbc = torch.zeros(H, dtype=BF, device=DEV), \
        torch.zeros(V, dtype=BF, device=DEV)
    mw, mh, mv = torch.zeros_like(wc), torch.zeros_like(hbc), \
        torch.zeros_like(vbc)

    def c():
        p0 = torch.sigmoid(v0 @ wc.t() + hbc)
        s0 = (torch.rand(B, H, device=DEV) < p0).to(BF)
        p1 = torch.sigmoid(s0 @ wc + vbc)
        s1 = (torch.rand(B, V, device=DEV) < p1).to(BF)
        pk = torch.sigmoid(s1 @ wc.t() + hbc)
        mw.mul_(MOM).add_((p0.t() @ v0 - pk.t() @ s1) * (LR / B))
        mh.mul_(MOM).add_((p0 - pk).sum(0) * (LR / B))
        mv.mul_(MOM).add_((v0 - s1).sum(0) * (LR / B))
        wc.add_(mw)
        hbc.add_(mh)
        vbc.add_(mv)

    return {"a fused": a, "b composed": b, "c torch": c}


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
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--limit", type=float, default=30.0)
    ap.add_argument("--out")
    args = ap.parse_args()
    ops.require_library()
    lines = ["device %s, %d rounds after one untimed, time limit %g s per "
             "variant; one CD-1 step, microseconds, median (minimum)" %
             (torch.cuda.get_device_name(0), args.rounds, args.limit)]
    for shape in SHAPES:
        runs = {}
        for name, fn in variants(*shape).items():
            try:
                fn()
                torch.cuda.synchronize()
            except Exception as e:  # noqa: BLE001 - reported, not hidden
                lines.append("  %s: failed (%s)" %
                             (name, str(e).splitlines()[0][:80]))
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
        for r in range(args.rounds + 1):
            for k, fn in runs.items():      # interleaved
                if spent[k] > args.limit:
                    continue
                t0 = time.time()
                us = timed(fn)
                spent[k] += time.time() - t0
                if r:
                    times[k].append(us)
        lines.append("B%d V%d H%d" % shape)
        for k in runs:
            v = times[k]
            lines.append("  %-20s %9.1f (%9.1f)  n=%d" % (
                k, statistics.median(v), min(v), len(v)) if v else
                "  %-20s no timed round" % k)
        print("\n".join(lines[-len(runs) - 1:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
