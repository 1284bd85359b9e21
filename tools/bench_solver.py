"""Times the fused update kernels at AlexNet's size on one GPU: 61 M float32
parameters with a bf16 copy, AlexNet's 16 segments (8 layers, weights and
bias, laid out as the parameter store does).

    (a) hvk_sgd4            momentum SGD, the yardstick      22 B / parameter
    (b) solver4_kernel      Adam, float4                     30 B / parameter
    (c) solver1_kernel      Adam, the scalar twin            30 B / parameter
    (d) torch.optim.Adam    fused (or foreach) on one tensor 28 B / parameter
    (e) ops.grad_sqnorm against torch.linalg.vector_norm      4 B / parameter

One process, the variants interleaved in every round, the first round
untimed, median and minimum over seven rounds; a round times ``--calls``
back-to-back launches of a variant between two device events.

    python tools/bench_solver.py [--rounds 7] [--calls 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from veles_amd import ops  # noqa: E402

# (weights, bias) element counts of AlexNet's eight layers, forward order
ALEXNET = [(96 * 11 * 11 * 3, 96), (256 * 5 * 5 * 48, 256),
           (384 * 3 * 3 * 256, 384), (384 * 3 * 3 * 192, 384),
           (256 * 3 * 3 * 192, 256), (4096 * 9216, 4096),
           (4096 * 4096, 4096), (1000 * 4096, 1000)]


def layout():
    """[(begin, end)] of the 16 parameters in reverse forward order, each
    64-element aligned (ParameterStore.finalize), and the buffer length."""
    off, spans = 0, []
    for w, b in reversed(ALEXNET):
        for size in (b, w):
            off = (off + 63) // 64 * 64
            spans.append((off, off + size))
            off += size
    return spans, (off + 3) // 4 * 4


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_solver needs the GPU")
    ops.require_library()
    lib = ops._lib.lib()
    dev = torch.device("cuda", 0)
    spans, n = layout()
    nparam = sum(e - b for b, e in spans)
    g = torch.Generator(device=dev).manual_seed(1)
    w = torch.randn(n, device=dev, generator=g) * 0.01
    grad = torch.randn(n, device=dev, generator=g) * 1e-3
    s1, s2 = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    lp = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    sgd = ops._segs_tensor(ops._pack_sgd_segs(
        [(b, e, 1e-2, 5e-4, 0.0, 0.9) for b, e in spans]), dev)
    adam = ops._segs_tensor(ops._pack_solver_segs(
        [(b, e, 1e-3, 5e-4, 0.0, 0.9, ops.SOLVERS["adam"], 1e-8, 0.999)
         for b, e in spans], step=10), dev)
    p = ops._p
    stream = torch.cuda.current_stream(dev).cuda_stream
    tw = torch.nn.Parameter(w.clone())
    tw.grad = grad.clone()
    try:
        topt, tname = torch.optim.Adam([tw], lr=1e-3, weight_decay=5e-4,
                                       fused=True), "fused"
        topt.step()
    except (RuntimeError, TypeError):
        topt, tname = torch.optim.Adam([tw], lr=1e-3, weight_decay=5e-4,
                                       foreach=True), "foreach"
    sq, ws = torch.zeros(1, device=dev), torch.zeros(2048, device=dev)

    def solver4(variant):
        def run():
            lib.hvk_set_gemm_variant(variant)
            rc = lib.hvk_solver4(p(w), p(grad), p(s1), p(s2), p(lp), p(adam),
                                 len(spans), n, 1.0, n, None, 0.0, stream)
            lib.hvk_set_gemm_variant(-1)
            assert rc == 0, rc
        return run

    def sgd4():
        rc = lib.hvk_sgd4(p(w), p(grad), p(s1), p(lp), p(sgd), len(spans), n,
                          1.0, n, stream)
        assert rc == 0, rc

    variants = [
        ("a hvk_sgd4 (momentum)", 22, sgd4),
        ("b adam solver4_kernel", 30, solver4(-1)),
        ("c adam solver1_kernel", 30, solver4(67)),
        ("d torch.optim.Adam %s" % tname, 28, topt.step),
        ("e ops.grad_sqnorm", 4, lambda: ops.grad_sqnorm(grad, out=sq,
                                                         ws=ws)),
        ("e torch.linalg.vector_norm", 4,
         lambda: torch.linalg.vector_norm(grad)),
    ]
    times = {name: [] for name, _, _ in variants}
    for rnd in range(a.rounds + 1):
        for name, _, fn in variants:
            fn()
            t0, t1 = (torch.cuda.Event(enable_timing=True) for _ in "01")
            t0.record()
            for _ in range(a.calls):
                fn()
            t1.record()
            t1.synchronize()
            if rnd:                      # the first round is untimed
                times[name].append(t0.elapsed_time(t1) * 1e3 / a.calls)
    assert torch.isfinite(w).all() and torch.isfinite(tw).all()
    rows = []
    print("%d parameters in %d segments, buffer of %d; %d rounds x %d calls"
          % (nparam, len(spans), n, a.rounds, a.calls))
    print("%-30s %10s %10s %10s %12s" % ("variant", "median us", "min us",
                                         "max us", "TB/s at min"))
    for name, bpp, _ in variants:
        t = times[name]
        row = {"variant": name, "bytes_per_param": bpp,
               "median_us": statistics.median(t), "min_us": min(t),
               "max_us": max(t), "rounds_us": t,
               "tb_per_s_at_min": bpp * n / min(t) / 1e6}
        rows.append(row)
        print("%-30s %10.1f %10.1f %10.1f %12.2f" % (
            name, row["median_us"], row["min_us"], row["max_us"],
            row["tb_per_s_at_min"]))
    print(json.dumps({"bench": "solver", "parameters": nparam, "rows": rows}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"parameters": nparam, "buffer": n, "rows": rows}, f,
                      indent=1)


if __name__ == "__main__":
    main()
