"""Times self-attention (the core: q, k, v -> o and do -> dq, dk, dv; bf16) on
one GPU at four shapes (B, T, NH, D), causal and not, Gaussian data:

    (a) this project's fused kernels: ops.attention_fwd / attention_bwd on
        column slices of one fused [B*T][3E] buffer
    (b) the unfused composition in torch: matmul / softmax / matmul in bf16
        with autograd (it materialises the [B][NH][T][T] scores)
    (c) torch.nn.functional.scaled_dot_product_attention in bf16; the SDPA
        backends that run here are listed (torch takes the first of flash,
        memory-efficient, math that does)

each forward and forward + backward, eager and as a replayed graph.  One
process, the variants interleaved in every round, the first round untimed,
median and min - max over the rounds; a round times ``calls`` back-to-back
calls between two device events.  TF/s counts 4 B NH T^2 D FLOPs for the
forward and 10 for the backward's five products (halved under the causal
mask), whatever the variant computes.

Acceptance (docs/OPS.md "Attention"): at every shape the forward + backward
median of (a) is below (b)'s by more than the two round-to-round spreads
(max - min) added together.

    python tools/bench_attention.py [--rounds 7] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from veles_amd import ops  # noqa: E402

SHAPES = [(256, 32, 4, 32), (64, 128, 8, 64), (16, 512, 8, 64),
          (8, 2048, 16, 128)]


def sdpa_backends(dev):
    """names of the SDPA backends that run a small bf16 case here"""
    try:
        from torch.nn.attention import SDPBackend, sdpa_kernel
    except ImportError:
        return ["unknown (no torch.nn.attention)"]
    q = torch.randn(2, 2, 64, 64, device=dev, dtype=torch.bfloat16)
    ok = []
    for name in ("FLASH_ATTENTION", "EFFICIENT_ATTENTION", "MATH"):
        b = getattr(SDPBackend, name, None)
        if b is None:
            continue
        try:
            with sdpa_kernel([b]):
                F.scaled_dot_product_attention(q, q, q)
            torch.cuda.synchronize()
            ok.append(name)
        except Exception:  # noqa: BLE001 - a backend that is not built in
            pass
    return ok


def graphed(fn):
    """fn captured once (after a warm-up on a side stream) -> its replay, or
    None when the capture fails"""
    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fn()
            fn()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        g.replay()
        torch.cuda.synchronize()
        return g.replay
    except Exception as e:  # noqa: BLE001
        print("  (no graph: %s)" % str(e).splitlines()[0][:100])
        torch.cuda.synchronize()
        return None


def variants(B, T, NH, D, causal, dev):
    E = NH * D
    gen = torch.Generator(device=dev).manual_seed(1)
    qkv = torch.randn(B, T, 3 * E, device=dev, generator=gen).bfloat16()
    do = torch.randn(B, T, E, device=dev, generator=gen).bfloat16()
    q, k, v = (qkv[:, :, n * E:(n + 1) * E] for n in range(3))
    o = torch.empty(B, T, E, dtype=torch.bfloat16, device=dev)
    dqkv = torch.empty_like(qkv)
    dq, dk, dv = (dqkv[:, :, n * E:(n + 1) * E] for n in range(3))
    save, ws = {}, {}

    def a_fwd():
        ops.attention_fwd(q, k, v, NH, causal=causal, out=o, save=save)

    def a_both():
        a_fwd()
        ops.attention_bwd(do, q, k, v, o, save, NH, causal=causal, dq=dq,
                          dk=dk, dv=dv, ws=ws)

    # torch: the same memory as [B][NH][T][D] views
    th = [t.view(B, T, NH, D).transpose(1, 2).detach().requires_grad_(True)
          for t in (q, k, v)]
    tdo = do.view(B, T, NH, D).transpose(1, 2)
    scale = 1.0 / math.sqrt(D)
    mask = torch.ones(T, T, device=dev).triu(1).bool() if causal else None

    def unfused():
        s = (th[0] @ th[1].transpose(2, 3)) * scale
        if causal:
            s = s.masked_fill(mask, float("-inf"))
        return torch.softmax(s, 3) @ th[2]

    def sdpa():
        return F.scaled_dot_product_attention(*th, is_causal=causal)

    def fwd_of(f):
        def run():
            with torch.no_grad():
                f()
        return run

    def both_of(f):
        def run():
            torch.autograd.grad(f(), th, tdo)
        return run

    out = []
    for name, f, b in (("a fused", a_fwd, a_both),
                       ("b unfused torch", fwd_of(unfused), both_of(unfused)),
                       ("c torch sdpa", fwd_of(sdpa), both_of(sdpa))):
        for what, fn in (("fwd", f), ("fwd+bwd", b)):
            out.append(("%s %s eager" % (name, what), what, fn))
            g = graphed(fn)
            if g is not None:
                out.append(("%s %s graph" % (name, what), what, g))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=None,
                    help="indices into SHAPES, e.g. 0,1")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_attention needs the GPU")
    ops.require_library()
    dev = torch.device("cuda", 0)
    lines, rows = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("%d rounds per variant, first round untimed; SDPA backends that run "
        "here: %s" % (a.rounds, ", ".join(sdpa_backends(dev)) or "none"))
    shapes = SHAPES if a.shapes is None else \
        [SHAPES[int(i)] for i in a.shapes.split(",")]
    for B, T, NH, D in shapes:
        for causal in (False, True):
            vs = variants(B, T, NH, D, causal, dev)
            flop = 4.0 * B * NH * T * T * D * (0.5 if causal else 1.0)
            calls = max(2, min(50, int(2e10 / flop)))
            times = {name: [] for name, _, _ in vs}
            for rnd in range(a.rounds + 1):
                for name, _, fn in vs:
                    fn()
                    t0, t1 = (torch.cuda.Event(enable_timing=True)
                              for _ in "01")
                    t0.record()
                    for _ in range(calls):
                        fn()
                    t1.record()
                    t1.synchronize()
                    if rnd:
                        times[name].append(t0.elapsed_time(t1) * 1e3 / calls)
            say("B %d T %d NH %d D %d%s: %d calls per round" % (
                B, T, NH, D, " causal" if causal else "", calls))
            say("  %-34s %10s %10s %10s %8s" % (
                "variant", "median us", "min us", "max us", "TF/s"))
            med = {}
            for name, what, _ in vs:
                t = times[name]
                f = flop * (3.5 if what == "fwd+bwd" else 1.0)
                row = {"shape": [B, T, NH, D], "causal": causal,
                       "variant": name, "median_us": statistics.median(t),
                       "min_us": min(t), "max_us": max(t), "rounds_us": t,
                       "tf_per_s": f / statistics.median(t) / 1e6}
                rows.append(row)
                med[name] = row
                say("  %-34s %10.1f %10.1f %10.1f %8.1f" % (
                    name, row["median_us"], row["min_us"], row["max_us"],
                    row["tf_per_s"]))
            for mode in ("eager", "graph"):
                ra = med.get("a fused fwd+bwd " + mode)
                rb = med.get("b unfused torch fwd+bwd " + mode)
                rc = med.get("c torch sdpa fwd+bwd " + mode)
                if ra and rb:
                    spread = (ra["max_us"] - ra["min_us"]) + \
                        (rb["max_us"] - rb["min_us"])
                    gain = rb["median_us"] - ra["median_us"]
                    say("  fwd+bwd %s: (b) - (a) = %.1f us, spreads added "
                        "%.1f us: %s; (b) / (a) = %.2f%s" % (
                            mode, gain, spread,
                            "accepted" if gain > spread else "NOT accepted",
                            rb["median_us"] / ra["median_us"],
                            "" if not rc else ", (c) / (a) = %.2f" % (
                                rc["median_us"] / ra["median_us"])))
            del vs
            torch.cuda.empty_cache()
    print(json.dumps({"bench": "attention", "rows": rows}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
