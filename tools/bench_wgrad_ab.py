"""Same-process A/B of the conv weight-gradient kernels on the AlexNet (and
VGG-16) layer shapes: the halo kernel (csrc/kernels/wgrad_halo.hip) against
the 128-row / T4 GEMM loops (ops.set_halo_wgrad(False)), interleaved round
by round in ONE process on random operands (cdna_hip_programming.md §5.4
rules 24-25), reporting the median TF/s per setting.

    python tools/bench_wgrad_ab.py [alexnet_batch] [rounds] [vgg_batch] [lean]

With a fourth argument ``lean`` the pair is the halo kernel's lean pixel
loop against its old loop (ops.set_halo_wgrad_lean(True / False)) instead:
per layer the median and minimum time of each, and for the layer sum the
old loop's own round-to-round spread next to the difference.  With
``stages`` the pair is the lean loop with one LDS array per stage against the
lean loop with both stages in one array (ops.set_halo_wgrad_stages), reported
the same way ("old" is then the one-array loop).

Writes gpurun_out/bench_wgrad_ab.json."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, ".")
import veles_amd.ops as ops  # noqa: E402

BF = torch.bfloat16


def timeit(fn, n=8, w=2):
    for _ in range(w):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e-3


def case(N, H, W, C, OC, k, p, g, st=1):
    OH, OW = ops.conv_out_size(H, W, k, k, (st, st), (p, p, p, p))
    x = (torch.rand(N, H, W, C, device="cuda") * 2 - 1).to(BF)
    dy = (torch.rand(N, OH, OW, OC, device="cuda") * 2 - 1).to(BF)
    dw = torch.zeros(OC, k, k, C // g, device="cuda")
    db = torch.zeros(OC, device="cuda")
    fl = 2.0 * N * OH * OW * OC * k * k * (C // g)
    return fl, lambda: ops.conv_wgrad(x, dy, dw, (st, st), (p, p, p, p), g,
                                      dbias=db)


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    VB = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    lean = len(sys.argv) > 4 and sys.argv[4] in ("lean", "stages")
    cases = [("alex_conv1", (B, 227, 227, 3, 96, 11, 0, 1, 4)),
             ("alex_conv2", (B, 27, 27, 96, 256, 5, 2, 2)),
             ("alex_conv3", (B, 13, 13, 256, 384, 3, 1, 1)),
             ("alex_conv4", (B, 13, 13, 384, 384, 3, 1, 2)),
             ("alex_conv5", (B, 13, 13, 384, 256, 3, 1, 2))]
    if VB:
        cases += [("vgg_conv1_2", (VB // 4, 224, 224, 64, 64, 3, 1, 1)),
                  ("vgg_conv2_2", (VB // 2, 112, 112, 128, 128, 3, 1, 1)),
                  ("vgg_conv3_2", (VB, 56, 56, 256, 256, 3, 1, 1)),
                  ("vgg_conv4_2", (VB, 28, 28, 512, 512, 3, 1, 1)),
                  ("vgg_conv5_2", (VB, 14, 14, 512, 512, 3, 1, 1))]
    out = {}
    if lean:   # the lean / old pair instead; the same output file
        setter = (ops.set_halo_wgrad_lean if sys.argv[4] == "lean"
                  else ops.set_halo_wgrad_stages)
        out, cases = main_lean(cases, rounds, setter, sys.argv[4]), []
    for name, shp in cases:
        fl, fn = case(*shp)
        res = {"halo": [], "gemm": []}
        for _ in range(rounds):
            for key, on in (("halo", True), ("gemm", False)):
                ops.set_halo_wgrad(on)
                res[key].append(fl / timeit(fn) / 1e12)
        ops.set_halo_wgrad(True)
        med = {k: statistics.median(v) for k, v in res.items()}
        out[name] = {"shape": shp, "tflops": med, "runs": res}
        print("%-12s halo %7.1f TF  gemm %7.1f TF  (%.2fx)" % (
            name, med["halo"], med["gemm"], med["halo"] / med["gemm"]),
            flush=True)
        del fn
        torch.cuda.empty_cache()
    os.makedirs("gpurun_out", exist_ok=True)
    with open("gpurun_out/bench_wgrad_ab.json", "w") as f:
        json.dump(out, f, indent=1)


def main_lean(cases, rounds, setter, new):
    """old / new loop alternating round by round; times in microseconds"""
    out = {}
    sums = {"old": [0.0] * rounds, "lean": [0.0] * rounds}
    for name, shp in cases:
        fl, fn = case(*shp)
        res = {"old": [], "lean": []}
        try:
            # one untimed round of both: the first timing of a layer (cold
            # caches and clocks) would otherwise always be the old loop's
            for on in (False, True):
                setter(on)
                timeit(fn)
            for r in range(rounds):
                for key, on in (("old", False), ("lean", True)):
                    setter(on)
                    t = timeit(fn) * 1e6
                    res[key].append(t)
                    sums[key][r] += t
        finally:
            setter(True)
        st = {k: {"median": statistics.median(v), "min": min(v)}
              for k, v in res.items()}
        out[name] = {"shape": shp, "us": st, "runs": res,
                     "tflops_median": {k: fl / st[k]["median"] / 1e6
                                       for k in st}}
        print("%-12s old %8.1f us (min %8.1f)  %s %8.1f us (min %8.1f)  "
              "%+.1f %%" % (name, st["old"]["median"], st["old"]["min"], new,
                            st["lean"]["median"], st["lean"]["min"],
                            (st["old"]["median"] / st["lean"]["median"] - 1)
                            * 100), flush=True)
        del fn
        torch.cuda.empty_cache()
    med = {k: statistics.median(v) for k, v in sums.items()}
    spread = max(sums["old"]) - min(sums["old"])
    out["sum"] = {"runs": sums, "median": med, "old_spread": spread}
    print("sum          old %8.1f us  %s %8.1f us  gain %.1f us, the old "
          "loop's own spread %.1f us" % (med["old"], new, med["lean"],
                                         med["old"] - med["lean"], spread))
    return out


if __name__ == "__main__":
    main()
