"""Float64 references for the kernels that end every training step - the
evaluators (softmax-CE, MSE), the fused updates (SGD, the solvers) and
dropout - with the cases and the checks that hold an implementation to them.

The references are plain NumPy, written from the formulas in docs/OPS.md and
the kernel comments of csrc/kernels/elementwise.hip; none of them calls into
veles_amd.ops.  Inputs are generated in the dtype the kernel reads and widened
exactly to float64, so argmax, ties and masks of the reference are exact.

The ``run_*`` functions run one case through ``veles_amd.ops`` on a device
and assert every bound.  The tests of this file do that for the float32 CPU
paths (no GPU needed: this is how the references themselves are checked);
tests/test_step_tail_gpu.py imports the same helpers for the HIP kernels.
Each ``run_*`` returns the worst measured error / bound ratios.

Bounds (u = 2^-24, one float32 rounding; all derived, none measured):

* softmax p and err, rows of spread <= 30: ``scale * (2e-5 * p + 1e-7)``.
  exp(x - max) is a base-2 exponential of (x - max) * log2(e): rounding the
  product moves the result by 1.44 |x - max| u, the exponential adds ~2 u,
  the same in numerator and sum: (1.44 * 30 + 2) * 2 u = 5.4e-6 relative,
  below 2e-5; 1e-7 absolute covers the products that underflow.  A bf16
  output adds one bf16 half-ulp of the value: 2^(e - 8) for a value in
  [2^e, 2^(e+1)), between 2^-9 and 2^-8 of it (bf16 keeps 8 significant
  bits, so 2^-9 relative is met only in the upper half of a binade and a
  correctly rounded store can miss it).  The loss keeps the project's
  1e-4 of the metric.
* MSE: ``(D / 64 + 8) u`` relative on sums of non-negative terms.
* SGD: the kernel rounds g six times (grad * gscale; 1 - l1; its product with
  w; the sum with l1 * sign(w); the product with decay; the sum with the
  scaled gradient), v three more times (lr * g; moment * v; their sum) and w
  once more: |dv| <= 9 u V, |dw| <= 10 u W with V = lr * G + |moment * v|,
  W = |w| + V and G the sum of the absolute terms of g.  A contraction to
  fma only removes roundings.
* Solvers: the error of g (6 u G) is propagated by evaluating the update at
  g +- 6 u G (each state is monotone or convex in g), plus the update's own
  roundings times the sum of the absolute terms of each result, SOLVER_K.
"""
import numpy as np
import pytest
import torch

import veles_amd.ops as ops

U = 2.0 ** -24
BF = torch.bfloat16
F32 = torch.float32


def gamma(k):
    return k * U / (1.0 - k * U)


def f32(x):
    return float(np.float32(x))


def bf_half_ulp(v):
    """Half the spacing of bfloat16 (8 significant bits) at |v|."""
    _, e = np.frexp(np.abs(v))             # |v| = m * 2^e, m in [0.5, 1)
    return np.where(np.abs(v) > 0, np.ldexp(1.0, e - 9), 0.0)


def f64(t):
    """A tensor of any float dtype, widened exactly to a float64 array."""
    return t.detach().cpu().to(torch.float64).numpy()


def bits(t):
    """The bit patterns of a float32 / bfloat16 tensor (CPU, integer)."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


class Ratios(dict):
    """Worst measured |error| / bound per checked quantity."""

    def see(self, name, err, bound):
        err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
        assert np.isfinite(err).all(), "%s: non-finite" % name
        if err.size == 0:
            return
        r = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
        k = int(r.argmax())
        self[name] = max(self.get(name, 0.0), float(r.flat[k]))
        assert r.flat[k] <= 1.0, "%s: |err| %g is %.3f x bound %g at %d" % (
            name, err.flat[k], r.flat[k], bound.flat[k], k)

    def merge(self, other):
        for k, v in other.items():
            self[k] = max(self.get(k, 0.0), v)
        return self


# ------------------------------------------------------------- evaluators
def softmax_ce_ref(logits, labels, scale):
    """logits float64 [B, C]; labels int [B] or None (-1 = no label)."""
    x = np.asarray(logits, np.float64)
    B, C = x.shape
    e = np.exp(x - x.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    amax = x.argmax(1)                      # first index on ties
    lab = np.full(B, -1, np.int64) if labels is None else \
        np.asarray(labels, np.int64)
    valid = lab >= 0
    rows = np.nonzero(valid)[0]
    oh = np.zeros_like(p)
    oh[rows, lab[rows]] = 1.0
    err = (p - oh) * scale
    err[~valid] = 0.0
    loss = np.zeros(B)
    loss[rows] = -np.log(np.maximum(p[rows, lab[rows]], 1e-30))
    conf = np.zeros((C, C), np.int64)
    np.add.at(conf, (amax[rows], lab[rows]), 1)
    n_err = float((amax[rows] != lab[rows]).sum())
    return dict(p=p, err=err, loss=loss, amax=amax, confusion=conf,
                metrics=np.array([n_err, loss.sum(), float(len(rows))]),
                spread=x.max(1) - x.min(1))


def mse_ref(y, t, scale, valid_rows):
    y, t = np.asarray(y, np.float64), np.asarray(t, np.float64)
    B = y.shape[0]
    d = y.reshape(B, -1) - t.reshape(B, -1)
    d[valid_rows:] = 0.0
    m = (d * d).mean(1)
    v = m[:valid_rows]
    return dict(err=d * scale, mse=m,
                metrics=np.array([v.sum(), np.sqrt(v).sum(),
                                  float(valid_rows)]))


# ---------------------------------------------------------------- updates
def _segment_of(n, segs):
    """Per element: the index of the segment that holds it, or -1."""
    seg = np.full(n, -1, np.int64)
    i = np.arange(n)
    for k, s in enumerate(segs):
        seg[(i >= s[0]) & (i < s[1])] = k
    return seg


def _gradient(w, grad, gscale, decay, l1):
    """g and the sum of the absolute values of its terms."""
    g = grad * gscale
    G = np.abs(g)
    if decay != 0.0:
        sg = np.sign(w)
        g = g + decay * ((1.0 - l1) * w + l1 * sg)
        G = G + abs(decay) * (abs(1.0 - l1) * np.abs(w) + abs(l1) * np.abs(sg))
    return g, G


def sgd_ref(w, grad, mom, segs, gscale, zero_from):
    """One fused SGD step on float64 copies of float32 state; hyper-parameters
    are taken through float32, as the packed table holds them.  Returns the
    new w / mom / grad, the per-element bounds and the in-segment mask."""
    w, grad = np.array(w, np.float64), np.array(grad, np.float64)
    n = w.size
    mom = None if mom is None else np.array(mom, np.float64)
    seg = _segment_of(n, segs)
    nw, nm = w.copy(), None if mom is None else mom.copy()
    bw, bm = np.zeros(n), np.zeros(n)
    for k, (b, e, lr, decay, l1, moment) in enumerate(segs):
        lr, decay, l1, moment = f32(lr), f32(decay), f32(l1), f32(moment)
        m = seg == k
        g, G = _gradient(w[m], grad[m], f32(gscale), decay, l1)
        v, V = -lr * g, abs(lr) * G
        if mom is not None:
            v = v + moment * mom[m]
            V = V + np.abs(moment * mom[m])
            nm[m] = v
        nw[m] = w[m] + v
        bm[m] = gamma(9) * V
        bw[m] = gamma(10) * (np.abs(w[m]) + V)
    ng = grad.copy()
    ng[zero_from:] = 0.0
    return dict(w=nw, mom=nm, grad=ng, bw=bw, bm=bm, inseg=seg >= 0)


# the update's own roundings (after g), relative to the sum of the absolute
# terms of each result.  mode 0: v = m*v - lr*g is 3, w += v one more.
# mode 1: a = s1 + g*g is 2; the step lr*g / (sqrt(a) + eps) takes 1 from a,
# up to 2 from sqrt, then +eps, lr*g and the division, 6, and w one more,
# 8 with a margin of one.  mode 2: a is 5 (rho*s1, 1-rho, two products, the
# sum); d = g*sqrt(s2+eps)/sqrt(a+eps) is 0.5+1+2 (numerator), 3+2 (denominator)
# and two more, 11 u, so s2' is 2*11+5 = 27 and w 11+1+1 = 13.  mode 3: the
# step is one product, w one difference, s2 is copied.
SOLVER_K = {0: (4, 3, 0), 1: (8, 2, 0), 2: (13, 5, 27), 3: (2, 1, 0)}
RPROP_UP, RPROP_DOWN = f32(1.2), 0.5
RPROP_MAX, RPROP_MIN = 50.0, f32(1e-6)


def _solver_modes(w, g, s1, s2, lr, moment, mode, eps, rho):
    """(w', s1', s2') and the sums of the absolute terms of each."""
    z = np.zeros_like(w)
    if mode == 1:
        a = s1 + g * g
        st = lr * g / (np.sqrt(a) + eps)
        return w - st, a, s2, np.abs(w) + np.abs(st), np.abs(s1) + g * g, z
    if mode == 2:
        a = rho * s1 + (1.0 - rho) * g * g
        d = g * np.sqrt(s2 + eps) / np.sqrt(a + eps)
        c = rho * s2 + (1.0 - rho) * d * d
        return (w - lr * d, a, c, np.abs(w) + np.abs(lr * d),
                np.abs(rho * s1) + (1.0 - rho) * g * g,
                np.abs(rho * s2) + (1.0 - rho) * d * d)
    if mode == 3:
        # iRprop-: decided by the SIGNS of the previous and the new gradient
        step = np.where(s1 > 0, s1, lr)
        same = np.sign(s2) * np.sign(g) > 0
        flip = np.sign(s2) * np.sign(g) < 0
        step = np.where(same, np.minimum(step * RPROP_UP, RPROP_MAX), step)
        step = np.where(flip, np.maximum(step * RPROP_DOWN, RPROP_MIN), step)
        g = np.where(flip, 0.0, g)
        return w - np.sign(g) * step, step, g, np.abs(w) + step, step, z
    v = moment * s1 - lr * g
    V = np.abs(moment * s1) + np.abs(lr * g)
    return w + v, v, s2, np.abs(w) + V, V, z


def solver_ref(w, grad, s1, s2, segs, gscale, zero_from):
    w, grad = np.array(w, np.float64), np.array(grad, np.float64)
    s1, s2 = np.array(s1, np.float64), np.array(s2, np.float64)
    n = w.size
    seg = _segment_of(n, segs)
    out = [w.copy(), s1.copy(), s2.copy()]
    bnd = [np.zeros(n), np.zeros(n), np.zeros(n)]
    for k, (b, e, lr, decay, l1, moment, mode, eps, rho) in enumerate(segs):
        hp = [f32(lr), f32(moment), int(mode), f32(eps), f32(rho)]
        m = seg == k
        g, G = _gradient(w[m], grad[m], f32(gscale), f32(decay), f32(l1))
        dg = gamma(6) * G
        mid = _solver_modes(w[m], g, s1[m], s2[m], *hp)
        lo = _solver_modes(w[m], g - dg, s1[m], s2[m], *hp)
        hi = _solver_modes(w[m], g + dg, s1[m], s2[m], *hp)
        for q in range(3):
            out[q][m] = mid[q]
            bnd[q][m] = np.maximum(np.abs(lo[q] - mid[q]),
                                   np.abs(hi[q] - mid[q])) + \
                gamma(SOLVER_K[hp[2]][q]) * mid[3 + q]
    ng = grad.copy()
    ng[zero_from:] = 0.0
    return dict(w=out[0], s1=out[1], s2=out[2], grad=ng, bw=bnd[0],
                b1=bnd[1], b2=bnd[2], inseg=seg >= 0)


# ---------------------------------------------------------------- dropout
M32 = 0xFFFFFFFF
_C0, _C1, _C2 = 0x9E3779B9, 0x7FEB352D, 0x846CA68B


def hash32(i, seed):
    """The mask hash of element index i (uint32 values in an int64 array)."""
    x = (np.asarray(i, np.int64) & M32) ^ ((int(seed) * _C0) & M32)
    x ^= x >> 16
    x = (x * _C1) & M32
    x ^= x >> 15
    x = (x * _C2) & M32
    x ^= x >> 16
    return x


def _unxorshift(x, s):
    y, t = x.copy(), x >> s
    while t.any():
        y ^= t
        t = t >> s
    return y


def hash32_inv(h, seed):
    """The index whose hash is h: the hash is a bijection on uint32."""
    x = _unxorshift(np.asarray(h, np.int64) & M32, 16)
    x = (x * pow(_C2, -1, 1 << 32)) & M32
    x = _unxorshift(x, 15)
    x = (x * pow(_C1, -1, 1 << 32)) & M32
    x = _unxorshift(x, 16)
    return x ^ ((int(seed) * _C0) & M32)


def dropout_thresh(p):
    """min(2^32 - 1, floor(float32(p) * 2^32)); the product is exact in
    double.  Elements whose hash is >= the threshold are kept."""
    t = int(float(np.float32(p)) * 4294967296.0)
    return max(0, min(M32, t))


def dropout_scale(p):
    """1 / (1 - p) in IEEE float32 throughout, 0 for p >= 1."""
    p = np.float32(p)
    return np.float32(1.0) / (np.float32(1.0) - p) if p < 1 else \
        np.float32(0.0)


def dropout_ref(x, p, seed, base=0):
    """x: float32 or bfloat16 tensor.  Returns (keep mask, float32 tensor
    keep ? float32(x) * scale : +0), both flat."""
    xf = x.detach().cpu().reshape(-1).float().numpy()
    i = np.arange(xf.size, dtype=np.int64) + int(base)
    keep = hash32(i, seed) >= dropout_thresh(p)
    y = np.where(keep, xf * dropout_scale(p), np.float32(0.0))
    return keep, torch.from_numpy(y.astype(np.float32))


# ============================================================ cases, runs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


# --------------------------------------------------------------- softmax
SOFTMAX_C = [1, 2, 63, 64, 65, 1000, 1024, 1025, 1031]
SOFTMAX_B = [1, 3, 5, 37]
SOFTMAX_SHAPES = [(B, C) for C in SOFTMAX_C for B in SOFTMAX_B] + \
    [(4099, 10), (1029, 1025)]


def softmax_inputs(B, C, dtype, seed=0, labels="mixed"):
    """Logits of spread <= 28 in ``dtype`` and int32 labels: mixed valid and
    -1, one of them in the last column."""
    g = _gen(1000 * C + B + seed)
    x = (torch.randn(B, C, generator=g) * 3.0).clamp_(-14.0, 14.0).to(dtype)
    if labels is None:
        return x, None
    lab = torch.randint(0, C, (B,), generator=g, dtype=torch.int32)
    lab[0] = C - 1
    if labels == "mixed" and B > 1:
        lab[1::4] = -1
    if labels == "none":
        lab[:] = -1
    return x, lab


def run_softmax(dev, x, lab, *, err_dtype=F32, want=("probs", "max_idx",
                                                     "confusion"),
                scale=None, calls=1, exact_only=False):
    """Runs ops.softmax_ce ``calls`` times on ``dev`` with metrics that start
    from non-zero values and checks every output against the reference.
    Returns (outputs, ratios)."""
    B, C = x.shape
    sc = 1.0 / B if scale is None else scale
    ref = softmax_ce_ref(f64(x), None if lab is None else lab.numpy(), sc)
    start = np.array([3.0, 1.5, 7.0])
    xd = x.to(dev)
    ld = None if lab is None else lab.to(dev)
    # outputs start from a pattern, so an element the kernel skips shows
    err = torch.full((B, C), 7.0, dtype=err_dtype, device=dev) \
        if lab is not None else None
    probs = torch.full((B, C), 7.0, device=dev) if "probs" in want else None
    amax = torch.full((B,), -7, dtype=torch.int32, device=dev) \
        if "max_idx" in want else None
    with_conf = "confusion" in want and lab is not None
    conf = torch.ones(C, C, dtype=torch.int32, device=dev) \
        if with_conf else None
    met = torch.tensor(start, dtype=F32, device=dev) \
        if lab is not None else None
    for _ in range(calls):
        ops.softmax_ce(xd, ld, scale=sc, err=err, probs=probs, max_idx=amax,
                       metrics=met, confusion=conf)
    r = Ratios()
    narrow = ref["spread"] <= 30.0
    b32 = sc * (2e-5 * ref["p"] + 1e-7)
    if amax is not None:
        assert np.array_equal(amax.cpu().numpy(), ref["amax"]), "max_idx"
    if probs is not None:
        d = np.abs(f64(probs) - ref["p"])
        assert np.isfinite(d).all()
        if not exact_only:
            r.see("ce_p", d[narrow], (b32 / sc)[narrow])
        r.see("ce_p_1e-4", d, np.full_like(d, 1e-4))
    if err is not None:
        d = np.abs(f64(err) - ref["err"])
        b = b32 if err_dtype == F32 else \
            b32 + bf_half_ulp(np.abs(ref["err"]) + b32)
        rows = np.nonzero(lab.numpy() < 0)[0]
        assert not f64(err)[rows].any(), "err of unlabelled rows"
        if not exact_only:
            r.see("ce_err_" + str(err_dtype)[6:], d[narrow], b[narrow])
        slack = 0.0 if err_dtype == F32 else \
            bf_half_ulp(np.abs(ref["err"]) + 1e-4 * sc)
        r.see("ce_err_1e-4_" + str(err_dtype)[6:], d, 1e-4 * sc + slack)
    if met is not None:
        m = f64(met)
        want_m = start + calls * ref["metrics"]
        assert m[0] == want_m[0] and m[2] == want_m[2], (m, want_m)
        r.see("ce_loss", abs(m[1] - want_m[1]), 1e-4 * (abs(want_m[1]) + 1e-6))
    if conf is not None:
        assert np.array_equal(conf.cpu().numpy().astype(np.int64),
                              1 + calls * ref["confusion"]), "confusion"
    return dict(err=err, probs=probs, max_idx=amax, metrics=met,
                confusion=conf), r


def softmax_tie_rows(C, dtype):
    """Rows whose maximum appears twice: in two lanes of one register
    (columns 5, 9), in one lane's two registers (7, 71), across the 64-column
    boundary (63, 64) and with the lower column in the higher lane (8, 70),
    then the same pairs moved to the end of the row."""
    pairs = [(5, 9), (7, 71), (63, 64), (8, 70)]
    pairs += [(C - 1 - b, C - 1 - a) for a, b in pairs]
    x = (torch.randn(len(pairs), C, generator=_gen(C)) * 2.0).clamp_(-6, 6)
    for r, (a, b) in enumerate(pairs):
        x[r, a] = x[r, b] = 9.0
    lab = torch.tensor([a if r % 2 else b for r, (a, b) in enumerate(pairs)],
                       dtype=torch.int32)
    return x.to(dtype), lab, [a for a, _ in pairs]


def softmax_range_rows(C, dtype):
    """Spread 160 (max 80, rest -80) with the label on and off the maximum, a
    row of equal values and, in float32, logits of +-1e4."""
    x = torch.full((6, C), -80.0)
    x[0, 3 % C] = x[1, C - 1] = 80.0
    x[2] = 1.25
    x[3] = torch.randn(C, generator=_gen(3)).clamp_(-3, 3)
    big = 1e4 if dtype == F32 else 80.0
    x[4] = -big
    x[4, C // 2] = big
    x[5] = big
    x[5, 0] = -big
    lab = torch.tensor([3 % C, 0, C - 1, -1, C // 2, 0], dtype=torch.int32)
    return x.to(dtype), lab


# ------------------------------------------------------------------- MSE
MSE_SHAPES = [(B, D) for D in (1, 63, 64, 65, 130) for B in (1, 5, 1029)]


def run_mse(dev, B, D):
    """Every dtype mix, err dtype, mse_out choice and valid_rows of one
    shape; returns the worst ratios."""
    r = Ratios()
    g = _gen(B * 1000 + D)
    y32 = torch.randn(B, D, generator=g)
    t32 = torch.randn(B, D, generator=g)
    start = np.array([2.0, 0.75, 5.0])
    scale = 0.37
    rows_per_wave = -(-B // 1024) + 1
    adds = rows_per_wave + 3 + min(256, -(-B // 4))     # per metric
    kb = D / 64.0 + 8
    for ydt, tdt in ((F32, F32), (BF, BF), (F32, BF), (BF, F32)):
        y, t = y32.to(ydt), t32.to(tdt)
        for vr in sorted({0, min(3, B), B}):
            ref = mse_ref(f64(y), f64(t), f32(scale), vr)
            for edt in (F32, BF):
                for with_out in (True, False):
                    err = torch.full((B, D), 7.0, dtype=edt, device=dev)
                    out = torch.full((B,), 7.0, device=dev) \
                        if with_out else None
                    met = torch.tensor(start, dtype=F32, device=dev)
                    ops.mse(y.to(dev), t.to(dev), scale=scale, err=err,
                            mse_out=out, metrics=met, valid_rows=vr)
                    e = f64(err)
                    assert not e[vr:].any(), "err of invalid rows"
                    b = gamma(2) * np.abs(ref["err"])
                    if edt == BF:
                        b = b + bf_half_ulp(np.abs(ref["err"]) + b)
                    r.see("mse_err_" + str(edt)[6:], np.abs(e - ref["err"]), b)
                    if out is not None:
                        o = f64(out)
                        assert not o[vr:].any(), "mse_out of invalid rows"
                        r.see("mse_out", np.abs(o - ref["mse"]),
                              gamma(kb) * ref["mse"])
                    if vr == 0:
                        assert same_bits(met, torch.tensor(start, dtype=F32))
                        continue
                    m, want = f64(met), start + ref["metrics"]
                    assert m[2] == want[2]
                    r.see("mse_metrics", np.abs(m[:2] - want[:2]),
                          gamma(kb + adds) * want[:2])
    return r


# ------------------------------------------------------------------- SGD
SGD_N = 4 * 256 * 5 + 8
_HP = [(0.1, 0.01, 0.0, 0.9), (0.2, 0.003, 0.5, 0.5), (0.05, 0.02, 1.0, 0.7),
       (0.3, 0.0, 0.0, 0.25), (0.07, 0.05, 0.25, 0.0)]


def _with_hp(bounds, shift=0):
    return [(b, e) + _HP[(k + shift) % len(_HP)]
            for k, (b, e) in enumerate(bounds)]


def sgd_tables(n=SGD_N):
    """name -> segment table.  Boundaries at every residue mod 4, a segment
    of length 1, gaps, first begin > 0, last end < n; 1, 2 and 40 segments."""
    t = {"one": _with_hp([(3, n - 2)], 1),
         "aligned": _with_hp([(0, 2048), (2048, 4096), (4096, n)])}
    for r in (1, 2, 3):
        t["two_r%d" % r] = _with_hp([(1, 2000 + r), (2000 + r, n - 1)], r)
        t["two_gap_r%d" % r] = _with_hp([(4 + r, 2000 + r),
                                         (2008 + r, n - 4 - r)], r + 1)
    t["len1_gaps"] = _with_hp([(2, 3), (9, 1030), (1031, 1032), (1037, 3003),
                               (3003, 3004), (3004, 3005), (3006, 3007),
                               (3012, 5001)])
    b, bounds = 1, []
    for k in range(40):
        ln = 90 + (k * 37) % 71
        bounds.append((b, min(b + ln, n - 3)))
        b += ln + (k % 3 == 1) * (1 + k % 7)     # every third: a gap of 1-7
    t["forty"] = _with_hp(bounds)
    return t


SGD_TABLES = sgd_tables()
SGD_ZERO = [True, False, 2000, 2001, 2002, 2003]


def sgd_state(n, seed=0):
    """Non-zero float32 w / grad / mom everywhere (gaps too, so a touched gap
    shows), with +0.0 and -0.0 weights planted in segments and gaps."""
    g = _gen(seed + n)
    w = torch.randn(n, generator=g)
    gr = torch.randn(n, generator=g)
    m = torch.randn(n, generator=g) * 0.1
    z = torch.arange(0, n, 7)
    w[z[0::2]] = 0.0
    w[z[1::2]] = -0.0
    return w, gr, m


def check_sgd(w0, g0, m0, w1, g1, m1, lp, segs, gscale, zf, r, tag="sgd"):
    """State before (``*0``, float32 CPU tensors) and after (``*1``) one
    update against sgd_ref."""
    ref = sgd_ref(f64(w0), f64(g0), None if m0 is None else f64(m0), segs,
                  gscale, zf)
    ins = ref["inseg"]
    gap = torch.from_numpy(~ins)
    assert torch.equal(bits(w1)[gap], bits(w0)[gap]), \
        "w touched outside every segment at %s" % (
            np.nonzero((bits(w1) != bits(w0)).numpy() & ~ins)[0][:8],)
    r.see(tag + "_w", np.abs(f64(w1) - ref["w"])[ins], ref["bw"][ins])
    if m0 is not None:
        assert torch.equal(bits(m1)[gap], bits(m0)[gap]), \
            "mom touched outside every segment at %s" % (
                np.nonzero((bits(m1) != bits(m0)).numpy() & ~ins)[0][:8],)
        r.see(tag + "_mom", np.abs(f64(m1) - ref["mom"])[ins], ref["bm"][ins])
    if lp is not None:
        assert same_bits(lp, w1.cpu().to(BF)), "w_lp is not bf16(w)"
    assert torch.equal(bits(g1)[:zf], bits(g0)[:zf]), "grad below zero_from"
    assert not bits(g1)[zf:].any(), "grad not cleared at %s" % (
        zf + np.nonzero(bits(g1)[zf:].numpy())[0][:8],)


def run_sgd(dev, segs, route="sgd4", zero=SGD_ZERO, gscale=0.3, seed=0):
    """One table through one route, for every zero_grad of ``zero``.
    Routes: sgd4 (n % 4 == 0, aligned base), grid1 / grid3 (max_blocks),
    odd (n % 4 != 0), view (w[1:] of a longer buffer), nomom (mom=None)."""
    r = Ratios()
    n = SGD_N - 1 if route == "odd" else SGD_N
    segs = [(min(b, n), min(e, n)) + tuple(hp) for b, e, *hp in segs]
    segs = [s for s in segs if s[0] < s[1]]
    for z in zero:
        w0, g0, m0 = sgd_state(n, seed)
        if route == "nomom":
            m0 = None
        if route == "view":
            hold = torch.zeros(n + 1, device=dev)
            w = hold[1:]
            w.copy_(w0)
        else:
            w = w0.clone().to(dev)
        gr = g0.clone().to(dev)
        m = None if m0 is None else m0.clone().to(dev)
        lp = torch.full((n,), 7.0, dtype=BF, device=dev)
        mb = {"grid1": 1, "grid3": 3}.get(route)
        ops.sgd_update(w, gr, m, segs, w_lp=lp, gscale=gscale, zero_grad=z,
                       max_blocks=mb)
        zf = 0 if z is True else (n if z is False else z)
        check_sgd(w0, g0, m0, w.cpu(), gr.cpu(),
                  None if m is None else m.cpu(), lp.cpu(), segs, gscale,
                  zf, r)
    return r


# --------------------------------------------------------------- solvers
SOLVER_N = 1500


def solver_tables(n=SOLVER_N):
    """name -> table (begin, end, lr, decay, l1, moment, mode, eps, rho):
    each mode alone with a gap, first begin > 0 and last end < n, and the
    four mixed.  The Rprop segments carry no decay, so the sign of g is the
    sign of the gradient."""
    t = {}
    for mode in range(4):
        d = 0.0 if mode == 3 else 1e-3
        t["mode%d" % mode] = [
            (3, 701, 0.1, d, 0.2 if d else 0.0, 0.9, mode, 1e-6, 0.95),
            (706, n - 5, 0.05, 0.0, 0.0, 0.5, mode, 1e-6, 0.9)]
    t["mixed"] = [(2, 301, 0.1, 1e-3, 0.2, 0.9, 0, 1e-6, 0.95),
                  (301, 602, 0.05, 2e-3, 0.5, 0.0, 1, 1e-6, 0.9),
                  (607, 903, 0.5, 1e-3, 1.0, 0.0, 2, 1e-6, 0.95),
                  (903, 904, 0.02, 0.0, 0.0, 0.0, 3, 1e-6, 0.9),
                  (909, n - 6, 0.02, 0.0, 0.0, 0.0, 3, 1e-6, 0.9)]
    return t


SOLVER_TABLES = solver_tables()


def check_solver(before, after, lp, segs, gscale, zf, r, tag):
    """before / after: (w, grad, s1, s2) float32 CPU tensors."""
    ref = solver_ref(*[f64(t) for t in before], segs, gscale, zf)
    ins = ref["inseg"]
    gap = torch.from_numpy(~ins)
    for q, name, bound in ((0, "w", "bw"), (2, "s1", "b1"), (3, "s2", "b2")):
        assert torch.equal(bits(after[q])[gap], bits(before[q])[gap]), \
            "%s touched outside every segment at %s" % (name, np.nonzero(
                (bits(after[q]) != bits(before[q])).numpy() & ~ins)[0][:8])
        r.see("%s_%s" % (tag, name), np.abs(f64(after[q]) - ref[name])[ins],
              ref[bound][ins])
    if lp is not None:
        assert same_bits(lp, after[0].to(BF)), "w_lp is not bf16(w)"
    assert torch.equal(bits(after[1])[:zf], bits(before[1])[:zf])
    assert not bits(after[1])[zf:].any(), "grad not cleared from zero_from"


def run_solver(dev, segs, tag, steps=4, zero=(701, False), s1_start=0.0):
    """``steps`` updates; each is compared from the implementation's own
    previous state, so one rounding cannot flip a later sign."""
    r = Ratios()
    n = SOLVER_N
    for z in zero:
        g = _gen(n + 17)
        w = torch.randn(n, generator=g).to(dev)
        s1 = torch.full((n,), s1_start, device=dev)
        s2 = torch.zeros(n, device=dev)
        lp = torch.full((n,), 7.0, dtype=BF, device=dev)
        zf = n if z is False else z
        for it in range(steps):
            gr = torch.randn(n, generator=g)
            if it == 2:
                gr[::5] = 0.0
            before = (w.cpu().clone(), gr.clone(), s1.cpu().clone(),
                      s2.cpu().clone())
            gd = gr.to(dev)
            ops.solver_update(w, gd, s1, s2, segs, w_lp=lp, gscale=0.5,
                              zero_grad=z)
            check_solver(before, (w.cpu(), gd.cpu(), s1.cpu(), s2.cpu()),
                         lp.cpu(), segs, 0.5, zf, r, tag)
    return r


def rprop_edge_state():
    """Every combination of step state (45 and 1.5e-6: one step reaches each
    clamp; 0 and -1: start from lr; 0.01), previous and new gradient (0, +-1,
    +-1e-25), inside one Rprop segment with two elements of gap either side."""
    s1v = [45.0, 1.5e-6, 0.0, -1.0, 0.01]
    gv = [0.0, 1.0, -1.0, 1e-25, -1e-25]
    s1, pg, g = np.meshgrid(s1v, gv, gv, indexing="ij")
    pad = [0.5, 0.5]
    mk = lambda a: torch.tensor(pad + list(a.ravel()) + pad, dtype=F32)
    n = s1.size + 4
    w = torch.linspace(-1.0, 1.0, n)
    segs = [(2, n - 2, 0.03, 0.0, 0.0, 0.0, 3, 1e-6, 0.9)]
    return w, mk(g), mk(s1), mk(pg), segs


def run_rprop_edges(dev):
    r = Ratios()
    w0, g0, s10, s20, segs = rprop_edge_state()
    w, g, s1, s2 = (t.clone().to(dev) for t in (w0, g0, s10, s20))
    lp = torch.zeros(w0.numel(), dtype=BF, device=dev)
    ops.solver_update(w, g, s1, s2, segs, w_lp=lp, gscale=1.0,
                      zero_grad=False)
    check_solver((w0, g0, s10, s20), (w.cpu(), g.cpu(), s1.cpu(), s2.cpu()),
                 lp.cpu(), segs, 1.0, w0.numel(), r, "rprop")
    # the cases by name, on top of the reference: +-1e-25 pairs grow or
    # shrink the step although their float32 product underflows to zero
    a, p, q = s10[2:-2].numpy(), s20[2:-2].numpy(), g0[2:-2].numpy()
    step, prev = s1.cpu()[2:-2].numpy(), s2.cpu()[2:-2].numpy()
    base = np.where(a > 0, a, np.float32(0.03))
    same, flip = np.sign(p) * np.sign(q) > 0, np.sign(p) * np.sign(q) < 0
    assert same.sum() == 40 and flip.sum() == 40
    assert ((step > base) | (step == 50.0))[same].all(), "step did not grow"
    assert ((step < base) | (step == np.float32(1e-6)))[flip].all(), \
        "step did not shrink"
    assert not prev[flip].any() and np.array_equal(prev[~flip], q[~flip])
    assert np.array_equal(step[~same & ~flip], base[~same & ~flip])
    assert (step[same & (a == 45.0)] == 50.0).all()
    assert (step[flip & (a == np.float32(1.5e-6))] == np.float32(1e-6)).all()
    return r


# ---------------------------------------------------------------- dropout
DROPOUT_P = [0.0, 0.1, 0.3, 0.4, 0.5, 0.9, 1.0 - 2.0 ** -24, 1.0]


def dropout_input(n, dtype, seed=0):
    """Values without zeros (so y != 0 is the mask), both signs."""
    x = torch.randn(n, generator=_gen(n + seed))
    x = torch.where(x.abs() < 0.05, torch.full_like(x, 0.75), x)
    return x.to(dtype)


def check_dropout(x, y, p, seed, base=0):
    """y against the exact mask and the IEEE float32 product, bit for bit."""
    keep, ref = dropout_ref(x, p, seed, base)
    yc = y.detach().cpu().reshape(-1)
    assert torch.isfinite(yc.float()).all()
    if np.float32(p) < 1:
        got = (yc.float() != 0).numpy()
        assert np.array_equal(got, keep), "mask differs at %s" % (
            np.nonzero(got != keep)[0][:8],)
    else:
        assert not yc.float().any(), "p = 1 keeps a value"
    if np.float32(p) == 0:
        assert same_bits(yc, x.detach().cpu().reshape(-1).to(yc.dtype))
    assert same_bits(yc, ref.to(yc.dtype)), "values differ at %s" % (
        np.nonzero((bits(yc) != bits(ref.to(yc.dtype))).numpy())[0][:8],)
    return keep


def dropout_boundary_cases(p, seed):
    """[(hash value, kept?)] around the threshold T of p: T - 1 is dropped, T
    kept; for p = 0.4 also both ends of the window between the double
    threshold int(0.4 * 2^32) and T, which the float32 rule drops."""
    T = dropout_thresh(p)
    cases = [(T, True)]
    if T > 0:
        cases.append((T - 1, False))
    if p == 0.4:
        T64 = int(0.4 * 4294967296.0)
        assert 0 < T - T64 < 1000
        cases += [(T64, False), (T - 1, False), (T64 - 1, False)]
    return cases


# ========================================================= CPU-path tests
CPU = "cpu"
_DT = {"f32": F32, "bf16": BF}


def test_hash_round_trip():
    h = np.concatenate([np.arange(0, 1 << 32, 1000003, dtype=np.int64),
                        np.array([0, 1, M32, M32 - 1, 1 << 31])])
    assert h.size > 4000
    for seed in (0, 1, 1234, M32):
        i = hash32_inv(h, seed)
        assert ((i >= 0) & (i <= M32)).all()
        assert np.array_equal(hash32(i, seed), h)
        assert np.array_equal(hash32_inv(hash32(h, seed), seed), h)


def test_dropout_thresh_values():
    """float32(p) * 2^32 against the double product the CPU mask used."""
    assert dropout_thresh(0.0) == 0 and dropout_thresh(1.0) == M32
    assert dropout_thresh(0.5) == 1 << 31 and dropout_thresh(0.25) == 1 << 30
    assert dropout_thresh(1.0 - 2.0 ** -24) == (1 << 32) - 256
    for p, d in ((0.4, 26), (0.3, 52), (0.9, -102)):
        assert dropout_thresh(p) - int(p * 4294967296.0) == d
    for p in DROPOUT_P:
        assert int(ops.dropout_mask_ref(1, 0, p).numel()) == 1


@pytest.mark.parametrize("B,C", SOFTMAX_SHAPES)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_cpu_softmax(B, C, dt):
    x, lab = softmax_inputs(B, C, _DT[dt])
    want = ("probs", "max_idx", "confusion") if C <= 1031 and B <= 37 \
        else ("probs", "max_idx")
    for edt in (F32, BF):
        run_softmax(CPU, x, lab, err_dtype=edt, want=want, calls=2)
    run_softmax(CPU, x, None, want=("probs", "max_idx"))


@pytest.mark.parametrize("C", [130, 1030])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_cpu_softmax_ties_range_unlabelled(C, dt):
    x, lab, first = softmax_tie_rows(C, _DT[dt])
    out, _ = run_softmax(CPU, x, lab)
    assert out["max_idx"].tolist() == first
    x, lab = softmax_range_rows(C, _DT[dt])
    run_softmax(CPU, x, lab, exact_only=True)
    x, lab = softmax_inputs(5, C, _DT[dt], labels="none")
    out, _ = run_softmax(CPU, x, lab)
    assert not out["err"].any()


@pytest.mark.parametrize("B,D", MSE_SHAPES)
def test_cpu_mse(B, D):
    run_mse(CPU, B, D)


@pytest.mark.parametrize("table", sorted(SGD_TABLES))
@pytest.mark.parametrize("route", ["sgd4", "odd", "nomom"])
def test_cpu_sgd(table, route):
    run_sgd(CPU, SGD_TABLES[table], route)


@pytest.mark.parametrize("table", sorted(SOLVER_TABLES))
def test_cpu_solver(table):
    run_solver(CPU, SOLVER_TABLES[table], table)


@pytest.mark.parametrize("mode", [1, 2])
def test_cpu_solver_large_state(mode):
    run_solver(CPU, SOLVER_TABLES["mode%d" % mode], "big", steps=2,
               zero=(False,), s1_start=1e6)


def test_cpu_rprop_edges():
    run_rprop_edges(CPU)


@pytest.mark.parametrize("p", DROPOUT_P)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_cpu_dropout(p, dt):
    for n, base in ((4099, 0), (16, (1 << 32) - 5)):
        x = dropout_input(n, _DT[dt])
        check_dropout(x, ops.dropout(x, p, 1234, base=base), p, 1234, base)
    seed = 77
    x = dropout_input(16, _DT[dt])
    for h, kept in dropout_boundary_cases(p, seed):
        j = int(hash32_inv(np.array([h]), seed)[0])
        for k in (0, 11):
            base = (j - k) & M32
            y = ops.dropout(x, p, seed, base=base)
            keep = check_dropout(x, y, p, seed, base)
            assert bool(keep[k]) == kept
