"""Float64 reference for the Adam, AdamW and RMSProp modes of the fused
update (``ops.solver_update`` modes 4 - 6), for clipping by the global
gradient norm and for ``ops.grad_sqnorm``, with the cases and the checks that
hold an implementation to them.

``adam_oracle`` is a float64 transcription of the formulae in docs/OPS.md
("Updates"); it calls nothing of veles_amd.ops and is itself checked against
float64 ``torch.optim.Adam`` / ``AdamW`` / ``RMSprop``.  ``run_adam`` runs a
case through ``ops.solver_update`` on a device, one update at a time, each
compared with the oracle started from the implementation's own float32 state
before that update; tests/test_adam_gpu.py imports the same helpers for the
HIP kernels.  The tests of this file do it for the float32 CPU path.

Bounds (u = 2^-24; all derived from the float32 roundings of the formulae,
none measured; a contraction to fma only removes roundings).  G is the sum of
the absolute terms of g, as in tests/test_step_tail_ref.py:

* g: at most 6 roundings (grad * gscale; 1 - l1; its product with w; the sum
  with l1 * sign(w); the product with decay; the sum), |dg| <= 6 u G.  With
  clipping the coefficient is recomputed on the device (a root, a product, a
  sum, a quotient, a product); the oracle takes the float32 coefficient, and
  a root or quotient that is faithfully, not correctly, rounded moves it by
  one more u each: 8 u G.
* s1 = m' = b1 m + (1 - b1) g (adam, adamw): 1 - b1, its product with g,
  b1 m and the sum, 4 u (|b1 m| + |(1 - b1) g|), plus (1 - b1) |dg|.
* v' = b2 v + ((1 - b2) g) g (s2 of adam / adamw, s1 of rmsprop): 1 - b2,
  two products, b2 v and the sum, 5 u v', plus v'(|g| + |dg|) - v'(|g|).
* the step st = (lr c1) m' / (sqrt(v') c2 + eps): the implementation forms
  it from ITS m' and v', anywhere inside their bounds bm and bv, so
  |st| <= st+ = (lr c1)(|m'| + bm) / (sqrt(v' - bv) c2 + eps) and the
  propagated error is at most st+ - |st| (st is linear in m' and convex,
  decreasing in v'); its own roundings are lr c1, the product with m', the
  root (2), the product with c2, the sum with eps and the quotient: 7 u st+.
  RMSProp's st = (lr g) / (sqrt(v') + eps) takes |g| + |dg| for |m'| + bm
  and 5 roundings.
* w' = w - st rounds once more, and AdamW's w - (lr decay) r before it once
  again, with r = (1 - l1) w + l1 sign(w) from 3 roundings and lr decay and
  the product one each: 6 u lr decay R.  Together
  |dw| <= (st+ - |st|) + 7 u st+ + 6 u lr decay R + 2 u (|w| + lr decay R
  + st+).

Per update and in units of lr that is 2 u |w| / lr + about 20 u |st| / lr:
with |w| < 5, lr = 1e-3 and |st| <= 3.2 lr (the first update, c1 m' /
(c2 sqrt(v')) = 1, and at most (1 - b1) / sqrt(1 - b2) later) at most
6e-4 lr + 4e-6 lr.  ``run_adam`` reports the largest bound / lr it used
(``*_bound_w/lr``: 3e-4 to 6e-4 on these tables, 1.6e-3 in the AdaGrad
segment of the mixed one, whose bound is test_step_tail_ref's).

Worst measured |error| / bound over the 12 updates (``pytest -s`` prints them
again); the float32 CPU path: adam w 0.48, s1 0.34, s2 0.34; adamw w 0.93,
s1 0.37, s2 0.35; rmsprop w 0.48, s1 0.35; mixed w 0.47, s1 0.43, s2 0.32;
grad_sqnorm 3e-4.  The HIP kernels on an MI355X: adam w 0.49, s1 0.24,
s2 0.24; adamw w 0.93, s1 0.21, s2 0.19; rmsprop w 0.48, s1 0.27; mixed
w 0.47, s1 0.44, s2 0.20; momentum with clipping w 0.24, s1 0.23;
grad_sqnorm 0.03.  The three wrong rules of ``test_discrimination`` reach
1e4 to 5e6 times the bound.
"""
import math

import numpy as np
import pytest
import torch

import veles_amd.ops as ops
from test_step_tail_ref import (BF, F32, U, Ratios, SOLVER_K, _gradient,
                                _segment_of, _solver_modes, bits, f32, f64,
                                gamma, same_bits)

N = 1031
BOUNDS = [(3, 130), (130, 517), (521, 1029)]
LR = (1e-3, 1e-2, 3e-3)
DECAY = (0.0, 1e-2, 5e-3)
L1 = (0.0, 0.0, 0.25)
EPS = (1e-8, 1e-3, 1e-8)
BETA1, BETA2, ALPHA = 0.9, 0.999, 0.99
ZERO_FROM = [0, 514, N]
GSCALE = 0.5
STEPS = 12


def table(name, bounds=BOUNDS):
    """adam / adamw / rmsprop: the three segments in that mode; mixed:
    adagrad, adam, momentum."""
    modes = {"adam": (4, 4, 4), "adamw": (5, 5, 5), "rmsprop": (6, 6, 6),
             "mixed": (1, 4, 0)}[name]
    segs = []
    for k, (b, e) in enumerate(bounds):
        rho = ALPHA if modes[k] == 6 else BETA2
        segs.append((b, e, LR[k], DECAY[k], L1[k], BETA1, modes[k], EPS[k],
                     rho))
    return segs


TABLES = ["adam", "adamw", "rmsprop", "mixed"]


def bias_correction_ref(b1, b2, t, exact=False):
    """(c1, c2); as the implementation carries them (from the float32 betas,
    rounded to float32) unless ``exact``."""
    if exact:
        return 1.0 / (1.0 - b1 ** t), 1.0 / math.sqrt(1.0 - b2 ** t)
    b1, b2 = f32(b1), f32(b2)
    return (f32(1.0 / (1.0 - b1 ** t)), f32(1.0 / math.sqrt(1.0 - b2 ** t)))


def _decay_term(w, decay, l1):
    r = (1.0 - l1) * w + l1 * np.sign(w)
    R = abs(1.0 - l1) * np.abs(w) + abs(l1) * np.abs(np.sign(w))
    return r, R


def adam_oracle(w, graw, s1, s2, hp, gscale, c1, c2, variant=None):
    """One update of modes 4 - 6 on float64 arrays, straight from the
    formulae.  hp = (lr, decay, l1, b1, mode, eps, b2).  ``variant``: a wrong
    rule, for the discrimination test: "nobias" (c1 = c2 = 1), "eps_in_root"
    (sqrt(v c2^2 + eps)), "decay_in_moments" (AdamW's decay fed through g)."""
    lr, decay, l1, b1, mode, eps, b2 = hp
    g = graw * gscale
    r, _ = _decay_term(w, decay, l1)
    if mode == 5 and variant != "decay_in_moments":
        w = w - lr * decay * r
    else:
        g = g + decay * r
    if mode == 6:
        v = b2 * s1 + (1.0 - b2) * g * g
        den = np.sqrt(v + eps) if variant == "eps_in_root" else \
            np.sqrt(v) + eps
        return w - lr * g / den, v, s2
    if variant == "nobias":
        c1 = c2 = 1.0
    m = b1 * s1 + (1.0 - b1) * g
    v = b2 * s2 + (1.0 - b2) * g * g
    den = np.sqrt(v * c2 * c2 + eps) if variant == "eps_in_root" else \
        np.sqrt(v) * c2 + eps
    return w - (lr * c1) * m / den, m, v


def _adam_bounds(w, graw, s1, s2, hp, gscale, c1, c2, kg):
    """(w', s1', s2') of the oracle and the bounds of the docstring."""
    lr, decay, l1, b1, mode, eps, b2 = hp
    g0 = graw * gscale
    r, R = _decay_term(w, decay, l1)
    G = np.abs(g0) + (0.0 if mode == 5 else abs(decay) * R)
    g = g0 if mode == 5 else g0 + decay * r
    dg = gamma(kg) * G
    nw, n1, n2 = adam_oracle(w, graw, s1, s2, hp, gscale, c1, c2)
    ag = np.abs(g)
    dec = abs(lr * decay) * R if mode == 5 else 0.0
    if mode == 6:
        v = n1
        bv = (1.0 - b2) * ((ag + dg) ** 2 - ag ** 2) + gamma(5) * v
        st = np.abs(lr * g) / (np.sqrt(v) + eps)
        stp = abs(lr) * (ag + dg) / (np.sqrt(np.maximum(v - bv, 0.0)) + eps)
        b1_, b2_, k = bv, np.zeros_like(w), 5
    else:
        m, v = n1, n2
        bm = (1.0 - b1) * dg + gamma(4) * (np.abs(b1 * s1) +
                                           np.abs((1.0 - b1) * g))
        bv = (1.0 - b2) * ((ag + dg) ** 2 - ag ** 2) + gamma(5) * v
        st = np.abs(lr * c1 * m) / (np.sqrt(v) * c2 + eps)
        stp = abs(lr * c1) * (np.abs(m) + bm) / (
            np.sqrt(np.maximum(v - bv, 0.0)) * c2 + eps)
        b1_, b2_, k = bm, bv, 7
    bw = (stp - st) + gamma(k) * stp + gamma(6) * dec + \
        gamma(2) * (np.abs(w) + dec + stp)
    return (nw, n1, n2), (bw, b1_, b2_)


def solver_ref(w, grad, s1, s2, segs, gscale, zero_from, step, kg=6,
               variant=None):
    """One update of a table of any modes on float64 copies of float32 state
    (hyper-parameters through float32, as the packed table holds them)."""
    w, grad = np.array(w, np.float64), np.array(grad, np.float64)
    s1, s2 = np.array(s1, np.float64), np.array(s2, np.float64)
    n = w.size
    seg = _segment_of(n, segs)
    out = [w.copy(), s1.copy(), s2.copy()]
    bnd = [np.zeros(n), np.zeros(n), np.zeros(n)]
    for k, (b, e, lr, decay, l1, moment, mode, eps, rho) in enumerate(segs):
        m = seg == k
        if mode >= 4:
            hp = (f32(lr), f32(decay), f32(l1), f32(moment), int(mode),
                  f32(eps), f32(rho))
            c1, c2 = bias_correction_ref(moment, rho, step) \
                if mode != 6 else (0.0, 0.0)
            args = (w[m], grad[m], s1[m], s2[m], hp, gscale, c1, c2)
            res, bd = _adam_bounds(*args, kg)
            if variant is not None:
                res = adam_oracle(*args, variant=variant)
        else:
            hp = [f32(lr), f32(moment), int(mode), f32(eps), f32(rho)]
            g, G = _gradient(w[m], grad[m], gscale, f32(decay), f32(l1))
            dg = gamma(kg) * G
            mid = _solver_modes(w[m], g, s1[m], s2[m], *hp)
            lo = _solver_modes(w[m], g - dg, s1[m], s2[m], *hp)
            hi = _solver_modes(w[m], g + dg, s1[m], s2[m], *hp)
            res = mid[:3]
            bd = [np.maximum(np.abs(lo[q] - mid[q]), np.abs(hi[q] - mid[q])) +
                  gamma(SOLVER_K[hp[2]][q]) * mid[3 + q] for q in range(3)]
        for q in range(3):
            out[q][m] = res[q]
            bnd[q][m] = bd[q]
    ng = grad.copy()
    ng[zero_from:] = 0.0
    lr_of = np.ones(n)
    for k, sg in enumerate(segs):
        lr_of[seg == k] = sg[2]
    return dict(w=out[0], s1=out[1], s2=out[2], grad=ng, bw=bnd[0],
                b1=bnd[1], b2=bnd[2], inseg=seg >= 0, lr=lr_of)


def check_update(before, after, lp, segs, gscale, zf, step, r, tag, kg=6):
    """before / after: (w, grad, s1, s2) float32 CPU tensors.  Returns the
    reference of this update."""
    ref = solver_ref(*[f64(t) for t in before], segs, gscale, zf, step, kg)
    ins = ref["inseg"]
    gap = torch.from_numpy(~ins)
    for q, name, bound in ((0, "w", "bw"), (2, "s1", "b1"), (3, "s2", "b2")):
        assert torch.equal(bits(after[q])[gap], bits(before[q])[gap]), \
            "%s touched outside every segment at %s" % (name, np.nonzero(
                (bits(after[q]) != bits(before[q])).numpy() & ~ins)[0][:8])
        r.see("%s_%s" % (tag, name), np.abs(f64(after[q]) - ref[name])[ins],
              ref[bound][ins])
    r["%s_bound_w/lr" % tag] = max(r.get("%s_bound_w/lr" % tag, 0.0),
                                   float((ref["bw"] / ref["lr"])[ins].max()))
    if lp is not None:
        assert same_bits(lp, after[0].to(BF)), "w_lp is not bf16(w)"
    assert torch.equal(bits(after[1])[:zf], bits(before[1])[:zf]), \
        "grad below zero_from"
    assert not bits(after[1])[zf:].any(), "grad not cleared from zero_from"
    return ref


def gradients(n, gen, zero=False):
    """|g| in [0.1, 1] with a random sign (sqrt(v) stays far above eps)."""
    if zero:
        return torch.zeros(n)
    mag = torch.rand(n, generator=gen) * 0.9 + 0.1
    sgn = torch.randint(0, 2, (n,), generator=gen).float() * 2.0 - 1.0
    return mag * sgn


def start_state(n, seed=0):
    """Non-zero w everywhere (+0 and -0 planted); states that start from a
    pattern in the gaps, so a touched gap shows, and from 0 in the segments."""
    g = torch.Generator().manual_seed(1000 + n + seed)
    w = torch.randn(n, generator=g)
    z = torch.arange(5, n, 11)
    w[z[0::2]] = 0.0
    w[z[1::2]] = -0.0
    return w, g


def place(t, dev, offset=0):
    """A device copy of t that starts ``offset`` elements into a buffer (1:
    off the 16-byte grid)."""
    hold = torch.zeros(t.numel() + offset, dtype=t.dtype, device=dev)
    v = hold[offset:]
    v.copy_(t)
    return v


def run_adam(dev, name, zero, steps=STEPS, first_step=1, n=N, offset=0,
             zero_grads=False, segs=None, gscale=GSCALE, clip=None,
             variants=()):
    """``steps`` updates of one table from update number ``first_step``.
    clip: None, or a factor: clip_norm = factor * the pre-clip norm of each
    update's scaled gradient.  Returns (ratios, final state on the CPU,
    worst |variant - oracle| / bound per variant)."""
    r = Ratios()
    segs = table(name) if segs is None else segs
    w0, gen = start_state(n)
    seg = _segment_of(n, segs)
    gapv = torch.from_numpy(np.where(seg < 0, 0.25, 0.0).astype(np.float32))
    w, s1, s2 = place(w0, dev, offset), place(gapv, dev, offset), \
        place(gapv * 2, dev, offset)
    lp = torch.full((n,), 7.0, dtype=BF, device=dev)
    zf = zero
    sq = torch.zeros(1, device=dev)
    wrong = {v: 0.0 for v in variants}
    for it in range(steps):
        t = first_step + it
        gr = gradients(n, gen, zero_grads)
        before = (w.cpu().clone(), gr.clone(), s1.cpu().clone(),
                  s2.cpu().clone())
        gd = place(gr, dev, offset)
        kw, gs, kg = {}, f32(gscale), 6
        if clip is not None:
            ops.grad_sqnorm(gd, out=sq)
            norm = f32(gscale) * math.sqrt(float(sq.cpu()[0]))
            kw = {"sqnorm": sq, "clip_norm": clip * norm}
            # the float32 coefficient, as the kernel's threads compute it
            c32 = np.float32(kw["clip_norm"]) / (
                np.float32(gscale) * np.sqrt(np.float32(float(sq.cpu()[0])))
                + np.float32(1e-6))
            gs = float(np.float32(gscale) * min(np.float32(1.0), c32))
            kg = 8
            assert (gs < f32(gscale)) == (clip < 1.0)
        ops.solver_update(w, gd, s1, s2, segs, w_lp=lp, gscale=gscale,
                          zero_grad=zf if zf < n else False, step=t, **kw)
        after = (w.cpu(), gd.cpu(), s1.cpu(), s2.cpu())
        ref = check_update(before, after, lp.cpu(), segs, gs, zf, t, r, name,
                           kg)
        for v in variants:
            bad = solver_ref(*[f64(x) for x in before], segs, gs, zf, t,
                             variant=v)
            ins = ref["inseg"]
            wrong[v] = max(wrong[v], float(
                (np.abs(bad["w"] - ref["w"])[ins] / ref["bw"][ins]).max()))
    return r, (w.cpu(), s1.cpu(), s2.cpu()), wrong


def sqnorm_bound(n, gpu):
    """Relative bound of the float32 sum of squares of n values.  Each square
    is one rounding (none as fma); a float32 sum of k non-negative terms in
    ANY order is within gamma(k - 1) of the exact one.  CPU path: chunks of
    4096, then the chunk sums.  Kernels: a thread's chain (its share of the
    float4s of at most 2048 x 256 threads, 4 terms each, plus up to 6 head
    and tail elements), 6 wave steps, 2 through LDS, then up to 8 partials
    per thread of the second launch and the same 8 steps."""
    if gpu:
        chain = 4 * -(-max(n // 4, 1) // (2048 * 256)) + 6
        return gamma(1 + chain + 8 + 8 + 8)
    return gamma(1 + 4096 + n // 4096 + 1)


def sqnorm_input(n, seed=0):
    g = torch.Generator().manual_seed(77 + n + seed)
    return torch.randn(n, generator=g)


def check_sqnorm(x, got, gpu, r=None):
    want = float((f64(x) ** 2).sum())
    r = Ratios() if r is None else r
    r.see("sqnorm", abs(float(got.cpu()[0]) - want),
          sqnorm_bound(x.numel(), gpu) * want)
    return r


# ========================================================= CPU-path tests
CPU = "cpu"


@pytest.mark.parametrize("rule", ["adam", "adamw", "rmsprop"])
def test_oracle_against_torch(rule):
    """The oracle (l1 = 0, exact c1 and c2) against float64 torch.optim over
    12 updates, to 1e-12 relative."""
    n, lr, decay, eps = 257, 1e-2, 1e-2, 1e-3
    gen = torch.Generator().manual_seed(5)
    w = torch.randn(n, generator=gen, dtype=torch.float64)
    p = torch.nn.Parameter(w.clone())
    opt = {"adam": lambda: torch.optim.Adam(
               [p], lr=lr, betas=(BETA1, BETA2), eps=eps, weight_decay=decay),
           "adamw": lambda: torch.optim.AdamW(
               [p], lr=lr, betas=(BETA1, BETA2), eps=eps, weight_decay=decay),
           "rmsprop": lambda: torch.optim.RMSprop(
               [p], lr=lr, alpha=ALPHA, eps=eps, weight_decay=decay)}[rule]()
    mode = ops.SOLVERS[rule]
    hp = (lr, decay, 0.0, BETA1, mode, eps, ALPHA if mode == 6 else BETA2)
    ww, s1, s2 = w.numpy().copy(), np.zeros(n), np.zeros(n)
    for t in range(1, STEPS + 1):
        g = gradients(n, gen).double()
        p.grad = g * GSCALE
        opt.step()
        c1, c2 = bias_correction_ref(BETA1, BETA2, t, exact=True)
        ww, s1, s2 = adam_oracle(ww, g.numpy(), s1, s2, hp, GSCALE, c1, c2)
        d = np.abs(p.detach().numpy() - ww).max()
        assert d <= 1e-12 * np.abs(ww).max(), (t, d)


def test_solver_codes_and_packing():
    assert ops.SOLVERS == {"momentum": 0, "adagrad": 1, "adadelta": 2,
                           "rprop": 3, "adam": 4, "adamw": 5, "rmsprop": 6}
    old = [(0, 8, 0.1, 0.0, 0.0, 0.9, m, 1e-6, 0.9) for m in range(4)]
    assert len(ops._pack_solver_segs(old)) % len(old) == 0
    one = ops._pack_solver_segs(table("adam"), step=3)
    assert len(one) == 3 * len(ops._pack_solver_segs(old)) // 4
    assert one != ops._pack_solver_segs(table("adam"), step=4)
    # rmsprop carries no bias correction: no step needed, none packed
    assert ops._pack_solver_segs(table("rmsprop")) == \
        ops._pack_solver_segs(table("rmsprop"), step=9)
    assert ops.bias_correction(BETA1, BETA2, 7) == \
        bias_correction_ref(BETA1, BETA2, 7)


@pytest.mark.parametrize("zero", ZERO_FROM)
@pytest.mark.parametrize("name", TABLES)
def test_cpu_update(name, zero):
    r, _, _ = run_adam(CPU, name, zero)
    print("worst |error| / bound, %s zero_from %d: %s" % (name, zero, dict(r)))
    assert all(("%s_%s" % (name, k)) in r for k in ("w", "s1", "s2"))


@pytest.mark.parametrize("name", TABLES)
def test_cpu_step_1000(name):
    r, _, _ = run_adam(CPU, name, 514, steps=1, first_step=1000)
    print("worst |error| / bound at step 1000, %s: %s" % (name, dict(r)))


@pytest.mark.parametrize("name", TABLES)
def test_cpu_zero_gradients(name):
    """m and v stay 0 where nothing but the gradient feeds them (AdamW
    everywhere, the other rules where decay = 0), and w moves by decay only."""
    r, (w, s1, s2), _ = run_adam(CPU, name, 0, steps=3, zero_grads=True)
    w0, _ = start_state(N)
    check_zero_gradients(name, w0, w, s1, s2)


def check_zero_gradients(name, w0, w, s1, s2):
    segs = table(name)
    seg = _segment_of(N, segs)
    for k, sg in enumerate(segs):
        m = torch.from_numpy(seg == k)
        if sg[3] == 0.0 or sg[6] == 5:
            assert not s1[m].any() and not s2[m].any(), (name, k)
        if sg[3] == 0.0:
            assert torch.equal(bits(w)[m], bits(w0)[m]), (name, k)
        else:
            moved = (w[m] != w0[m]) | (w0[m] == 0)
            assert moved.all(), (name, k)


def test_discrimination():
    """Wrong rules leave the bound by step 12: an implementation of one of
    them cannot pass ``run_adam``."""
    for name, variants in (("adam", ("nobias", "eps_in_root")),
                           ("rmsprop", ("eps_in_root",)),
                           ("adamw", ("decay_in_moments",))):
        _, _, wrong = run_adam(CPU, name, N, variants=variants)
        print("wrong variants, |variant - oracle| / bound:", name, wrong)
        for v in variants:
            assert wrong[v] > 1.0, (name, v, wrong[v])


@pytest.mark.parametrize("name", TABLES + ["momentum"])
def test_cpu_clip(name):
    run_clip(CPU, name)


def momentum_table():
    return [(b, e, LR[k], DECAY[k], L1[k], 0.9, 0, 0.0, 0.0)
            for k, (b, e) in enumerate(BOUNDS)]


def run_clip(dev, name, n=N, offset=0):
    segs = momentum_table() if name == "momentum" else table(name)
    # clip_norm above the norm: the bits of the unclipped call.  On the GPU
    # an unclipped table of modes 0 - 3 runs the older solver_kernel, whose
    # product-sums the compiler contracts as it likes; there the call that
    # cannot clip (clip_norm = inf) stands for it, and run_adam holds both
    # to the oracle with the coefficient 1.
    old_only = all(sg[6] < 4 for sg in segs) and str(dev) != "cpu"
    _, free, _ = run_adam(dev, name, 514, steps=3, segs=segs, n=n,
                          offset=offset,
                          clip=float("inf") if old_only else None)
    _, loose, _ = run_adam(dev, name, 514, steps=3, segs=segs, clip=1.5, n=n,
                           offset=offset)
    for a, b in zip(free, loose):
        assert same_bits(a, b), "a clip above the norm changed the update"
    # at half the norm: the oracle with the float32 coefficient
    r, tight, _ = run_adam(dev, name, 514, steps=3, segs=segs, clip=0.5, n=n,
                           offset=offset)
    assert not same_bits(free[0], tight[0])
    return r


@pytest.mark.parametrize("n", [1, 3, 4, 255, 1027, 4096 * 3 + 5])
def test_cpu_sqnorm(n):
    x = sqnorm_input(n)
    r = check_sqnorm(x, ops.grad_sqnorm(x), False)
    out = torch.full((1,), 7.0)
    assert ops.grad_sqnorm(x[1:] if n > 1 else x, out=out) is out
    assert float(ops.grad_sqnorm(torch.zeros(n))[0]) == 0.0
    print("sqnorm n %d: |error| / bound %s" % (n, dict(r)))


def test_errors():
    w, _ = start_state(N)
    z = torch.zeros(N)
    for name in ("adam", "adamw", "mixed"):
        for kw in ({}, {"step": 0}, {"step": None}):
            with pytest.raises(ValueError):
                ops.solver_update(w.clone(), z.clone(), z.clone(), z.clone(),
                                  table(name), **kw)
    # rmsprop and the old modes need none
    ops.solver_update(w.clone(), z.clone(), z.clone(), z.clone(),
                      table("rmsprop"))
    ops.solver_update(w.clone(), z.clone(), z.clone(), z.clone(),
                      momentum_table())
