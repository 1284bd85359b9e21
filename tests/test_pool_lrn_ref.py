"""Float64 references for pooling (max / avg / maxabs, the 2 x 2 argmax-free
pair), across-channel LRN and the fused LRN -> 3 x 3 max pooling, with the
cases and the checks that hold an implementation to them.

The references are plain vectorised NumPy, written from the formulas in
docs/OPS.md and the kernel comments of csrc/kernels/pool_lrn.hip; none of them
calls into veles_amd.ops (the output geometry is counted window by window in
``out_size`` and ``ops.pool_out_size`` is held to it).  Inputs are drawn in
bfloat16 and widened exactly, so maxima, ties and indices of the references
are exact.

The ``run_*`` functions run one case through ``veles_amd.ops`` on a device and
assert every bound.  The tests of this file do that for the float32 CPU paths
(no GPU needed: this is how the references themselves are checked);
tests/test_pool_lrn_gpu.py imports the same helpers for the HIP kernels.
Each ``run_*`` returns the worst measured error / bound ratios.

Checks and bounds (u = 2^-24, one float32 rounding; gamma(k) = k u / (1 - k u);
all derived, none measured):

* max / maxabs forward: selection, no arithmetic.  y is bitwise the bf16 input
  element the reference chose (first in row-major window order on a tie,
  maxabs by |v| with the signed value kept), argmax equal everywhere.
* avg forward and every pooling backward: ``bf_half_ulp(ref) + gamma(m + 2) A
  |d| + A e_d``.  m is the number of summed terms, A the sum of their absolute
  values (avg: divided by the clipped count), d the activation derivative of
  aux and e_d its own evaluation error.  The m - 1 additions, the reciprocal
  count and its product (avg) and the product with d are at most m + 2
  roundings.  A pixel that no window covers has A = 0: exactly 0 is required.
* the activation derivative (hvk_common.h act_bwd), e_d:
  tanh, c1 - c2 y^2 with c1 = 0.6666 * 1.7159 and c2 = 0.6666 / 1.7159 folded
  in float32 (3 roundings each), two products and the difference:
  gamma(6) (c1 + c2 y^2);
  softplus, 1 - __expf(-y): __expf is 2^(y log2 e); rounding log2 e and the
  product moves the result by 2 |y| u relatively, the hardware exponential is
  taken as 1 ulp = 2 u and counted twice (see below), the difference rounds
  once: exp(-y) (2 |y| + 5) u + u |d|;
  strict ReLU: exact;  sigmoid, y (1 - y): gamma(2) |d|.
* standalone LRN, y = x s^-beta with s = k + alpha sum x^2 over m = 2 (n // 2)
  + 1 channels: ``bf_half_ulp(ref) + e32``, e32 = |y| (beta e_s + ln 2 beta L
  5 u + 5 u): e_s = gamma(m + 4) is the relative error of s (m squares, m - 1
  additions, alpha and k, all terms non-negative; two more for alpha and k
  passing through float32); the rounding of -beta log2(s) moves the result by
  ln 2 beta |log2 s| u relatively; the hardware logarithm and exponential
  (v_log_f32, v_exp_f32) are TAKEN AS 1 ulp each, AMD's published figure,
  ASSUMED here and not measured - nothing in this repository states or
  measures their accuracy - and counted twice, 4 u each: the logarithm's 4 u
  is relative to L = max(|log2 s|, 1) (an error in ulps of a result near 0,
  s near 1, is read as the same error at 1), the exponential's to y; the last
  u is the product with x.  About 2^-19 of y against a half-ulp of at least
  2^-9: the term decides near-ties and cancellation only.
* LRN backward, dx_c = g_c s_c^-beta - 2 alpha beta x_c sum_j t_j with t_j =
  g_j x_j s_j^(-beta-1): the two terms cancel, so e32 scales with their
  absolute values, ``|g| s^-beta r(beta) + 2 alpha beta |x_c| (sum_j |t_j|
  r_j(beta + 1) + gamma(m + 14) sum_wide |t_j|)`` plus one u of both for the
  difference.  r(b) = b e_sb + ln 2 b Lb 6 u + e_sb + 8 u.  The block kernel
  slides its window sums along the 8 channels of a lane (w_q = w_(q-1) +
  e_new - e_old): a sum then carries the roundings of up to 14 more
  operations, each relative to a partial sum over channels at most n // 2 + 7
  away, hence e_sb = gamma(m + 22) s_wide / s and the gamma(m + 14) term over
  the wide window (sum_wide, s_wide: half-width n // 2 + 7).  The same kernel
  works with s / c and c s^(-beta-1), c = 2 alpha beta, so its logarithm and
  the sum with -beta log2 c round relative to Lb = |log2 s| + |log2 c| + 1
  (one rounding more than the forward: 6 u); s^-beta as the product
  s^(-beta-1) s adds e_sb + u; the remaining products are inside the 8 u.
  g is dy itself (standalone) or the sum of the at most four window gradients
  that chose the pixel (fused): three additions, gamma(3) of the sum of their
  absolute values, which replaces |g| throughout.
* fused LRN -> pool forward: the LRN output is NOT rounded before the maximum
  (the kernels never store it).  y: ``bf_half_ulp(ref) + E`` with E the
  largest e32 of the window.  argmax: (1) the element the implementation
  chose must be a near-maximiser, its reference value at least the reference
  maximum minus 2 E; (2) wherever the float64 gap between the best and the
  second-best window element exceeds 2 E the index must equal the
  reference's; so it must where n // 2 = 0 or alpha = 0 and the window's
  maximisers hold the same bf16 input (a value then depends on its own
  element alone, equal inputs are equal in any arithmetic, and the first
  wins).  The share of windows that rule (2) leaves out is asserted to
  be at most 0.5 % on the reference alone, before the implementation is
  looked at.
"""
import functools

import numpy as np
import pytest
import torch

import veles_amd.ops as ops
from test_step_tail_ref import (BF, U, Ratios, bf_half_ulp, f32, f64, gamma,
                                same_bits)

LN2 = float(np.log(2.0))
MODES = ["max", "avg", "maxabs"]
# gap-rule shares per fused case (filled by run_lrn_pool, printed by the GPU
# file's report)
LEFT_OUT = {}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def bf_normal(shape, seed, scale=2.0):
    return (torch.randn(shape, generator=_gen(seed)) * scale).to(BF)


def bf_ties(shape, seed):
    """Multiples of 0.25 in [-2, 2] with sign pairs: a 3 x 3 window usually
    holds ties, maxabs meets +a against -a; no negative zero."""
    g = _gen(seed)
    q = torch.randint(0, 9, shape, generator=g).float() * 0.25
    s = torch.randint(0, 2, shape, generator=g).float() * 2.0 - 1.0
    return (q * s + 0.0).to(BF)


# ================================================================ references
def out_size(size, kernel, stride):
    """Windows start at 0, stride, ...: another one is added while the last
    one ends before the input does (partial windows at the far edge are kept)
    and the new one still starts inside the input."""
    n = 1
    while (n - 1) * stride + kernel < size and n * stride < size:
        n += 1
    return n


def windows(x, ky, kx, sy, sx):
    """The taps of every window, row-major window order on axis 0:
    values [T, N, OH, OW, C], flat input indices, validity [T, 1, OH, OW, 1]
    (the window is clipped at the far edge)."""
    N, H, W, C = x.shape
    OH, OW = out_size(H, ky, sy), out_size(W, kx, sx)
    flat = np.arange(x.size, dtype=np.int64).reshape(x.shape)
    vals, idx, valid = [], [], []
    for dy in range(ky):
        for dx in range(kx):
            h, w = np.arange(OH) * sy + dy, np.arange(OW) * sx + dx
            hc, wc = np.minimum(h, H - 1), np.minimum(w, W - 1)
            vals.append(x[:, hc][:, :, wc])
            idx.append(flat[:, hc][:, :, wc])
            valid.append(((h < H)[:, None] & (w < W)[None, :])[None, :, :, None])
    return (np.ascontiguousarray(np.stack(vals)),
            np.ascontiguousarray(np.stack(idx)), np.stack(valid))


def _pick(a, t):
    return np.take_along_axis(a, t[None], 0)[0]


def pool_ref(x, ky, kx, sy, sx, mode):
    """y and the flat argmax (None for avg) of an NHWC float64 array."""
    x = np.asarray(x, np.float64)
    vals, idx, valid = windows(x, ky, kx, sy, sx)
    if mode == "avg":
        return np.where(valid, vals, 0.0).sum(0) / valid.sum(0), None
    key = np.abs(vals) if mode == "maxabs" else vals
    t = np.where(valid, key, -np.inf).argmax(0)     # first maximiser
    return _pick(vals, t), _pick(idx, t)


def act_bwd_ref(y, code):
    """The activation derivative through the output y, and the bound on the
    float32 evaluation error of it (module docstring)."""
    y = np.asarray(y, np.float64)
    if code == 1:
        c1, c2 = 0.6666 * 1.7159, 0.6666 / 1.7159
        return c1 - c2 * y * y, gamma(6) * (c1 + c2 * y * y)
    if code == 2:
        d = 1.0 - np.exp(-y)
        return d, np.exp(-y) * (2.0 * np.abs(y) + 5.0) * U + U * np.abs(d)
    if code == 3:
        return (y > 0).astype(np.float64), np.zeros_like(y)
    if code == 4:
        d = y * (1.0 - y)
        return d, gamma(2) * np.abs(d)
    return np.ones_like(y), np.zeros_like(y)


def _pool_scatter(dy, argmax, x_shape, ky, kx, sy, sx, mode):
    """The gathered gradient before the activation derivative, the sum of the
    absolute values of its terms, and the number of terms per pixel."""
    dy = np.asarray(dy, np.float64)
    N, H, W, C = x_shape
    out = [np.zeros(x_shape), np.zeros(x_shape), np.zeros(x_shape)]
    one = np.ones_like(dy)
    if mode != "avg":
        am = np.asarray(argmax, np.int64).ravel()
        for o, t in zip(out, (dy, np.abs(dy), one)):
            np.add.at(o.reshape(-1), am, t.ravel())
        return out
    _, OH, OW, _ = dy.shape
    cnt = windows(np.zeros(x_shape), ky, kx, sy, sx)[2].sum(0)
    n = np.arange(N)
    for dh in range(ky):
        for dw in range(kx):
            h, w = np.arange(OH) * sy + dh, np.arange(OW) * sx + dw
            vh, vw = h < H, w < W
            at = np.ix_(n, h[vh], w[vw])    # one tap: every target differs
            for o, t in zip(out, (dy / cnt, np.abs(dy) / cnt, one)):
                o[at] += t[:, vh][:, :, vw]
    return out


def pool_bwd_ref(dy, argmax, x_shape, ky, kx, sy, sx, mode, aux=None, code=0,
                 bound=False):
    """dx: the scatter by index (max, maxabs) or dy / count over every
    covered pixel (avg), times the activation derivative of aux.  With
    ``bound`` also the per-element bound without the half-ulp of the store."""
    s, a, m = _pool_scatter(dy, argmax, x_shape, ky, kx, sy, sx, mode)
    d, ed = act_bwd_ref(aux, code) if aux is not None else (1.0, 0.0)
    dx = s * d
    if not bound:
        return dx
    return dx, gamma(m + 2) * a * np.abs(d) + a * ed


def wsum(a, half):
    """Sum over channels |j - c| <= half (last axis), zero outside."""
    C = a.shape[-1]
    p = np.pad(a, [(0, 0)] * (a.ndim - 1) + [(half, half)])
    return sum(p[..., i:i + C] for i in range(2 * half + 1))


def _lrn_par(alpha, beta, k):
    """The parameters as the library's C interface holds them."""
    return f32(alpha), f32(beta), f32(k)


def lrn_s(x, n, alpha, k):
    return k + alpha * wsum(x * x, n // 2)


def lrn_ref(x, n, alpha, beta, k):
    x = np.asarray(x, np.float64)
    alpha, beta, k = _lrn_par(alpha, beta, k)
    return x * lrn_s(x, n, alpha, k) ** -beta


def lrn_e32(x, n, alpha, beta, k):
    """The float32 error bound of lrn_ref's result (module docstring)."""
    x = np.asarray(x, np.float64)
    alpha, beta, k = _lrn_par(alpha, beta, k)
    s = lrn_s(x, n, alpha, k)
    m = 2 * (n // 2) + 1
    L = np.maximum(np.abs(np.log2(s)), 1.0)
    rel = beta * gamma(m + 4) + LN2 * beta * L * 5 * U + 5 * U
    return np.abs(x) * s ** -beta * rel


def lrn_bwd_ref(x, dy, n, alpha, beta, k, gabs=None, geps=0.0, bound=False):
    """The closed form (not autograd).  ``gabs`` / ``geps``: dy is itself a
    float32 sum, in error by geps of gabs, the sum of its absolute terms."""
    x, g = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    alpha, beta, k = _lrn_par(alpha, beta, k)
    half = n // 2
    s = lrn_s(x, n, alpha, k)
    sb, sb1 = s ** -beta, s ** (-beta - 1.0)
    cs = 2.0 * alpha * beta
    dx = g * sb - cs * x * wsum(g * x * sb1, half)
    if not bound:
        return dx
    ga = np.abs(g) if gabs is None else gabs
    m = 2 * half + 1
    wide = half + 7
    e_sb = gamma(m + 22) * (k + alpha * wsum(x * x, wide)) / s
    Lb = np.abs(np.log2(s)) + (abs(np.log2(cs)) if cs > 0 else 0.0) + 1.0

    def r(b):
        return b * e_sb + LN2 * b * Lb * 6 * U + e_sb + 8 * U
    ta = ga * np.abs(x) * sb1
    t1 = ga * sb
    t2 = cs * np.abs(x) * wsum(ta, half)
    e = t1 * (r(beta) + geps) + \
        cs * np.abs(x) * (wsum(ta * (r(beta + 1.0) + geps), half) +
                          gamma(m + 14) * wsum(ta, wide)) + U * (t1 + t2)
    return dx, e, t1 + t2


def lrn_pool_ref(x, n, alpha, beta, k, sy, sx):
    """3 x 3 max pooling of the UNROUNDED LRN.  Returns y, the flat argmax,
    the window-local index, the bound E, and the gap between the best and the
    second-best element of each window (inf for a single-element window)."""
    yl = lrn_ref(x, n, alpha, beta, k)
    vals, idx, valid = windows(yl, 3, 3, sy, sx)
    key = np.where(valid, vals, -np.inf)
    t = key.argmax(0)
    ev, _, _ = windows(lrn_e32(x, n, alpha, beta, k), 3, 3, sy, sx)
    E = np.where(valid, ev, 0.0).max(0)
    top = np.sort(key, 0)
    with np.errstate(invalid="ignore"):
        gap = top[-1] - top[-2]
    # n // 2 = 0 or alpha = 0: a value depends on its own element alone, so
    # maximisers that hold the same bf16 input are equal in any arithmetic
    # and the tie rule (the first wins) decides the window
    same = np.zeros(gap.shape, bool)
    if n // 2 == 0 or f32(alpha) == 0.0:
        xv, _, _ = windows(np.asarray(x, np.float64), 3, 3, sy, sx)
        xb = _pick(xv, t)
        same = (gap == 0) & np.where(key == top[-1], xv == xb, True).all(0)
    return dict(y=_pick(vals, t), argmax=_pick(idx, t), local=t, E=E,
                gap=gap, lrn=yl, same_input=same)


def lrn_pool_bwd_ref(x, dp, argmax, n, alpha, beta, k, aux=None, code=0):
    """lrn_bwd_ref of the pool gradient scattered by ``argmax`` (flat
    indices), times the activation derivative; returns dx and its bound
    without the half-ulp of the store."""
    x = np.asarray(x, np.float64)
    g, ga, _ = _pool_scatter(dp, argmax, x.shape, 3, 3, 0, 0, "max")
    dx, e, A = lrn_bwd_ref(x, g, n, alpha, beta, k, gabs=ga, geps=gamma(3),
                           bound=True)
    return _with_act(dx, e, A, aux, code)


def _with_act(dx, e, A, aux, code):
    """dx d and its bound: e |d| for the value, A e_d for the derivative's
    own error, one rounding of the product."""
    if aux is None:
        return dx, e
    d, ed = act_bwd_ref(aux, code)
    return dx * d, e * np.abs(d) + (A + e) * ed + U * np.abs(dx * d)


# ============================================================ cases and runs
# (N, H, W), ky, kx, sy, sx - numbered as in the pooling list of the tests'
# docstrings
POOL_GEOM = {
    1: ((2, 13, 13), 3, 3, 2, 2),     # full windows, odd sides
    2: ((2, 14, 12), 3, 3, 2, 2),     # last window clipped in both axes
    3: ((1, 9, 10), 3, 3, 3, 3),
    4: ((1, 11, 10), 3, 3, 4, 2),     # rows no window covers: exactly 0
    5: ((1, 7, 8), 3, 3, 1, 1),       # nine windows per pixel
    6: ((2, 8, 6), 2, 2, 2, 2),
    7: ((1, 7, 5), 2, 2, 2, 2),       # clipped
    8: ((1, 9, 7), 2, 3, 1, 2),       # ky != kx, sy != sx
    9: ((1, 8, 9), 3, 2, 3, 1),
    10: ((2, 2, 5), 3, 3, 2, 2),      # H below the window
    11: ((1, 1, 1), 3, 3, 2, 2),
    12: ((1, 3, 3), 3, 3, 2, 2),
    13: ((1, 12, 12), 3, 3, 4, 4),    # the ceil alone gave a 4th window
    14: ((1, 6, 6), 2, 2, 3, 3),      # likewise
}
# aux forms: none, a separate tensor with each code, aux is x with code 3
AUX_FORMS = [None, 1, 2, 3, 4, "x"]
POOL_CASES = [(g, C) for g in sorted(POOL_GEOM) for C in (16, 5)] + \
    [(g, C) for g in (2, 8) for C in (24, 20, 6)] + [(1, 256)]

POOL2_SHAPES = [(3, 14, 10, 24), (1, 2, 2, 8)]

LRN_SETS = {"main": (0.05, 0.75, 1.0), "alexnet": None,   # alpha 1e-4 / n
            "alpha0": (0.0, 0.75, 1.0), "k2": (0.05, 0.5, 2.0)}
LRN_P = (1, 5, 7)                 # 35 pixels
LRN_VEC = [(C, n) for C in (8, 16, 24, 96) for n in (1, 3, 4, 5, 7, 9)]
LRN_SCALAR = [(C, n) for C in (13, 5, 1, 70) for n in (3, 5, 11)] + [(16, 11)]

FUSED_I32 = [((2, 13, 13, 16), 2, 2), ((2, 14, 12, 8), 2, 2),
             ((1, 15, 15, 40), 3, 3), ((1, 11, 10, 16), 4, 2)]
FUSED_I32_N = (1, 5, 9)
# (1, 16, 17, 24): 64 % CV != 0, the last lane of a wave idles - in the
# backward; its last window row is clipped, so (1, 17, 17, 24) does the same
# for the forward walk
FUSED_U8 = [(2, 13, 13, 16), (1, 16, 17, 24), (1, 15, 15, 40), (1, 9, 9, 512),
            (1, 7, 7, 528), (2, 14, 12, 8), (1, 31, 9, 16), (1, 11, 133, 16),
            (1, 17, 17, 24)]
FUSED_U8_N = (1, 3, 5, 7, 9)


def lrn_params(name, n):
    return (1e-4 / n, 0.75, 1.0) if name == "alexnet" else LRN_SETS[name]


def placed(t, dev, skip=0):
    """``t`` on ``dev``, starting ``skip`` elements into a larger buffer."""
    if not skip:
        return t.contiguous().to(dev)
    hold = torch.zeros(t.numel() + skip, dtype=t.dtype, device=dev)
    v = hold[skip:].view(t.shape)
    v.copy_(t)
    return v


def blank(shape, dtype, dev, skip=0):
    return placed(torch.zeros(shape, dtype=dtype), dev, skip)


def _aux_for(form, x, shape, seed, dev, skip=0):
    """(tensor on dev or None, its float64 values or None, code)"""
    if form is None:
        return None, None, 0
    if form == "x":
        return x, f64(x), 3
    a = bf_normal(shape, seed + 977, 1.0)
    return placed(a, dev, skip), f64(a), form


def check_store(r, name, got, ref, extra):
    """A bf16 (or float32: the CPU paths of the fused forward) store of a
    float32 value within ``extra`` of ``ref``."""
    assert tuple(got.shape) == tuple(ref.shape), (name, got.shape, ref.shape)
    hu = bf_half_ulp(ref) if got.dtype == BF else 0.0
    r.see(name, np.abs(f64(got) - ref), hu + extra)


def run_pool(dev, geom, C, mode, data="normal", aux=None, skip=0,
             backward=True):
    """Forward and backward of one geometry; the backward is fed the
    reference's argmax, so it is tested apart from the forward.  ``skip``:
    every tensor starts that many bytes / 2 elements into a larger buffer."""
    (N, H, W), ky, kx, sy, sx = POOL_GEOM[geom] if isinstance(geom, int) \
        else geom
    r = Ratios()
    seed = 100 * H + 10 * W + C + 7 * ky + sy
    shape = (N, H, W, C)
    x0 = (bf_ties if data == "ties" else bf_normal)(shape, seed)
    xr = f64(x0)
    yr, amr = pool_ref(xr, ky, kx, sy, sx, mode)
    x = placed(x0, dev, skip)
    out = blank(yr.shape, BF, dev, skip)
    am = None if mode == "avg" else blank(yr.shape, torch.int32, dev,
                                          skip // 2)
    y, am = ops.pool_fwd(x, ky, kx, (sx, sy), mode, out=out, argmax=am)
    assert tuple(y.shape) == yr.shape
    if mode == "avg":
        ya, _ = pool_ref(np.abs(xr), ky, kx, sy, sx, "avg")
        cnt = windows(xr, ky, kx, sy, sx)[2].sum(0)
        check_store(r, "pool avg y", y, yr, (cnt + 2) * U * 1.0001 * ya)
    else:
        chosen = x0.reshape(-1)[torch.from_numpy(amr.reshape(-1))]
        assert same_bits(y.reshape(-1), chosen), "y is not the chosen input"
        assert np.array_equal(am.cpu().numpy().astype(np.int64), amr)
    if not backward:
        return r
    dy0 = bf_normal(yr.shape, seed + 1)
    a_dev, a_ref, code = _aux_for(aux, x, shape, seed, dev, skip)
    amd = None if mode == "avg" else placed(
        torch.from_numpy(amr.astype(np.int32)), dev, skip // 2)
    dx = ops.pool_bwd(placed(dy0, dev, skip), amd, shape, ky, kx, (sx, sy),
                      mode, aux=a_dev, aux_act=code,
                      out=blank(shape, BF, dev, skip))
    dxr, bnd = pool_bwd_ref(f64(dy0), amr, shape, ky, kx, sy, sx, mode,
                            aux=a_ref, code=code, bound=True)
    check_store(r, "pool %s dx" % ("avg" if mode == "avg" else "max"), dx,
                dxr, bnd)
    return r


def run_pool2(dev, shape, mode, aux=None):
    """The argmax-free 2 x 2 / stride-2 pair on tie data: the backward
    recomputes the choice from x."""
    N, H, W, C = shape
    r = Ratios()
    seed = 31 * H + W + C
    x0 = bf_ties(shape, seed)
    xr = f64(x0)
    yr, amr = pool_ref(xr, 2, 2, 2, 2, mode)
    x = x0.to(dev)
    y = ops.pool2_fwd(x, mode)
    if mode == "avg":
        ya, _ = pool_ref(np.abs(xr), 2, 2, 2, 2, "avg")
        check_store(r, "pool2 avg y", y, yr, gamma(6) * ya)
    else:
        chosen = x0.reshape(-1)[torch.from_numpy(amr.reshape(-1))]
        assert same_bits(y.cpu().reshape(-1), chosen)
    dy0 = bf_normal(yr.shape, seed + 1)
    a_dev, a_ref, code = _aux_for(aux, x, shape, seed, dev)
    dx = ops.pool2_bwd(x, dy0.to(dev), mode, aux=a_dev, aux_act=code)
    dxr, bnd = pool_bwd_ref(f64(dy0), amr, shape, 2, 2, 2, 2, mode,
                            aux=a_ref, code=code, bound=True)
    check_store(r, "pool2 %s dx" % ("avg" if mode == "avg" else "max"), dx,
                dxr, bnd)
    return r


def run_lrn(dev, C, n, pset="main", aux=None, backward=True):
    r = Ratios()
    par = lrn_params(pset, n)
    shape = LRN_P + (C,)
    seed = 13 * C + n
    x0 = bf_normal(shape, seed)
    xr = f64(x0)
    x = x0.to(dev)
    y = ops.lrn_fwd(x, n, *par)
    check_store(r, "lrn y", y, lrn_ref(xr, n, *par), lrn_e32(xr, n, *par))
    if not backward:
        return r
    dy0 = bf_normal(shape, seed + 1)
    a_dev, a_ref, code = _aux_for(aux, x, shape, seed, dev)
    dx = ops.lrn_bwd(x, dy0.to(dev), n, *par, aux=a_dev, aux_act=code)
    dxr, e, A = lrn_bwd_ref(xr, f64(dy0), n, *par, bound=True)
    dxr, e = _with_act(dxr, e, A, a_ref, code)
    check_store(r, "lrn dx", dx, dxr, e)
    return r


@functools.lru_cache(maxsize=None)
def fused_reference(shape, sy, sx, n, pset):
    """x (bf16, CPU), lrn_pool_ref of it with the windows the gap rule
    decides and the share it leaves out, and the parameters.  Computed once
    per case and shared; nothing changes it."""
    par = lrn_params(pset, n)
    x0 = bf_normal(shape, 17 * shape[1] + shape[3] + n)
    ref = lrn_pool_ref(f64(x0), n, *par, sy, sx)
    decided = (ref["gap"] > 2.0 * ref["E"]) | ref["same_input"]
    share = 1.0 - decided.mean()
    ref["decided"], ref["share"] = decided, share
    ref["name"] = "%s s%d%d n%d %s" % ("x".join(map(str, shape)), sy, sx, n,
                                       pset)
    return x0, ref, par


def check_fused_fwd(r, name, x_shape, ref, y, offsets):
    """y and the two argmax rules; ``offsets``: flat int64 indices."""
    check_store(r, name + " y", y, ref["y"], ref["E"])
    off = np.asarray(offsets, np.int64)
    assert off.shape == ref["argmax"].shape
    assert (off >= 0).all() and (off < ref["lrn"].size).all()
    chosen = ref["lrn"].reshape(-1)[off]
    # inside the window: same image, same channel, rows / columns of it
    assert np.array_equal(off % x_shape[3], ref["argmax"] % x_shape[3])
    short = ref["y"] - chosen
    r.see(name + " argmax near-maximiser", np.maximum(short, 0.0),
          2.0 * ref["E"])
    d = ref["decided"]
    assert np.array_equal(off[d], ref["argmax"][d]), \
        "%s: %d decided windows differ" % (
            name, int((off[d] != ref["argmax"][d]).sum()))


def run_lrn_pool_fwd(dev, shape, sy, sx, n, pset="main", u8=False):
    r = Ratios()
    x0, ref, par = fused_reference(shape, sy, sx, n, pset)
    # on the reference alone, before the implementation is looked at
    LEFT_OUT[ref["name"]] = ref["share"]
    assert ref["share"] <= 0.005, "gap rule leaves out %.3f %% of %s" % (
        100 * ref["share"], ref["name"])
    x = x0.to(dev)
    am = torch.zeros(ref["y"].shape, device=dev,
                     dtype=torch.uint8 if u8 else torch.int32)
    y, am = ops.lrn_pool_fwd(x, n, *par, 3, 3, (sx, sy), argmax=am)
    if u8:
        assert int(am.max()) <= 8
        am = ops.window_index_to_offsets(am, shape, 3, 3, (sx, sy))
    check_fused_fwd(r, "lrn_pool u8" if u8 else "lrn_pool i32", shape, ref, y,
                    am.cpu().numpy())
    return r


def run_lrn_pool_bwd(dev, shape, sy, sx, n, pset="main", u8=False, aux=None,
                     crafted=False):
    """The fused backward on REFERENCE-made argmax tensors: the reference's
    own, or crafted ones (full windows, stride 2): ``"corner"``, every window
    names its bottom-right element, a pixel that four windows share;
    ``"shared"``, the four windows that share such a pixel all name it
    (window (oh, ow) names row 2 if oh is even, else row 0, columns
    likewise), so it sums four gradients."""
    r = Ratios()
    x0, ref, par = fused_reference(shape, sy, sx, n, pset)
    xr = f64(x0)
    local, flat = ref["local"], ref["argmax"]
    if crafted:
        vals, idx, valid = windows(xr, 3, 3, sy, sx)
        assert valid.all() and (sy, sx) == (2, 2), "crafted: full windows"
        N, OH, OW, C = local.shape
        row = np.where(np.arange(OH) % 2 == 0, 2, 0)[None, :, None, None]
        col = np.where(np.arange(OW) % 2 == 0, 2, 0)[None, None, :, None]
        local = np.broadcast_to(row * 3 + col, local.shape) if \
            crafted == "shared" else np.full(local.shape, 8, np.int64)
        local = np.ascontiguousarray(local, np.int64)
        flat = _pick(idx, local)
        terms = _pool_scatter(np.ones(flat.shape), flat, xr.shape, 3, 3, 0,
                              0, "max")[2]
        assert terms.max() == (4 if crafted == "shared" else 1)
    x = x0.to(dev)
    dp0 = bf_normal(flat.shape, 3 * shape[2] + n)
    am = torch.from_numpy(np.ascontiguousarray(
        local.astype(np.uint8) if u8 else flat.astype(np.int32))).to(dev)
    a_dev, a_ref, code = _aux_for(aux, x, shape, 5 + n, dev)
    dx = ops.lrn_pool_bwd(x, dp0.to(dev), am, n, *par, 3, 3, (sx, sy),
                          aux=a_dev, aux_act=code)
    dxr, e = lrn_pool_bwd_ref(xr, f64(dp0), flat, n, *par, aux=a_ref,
                              code=code)
    check_store(r, "lrn_pool dx u8" if u8 else "lrn_pool dx i32", dx, dxr, e)
    return r


# ===================================================== the float32 CPU paths
DEV = "cpu"


def test_pool_out_size():
    """ops.pool_out_size against the window count, everywhere; never a start
    outside the input; unchanged from the plain ceil wherever the stride is
    at most the kernel size; the two shapes of the defect."""
    for k in range(1, 5):
        for s in range(1, 7):
            for h in range(1, 41):
                got = ops.pool_out_size(h, h, k, k, s, s)
                assert got == (out_size(h, k, s),) * 2, (h, k, s)
                assert (got[0] - 1) * s < h
                if s <= k and h > k:
                    assert got[0] == (h - k + s - 1) // s + 1
    assert ops.pool_out_size(12, 12, 3, 3, 4, 4) == (3, 3)
    assert ops.pool_out_size(6, 7, 2, 2, 3, 3) == (2, 3)
    assert ops.pool_out_size(11, 10, 3, 3, 4, 2) == (3, 5)


@pytest.mark.parametrize("geom,C", POOL_CASES)
@pytest.mark.parametrize("mode", MODES)
def test_pool(geom, C, mode):
    for data in ("normal", "ties"):
        run_pool(DEV, geom, C, mode, data=data)


@pytest.mark.parametrize("geom", [2, 4, 5, 8, 13, 14])
@pytest.mark.parametrize("mode", MODES)
def test_pool_bwd_aux(geom, mode):
    for aux in AUX_FORMS[1:]:
        run_pool(DEV, geom, 16, mode, aux=aux)
        run_pool(DEV, geom, 5, mode, aux=aux)


@pytest.mark.parametrize("shape", POOL2_SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_pool2(shape, mode):
    for aux in (None, 1, "x"):
        run_pool2(DEV, shape, mode, aux=aux)


@pytest.mark.parametrize("C,n", LRN_VEC + LRN_SCALAR)
def test_lrn(C, n):
    for pset in sorted(LRN_SETS):
        run_lrn(DEV, C, n, pset)


@pytest.mark.parametrize("C,n", [(16, 5), (24, 9), (13, 5), (70, 11)])
def test_lrn_bwd_aux(C, n):
    for aux in AUX_FORMS[1:]:
        run_lrn(DEV, C, n, "main", aux=aux)


@pytest.mark.parametrize("shape,sy,sx", FUSED_I32)
@pytest.mark.parametrize("n", FUSED_I32_N)
def test_lrn_pool_i32(shape, sy, sx, n):
    for pset in ("main", "k2"):
        run_lrn_pool_fwd(DEV, shape, sy, sx, n, pset)
        run_lrn_pool_bwd(DEV, shape, sy, sx, n, pset)
    run_lrn_pool_bwd(DEV, shape, sy, sx, n, aux="x")


@pytest.mark.parametrize("shape", FUSED_U8)
@pytest.mark.parametrize("n", FUSED_U8_N)
def test_lrn_pool_u8(shape, n):
    run_lrn_pool_fwd(DEV, shape, 2, 2, n, u8=True)
    run_lrn_pool_bwd(DEV, shape, 2, 2, n, u8=True)


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("crafted", ["corner", "shared"])
def test_lrn_pool_bwd_crafted(u8, crafted):
    for aux in (None, 2, "x"):
        run_lrn_pool_bwd(DEV, (2, 13, 13, 16), 2, 2, 5, u8=u8, aux=aux,
                         crafted=crafted)


def test_references_see_the_window():
    """The mutants the older tests could not see move the references by many
    bounds: a window one channel narrower on each side, and the backward
    without its cross-channel term."""
    x = f64(bf_normal(LRN_P + (16,), 1))
    g = f64(bf_normal(LRN_P + (16,), 2))
    par = LRN_SETS["main"]
    y, e = lrn_ref(x, 5, *par), lrn_e32(x, 5, *par) + bf_half_ulp(
        lrn_ref(x, 5, *par))
    assert np.median(np.abs(lrn_ref(x, 3, *par) - y) / e) > 10
    dx, eb, _ = lrn_bwd_ref(x, g, 5, *par, bound=True)
    eb = eb + bf_half_ulp(dx)
    assert np.median(np.abs(lrn_bwd_ref(x, g, 3, *par) - dx) / eb) > 5
    a, b, k = _lrn_par(*par)
    no_cross = g * lrn_s(x, 5, a, k) ** -b
    assert np.median(np.abs(no_cross - dx) / eb) > 5
