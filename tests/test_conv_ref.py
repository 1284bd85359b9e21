"""Float64 references for the convolution forward, backward-data and weight
gradient (with the bias gradient), the integer data on which every kernel must
equal them bit for bit, the derived bounds for the epilogues that are not
exact, the cases per kernel path, and the wrong-rule references ("mutants")
that the cases must be able to tell from the true one.

The references are explicit tap loops in NumPy, written from the formulas in
docs/OPS.md: x is NHWC, w is [OC][KH][KW][C/g], ``sliding = (sx, sy)``,
``padding = (l, t, r, b)``, groups are blocked (group g owns input channels
[g C/g, (g + 1) C/g) and output channels [g OC/g, (g + 1) OC/g)):

    y[n, oh, ow, oc]   = bias[oc] + sum_{kh, kw, c} x[n, oh sy + kh - t,
                                    ow sx + kw - l, g C/g + c] w[oc, kh, kw, c]
    dx[n, ih, iw, g C/g + c] = f'(aux) sum over the (oh, kh), (ow, kw) with
                         oh sy + kh - t = ih, ow sx + kw - l = iw, and the oc
                         of group g, of dy[n, oh, ow, oc] w[oc, kh, kw, c]
    dW[oc, kh, kw, c] += sum_{n, oh, ow} dy[n, oh, ow, oc] x[n, oh sy + kh - t,
                         ow sx + kw - l, g C/g + c];  db[oc] += sum dy

(x outside the image is 0).  None of them calls into veles_amd.ops; the
output size is counted window by window (``out_len``) and
``ops.conv_out_size`` is held to it; the references are held to float64
torch (conv2d, conv2d_input, conv2d_weight) at 1e-12 relative on every case.
Each reference also returns A, the sum of the absolute values of the products
(plus |bias|, |dW0|, |db0|) per output, for the bounds.

Integer mode.  Every kernel multiplies bf16 values, accumulates in float32
and rounds once to bf16 (the weight gradient stays float32).  With x, dy in
{-1, 0, 1}, w in {-1, 0, 1} with a non-zero share of min(1, 1024 / K), K =
KH KW C/g, an integer bias in [-8, 8] and integer dW0 / db0 in
[-4, 4], every product and every partial sum is an integer below 2^24 in any
order, split or atomic, so the float32 sum is exact; with |pre-activation| <=
256 the result is a bf16 value.  The kernel must then equal the reference bit
for bit (linear and strict-ReLU epilogues, strict-ReLU derivative; the sign of
a zero is not compared: -5 * 0 and a select of 0 differ in it and in nothing
else).  The cap is a condition, not a measurement: ``assert_cap`` checks it on
the reference alone before a device result is looked at.  One dropped,
doubled or misplaced non-zero product moves an output by at least 1.

Bounded mode (u = 2^-24, gamma(k) = k u / (1 - k u); derived, not measured),
on bf16 normal data widened exactly, z the float64 pre-activation:

* forward: ``bf_half_ulp(ref) + L gamma(K + 3) A + e_act``, K the reduction
  length plus one for the bias; L the largest |f'| over [z - e, z + e], e =
  gamma(K + 3) A (tanh and sigmoid: |f'| is even and falls with |z|, taken at
  max(|z| - e, 0); softplus: f' rises, taken at z + e; else 1).  e_act, the
  activation's own float32 evaluation (hvk_common.h act_fwd), with the library
  functions tanhf and log1pf TAKEN AS accurate to ACT_ULPS = 16 units in the
  last place (the assumption of test_batchnorm_ref.py, one ulp <= 2 u of the
  value) and __expf(t) in error by (2 |t| + 4) u relatively (rounding log2 e
  and the product moves 2^(t log2 e) by 2 |t| u, the hardware exponential is
  taken as 1 ulp = 2 u and counted twice: test_pool_lrn_ref.py):
    tanh, 1.7159f * tanhf(0.6666f * z): the constant and the product move t =
    0.6666 z by 2 u relatively, tanh by sech^2(t) |t| 2 u; tanhf adds
    2 ACT_ULPS u |tanh t|; the outer constant and product 2 u |y|:
    1.7159 (sech^2(t) |t| + ACT_ULPS |tanh t|) 2 u + 2 u |y|;
    softplus, z > 15 ? z : log1pf(__expf(z)): with s = e^z / (1 + e^z) the
    exponential's error moves y by s (2 |z| + 4) u, log1pf adds 2 ACT_ULPS u y;
    where 15 lies within e of z the two branches may be taken differently,
    they differ by log1p(e^-15) < 3.1e-7;
    sigmoid, 1 / (1 + __expf(-z)): the exponential moves y by y (1 - y) (2 |z|
    + 4) u, the sum rounds once and the division is taken as 2.5 ulp = 5 u:
    y ((1 - y) (2 |z| + 4) + 6) u;
    linear and strict ReLU: 0.
* backward-data, dx = d dx0 with d the derivative through aux and e_d its own
  error (test_pool_lrn_ref.act_bwd_ref): ``bf_half_ulp(ref) + gamma(K + 3) A
  |d| + A e_d``, K = KH KW OC/g + 1 (the product with d is the one more), A >=
  |dx0| the sum of the absolute products.
* weight gradient: dW and db to ``gamma(P + splits + 2) A``, P = N OH OW terms,
  one more addition per split slice and for dW0.

gamma(n) A for a sum accumulated by MFMA instructions is the form
test_attention_ref.py uses: any order of n - 1 float32 additions of exact
bf16 products.

The tests of this file run every case through the float32 CPU paths of
``ops.conv_fwd`` / ``conv_dgrad`` / ``conv_wgrad`` (there the bf16 half-ulp is
the only output rounding): this is how the references themselves are checked.
tests/test_conv_exact_gpu.py imports the same helpers for the HIP kernels.
"""
import collections
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import veles_amd.ops as ops
from test_pool_lrn_ref import act_bwd_ref
from test_step_tail_ref import BF, U, Ratios, bf_half_ulp, f64, gamma, same_bits
from test_wgrad_halo_lean_model import CANDS as HALO_CANDS
from test_wgrad_halo_lean_model import SHAPES as HALO_MODEL_SHAPES
from test_wgrad_halo_lean_model import plan as halo_plan_square

ACT_ULPS = 16
CAP_BF16 = 256
CAP_F32 = 2 ** 24

_Case = collections.namedtuple(
    "Case", "name N H W C OC KH KW sliding padding groups tags")


class Case(_Case):
    """One convolution geometry; ``tags``: hashable (key, value) pairs the GPU
    tests read (forced configuration, which operations to run, ...)."""
    __slots__ = ()

    def tag(self, key, default=None):
        return dict(self.tags).get(key, default)

    @property
    def out(self):
        sx, sy = self.sliding
        pl, pt, pr, pb = self.padding
        return (out_len(self.H, self.KH, sy, pt, pb),
                out_len(self.W, self.KW, sx, pl, pr))

    @property
    def Cg(self):
        return self.C // self.groups

    @property
    def OCg(self):
        return self.OC // self.groups

    @property
    def P(self):
        OH, OW = self.out
        return self.N * OH * OW

    def does(self, op):
        return op in self.tag("ops", "fdw")

    def __str__(self):
        return self.name


def mk(name, N, H, W, C, OC, KH, KW, sliding=(1, 1), padding=(0, 0, 0, 0),
       groups=1, **tags):
    return Case(name, N, H, W, C, OC, KH, KW, tuple(sliding), tuple(padding),
                groups, tuple(sorted(tags.items())))


def swapped(c, name=None, **tags):
    """The case with C and OC exchanged: the backward-data of a kernel whose
    plan sees dY as its input needs the forward's channel counts mirrored."""
    t = dict(c.tags)
    t.update(tags)
    return c._replace(name=name or c.name + "_T", C=c.OC, OC=c.C,
                      tags=tuple(sorted(t.items())))


# ================================================================ references
def out_len(size, k, stride, p0, p1):
    """Windows start at -p0, -p0 + stride, ...: one is counted while it still
    ends inside the padded input."""
    n = 0
    while n * stride + k <= size + p0 + p1:
        n += 1
    return n


Rule = collections.namedtuple(
    "Rule", "swap_k flip swap_pad far_pad swap_stride interleave")
TRUE = Rule(False, False, False, False, False, False)


def _geometry(c, rule):
    """Row / column input indices per tap and the weight tap each one reads:
    [(flat weight tap, ih [OH], iw [OW])], and the channel lists per group."""
    sx, sy = c.sliding
    pl, pt, pr, pb = c.padding
    if rule.swap_stride:
        sx, sy = sy, sx
    if rule.swap_pad:
        pl, pt = pt, pl
    if rule.far_pad:
        pl, pt = pr, pb
    OH, OW = c.out
    taps = []
    for kh in range(c.KH):
        for kw in range(c.KW):
            wkh, wkw = (c.KH - 1 - kh, c.KW - 1 - kw) if rule.flip else (kh, kw)
            flat = wkw * c.KH + wkh if rule.swap_k else wkh * c.KW + wkw
            taps.append((flat, np.arange(OH) * sy + kh - pt,
                         np.arange(OW) * sx + kw - pl))
    G = c.groups
    if rule.interleave:
        cin = [np.arange(c.Cg) * G + g for g in range(G)]
        cout = [np.arange(c.OCg) * G + g for g in range(G)]
    else:
        cin = [np.arange(c.Cg) + g * c.Cg for g in range(G)]
        cout = [np.arange(c.OCg) + g * c.OCg for g in range(G)]
    return taps, cin, cout


def _a(v):
    """A tensor or an array as a float64 array (exactly)."""
    return f64(v) if torch.is_tensor(v) else np.asarray(v, np.float64)


def _gather(x, ih, iw):
    """x[:, ih][:, :, iw], zero where an index lies outside the image."""
    H, W = x.shape[1], x.shape[2]
    ok = ((ih >= 0) & (ih < H))[:, None] & ((iw >= 0) & (iw < W))[None, :]
    v = x[:, np.clip(ih, 0, H - 1)][:, :, np.clip(iw, 0, W - 1)]
    return v * ok[None, :, :, None]


def _wflat(c, w):
    return _a(w).reshape(c.OC, c.KH * c.KW, c.Cg)


def fwd_ref(c, x, w, bias=None, rule=TRUE):
    """The pre-activation y [N, OH, OW, OC] and A."""
    x = _a(x)
    wf = _wflat(c, w)
    taps, cin, cout = _geometry(c, rule)
    OH, OW = c.out
    y = np.zeros((c.N, OH, OW, c.OC))
    A = np.zeros_like(y)
    for g in range(c.groups):
        xg = x[..., cin[g]]
        for flat, ih, iw in taps:
            xs = _gather(xg, ih, iw)
            wk = wf[cout[g], flat, :]
            y[..., cout[g]] += xs @ wk.T
            A[..., cout[g]] += np.abs(xs) @ np.abs(wk).T
    if bias is not None:
        b = _a(bias)
        y += b
        A += np.abs(b)
    return y, A


def dgrad_ref(c, dy, w, rule=TRUE):
    """dx before the activation derivative, [N, H, W, C], and A."""
    dy = _a(dy)
    wf = _wflat(c, w)
    taps, cin, cout = _geometry(c, rule)
    dx = np.zeros((c.N, c.H, c.W, c.C))
    A = np.zeros_like(dx)
    n = np.arange(c.N)
    for g in range(c.groups):
        dg = dy[..., cout[g]]
        for flat, ih, iw in taps:
            okh, okw = (ih >= 0) & (ih < c.H), (iw >= 0) & (iw < c.W)
            wk = wf[cout[g], flat, :]
            at = np.ix_(n, ih[okh], iw[okw], cin[g])   # one tap: all differ
            dx[at] += (dg @ wk)[:, okh][:, :, okw]
            A[at] += (np.abs(dg) @ np.abs(wk))[:, okh][:, :, okw]
    return dx, A


def wgrad_ref(c, x, dy, dw0=None, db0=None, rule=TRUE):
    """dW [OC, KH, KW, C/g], its A, db [OC], its A."""
    x, dy = _a(x), _a(dy)
    taps, cin, cout = _geometry(c, rule)
    dw = np.zeros((c.OC, c.KH * c.KW, c.Cg))
    A = np.zeros_like(dw)
    for g in range(c.groups):
        xg = x[..., cin[g]]
        dg = dy[..., cout[g]].reshape(-1, c.OCg)
        for flat, ih, iw in taps:
            xs = _gather(xg, ih, iw).reshape(-1, c.Cg)
            dw[cout[g], flat, :] += dg.T @ xs
            A[cout[g], flat, :] += np.abs(dg).T @ np.abs(xs)
    dw, A = dw.reshape(c.OC, c.KH, c.KW, c.Cg), A.reshape(
        c.OC, c.KH, c.KW, c.Cg)
    db, Ab = dy.reshape(-1, c.OC).sum(0), np.abs(dy).reshape(-1, c.OC).sum(0)
    if dw0 is not None:
        dw, A = dw + _a(dw0), A + np.abs(_a(dw0))
    if db0 is not None:
        db, Ab = db + _a(db0), Ab + np.abs(_a(db0))
    return dw, A, db, Ab


def border_product(c, x, w, dy=None):
    """One non-zero product at a border pixel: (n, oh, ow, kh, kw, channel of
    x, ih, iw), the first in row-major order whose output pixel lies on the
    image's edge, whose tap reads inside the image and whose x (and, given dy,
    whose dy for some output channel; else whose w) is not zero."""
    x = _a(x)
    w = None if w is None else _a(w)
    dy = None if dy is None else _a(dy)
    sx, sy = c.sliding
    pl, pt = c.padding[0], c.padding[1]
    OH, OW = c.out
    for oh in range(OH):
        for ow in (range(OW) if oh in (0, OH - 1) else (0, OW - 1)):
            for kh in range(c.KH):
                for kw in range(c.KW):
                    ih, iw = oh * sy + kh - pt, ow * sx + kw - pl
                    if not (0 <= ih < c.H and 0 <= iw < c.W):
                        continue
                    for ch in range(c.C):
                        g = ch // c.Cg
                        oc = slice(g * c.OCg, (g + 1) * c.OCg)
                        other = w[oc, kh, kw, ch % c.Cg] if dy is None else \
                            dy[0, oh, ow, oc]
                        if x[0, ih, iw, ch] != 0 and other.any():
                            return 0, oh, ow, kh, kw, ch, ih, iw
    raise AssertionError("%s: no non-zero border product" % c.name)


def drop_fwd(c, y, x, w):
    """y without one tap's one channel at one border pixel."""
    n, oh, ow, kh, kw, ch, ih, iw = border_product(c, x, w)
    g = ch // c.Cg
    oc = slice(g * c.OCg, (g + 1) * c.OCg)
    y = np.array(y, np.float64)
    y[n, oh, ow, oc] -= _a(x)[n, ih, iw, ch] * _a(w)[oc, kh, kw, ch % c.Cg]
    return y


def drop_dgrad(c, dx, dy, w):
    """dx without the same product's transpose: one tap of one output pixel
    no longer reaches one input channel."""
    ones = np.ones((c.N, c.H, c.W, c.C))
    n, oh, ow, kh, kw, ch, ih, iw = border_product(c, ones, w, dy=dy)
    g = ch // c.Cg
    oc = slice(g * c.OCg, (g + 1) * c.OCg)
    dx = np.array(dx, np.float64)
    dx[n, ih, iw, ch] -= (_a(dy)[n, oh, ow, oc] *
                          _a(w)[oc, kh, kw, ch % c.Cg]).sum()
    return dx


def drop_wgrad(c, dw, x, dy):
    """dW without one border pixel's product for one tap and channel."""
    n, oh, ow, kh, kw, ch, ih, iw = border_product(c, x, None, dy=dy)
    g = ch // c.Cg
    oc = slice(g * c.OCg, (g + 1) * c.OCg)
    dw = np.array(dw, np.float64)
    dw[oc, kh, kw, ch % c.Cg] -= _a(dy)[n, oh, ow, oc] * _a(x)[n, ih, iw, ch]
    return dw


# the wrong rules: name -> (rule, operations it is a different rule for)
MUTANTS = {
    "kh_kw_swapped": (TRUE._replace(swap_k=True), "fdw"),
    "taps_flipped": (TRUE._replace(flip=True), "fw"),
    "pt_pl_swapped": (TRUE._replace(swap_pad=True), "fdw"),
    "far_padding_for_near": (TRUE._replace(far_pad=True), "fdw"),
    "sx_sy_swapped": (TRUE._replace(swap_stride=True), "fdw"),
    "groups_interleaved": (TRUE._replace(interleave=True), "fdw"),
    "one_product_dropped": (None, "fdw"),
    "dgrad_without_flip": (TRUE._replace(flip=True), "d"),
}


# ================================================================ activations
def act_ref(z, act):
    """f(z), the largest |f'| over [z - e, z + e] as a function of e, and the
    float32 evaluation error e_act (module docstring)."""
    z = np.asarray(z, np.float64)
    if act == 1:
        c, a = 0.6666, 1.7159
        t = c * z
        y = a * np.tanh(t)
        e_act = a * (np.abs(t) / np.cosh(t) ** 2 + ACT_ULPS * np.abs(
            np.tanh(t))) * 2 * U + 2 * U * np.abs(y)

        def lip(e):
            return a * c / np.cosh(c * np.maximum(np.abs(z) - e, 0.0)) ** 2
        return y, lip, e_act
    if act == 2:
        zc = np.minimum(z, 15.0)
        y = np.where(z > 15, z, np.log1p(np.exp(zc)))
        s = np.exp(zc) / (1.0 + np.exp(zc))
        e_act = np.where(z > 15, 0.0, s * (2 * np.abs(z) + 4) * U +
                         2 * ACT_ULPS * U * y)

        def lip(e):
            return 1.0 / (1.0 + np.exp(-(z + e)))
        return y, lip, (e_act, 3.1e-7)
    if act == 3:
        return np.maximum(z, 0.0), lambda e: 1.0, 0.0
    if act == 4:
        y = 1.0 / (1.0 + np.exp(-z))
        e_act = y * ((1.0 - y) * (2 * np.abs(z) + 4) + 6) * U

        def lip(e):
            s = 1.0 / (1.0 + np.exp(-np.maximum(np.abs(z) - e, 0.0)))
            return s * (1.0 - s)
        return y, lip, e_act
    return z, lambda e: 1.0, 0.0


def fwd_bound(z, A, K, act):
    """act(z) and the bound on a float32 evaluation of it from products
    summed in float32, without the half-ulp of the store."""
    e = gamma(K + 3) * A
    y, lip, e_act = act_ref(z, act)
    if isinstance(e_act, tuple):      # softplus: the branch at 15
        e_act = e_act[0] + np.where(np.abs(z - 15.0) <= e, e_act[1], 0.0)
    return y, lip(e) * e + e_act


# ====================================================================== data
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _seed(c, salt):
    return (1009 * c.H + 101 * c.W + 13 * c.C + 7 * c.OC + 3 * c.KH + c.KW +
            31 * c.N + salt) % (2 ** 31)


def _tri(shape, g):
    return torch.randint(-1, 2, shape, generator=g).float()


@functools.lru_cache(maxsize=None)
def data(c, mode):
    """CPU tensors of one case: x, dy, aux (bf16), w (bf16), bias, dw0, db0
    (float32).  Computed once per case and mode and shared; nothing changes
    them (the runs clone what a kernel writes into)."""
    OH, OW = c.out
    xs, ys = (c.N, c.H, c.W, c.C), (c.N, OH, OW, c.OC)
    ws = (c.OC, c.KH, c.KW, c.Cg)
    K = c.KH * c.KW * c.Cg
    if mode == "int":
        g = _gen(_seed(c, 1))
        x, dy, aux = _tri(xs, g), _tri(ys, g), _tri(xs, g)
        share = min(1.0, 1024.0 / K)
        w = _tri(ws, g)
        w = w * (torch.rand(ws, generator=g) < share)
        # a zero that no product stands behind tells nothing: keep the two
        # signs equally likely and the zeros of x / dy at a third
        bias = torch.randint(-8, 9, (c.OC,), generator=g).float()
        dw0 = torch.randint(-4, 5, ws, generator=g).float()
        db0 = torch.randint(-4, 5, (c.OC,), generator=g).float()
    else:
        g = _gen(_seed(c, 2))
        x = torch.randn(xs, generator=g)
        dy = torch.randn(ys, generator=g)
        aux = torch.randn(xs, generator=g)
        w = torch.randn(ws, generator=g) / float(c.KH * c.KW * c.Cg) ** 0.5
        bias = (torch.randn(c.OC, generator=g) * 0.5).to(BF).float()
        dw0 = torch.randn(ws, generator=g)
        db0 = torch.randn(c.OC, generator=g)
    return dict(x=x.to(BF), dy=dy.to(BF), aux=aux.to(BF), w=w.to(BF),
                bias=bias, dw0=dw0, db0=db0)


@functools.lru_cache(maxsize=None)
def reference(c, mode, op, bias=True):
    """The true reference of one case, operation ("f", "d", "w") and mode."""
    d = data(c, mode)
    if op == "f":
        return fwd_ref(c, f64(d["x"]), f64(d["w"]),
                       f64(d["bias"]) if bias else None)
    if op == "d":
        return dgrad_ref(c, f64(d["dy"]), f64(d["w"]))
    return wgrad_ref(c, f64(d["x"]), f64(d["dy"]), f64(d["dw0"]),
                     f64(d["db0"]))


def assert_cap(c, op, *refs):
    """The integer-mode condition, on the reference alone."""
    cap = CAP_F32 if op == "w" else CAP_BF16 + 1
    for r in refs:
        assert np.array_equal(r, np.round(r)), "%s: not integer" % c.name
        assert np.abs(r).max() < cap, "%s %s: |ref| up to %g" % (
            c.name, op, np.abs(r).max())


def _canon(t):
    """Without the sign of zero (module docstring)."""
    return t.detach().cpu() + 0.0


def exact_bf16(got, ref):
    """A bf16 result that is the float64 reference bit for bit."""
    want = torch.from_numpy(np.ascontiguousarray(ref)).to(BF)
    return tuple(got.shape) == ref.shape and got.dtype == BF and \
        np.array_equal(f64(want), ref) and same_bits(_canon(got), _canon(want))


def exact_f32(got, ref):
    want = torch.from_numpy(np.ascontiguousarray(ref)).float()
    return tuple(got.shape) == ref.shape and got.dtype == torch.float32 and \
        np.array_equal(f64(want), ref) and torch.equal(got.detach().cpu(), want)


def old_close(got, ref, tol=1e-2):
    """The rule of the older convolution tests."""
    return np.abs(f64(got) - ref).max() <= tol * (np.abs(ref).max() + 1e-6)


def _where(got, ref):
    bad = np.argwhere(f64(got) != ref)
    return "%d of %d differ, first at %s: got %s, reference %s" % (
        len(bad), ref.size, tuple(bad[0]), f64(got)[tuple(bad[0])],
        ref[tuple(bad[0])]) if len(bad) else "signs of zero / dtype / shape"


# ====================================================================== runs
def ops_fwd(c, x, w, bias, act, **kw):
    return ops.conv_fwd(x, w, bias, c.sliding, c.padding, c.groups, act, **kw)


def ops_dgrad(c, dy, w, aux, aux_act):
    return ops.conv_dgrad(dy, w, (c.N, c.H, c.W, c.C), c.sliding, c.padding,
                          c.groups, aux=aux, aux_act=aux_act)


def ops_wgrad(c, x, dy, dw, db, splits=None, col=None):
    ops.conv_wgrad(x, dy, dw, c.sliding, c.padding, c.groups, splits=splits,
                   col=col, dbias=db)


def run_fwd(c, dev, mode="int", act=3, bias=True, call=ops_fwd, tag="fwd"):
    """One forward: integer mode (act 0 or 3) bit for bit, bounded mode to the
    derived bound.  ``call(case, x, w, bias, act)`` returns y."""
    r = Ratios()
    d = data(c, mode)
    z, A = reference(c, mode, "f", bias)
    if mode == "int":
        assert act in (0, 3)
        assert_cap(c, "f", z)
    y = call(c, d["x"].to(dev), d["w"].to(dev),
             d["bias"].to(dev) if bias else None, act)
    assert tuple(y.shape) == z.shape
    if mode == "int":
        ref = np.maximum(z, 0.0) if act == 3 else z
        assert exact_bf16(y, ref), "%s %s act %d: %s" % (c.name, tag, act,
                                                         _where(y, ref))
        return r
    ref, bnd = fwd_bound(z, A, c.KH * c.KW * c.Cg + 1, act)
    r.see("%s act %d" % (tag, act), np.abs(f64(y) - ref),
          bf_half_ulp(ref) + bnd)
    return r


def run_dgrad(c, dev, mode="int", aux_act=3, call=ops_dgrad, tag="dgrad"):
    """One backward-data; ``aux_act`` None: no derivative operand.
    ``call(case, dy, w, aux, aux_act)`` returns dx."""
    r = Ratios()
    d = data(c, mode)
    dx0, A = reference(c, mode, "d")
    if mode == "int":
        assert aux_act in (None, 0, 3)
        assert_cap(c, "d", dx0)
    if aux_act is None:
        dd, ed, aux = 1.0, 0.0, None
    else:
        dd, ed = act_bwd_ref(f64(d["aux"]), aux_act)
        aux = d["aux"].to(dev)
    dx = call(c, d["dy"].to(dev), d["w"].to(dev), aux, aux_act or 0)
    ref = dx0 * dd
    assert tuple(dx.shape) == ref.shape
    if mode == "int":
        assert exact_bf16(dx, ref), "%s %s aux_act %s: %s" % (
            c.name, tag, aux_act, _where(dx, ref))
        return r
    K = c.KH * c.KW * c.OCg + 1
    r.see("%s aux_act %s" % (tag, aux_act), np.abs(f64(dx) - ref),
          bf_half_ulp(ref) + gamma(K + 3) * A * np.abs(dd) + A * ed)
    return r


def run_wgrad(c, dev, mode="int", dbias=True, call=ops_wgrad, splits=1,
              tag="wgrad"):
    """One weight gradient accumulating into the non-zero dW0 / db0.
    ``call(case, x, dy, dw, db)`` adds into dw / db; ``splits``: the pixel
    splits of the call, for the bound."""
    r = Ratios()
    d = data(c, mode)
    dwr, Aw, dbr, Ab = reference(c, mode, "w")
    if mode == "int":
        assert_cap(c, "w", dwr, dbr, Aw, Ab)
    dw = d["dw0"].clone().to(dev)
    db = d["db0"].clone().to(dev) if dbias else None
    call(c, d["x"].to(dev), d["dy"].to(dev), dw, db)
    if mode == "int":
        assert exact_f32(dw, dwr), "%s %s dW: %s" % (c.name, tag,
                                                     _where(dw, dwr))
        assert db is None or exact_f32(db, dbr), "%s %s db: %s" % (
            c.name, tag, _where(db, dbr))
        return r
    g = gamma(c.P + max(int(splits), 1) + 2)
    r.see(tag + " dW", np.abs(f64(dw) - dwr), g * Aw)
    if db is not None:
        r.see(tag + " db", np.abs(f64(db) - dbr), g * Ab)
    return r


# ============================================== models of the kernels' plans
# conv_hc.hip kHcCands: var -> (KH, KW, KHS, WM, WN, NJW, NBW, m32)
HC_CANDS = collections.OrderedDict([
    (21, (3, 3, 3, 8, 1, 4, 5, 1)), (22, (3, 3, 3, 8, 1, 3, 5, 1)),
    (23, (3, 3, 3, 8, 1, 2, 8, 1)), (24, (5, 5, 5, 8, 1, 2, 4, 1)),
    (6, (3, 3, 3, 8, 1, 8, 5, 0)), (7, (3, 3, 3, 8, 1, 6, 5, 0)),
    (1, (3, 3, 3, 4, 2, 4, 8, 0)), (2, (3, 3, 3, 4, 2, 3, 8, 0)),
    (3, (3, 3, 3, 8, 1, 4, 8, 0)), (11, (5, 5, 5, 8, 1, 2, 8, 0)),
    (4, (5, 5, 5, 4, 2, 2, 8, 0)), (5, (5, 5, 5, 8, 1, 3, 8, 0)),
    (8, (5, 5, 3, 8, 1, 4, 8, 0))])


def hc_bn(var):
    KH, KW, KHS, WM, WN, NJW, NBW, m32 = HC_CANDS[var]
    return WN * NJW * (32 if m32 else 16)


def hc_plan(c, dgrad, var, hc32=True, max_wgs=256):
    """conv_hc.hip hc_plan for a forced configuration ``var`` (or -1: the
    first that fits): None when the call is not taken, else dict(var, tiles,
    items, grid, TPX).  Backward-data plans on dY: channels mirrored."""
    OH, OW = c.out
    if c.sliding != (1, 1):
        return None
    if dgrad:
        H, W, OH, OW, CG, OCg = OH, OW, c.H, c.W, c.OCg, c.Cg
        OCT = c.C
    else:
        H, W, CG, OCg, OCT = c.H, c.W, c.Cg, c.OCg, c.OC
    if CG % 16 or OCg % 16 or OCT % 4:
        return None
    P, OHW = c.N * OH * OW, OH * OW
    for v, (KH, KW, KHS, WM, WN, NJW, NBW, m32) in HC_CANDS.items():
        if (KH, KW) != (c.KH, c.KW) or (var > 0 and v != var):
            continue
        Wp = OW + (KW - 1 if m32 and KW == 5 else max(8, KW - 1))
        if m32 and (not hc32 or CG < 48 or OCT % 8):
            continue
        if not m32 and NJW > 3 and CG < 48:
            continue
        BN, TPX = hc_bn(v), WM * 64
        if OCg % BN:
            continue
        tiles = -(-P // TPX)
        per = OHW // np.gcd(TPX, OHW)
        wr = 0
        for tl in range(int(min(tiles, per))):
            p0, p1 = tl * TPX, min(tl * TPX + TPX, P) - 1
            n0, oh0 = p0 // OHW, p0 % OHW // OW
            n1, oh1 = p1 // OHW, p1 % OHW // OW
            rc, j = OH - oh0 + KH - 1, n1 - n0
            row = oh1 - oh0 if j == 0 else rc + (j - 1) * (OH + KH - 1) + oh1
            wr = max(wr, row + KHS)
        WIN = (wr * Wp * 32 + 1023) // 1024 * 1024
        if wr >= 1024 or WIN // 1024 > WM * WN * NBW:
            continue
        T = KHS * KW
        if m32:
            nb = (BN * T * 32 + 1023) // 1024 * 1024 + 1024
        else:
            nb = (BN * (2 * ((T + 1) // 2) + 1) * 32 + 1023) // 1024 * 1024 + \
                (0 if NJW <= 3 else 1024)
        if 2 * (WIN + nb) > 160 * 1024:
            continue
        items = tiles * c.groups * (OCg // BN)
        return dict(var=v, tiles=tiles, items=items, TPX=TPX,
                    grid=min(items, max_wgs), OHW=OHW, P=P)
    return None


def conv_halo_fill(oh, ow, KH, KW):
    """conv_halo.hip pick_tile and the share of the 128 GEMM rows that the
    spatial tiles of an oh x ow output fill (the kernel asks for 85 %)."""
    best = None
    for th in range(1, min(128, oh + 7) + 1):
        tw = min(128 // th, ow)
        if tw < 1:
            break
        tiles = -(-oh // th) * -(-ow // tw)
        score = oh * ow / (tiles * 128.0) - 1e-6 * (th + KH - 1) * (tw + KW - 1)
        if best is None or score > best[0]:
            best = (score, tiles)
    return oh * ow / (best[1] * 128.0)


def halo_plan(c, splits=0, pad=2):
    """wgrad_halo.hip make_plan for any stride-1 case (rectangular images,
    any padding): None when the kernel does not take it, else (var, dict).
    Held to test_wgrad_halo_lean_model.plan on that file's square cases."""
    OH, OW = c.out
    if c.sliding != (1, 1) or OH * OW < 64 or c.KW > 9 or c.C % 16 or \
            c.OC % 16:
        return None
    OHW, P, Wp = OH * OW, c.N * OH * OW, OW + max(pad, c.KW - 1)
    span = (OW - 1 + 63) // OW + 1
    cross = 2 if OHW % 64 else 1
    spi = (OHW + 63) // 64
    dmax = 0
    for st in range(spi):
        pin, last = 64 * st, min(64 * st + 63, OHW - 1)
        dmax = max(dmax, (last // OW - pin // OW) * Wp + last % OW - pin % OW)
    for var, MT, NP, KHT, KW, PB, seg in HALO_CANDS:
        if c.KW != KW or c.KH % KHT or c.OCg % MT or c.Cg % (16 * NP):
            continue
        if seg:
            if spi * 64 * 100 > OHW * 103 or KHT * (dmax + c.KW) * 32 > PB:
                continue
        elif (span + cross * (KHT - 1)) * Wp * 32 > PB:
            continue
        tiles = c.groups * (c.OCg // MT) * (c.Cg // (16 * NP)) * (c.KH // KHT)
        steps = c.N * spi if seg else (P + 63) // 64
        s = max(1, min(splits if splits > 0 else 512 // tiles, steps))
        ks = (steps + s - 1) // s
        return var, dict(seg=bool(seg), steps=steps, ks=ks, tiles=tiles,
                         splits=(steps + ks - 1) // ks, spi=spi, OHW=OHW)
    return None


# ===================================================================== cases
SAME3, SAME5 = (1, 1, 1, 1), (2, 2, 2, 2)

GEMM_CASES = [
    mk("gemm_3x2_s21", 3, 9, 11, 8, 16, 3, 2, (2, 1), (2, 1, 0, 1)),
    mk("gemm_g2_3x5", 2, 12, 9, 32, 48, 3, 5, (1, 1), (2, 1, 1, 0), 2),
    mk("gemm_1x1", 3, 10, 12, 128, 64, 1, 1),
    mk("gemm_s2_ohw64", 2, 16, 15, 16, 32, 3, 3, (2, 2), (1, 1, 1, 1)),
    mk("gemm_ohw_lt64", 3, 7, 6, 16, 24, 3, 3, (1, 1), (1, 0, 1, 2)),
    mk("gemm_oc50", 2, 9, 8, 24, 50, 3, 3, (1, 1), (0, 0, 0, 0)),
]

HALO_CASES = [
    mk("halo_3x3_asym", 3, 14, 9, 16, 32, 3, 3, (1, 1), (2, 1, 0, 1),
       ops="fd"),
    mk("halo_g2_3x3", 2, 12, 10, 32, 48, 3, 3, (1, 1), SAME3, 2, ops="fd"),
    mk("halo_5x5", 2, 11, 11, 24, 64, 5, 5, (1, 1), (1, 2, 3, 2), ops="fd"),
    # without padding the image is larger than the output: no shape fills
    # the tiles of both, the backward-data stays with the padded cases
    mk("halo_nopad", 2, 16, 11, 16, 40, 3, 3, ops="f"),
]


def _hc(var, N, H, W, CG, pad, groups=1, **tags):
    """A forward case of conv_hc configuration ``var`` with OC/g its n-tile,
    and the mirrored backward-data case."""
    KH, KW = HC_CANDS[var][:2]
    f = mk("hc%d_%dx%d" % (var, H, W), N, H, W, CG * groups,
           hc_bn(var) * groups, KH, KW, (1, 1), pad, groups, var=var, ops="f",
           **tags)
    return [f, swapped(f, ops="d")]


# the smallest non-square shapes at which hc_plan takes the row for the case
# and its mirror with a partial last tile, tiles that cut images and three
# items or more (the window rows of a tile that spans several small images
# bound the shape from below)
HC_CASES = (
    _hc(6, 6, 9, 19, 48, (1, 1, 1, 1)) +
    _hc(7, 7, 7, 21, 48, (2, 1, 0, 1)) +
    _hc(1, 4, 13, 10, 48, (2, 1, 0, 1)) +
    _hc(2, 3, 11, 8, 16, (2, 1, 0, 1), groups=2) +
    _hc(3, 6, 19, 9, 48, (0, 1, 2, 1)) +
    _hc(11, 6, 9, 19, 16, (3, 2, 1, 2)) +
    _hc(4, 5, 8, 13, 16, (3, 2, 1, 2)) +
    _hc(5, 7, 7, 21, 16, (2, 2, 2, 2)) +
    _hc(8, 6, 19, 9, 48, (3, 2, 1, 2)) +
    _hc(3, 3, 21, 20, 48, (0, 0, 0, 0)))

HC32_CASES = (
    _hc(21, 6, 19, 9, 48, (1, 1, 1, 1)) +
    _hc(22, 5, 13, 8, 48, (2, 1, 0, 1), groups=2) +
    _hc(23, 6, 9, 19, 48, (2, 1, 0, 1)) +
    _hc(24, 5, 23, 9, 48, (3, 2, 1, 2)))


def _wh(var, N, H, W, Cg, OCg, K=3, pad=None, groups=1, KH=None, **tags):
    KH = KH or K
    pad = pad if pad is not None else ((K - 1) // 2, (KH - 1) // 2) * 2
    return mk("wh%d_%dx%d_g%d" % (var, H, W, groups), N, H, W, Cg * groups,
              OCg * groups, KH, K, (1, 1), pad, groups, cand=var, ops="w",
              **tags)


WGRAD_HALO_CASES = [
    _wh(1, 3, 8, 8, 32, 128),                          # OH OW % 64 == 0
    _wh(1, 3, 9, 8, 32, 128, pad=(2, 1, 0, 1), groups=2),
    _wh(2, 3, 8, 8, 32, 96),
    _wh(2, 4, 11, 9, 32, 96, pad=(2, 1, 0, 1)),
    _wh(3, 3, 8, 8, 48, 128, K=5),
    _wh(3, 3, 11, 9, 48, 128, K=5, KH=3, pad=(3, 1, 1, 1), groups=2),
    _wh(4, 3, 27, 27, 32, 128),
    _wh(4, 3, 25, 27, 32, 128, pad=(2, 1, 0, 1)),
    _wh(5, 3, 37, 37, 32, 128),
    _wh(5, 3, 4, 64, 32, 128, pad=(2, 1, 0, 1)),       # OH OW % 64 == 0
    _wh(6, 3, 16, 16, 64, 64),
    _wh(6, 3, 18, 21, 64, 64, pad=(2, 1, 0, 1), groups=2),
    _wh(7, 3, 8, 8, 48, 96),
    _wh(7, 3, 9, 14, 48, 96, pad=(0, 1, 2, 1)),
]

# one workgroup (splits 1, one tile) walking 1, 2 and 3 steps
WGRAD_HALO_STEPS = [
    mk("wh1_steps%d" % n, n, 8, 8, 32, 128, 3, 3, (1, 1), (1, 1, 1, 1), 1,
       cand=1, ops="w") for n in (1, 2, 3)]

SMALL_CASES = [
    mk("s2d_c3_11x11_s4", 2, 35, 39, 3, 96, 11, 11, (4, 4), route="s2d", ops="fw"),
    mk("s2d_c3_8x8_s4", 2, 30, 26, 3, 32, 8, 8, (4, 4), (2, 1, 2, 1),
       route="s2d", ops="fw"),
    mk("s2d_c2_s2", 3, 13, 11, 2, 24, 3, 3, (2, 2), (1, 0, 1, 2),
       route="s2d", ops="fw"),
    mk("pad8_c3", 2, 13, 11, 3, 32, 3, 3, (1, 1), (2, 1, 0, 1), route="pad8",
       ops="fw"),
    mk("pad8_c20", 2, 9, 8, 20, 48, 5, 5, (1, 1), (1, 2, 3, 2),
       route="pad8", ops="fw"),
    mk("direct_c1_5x5", 3, 14, 12, 1, 20, 5, 5, route="direct", ops="fw"),
    mk("direct_c1_s21", 2, 13, 12, 1, 40, 3, 3, (2, 1), (2, 1, 0, 1),
       route="direct", ops="fw"),
    mk("run_c2", 2, 11, 9, 2, 72, 3, 3, (1, 1), (2, 1, 0, 1), route="run",
       ops="fw"),
]

CHUNK_CASES = [
    mk("chunk_hc", 5, 13, 11, 48, 64, 3, 3, (1, 1), (2, 1, 0, 1)),
    mk("chunk_c3", 5, 13, 11, 3, 32, 3, 3, (1, 1), (2, 1, 0, 1)),
]

# mutants a path's shape conditions leave no case for
STRIDE1 = {"sx_sy_swapped"}
PATHS = collections.OrderedDict([
    ("implicit_gemm", (GEMM_CASES, set())),
    ("conv_halo", (HALO_CASES, STRIDE1)),
    ("conv_hc", (HC_CASES, STRIDE1)),
    ("conv_hc32", (HC32_CASES, STRIDE1)),
    ("wgrad_halo", (WGRAD_HALO_CASES + WGRAD_HALO_STEPS, STRIDE1)),
    ("small_channel", (SMALL_CASES, {"groups_interleaved"})),
    ("image_chunks", (CHUNK_CASES, STRIDE1 | {"groups_interleaved"})),
])
ALL_CASES = [c for cases, _ in PATHS.values() for c in cases]
assert len({c.name for c in ALL_CASES}) == len(ALL_CASES)
# bounded mode: one case per family
BOUNDED = {"implicit_gemm": GEMM_CASES[1], "conv_halo": HALO_CASES[0],
           "conv_hc": HC_CASES[4], "conv_hc32": HC32_CASES[2],
           "wgrad_halo": WGRAD_HALO_CASES[1]}


# the cases of check_blindness, outputs up to 100 and more: AlexNet conv2 at
# the batch the older tests use, and the largest weight-gradient case
BLIND_FWD = mk("alexnet_conv2", 3, 27, 27, 96, 256, 5, 5, (1, 1), SAME5, 2)
BLIND_WGRAD = WGRAD_HALO_CASES[8]


def mutant_differs(c, op, name):
    """Whether the wrong rule ``name`` changes operation ``op`` of case ``c``
    on the integer data."""
    rule, where = MUTANTS[name]
    if op not in where:
        return False
    d = data(c, "int")
    x, w, dy = f64(d["x"]), f64(d["w"]), f64(d["dy"])
    true = reference(c, "int", op)
    if rule is None:
        if op == "f":
            return not np.array_equal(drop_fwd(c, true[0], x, w), true[0])
        if op == "d":
            return not np.array_equal(drop_dgrad(c, true[0], dy, w), true[0])
        return not np.array_equal(drop_wgrad(c, true[0], x, dy), true[0])
    if op == "f":
        return not np.array_equal(fwd_ref(c, x, w, f64(d["bias"]), rule)[0],
                                  true[0])
    if op == "d":
        return not np.array_equal(dgrad_ref(c, dy, w, rule)[0], true[0])
    return not np.array_equal(
        wgrad_ref(c, x, dy, f64(d["dw0"]), f64(d["db0"]), rule)[0], true[0])


# ===================================================== the float32 CPU paths
DEV = "cpu"
_ids = dict(ids=str)


def test_conv_out_size():
    """ops.conv_out_size against the window count, everywhere; sliding is
    (sx, sy) and padding (l, t, r, b)."""
    for k in range(1, 6):
        for s in range(1, 5):
            for p0 in range(0, 3):
                for p1 in range(0, 3):
                    for h in range(max(1, k - p0 - p1), 20):
                        n = out_len(h, k, s, p0, p1)
                        assert ops.conv_out_size(h, 7, k, 3, (1, s),
                                                 (1, p0, 1, p1)) == (n, 7)
                        assert ops.conv_out_size(7, h, 3, k, (s, 1),
                                                 (p0, 1, p1, 1)) == (7, n)
    for c in ALL_CASES:
        assert ops.conv_out_size(c.H, c.W, c.KH, c.KW, c.sliding,
                                 c.padding) == c.out


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2)


@pytest.mark.parametrize("c", ALL_CASES, **_ids)
def test_references_against_torch(c):
    """float64 conv2d / conv2d_input / conv2d_weight, 1e-12 relative."""
    pl, pt, pr, pb = c.padding
    sx, sy = c.sliding
    OH, OW = c.out
    for mode in ("int", "bounded"):
        d = data(c, mode)
        x, w, dy, b = (f64(d[k]) for k in ("x", "w", "dy", "bias"))
        xp = F.pad(_nchw(x), (pl, pr, pt, pb))
        wt = _nchw(w)
        y = F.conv2d(xp, wt, torch.from_numpy(b), stride=(sy, sx),
                     groups=c.groups).permute(0, 2, 3, 1).numpy()
        z, A = reference(c, mode, "f")
        assert A.min() >= 0 and (np.abs(z) <= A * (1 + 1e-12)).all()
        assert np.abs(z - y).max() <= 1e-12 * np.abs(y).max()
        dxp = torch.nn.grad.conv2d_input(
            tuple(xp.shape), wt, _nchw(dy), stride=(sy, sx), groups=c.groups)
        # rows / columns of the padded image that no window reaches
        dxp = F.pad(dxp, (0, xp.shape[3] - dxp.shape[3], 0,
                          xp.shape[2] - dxp.shape[2]))
        dxt = dxp[:, :, pt:pt + c.H, pl:pl + c.W].permute(0, 2, 3, 1).numpy()
        dx, Ad = reference(c, mode, "d")
        assert np.abs(dx - dxt).max() <= 1e-12 * np.abs(dxt).max()
        assert (np.abs(dx) <= Ad * (1 + 1e-12)).all()
        gw = torch.nn.grad.conv2d_weight(
            xp, (c.OC, c.Cg, c.KH, c.KW), _nchw(dy), stride=(sy, sx),
            groups=c.groups).permute(0, 2, 3, 1).numpy()
        dw, Aw, db, Ab = wgrad_ref(c, x, dy)
        assert np.abs(dw - gw).max() <= 1e-12 * np.abs(gw).max()
        assert np.abs(db - dy.reshape(-1, c.OC).sum(0)).max() <= \
            1e-12 * np.abs(db).max()
        assert (np.abs(dw) <= Aw * (1 + 1e-12)).all()


@pytest.mark.parametrize("c", ALL_CASES, **_ids)
def test_integer_data_meets_the_cap(c):
    """The cap on the references alone, and data that says something: more
    than 90 % of the outputs are not zero."""
    z, _ = reference(c, "int", "f")
    dx, _ = reference(c, "int", "d")
    dw, Aw, db, Ab = reference(c, "int", "w")
    assert_cap(c, "f", z)
    assert_cap(c, "d", dx)
    assert_cap(c, "w", dw, db, Aw, Ab)
    assert (z != 0).mean() > 0.9 and (dw != 0).mean() > 0.5
    if min(c.KH, c.KW) > 1 or c.OCg >= 16:
        assert (dx != 0).mean() > 0.5


@pytest.mark.parametrize("c", ALL_CASES, **_ids)
def test_cpu_paths(c):
    """The float32 CPU paths of ops, integer mode exact and every activation
    and derivative in bounded mode."""
    r = Ratios()
    for act, bias in ((3, True), (0, True), (0, False)):
        run_fwd(c, DEV, "int", act, bias)
    for aux_act in (3, None):
        run_dgrad(c, DEV, "int", aux_act)
    run_wgrad(c, DEV, "int")
    run_wgrad(c, DEV, "int", dbias=False)
    for act in (0, 1, 2, 3, 4):
        r.merge(run_fwd(c, DEV, "bounded", act))
        r.merge(run_dgrad(c, DEV, "bounded", act or None))
    r.merge(run_wgrad(c, DEV, "bounded"))


def test_mutants_differ_and_every_path_sees_them():
    """Each wrong rule differs from the true reference on the integer data,
    and every path has, per operation it runs, a case that tells each wrong
    rule that applies to it from the true one."""
    blind = []
    for path, (cases, exempt) in PATHS.items():
        for name, (_, where) in MUTANTS.items():
            if name in exempt:
                continue
            for op in where:
                run = [c for c in cases if c.does(op)]
                if run and not any(mutant_differs(c, op, name) for c in run):
                    blind.append((path, op, name))
    assert not blind, blind
    # a wrong rule that a path is exempt from must be one its cases cannot
    # show: stride 1 everywhere, one group everywhere
    for path, (cases, exempt) in PATHS.items():
        if "sx_sy_swapped" in exempt:
            assert all(c.sliding == (1, 1) for c in cases), path
        if "groups_interleaved" in exempt:
            assert all(c.groups == 1 for c in cases), path


def check_blindness(dev):
    """One forward and one weight-gradient result, perturbed after the fact
    by one product at one border pixel: the exact check rejects it, the
    older tests' close(..., 1e-2) accepts it.  (That rule passes an error of
    1 wherever the largest output is at least 100: asserted on the
    reference.)"""
    c = BLIND_FWD
    d = data(c, "int")
    z, _ = reference(c, "int", "f")
    assert np.abs(z).max() >= 100
    y = ops_fwd(c, d["x"].to(dev), d["w"].to(dev), d["bias"].to(dev), 0)
    assert exact_bf16(y, z)
    bad = torch.from_numpy(drop_fwd(c, f64(y), d["x"], d["w"])).to(BF)
    assert np.abs(f64(bad) - z).max() == 1 and (f64(bad) != z).sum() <= c.OCg
    assert not exact_bf16(bad, z) and old_close(bad, z)
    c = BLIND_WGRAD
    d = data(c, "int")
    dwr = reference(c, "int", "w")[0]
    assert np.abs(dwr).max() >= 100
    dw = d["dw0"].clone().to(dev)
    ops_wgrad(c, d["x"].to(dev), d["dy"].to(dev), dw, None)
    assert exact_f32(dw, dwr)
    bad = torch.from_numpy(drop_wgrad(c, f64(dw), d["x"], d["dy"])).float()
    assert np.abs(f64(bad) - dwr).max() == 1
    assert not exact_f32(bad, dwr) and old_close(bad, dwr)


def test_one_product_is_seen_where_the_old_rule_is_blind():
    check_blindness(DEV)


def test_plan_models():
    """The rectangular halo weight-gradient plan equals the square model of
    test_wgrad_halo_lean_model.py on that file's cases; every conv_hc /
    conv_hc32 / wgrad_halo case reaches its configuration, with a partial
    last tile, a tile or step that spans two images and several items per
    workgroup where the GPU tests ask for them."""
    for name, (N, H, W, C, OC, K, p, g) in HALO_MODEL_SHAPES.items():
        c = mk(name, N, H, W, C, OC, K, K, (1, 1), (p,) * 4, g)
        for splits in (0, 1, 2, 7):
            _, k = halo_plan_square(HALO_MODEL_SHAPES[name], splits)
            var, m = halo_plan(c, splits)
            mine = [v for v in HALO_CANDS if v[0] == var][0]
            assert (k["MT"], k["NP"], k["KHT"], k["PB"], k["SEG"]) == (
                mine[1], mine[2], mine[3], mine[5], bool(mine[6])), name
            assert m["splits"] == k["splits"], (name, splits)
    for c in WGRAD_HALO_CASES:
        plan = halo_plan(c)
        assert plan is not None and plan[0] == c.tag("cand"), (c.name, plan)
        assert c.N >= 3
    reached = {c.tag("cand") for c in WGRAD_HALO_CASES}
    assert reached == {v[0] for v in HALO_CANDS}
    for var in reached:
        mods = {c.out[0] * c.out[1] % 64 == 0 for c in WGRAD_HALO_CASES
                if c.tag("cand") == var}
        # candidate 4 is what the full-row window of candidate 1 is too
        # small for and the segments of candidate 5 waste too much on: with
        # OH OW a multiple of 64 the segments waste nothing and take it
        assert mods == {True, False} or var == 4, (var, mods)
    for c in HALO_CASES:
        assert c.KH * c.KW * c.Cg <= 1024 and c.OCg % 8 == 0 and c.Cg % 8 == 0
        assert conv_halo_fill(*c.out, c.KH, c.KW) >= 0.85, c.name
        if c.does("d"):
            assert conv_halo_fill(c.H, c.W, c.KH, c.KW) >= 0.85, c.name
    rows = set()
    for c in HC_CASES + HC32_CASES:
        p = hc_plan(c, c.does("d"), c.tag("var"), max_wgs=2)
        assert p is not None and p["var"] == c.tag("var"), (c.name, p)
        rows.add(p["var"])
        assert p["P"] % p["TPX"], c.name               # partial last tile
        assert p["TPX"] % p["OHW"] and p["OHW"] < p["TPX"], c.name   # cut
        assert p["items"] > p["grid"], (c.name, p)     # items per workgroup
    assert rows == set(HC_CANDS)
