"""Every convolution kernel path against the float64 references of
tests/test_conv_ref.py: in integer mode bit for bit (one dropped, doubled or
misplaced product moves an output by at least 1), in bounded mode to the
derived per-element bounds for the epilogues that round (tanh, softplus,
sigmoid and their derivatives, and the float32 weight gradient of normal
data).  Each path is held to the reference on its own, none only to another
path, and every case asserts that the kernel it is meant for ran: the return
code of the direct ``hvk_*`` call with ``conv_hc_last_variant()``, the plan
model of test_conv_ref.py for the halo weight gradient (the library has no
query for its candidate), the route predicates for the small-channel
convolutions.  A silent fallback fails the case.

Paths (cases in test_conv_ref.py, each the smallest shape that reaches its
path with a partial last tile, tiles or steps that cut images and several
items per persistent workgroup; non-square images, pt != pl):
  1 implicit GEMM (hc, halo, halo weight gradient off), schedules -1 and 54
  2 conv_halo forward and backward-data
  3 conv_hc 16x16x32, rows 1-8 and 11 of kHcCands
  4 conv_hc32 rows 21-24: three forward epilogues; backward-data epilogues 0
    and 2, staged stores on and off, both weight layouts; hand-over on / off
  5 wgrad_halo, seven candidates: splits 0 / 2 / 7, the old, lean and
    two-stage loops, groups 1 and 2, with and without dbias, one workgroup
    with 1, 2 and 3 steps
  6 small-channel routes: space-to-depth, channel padding, the direct kernel,
    the packed-run kernels, with and without the col_out hand-over
  7 image chunks (N = 5 in three launches)
  8 bounded mode per family and inexact epilogue

``pytest -s`` prints the count of cases per path and the worst measured
|error| / bound per path and epilogue (profiles/conv_exact/ratios.txt)."""
import collections
import time

import pytest
import torch

import veles_amd.ops as ops
from test_conv_ref import (
    BOUNDED, CHUNK_CASES, GEMM_CASES, HALO_CASES, HC32_CASES, HC_CASES,
    SMALL_CASES, WGRAD_HALO_CASES, WGRAD_HALO_STEPS, Ratios, check_blindness,
    halo_plan, hc_plan, run_dgrad, run_fwd, run_wgrad)

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = collections.OrderedDict()     # path -> Ratios
COUNT = collections.Counter()         # path -> integer-mode runs
_ids = dict(ids=str)


def _lib():
    return ops._lib.lib()


class Knobs(object):
    """Every A/B knob the tests touch: the first ``set`` of a knob records
    the value to put back (the library's knobs have no getter: their
    documented defaults), ``restore`` puts all of them back."""
    SET = {
        "hc": lambda v: ops.set_conv_hc(*v),
        "hc32": lambda v: ops.set_conv_hc32(v),
        "handover": lambda v: ops.set_conv_hc32_handover(v),
        "ts": lambda v: _lib().hvk_hc32_ts(int(v)),
        "max_wgs": lambda v: ops.set_conv_hc_max_wgs(v),
        "halo": lambda v: ops.set_conv_halo(v[0], dgrad=v[1]),
        "halo_wgrad": lambda v: ops.set_halo_wgrad(v),
        "lean": lambda v: ops.set_halo_wgrad_lean(v),
        "stages": lambda v: ops.set_halo_wgrad_stages(v),
        "gemm_variant": lambda v: _lib().hvk_set_gemm_variant(int(v)),
    }

    def __init__(self):
        self.saved = {}

    def _default(self, name):
        return {"hc": (ops._CONV_HC, -2), "hc32": True, "handover": True,
                "ts": True, "max_wgs": 256,
                "halo": (ops._HALO, ops._HALO_DGRAD),
                "halo_wgrad": ops._HALO_WGRAD, "lean": True, "stages": True,
                "gemm_variant": -1}[name]

    def set(self, name, value):
        if name not in self.saved:
            self.saved[name] = self._default(name)
        self.SET[name](value)

    def restore(self):
        for name, value in list(self.saved.items()):
            self.SET[name](value)
        self.saved.clear()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.restore()
        return False

    def plain(self):
        """Only the implicit GEMM is left."""
        self.set("hc", (False, -2))
        self.set("halo", (False, False))
        self.set("halo_wgrad", False)


@pytest.fixture(scope="module", autouse=True)
def knobs():
    k = Knobs()
    t0 = time.time()
    try:
        yield k
    finally:
        k.restore()
        print("\ninteger-mode runs per path: " + ", ".join(
            "%s %d" % kv for kv in sorted(COUNT.items())))
        for path, r in WORST.items():
            print("worst |error| / bound, %s: " % path + ", ".join(
                "%s %.3f" % kv for kv in sorted(r.items())))
        print("wall time of this file: %.1f s" % (time.time() - t0))


def _seen(path, n):
    COUNT[path] += n


def _bounded(path, r):
    WORST.setdefault(path, Ratios()).merge(r)


# ------------------------------------------------------------- direct calls
def _geo(c):
    OH, OW = c.out
    return (c.N, c.H, c.W, c.C, c.OC, c.KH, c.KW, c.padding[1], c.padding[0],
            OH, OW, c.groups)


def _permuted(c, w):
    """[OC][KH][KW][C/g] -> [g][c][kh][kw][oc], as ops.conv_dgrad does."""
    return w.view(c.groups, c.OCg, c.KH, c.KW, c.Cg).permute(
        0, 4, 2, 3, 1).contiguous()


def hc_fwd(var):
    """hvk_conv_fwd_hc as ops._conv_fwd_call issues it; the forced row ran."""
    def call(c, x, w, bias, act):
        OH, OW = c.out
        out = torch.empty(c.N, OH, OW, c.OC, dtype=x.dtype, device=x.device)
        wp = ops._hc_wpack(0, *_geo(c), out, None, x.device)
        assert (wp is not None) == (var >= 21)
        rc = _lib().hvk_conv_fwd_hc(
            ops._p(x), ops._p(w), ops._p(bias), ops._p(out), *_geo(c), act,
            ops._p(wp), ops._s(x))
        assert rc == 0, (c.name, rc)
        assert ops.conv_hc_last_variant() == var
        return out
    return call


def hc_dgrad(var, fwd_layout=False):
    """hvk_conv_dgrad_hc on the permuted weights, or hvk_conv_dgrad_hc_w on
    the forward layout, as ops.conv_dgrad issues them."""
    def call(c, dy, w, aux, aux_act):
        out = torch.empty(c.N, c.H, c.W, c.C, dtype=dy.dtype, device=dy.device)
        wp = ops._hc_wpack(1, *_geo(c), out, aux, dy.device)
        assert (wp is not None) == (var >= 21)
        fn = _lib().hvk_conv_dgrad_hc_w if fwd_layout else \
            _lib().hvk_conv_dgrad_hc
        ww = w if fwd_layout else _permuted(c, w)
        rc = fn(ops._p(dy), ops._p(ww), ops._p(out), *_geo(c), ops._p(aux),
                aux_act, ops._p(wp), ops._s(dy))
        assert rc == 0, (c.name, rc)
        assert ops.conv_hc_last_variant() == var
        return out
    return call


def halo_fwd(c, x, w, bias, act):
    OH, OW = c.out
    out = torch.empty(c.N, OH, OW, c.OC, dtype=x.dtype, device=x.device)
    rc = _lib().hvk_conv_fwd_halo(
        ops._p(x), ops._p(w), ops._p(bias), ops._p(out), *_geo(c), act,
        ops._s(x))
    assert rc == 0, (c.name, rc)
    return out


def halo_dgrad(c, dy, w, aux, aux_act):
    out = torch.empty(c.N, c.H, c.W, c.C, dtype=dy.dtype, device=dy.device)
    wt = _permuted(c, w)
    rc = _lib().hvk_conv_dgrad_halo(
        ops._p(dy), ops._p(wt), ops._p(out), *_geo(c), ops._p(aux), aux_act,
        ops._s(dy))
    assert rc == 0, (c.name, rc)
    return out


def halo_wgrad(splits):
    """hvk_conv_wgrad_halo as ops._halo_wgrad issues it (plan-only call for
    the workspace, then the launch); the split count is the model's."""
    def call(c, x, dy, dw, db):
        fn = _lib().hvk_conv_wgrad_halo
        geo = _geo(c) + (splits,)
        need = fn(ops._p(x), ops._p(dy), ops._p(dw), ops._p(db), None, *geo,
                  ops._s(x))
        assert need > 0, "%s does not take the halo kernel" % c.name
        model = halo_plan(c, splits)[1]
        kk = c.KH * c.KW * c.Cg
        assert need == model["splits"] * c.OC * (kk + 1)
        assert _lib().hvk_conv_wgrad_halo_splits(*geo) == model["splits"]
        ws = torch.empty(int(need), dtype=torch.float32, device=x.device)
        rc = fn(ops._p(x), ops._p(dy), ops._p(dw), ops._p(db), ops._p(ws),
                *geo, ops._s(x))
        assert rc == 0, (c.name, rc)
    return call


FWD_EPI = ((3, True), (0, True), (0, False))     # act, bias
DGRAD_EPI = (3, None)                            # aux_act


# ------------------------------------------------------------ 1 implicit GEMM
@pytest.mark.parametrize("variant", [-1, 54])
@pytest.mark.parametrize("c", GEMM_CASES, **_ids)
def test_implicit_gemm(knobs, c, variant):
    with knobs:
        knobs.plain()
        knobs.set("gemm_variant", variant)
        for act, bias in FWD_EPI:
            run_fwd(c, DEV, "int", act, bias)
        for aux_act in DGRAD_EPI:
            run_dgrad(c, DEV, "int", aux_act)
        for dbias in (True, False):
            for splits in (None, 1, 3):
                run_wgrad(c, DEV, "int", dbias, lambda c, x, dy, dw, db:
                          ops.conv_wgrad(x, dy, dw, c.sliding, c.padding,
                                         c.groups, splits=splits, dbias=db))
        torch.cuda.synchronize()
    _seen("implicit_gemm", n=11)


# -------------------------------------------------------------- 2 conv_halo
@pytest.mark.parametrize("variant", [-1, 54])
@pytest.mark.parametrize("c", HALO_CASES, **_ids)
def test_conv_halo(knobs, c, variant):
    with knobs:
        knobs.set("gemm_variant", variant)
        for act, bias in FWD_EPI:
            run_fwd(c, DEV, "int", act, bias, halo_fwd)
        if c.does("d"):
            for aux_act in DGRAD_EPI:
                run_dgrad(c, DEV, "int", aux_act, halo_dgrad)
        # and through the dispatch of ops with the kernels switched on
        knobs.set("hc", (False, -2))
        knobs.set("halo", (True, True))
        run_fwd(c, DEV, "int", 3)
        run_dgrad(c, DEV, "int", 3)
        torch.cuda.synchronize()
    _seen("conv_halo", n=7 if c.does("d") else 5)


# ---------------------------------------------------------------- 3 conv_hc
@pytest.mark.parametrize("max_wgs", [2, 256])
@pytest.mark.parametrize("c", HC_CASES, **_ids)
def test_conv_hc(knobs, c, max_wgs):
    var = c.tag("var")
    dgrad = c.does("d")
    plan = hc_plan(c, dgrad, var, hc32=False, max_wgs=max_wgs)
    assert plan is not None and plan["var"] == var
    with knobs:
        knobs.set("hc", (True, var))
        knobs.set("hc32", False)
        knobs.set("max_wgs", max_wgs)
        if dgrad:
            for aux_act in DGRAD_EPI:
                run_dgrad(c, DEV, "int", aux_act, hc_dgrad(var))
        else:
            for act, bias in FWD_EPI:
                run_fwd(c, DEV, "int", act, bias, hc_fwd(var))
        torch.cuda.synchronize()
    _seen("conv_hc row %d" % var, n=2 if dgrad else 3)


# -------------------------------------------------------------- 4 conv_hc32
@pytest.mark.parametrize("handover", [True, False])
@pytest.mark.parametrize("c", HC32_CASES, **_ids)
def test_conv_hc32(knobs, c, handover):
    var = c.tag("var")
    dgrad = c.does("d")
    plan = hc_plan(c, dgrad, var, max_wgs=2)
    assert plan is not None and plan["var"] == var
    n = 0
    with knobs:
        knobs.set("hc", (True, var))
        knobs.set("hc32", True)
        knobs.set("handover", handover)
        for max_wgs in (2, 256):
            knobs.set("max_wgs", max_wgs)
            if not dgrad:
                for act, bias in FWD_EPI:      # epilogues 1, 0, 0
                    run_fwd(c, DEV, "int", act, bias, hc_fwd(var))
                    n += 1
                continue
            for ts in (True, False):
                knobs.set("ts", ts)
                for fwd_layout in (False, True):
                    for aux_act in DGRAD_EPI:  # epilogues 2 and 0
                        run_dgrad(c, DEV, "int", aux_act,
                                  hc_dgrad(var, fwd_layout))
                        n += 1
        torch.cuda.synchronize()
    _seen("conv_hc32 row %d" % var, n=n)


# ------------------------------------------------------------- 5 wgrad_halo
LOOPS = {"old": (False, False), "lean": (True, False), "stages": (True, True)}


@pytest.mark.parametrize("loop", sorted(LOOPS))
@pytest.mark.parametrize("c", WGRAD_HALO_CASES, **_ids)
def test_wgrad_halo(knobs, c, loop):
    assert halo_plan(c)[0] == c.tag("cand")
    with knobs:
        knobs.set("lean", LOOPS[loop][0])
        knobs.set("stages", LOOPS[loop][1])
        for splits in (0, 2, 7):
            for dbias in (True, False):
                run_wgrad(c, DEV, "int", dbias, halo_wgrad(splits))
        torch.cuda.synchronize()
    _seen("wgrad_halo candidate %d" % c.tag("cand"), n=6)


@pytest.mark.parametrize("c", WGRAD_HALO_STEPS, **_ids)
def test_wgrad_halo_one_workgroup(knobs, c):
    """One tile, one split: a single workgroup walks 1, 2 and 3 steps."""
    var, plan = halo_plan(c, 1)
    assert var == 1 and plan["tiles"] == 1 and plan["splits"] == 1 and \
        plan["steps"] == c.N
    with knobs:
        for loop in sorted(LOOPS):
            knobs.set("lean", LOOPS[loop][0])
            knobs.set("stages", LOOPS[loop][1])
            run_wgrad(c, DEV, "int", True, halo_wgrad(1))
        torch.cuda.synchronize()
    _seen("wgrad_halo candidate 1", n=3)


def test_wgrad_halo_through_ops(knobs):
    """ops.conv_wgrad takes the halo kernel for these shapes (its plan-only
    call says so) and stays exact with the caller's splits."""
    for c in WGRAD_HALO_CASES[:4]:
        geo = _geo(c) + (0,)
        assert _lib().hvk_conv_wgrad_halo(None, None, None, None, None, *geo,
                                          None) > 0
        for splits in (None, 2):
            run_wgrad(c, DEV, "int", True, lambda c, x, dy, dw, db:
                      ops.conv_wgrad(x, dy, dw, c.sliding, c.padding,
                                     c.groups, splits=splits, dbias=db))
    torch.cuda.synchronize()
    _seen("wgrad_halo through ops", n=8)


# --------------------------------------------------- 6 small-channel routes
def _route(c):
    s2 = ops.s2d_factor(c.C, c.groups, c.sliding, c.KH, c.KW)
    if s2:
        return "s2d"
    if ops.pad8_ok(c.C, c.groups):
        return "pad8"
    if c.C < 3 and c.KH * c.KW * c.C <= 64 and c.OC <= 64:
        return "direct"
    assert ops.needs_im2col(c.C, c.groups)
    return "run"


def direct_fwd(c, x, w, bias, act):
    OH, OW = c.out
    sx, sy = c.sliding
    out = torch.empty(c.N, OH, OW, c.OC, dtype=x.dtype, device=x.device)
    rc = _lib().hvk_conv_fwd_direct(
        ops._p(x), ops._p(w), ops._p(bias), ops._p(out), c.N, c.H, c.W, c.C,
        c.OC, c.KH, c.KW, sy, sx, c.padding[1], c.padding[0], OH, OW, act,
        ops._s(x))
    assert rc == 0, (c.name, rc)
    return out


@pytest.mark.parametrize("c", SMALL_CASES, **_ids)
def test_small_channel_routes(knobs, c):
    route = c.tag("route")
    assert _route(c) == route
    kept = {}

    def fwd_keep(c, x, w, bias, act):
        kept.clear()
        return ops.conv_fwd(x, w, bias, c.sliding, c.padding, c.groups, act,
                            col_out=kept)

    def wgrad_kept(c, x, dy, dw, db):
        # the forward ran on another copy of x: its image is of the same data
        ops.conv_wgrad(x, dy, dw, c.sliding, c.padding, c.groups,
                       col=kept.get("col"), dbias=db)
    n = 0
    for act, bias in FWD_EPI:
        run_fwd(c, DEV, "int", act, bias)
        n += 1
    if route == "direct":
        for act, bias in FWD_EPI:
            run_fwd(c, DEV, "int", act, bias, direct_fwd)
            n += 1
    for dbias in (True, False):
        run_wgrad(c, DEV, "int", dbias)                  # no hand-over
        run_fwd(c, DEV, "int", 3, True, fwd_keep)
        if route in ("s2d", "pad8"):
            assert isinstance(kept.get("col"), ops.S2DImage if route == "s2d"
                              else ops.PaddedImage)
        run_wgrad(c, DEV, "int", dbias, wgrad_kept)      # hand-over used
        n += 3
    torch.cuda.synchronize()
    _seen("small-channel " + route, n=n)


# ------------------------------------------------------------ 7 image chunks
def _three_chunks(monkeypatch, *tensors):
    """ops._BUF_MAX so low that five images of the largest of ``tensors`` run
    as 2 + 2 + 1."""
    per = max(t.numel() // t.shape[0] * t.element_size() for t in tensors)
    monkeypatch.setattr(ops, "_BUF_MAX", per * 2 + 1)
    assert ops._image_chunks(5, *tensors) == [(0, 2), (2, 4), (4, 5)]


@pytest.mark.parametrize("c", CHUNK_CASES, **_ids)
def test_image_chunks(knobs, monkeypatch, c):
    assert c.N == 5
    hc = c.C % 16 == 0
    with knobs:
        if hc:      # the chunks of two images and of one take conv_hc
            knobs.set("hc", (True, -1))
            for n in (1, 2):
                assert hc_plan(c._replace(N=n), False, -1) is not None

        def fwd(c, x, w, bias, act):
            # the channel-padded image is the one the launches are cut by
            _three_chunks(monkeypatch, x if hc else torch.empty(
                c.N, c.H, c.W, 8, dtype=x.dtype, device="meta"))
            return ops.conv_fwd(x, w, bias, c.sliding, c.padding, c.groups,
                                act)

        def dgrad(c, dy, w, aux, aux_act):
            _three_chunks(monkeypatch, dy)
            return ops.conv_dgrad(dy, w, (c.N, c.H, c.W, c.C), c.sliding,
                                  c.padding, c.groups, aux=aux,
                                  aux_act=aux_act)

        def wgrad(c, x, dy, dw, db):
            _three_chunks(monkeypatch, x, dy)
            ops.conv_wgrad(x, dy, dw, c.sliding, c.padding, c.groups,
                           dbias=db)
        for act, bias in FWD_EPI:
            run_fwd(c, DEV, "int", act, bias, fwd)
        for aux_act in DGRAD_EPI:
            run_dgrad(c, DEV, "int", aux_act, dgrad)
        for dbias in (True, False):
            run_wgrad(c, DEV, "int", dbias, wgrad)
        torch.cuda.synchronize()
    _seen("image chunks", n=7)


# ------------------------------------------------------------ 8 bounded mode
ACTS = (1, 2, 4)     # tanh, softplus, sigmoid


def test_bounded_implicit_gemm(knobs):
    c = BOUNDED["implicit_gemm"]
    r = Ratios()
    with knobs:
        knobs.plain()
        for variant in (-1, 54):
            knobs.set("gemm_variant", variant)
            for act in ACTS:
                r.merge(run_fwd(c, DEV, "bounded", act))
                r.merge(run_dgrad(c, DEV, "bounded", act))
            r.merge(run_wgrad(
                c, DEV, "bounded", True, lambda c, x, dy, dw, db:
                ops.conv_wgrad(x, dy, dw, c.sliding, c.padding, c.groups,
                               splits=3, dbias=db), splits=3))
        torch.cuda.synchronize()
    _bounded("implicit GEMM", r)


def test_bounded_conv_halo(knobs):
    c = BOUNDED["conv_halo"]
    r = Ratios()
    for act in ACTS:
        r.merge(run_fwd(c, DEV, "bounded", act, True, halo_fwd))
        r.merge(run_dgrad(c, DEV, "bounded", act, halo_dgrad))
    torch.cuda.synchronize()
    _bounded("conv_halo", r)


@pytest.mark.parametrize("path", ["conv_hc", "conv_hc32"])
def test_bounded_conv_hc(knobs, path):
    f = BOUNDED[path]
    d = (HC_CASES if path == "conv_hc" else HC32_CASES)[
        (HC_CASES if path == "conv_hc" else HC32_CASES).index(f) + 1]
    var = f.tag("var")
    assert d.tag("var") == var and d.does("d")
    r = Ratios()
    with knobs:
        knobs.set("hc", (True, var))
        knobs.set("hc32", path == "conv_hc32")
        knobs.set("max_wgs", 2)
        for act in ACTS:
            r.merge(run_fwd(f, DEV, "bounded", act, True, hc_fwd(var)))
            r.merge(run_dgrad(d, DEV, "bounded", act, hc_dgrad(var)))
        torch.cuda.synchronize()
    _bounded(path, r)


def test_bounded_wgrad_halo(knobs):
    c = BOUNDED["wgrad_halo"]
    r = Ratios()
    for splits in (0, 2, 7):
        s = halo_plan(c, splits)[1]["splits"]
        r.merge(run_wgrad(c, DEV, "bounded", True, halo_wgrad(splits),
                          splits=s))
    torch.cuda.synchronize()
    _bounded("wgrad_halo", r)


# ---------------------------------------------------------------- blindness
def test_one_product_is_seen_where_the_old_rule_is_blind():
    """The device results of one forward and one weight gradient, perturbed
    after the fact by one product at one border pixel: rejected by the exact
    check, accepted by close(..., 1e-2)."""
    check_blindness(DEV)
