"""Every kernel path of csrc/kernels/pool_lrn.hip that a shape, an alignment
or a variant selects, against the float64 references, cases and derived
bounds of tests/test_pool_lrn_ref.py.  Each path is held to the reference on
its own, none only to another path.

Pooling geometries, (N, H, W), ky x kx, strides (test_pool_lrn_ref.POOL_GEOM):
 1 (2,13,13) 3x3 / 2 full windows, odd sides      pool_fwd3, pool_bwd3s2_blk
 2 (2,14,12) 3x3 / 2 clipped in both axes         (variant 1: pool_bwd3)
 3 (1,9,10) 3x3 / 3                               pool_bwd3
 4 (1,11,10) 3x3 / sy 4, sx 2: rows that no window covers get exactly 0
 5 (1,7,8) 3x3 / 1: nine windows per pixel        pool_bwd<8> (generic)
 6 (2,8,6) 2x2 / 2    7 (1,7,5) 2x2 / 2 clipped   pool_fwd<8>, pool_bwd<8>
 8 (1,9,7) 2x3 / sy 1, sx 2    9 (1,8,9) 3x2 / sy 3, sx 1
10 (2,2,5) 3x3 / 2, H below the window   11 (1,1,1)   12 (1,3,3)
13 (1,12,12) 3x3 / 4 and 14 (1,6,6) 2x2 / 3: the plain ceil counted a window
   that starts outside the input here
C = 16 and 5 everywhere (8- and 1-channel lanes), 24 / 20 / 6 at 2 and 8
(8, 4, 2), 256 at 1; tensors 8 and 2 bytes into a larger buffer (4, 1).

Indices, selected values and uncovered pixels are compared exactly; values
against the bounds derived in test_pool_lrn_ref.py.  Worst measured |error| /
bound on an MI355X (``pytest -s`` prints them again, with the share of
windows that the argmax gap rule left out per fused case):

    pooling    avg y 1.000, avg dx 1.000, max / maxabs dx 1.000 (the half-ulp
               of the bf16 store itself); max / maxabs y and every argmax
               exact; 2 x 2 pair: dx 1.000, avg y exact (tie data)
    LRN        y 1.000, dx 0.998
    fused      y 0.999 (int32) / 1.000 (uint8), dx 0.999 / 0.999; no chosen
               element below its window's reference maximum (0.000 of 2 E);
               the gap rule left out at most 0.149 % of a case's windows
               (cap 0.5 %), none in 165 of the 172 cases
    (profiles/pool_lrn/gpu_tests_figures.txt, with the mutants these tests
    were checked against)
"""
import pytest
import torch

import veles_amd.ops as ops
from test_pool_lrn_ref import (
    AUX_FORMS, FUSED_I32, FUSED_I32_N, FUSED_U8, FUSED_U8_N, LEFT_OUT,
    LRN_SCALAR, LRN_SETS, LRN_VEC, MODES, POOL2_SHAPES, POOL_CASES, Ratios,
    run_lrn, run_lrn_pool_bwd, run_lrn_pool_fwd, run_pool, run_pool2)

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = Ratios()


@pytest.fixture(autouse=True, scope="module")
def _report():
    yield
    print("\nworst |error| / bound: " + ", ".join(
        "%s %.3f" % kv for kv in sorted(WORST.items())))
    print("windows the argmax gap rule left out (cap 0.5 %):")
    for k, v in sorted(LEFT_OUT.items()):
        print("    %-32s %.3f %%" % (k, 100.0 * v))


def _set(name, v):
    getattr(ops._lib.lib(), "hvk_set_%s_variant" % name)(v)


# ---------------------------------------------------------------- pooling
@pytest.mark.parametrize("geom,C", POOL_CASES)
@pytest.mark.parametrize("mode", MODES)
def test_pool(geom, C, mode):
    """Forward (bitwise selection or the avg bound) and backward from the
    reference's argmax, on normal and on tie data."""
    for data in ("normal", "ties"):
        WORST.merge(run_pool(DEV, geom, C, mode, data=data))


@pytest.mark.parametrize("geom", [1, 2, 4, 5, 8, 13, 14])
@pytest.mark.parametrize("mode", MODES)
def test_pool_bwd_aux(geom, mode):
    """The activation derivative of a separate aux (codes 1 to 4) and of
    aux = x (strict ReLU), 8-channel and scalar lanes."""
    for aux in AUX_FORMS[1:]:
        for C in (16, 5):
            WORST.merge(run_pool(DEV, geom, C, mode, aux=aux))


@pytest.mark.parametrize("geom", [1, 2])
@pytest.mark.parametrize("mode", ["max", "maxabs"])
@pytest.mark.parametrize("v", [0, 1])
def test_pool_bwd_variants(geom, mode, v):
    """The 2 x 2 block kernel (0) and the per-pixel kernel (1), each against
    the reference; geometry 2 has absent windows whose clamped twin names a
    pixel of the block."""
    try:
        _set("pool_bwd", v)
        for aux in (None, 2, "x"):
            for data in ("normal", "ties"):
                for C in (16, 256 if geom == 1 else 24):
                    WORST.merge(run_pool(DEV, geom, C, mode, data=data,
                                         aux=aux))
    finally:
        _set("pool_bwd", 0)


@pytest.mark.parametrize("geom", [2, 8])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("skip", [4, 1])
def test_pool_unaligned(geom, mode, skip):
    """C = 16 tensors that start 8 bytes (4-channel lanes) and 2 bytes
    (scalar lanes) into a larger buffer."""
    for aux in (None, 1):
        WORST.merge(run_pool(DEV, geom, 16, mode, data="ties", aux=aux,
                             skip=skip))


@pytest.mark.parametrize("shape", POOL2_SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_pool2(shape, mode):
    """The argmax-free pair on tie data: the backward's recomputed choice
    must be the forward's (the first maximum)."""
    for aux in (None, 1, 2, 4, "x"):
        WORST.merge(run_pool2(DEV, shape, mode, aux=aux))


# -------------------------------------------------------------------- LRN
@pytest.mark.parametrize("C,n", LRN_VEC)
def test_lrn_vec(C, n):
    """lrn_fwd_vec / lrn_bwd_vec: C = 8 is a single chunk without a halo on
    either side, n // 2 from 0 to 4."""
    for pset in sorted(LRN_SETS):
        WORST.merge(run_lrn(DEV, C, n, pset))


@pytest.mark.parametrize("C,n", LRN_SCALAR)
def test_lrn_scalar(C, n):
    """The wave-per-pixel kernels: C off the 8-grid, C = 70 over two wave
    passes, and C = 16 with n // 2 = 5 beyond the vector kernels' halo."""
    for pset in sorted(LRN_SETS):
        WORST.merge(run_lrn(DEV, C, n, pset))


@pytest.mark.parametrize("C,n", [(8, 1), (16, 5), (24, 9), (96, 3), (13, 5),
                                 (70, 11)])
def test_lrn_bwd_aux(C, n):
    for aux in AUX_FORMS[1:]:
        WORST.merge(run_lrn(DEV, C, n, "main", aux=aux))


# -------------------------------------------------------- fused LRN -> pool
@pytest.mark.parametrize("shape,sy,sx", FUSED_I32)
@pytest.mark.parametrize("n", FUSED_I32_N)
def test_lrn_pool_i32(shape, sy, sx, n):
    """lrn_pool3_fwd; lrn_pool3s2_bwd at stride 2, lrn_pool3_bwd otherwise."""
    for pset in sorted(LRN_SETS):
        WORST.merge(run_lrn_pool_fwd(DEV, shape, sy, sx, n, pset))
        WORST.merge(run_lrn_pool_bwd(DEV, shape, sy, sx, n, pset))
    for aux in AUX_FORMS[1:]:
        WORST.merge(run_lrn_pool_bwd(DEV, shape, sy, sx, n, aux=aux))


@pytest.mark.parametrize("shape", FUSED_U8)
@pytest.mark.parametrize("n", FUSED_U8_N)
def test_lrn_pool_u8(shape, n):
    """The default paths: the DPP walk (n = 3, 5, full windows, at most 64
    chunks), the loading walk (528 channels), u8p (clipped), the per-output
    kernel (n = 1, 7, 9); backward the DPP block kernel, the per-thread one
    past 64 chunks and at alpha = 0."""
    for pset in ("main", "alexnet", "alpha0"):
        WORST.merge(run_lrn_pool_fwd(DEV, shape, 2, 2, n, pset, u8=True))
        WORST.merge(run_lrn_pool_bwd(DEV, shape, 2, 2, n, pset, u8=True))
    for aux in (2, "x"):
        WORST.merge(run_lrn_pool_bwd(DEV, shape, 2, 2, n, u8=True, aux=aux))


@pytest.mark.parametrize("shape", FUSED_U8[:4])
@pytest.mark.parametrize("v", [0, 1, 2, 3, 4, 5])
def test_lrn_pool_u8_fwd_variants(shape, v):
    """0 the DPP walk, 5 the loading walk, 1 the preloading per-output
    kernel, 2 the walk without prefetch, 3 / 4 strips of 5 / 9 rows."""
    try:
        _set("lrn_fwd", v)
        for n in (3, 5):
            for pset in ("main", "k2"):
                WORST.merge(run_lrn_pool_fwd(DEV, shape, 2, 2, n, pset,
                                             u8=True))
    finally:
        _set("lrn_fwd", 0)


@pytest.mark.parametrize("shape", FUSED_U8[:4])
@pytest.mark.parametrize("v", [0, 1])
def test_lrn_pool_u8_bwd_variants(shape, v):
    """Loads issued first (0: one kernel per activation form) or next to
    their use (1), n // 2 from 1 to 4."""
    try:
        _set("lrn_bwd", v)
        for n in (3, 5, 7, 9):
            for aux in (None, 1, "x"):
                WORST.merge(run_lrn_pool_bwd(DEV, shape, 2, 2, n, u8=True,
                                             aux=aux))
    finally:
        _set("lrn_bwd", 0)


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("crafted", ["corner", "shared"])
@pytest.mark.parametrize("n", [1, 5, 9])
def test_lrn_pool_bwd_crafted(u8, crafted, n):
    """Reference-made argmax tensors in which every window names its
    bottom-right element (a pixel four windows share), and in which the four
    windows that share a pixel all name it: it sums four gradients."""
    for aux in (None, 2, "x"):
        for shape in ((2, 13, 13, 16), (1, 15, 15, 40)):
            WORST.merge(run_lrn_pool_bwd(DEV, shape, 2, 2, n, u8=u8, aux=aux,
                                         crafted=crafted))
