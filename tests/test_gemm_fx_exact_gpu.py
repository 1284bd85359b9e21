"""Exact-precision SGEMM / DGEMM (csrc/kernels/gemm_f32.hip) over the whole
template space: both types, the three precision levels and the four layouts,
at tile, wave, fragment and K-tile edges, on every loader path, with alpha /
beta / accumulate, and against per-element rounding-error bounds.

Sections 1-3 use integer-valued operands in [-8, 8] with K <= 4096: every
partial sum is below 2^18, every addition is exact in any order and every
compensation term is zero, so the kernel must reproduce the int64 product
bit for bit (torch.equal, no tolerance).  Section 4 uses real-valued inputs
and the standard bounds; tests/test_gemm_fx_model.py shows, without a GPU,
that those bounds separate the compensated levels from the plain one.

Which tests launch which (dtype, level, layout) instance: every one of the
24 is launched by test_exact_integer_product and test_alpha_beta_accumulate;
levels 0 and 2 of both types in all four layouts also by
test_loader_paths_poisoned; levels 1 and 2 in all layouts by
test_long_k_compensated_bound, level 0 by test_long_k_plain_exceeds_bound
and (f32) test_level0_f32_bound."""
import numpy as np
import pytest
import torch

import veles_amd.ops as ops
from test_gemm_fx_model import BK, U, four_value_row, long_k_case

pytestmark = pytest.mark.gpu
DEV = "cuda"

DTYPES = [torch.float32, torch.float64]
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]
NPT = {torch.float32: np.float32, torch.float64: np.float64}
EPC = {torch.float32: 4, torch.float64: 2}   # elements per 16-byte chunk


def _ints(rows, cols, salt):
    """An asymmetric integer matrix in [-8, 8] (int64): no two rows and no
    two columns agree, and it is not its own transpose."""
    i = torch.arange(rows, dtype=torch.int64).view(-1, 1)
    k = torch.arange(cols, dtype=torch.int64).view(1, -1)
    return (i * 5 + k * 3 + (i * k) % 7 + (i // 16) + salt) % 17 - 8


_CASES = {}


def _int_case(M, N, K):
    """(A[M][K], B[K][N], A @ B) in int64; computed once per shape."""
    if (M, N, K) not in _CASES:
        A, B = _ints(M, K, 1), _ints(K, N, 4)
        _CASES[M, N, K] = (A, B, A @ B)
    return _CASES[M, N, K]


def _stored(X, trans, dtype):
    """The logical operand as the layout stores it, on the device."""
    return (X.t() if trans else X).contiguous().to(DEV, dtype)


# ------------------------------------------------ 1. bit-exact products
SHAPES = [(1, 1, 1), (15, 17, 3), (63, 65, 31), (65, 63, 33), (127, 129, 65),
          (129, 127, 64), (257, 130, 100), (128, 256, 96)]


@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_integer_product(dtype, level, M, N, K, ta, tb):
    A, B, ref = _int_case(M, N, K)
    # op(a) = A: a transposed operand is stored [K][M]; op(b) = B: trans_b
    # means b is stored [N][K]
    got = ops.gemm(_stored(A, ta, dtype), _stored(B, tb, dtype),
                   trans_a=bool(ta), trans_b=bool(tb), precision_level=level)
    assert got.dtype == dtype and got.shape == (M, N)
    assert torch.equal(got.cpu(), ref.to(dtype))


# ------------------------------------- 2. loader paths, poisoned padding
def _poisoned_view(X, dtype, pitch, offset):
    """X (int64 [r][c]) as the view [:r, :c] of a NaN-filled parent with
    three more rows and row pitch ``pitch``, starting ``offset`` elements
    into the allocation."""
    r, c = X.shape
    assert pitch >= c
    flat = torch.full((offset + (r + 3) * pitch,), float("nan"), dtype=dtype,
                      device=DEV)
    view = flat[offset:].view(r + 3, pitch)[:r, :c]
    view.copy_(X.to(DEV, dtype))
    return view


def _pitch(cols):
    """A row pitch > cols that is a multiple of 8 (so of either EPC)."""
    return (cols + 8) // 8 * 8 + 8


SENTINEL = {torch.float32: (torch.int32, 0x7FC0DEAD),
            torch.float64: (torch.int64, 0x7FF8DEAD0000BEEF)}

# (name, M, N, K per dtype, element offset of the operand views)
#  ktail / rowtail: aligned base and pitch, K and the MN extents not
#  multiples of EPC - the vector path meets a K tail (K-major operand) and a
#  row tail (MN-major operand); f32 K = 30 is below one K tile, 71 gives an
#  odd number of K tiles for both types.
#  unaligned: every extent and pitch a multiple of EPC, the base one element
#  off the 16-byte grid - the scalar path with nothing else odd.
LOADER_CASES = [
    ("ktail", 131, 45, {torch.float32: 30, torch.float64: 31}, 0),
    ("ktail3", 67, 133, {torch.float32: 71, torch.float64: 71}, 0),
    ("unaligned", 68, 132, {torch.float32: 64, torch.float64: 64}, 1),
]


@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("case", LOADER_CASES, ids=lambda c: c[0])
@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_loader_paths_poisoned(dtype, level, case, ta, tb):
    name, M, N, Ks, off = case
    K, epc = Ks[dtype], EPC[dtype]
    A, B, ref = _int_case(M, N, K)
    sa = A.t() if ta else A
    sb = B.t() if tb else B
    a = _poisoned_view(sa, dtype, _pitch(sa.shape[1]), off)
    b = _poisoned_view(sb, dtype, _pitch(sb.shape[1]), off)
    if name == "unaligned":
        assert M % epc == 0 and N % epc == 0 and K % epc == 0
        assert a.data_ptr() % 16 and b.data_ptr() % 16
    else:
        assert M % epc and N % epc and K % epc
        assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
    assert a.stride(0) % epc == 0 and b.stride(0) % epc == 0
    # the output: a view of a parent holding a NaN sentinel bit pattern
    it, bits = SENTINEL[dtype]
    ldc = N + 5
    parent = torch.full((M + 2, ldc), bits, dtype=it, device=DEV).view(dtype)
    out = parent[:M, :N]
    ret = ops.gemm(a, b, trans_a=bool(ta), trans_b=bool(tb), out=out,
                   beta=0.0, precision_level=level)
    assert ret.data_ptr() == out.data_ptr()
    res = parent.cpu()
    # beta == 0 overwrites the NaN, it does not multiply it
    assert torch.equal(res[:M, :N], ref.to(dtype))
    # and nothing outside the view has changed, bit for bit
    raw = res.view(it).clone()
    raw[:M, :N] = bits
    assert torch.equal(raw, torch.full_like(raw, bits))


# --------------------------------------- 3. alpha / beta / accumulate
@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_alpha_beta_accumulate(dtype, level, ta, tb):
    M, N, K = 130, 70, 50
    A, B, ref = _int_case(M, N, K)
    C = _ints(M, N, 9)
    a, b = _stored(A, ta, dtype), _stored(B, tb, dtype)
    kw = dict(trans_a=bool(ta), trans_b=bool(tb), precision_level=level)
    # |A @ B| <= 64 K: halving it and doubling C are exact
    out = C.to(DEV, dtype)
    ops.gemm(a, b, out=out, alpha=0.5, beta=2.0, **kw)
    assert torch.equal(out.cpu(), 0.5 * ref.to(dtype) + 2.0 * C.to(dtype))
    out = C.to(DEV, dtype)
    ops.gemm(a, b, out=out, accumulate=True, **kw)
    assert torch.equal(out.cpu(), (C + ref).to(dtype))
    out = torch.full((M, N), float("nan"), dtype=dtype, device=DEV)
    ops.gemm(a, b, out=out, accumulate="overwrite", **kw)
    assert torch.equal(out.cpu(), ref.to(dtype))


# ----------------------------------------- 4. rounding-error bounds
def _run(A, B, dtype, ta, tb, level):
    """ops.gemm on float64 host operands A[M][K], B[K][N] rounded to dtype;
    the result as float64 on the host."""
    a = (A.t() if ta else A).contiguous().to(DEV, dtype)
    b = (B.t() if tb else B).contiguous().to(DEV, dtype)
    kw = {} if level is None else {"precision_level": level}
    return ops.gemm(a, b, trans_a=bool(ta), trans_b=bool(tb), **kw) \
        .double().cpu()


_UNIFORM = {}


def _uniform_case(M, N, K):
    """Inputs uniform in +-0.5 rounded to float32, their float64 product and
    S = |A| @ |B| (float64, from the rounded inputs); computed once."""
    if (M, N, K) not in _UNIFORM:
        g = torch.Generator().manual_seed(M + N + K)
        A = (torch.rand(M, K, generator=g, dtype=torch.float64) - 0.5) \
            .float().double()
        B = (torch.rand(K, N, generator=g, dtype=torch.float64) - 0.5) \
            .float().double()
        _UNIFORM[M, N, K] = (A, B, A @ B, A.abs() @ B.abs())
    return _UNIFORM[M, N, K]


@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("M,N,K", [(17, 1999, 231), (7777, 17, 219),
                                   (9, 7, 800)])
def test_level0_f32_bound(M, N, K, ta, tb):
    """|got - ref| <= (K + 2) u S per element: gamma_K for the products and
    the K - 1 additions in any order, the rest slack; the float64
    reference's own K 2^-53 S is far below it."""
    A, B, ref, S = _uniform_case(M, N, K)
    got = _run(A, B, torch.float32, ta, tb, 0)
    err = (got - ref).abs()
    bound = (K + 2) * U[np.float32] * S
    print("max error / (u S): %.2f of %d" %
          ((err / (U[np.float32] * S)).max().item(), K + 2))
    assert (err <= bound).all()


K_LONG = 1 << 17


_LONG = []


def _long_case():
    """(A, B, fsum reference, S) as float64 tensors; computed once."""
    if not _LONG:
        _LONG.extend(torch.tensor(x) for x in long_k_case(K_LONG))
    return _LONG


def _ratio(got, ref, S, dtype):
    return ((got - ref).abs() / (U[NPT[dtype]] * S)).max().item()


@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_long_k_compensated_bound(dtype, level, ta, tb):
    """8 x 8 outputs over K = 2^17 against math.fsum of the exact products:
    |got - ref| <= (BK + 4) u S per element - each tile sum carries at most
    gamma_BK, the Kahan / TwoSum sum over the tiles 2u + O(nk u^2), the last
    u is slack.  The bound does not grow with K."""
    A, B, ref, S = _long_case()
    got = _run(A, B, dtype, ta, tb, level)
    bk, u = BK[NPT[dtype]], U[NPT[dtype]]
    print("max error / (u S): %.2f of %d" % (_ratio(got, ref, S, dtype),
                                             bk + 4))
    assert ((got - ref).abs() <= (bk + 4) * u * S).all()


@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_long_k_plain_exceeds_bound(dtype, ta, tb):
    """The same inputs at level 0 leave the compensated levels' bound for at
    least one element: the inputs discriminate."""
    A, B, ref, S = _long_case()
    got = _run(A, B, dtype, ta, tb, 0)
    bk, u = BK[NPT[dtype]], U[NPT[dtype]]
    print("max error / (u S): %.2f, bound %d" % (_ratio(got, ref, S, dtype),
                                                 bk + 4))
    assert ((got - ref).abs() > (bk + 4) * u * S).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_level2_is_twosum(dtype):
    """1 + 2^100 + 1 - 2^100, the four values in four different K tiles:
    TwoSum keeps both ones, the plain chain loses both.  (Level 1 is not
    pinned: Kahan's answer depends on the type here.)"""
    a, b = (torch.from_numpy(x) for x in four_value_row())
    for ta, tb in LAYOUTS:
        got2 = _run(a, b, dtype, ta, tb, 2)
        got0 = _run(a, b, dtype, ta, tb, 0)
        assert torch.equal(got2, torch.full_like(got2, 2.0)), (ta, tb)
        assert torch.equal(got0, torch.zeros_like(got0)), (ta, tb)


# ------------------------------------------------- 5. config default
@pytest.fixture
def engine_level():
    from veles_amd.utils.config import root, get
    old = get(root.common.engine.precision_level, 0)
    try:
        yield root.common.engine
    finally:
        root.common.engine.precision_level = old


@pytest.mark.parametrize("dtype", DTYPES)
def test_config_default_level(dtype, engine_level):
    A, B, _, _ = _long_case()
    engine_level.precision_level = 2
    default = _run(A, B, dtype, 0, 0, None)
    assert torch.equal(default, _run(A, B, dtype, 0, 0, 2))
    assert not torch.equal(default, _run(A, B, dtype, 0, 0, 0))


def test_device_benchmark_f64_level1():
    from veles_amd.accelerated_units import DeviceBenchmark
    from veles_amd.backends import Device
    from veles_amd.dummy import DummyWorkflow
    bench = DeviceBenchmark(DummyWorkflow(), size=200, repeats=2,
                            dtype="float64", precision_level=1)
    bench.initialize(device=Device(backend="hip"))
    bench.run()
    assert bench.seconds > 0 and bench.gflops > 0
    assert bench.c_.dtype == torch.float64
    assert torch.isfinite(bench.c_).all()
