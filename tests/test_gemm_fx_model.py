"""The arithmetic of the exact-precision GEMM's three precision levels
(csrc/kernels/gemm_f32.hip) in a NumPy model, and the error bounds that
tests/test_gemm_fx_exact_gpu.py holds the kernel to.

The model follows the kernel: every K tile (BK = 32 f32 / 16 f64 elements)
is summed sequentially, one rounding per product-and-add as in an fma chain,
in the operand type; level 0 carries one accumulator through all tiles,
levels 1 and 2 start every tile from zero and add the tile sum to the running
sum with the Kahan / TwoSum update written exactly as in the kernel's fold().
(The order of the four products inside one MFMA is not modelled; none of the
bounds below depends on it.)

With u the unit roundoff and S = |A| @ |B|:
  * a tile sum carries at most gamma_BK * S_tile;
  * a Kahan or TwoSum sum over the nk tile sums adds 2u + O(nk u^2);
so levels 1 and 2 stay inside (BK + 4) * u * S whatever K is, and a plain
chain over a long K does not.  The model shows both on the GPU test's inputs,
on a machine without a GPU."""
import math
from functools import lru_cache

import numpy as np
import pytest

BK = {np.float32: 32, np.float64: 16}
U = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
BIG = 2.0 ** 100


def long_k_inputs(K, M=8, N=8, seed=11):
    """A[M][K], B[K][N] (float64) with entries 1 + j / 2^20, j in [0, 2^20):
    21 significant bits, so the entries are float32 numbers and every
    product is exact in float64."""
    rs = np.random.RandomState(seed)
    a = 1.0 + rs.randint(0, 1 << 20, size=(M, K)).astype(np.float64) / (1 << 20)
    b = 1.0 + rs.randint(0, 1 << 20, size=(K, N)).astype(np.float64) / (1 << 20)
    return a, b


def fsum_ref(a, b):
    """The correctly rounded float64 value of every dot product: math.fsum
    over the exact float64 products."""
    M, N = a.shape[0], b.shape[1]
    ref = np.empty((M, N), dtype=np.float64)
    for i in range(M):
        for j in range(N):
            ref[i, j] = math.fsum(a[i, :] * b[:, j])
    return ref


@lru_cache(maxsize=None)
def long_k_case(K):
    """(a, b, ref, S) of long_k_inputs(K); computed once, never modified."""
    a, b = long_k_inputs(K)
    ref = fsum_ref(a, b)
    S = np.abs(a) @ np.abs(b)
    for x in (a, b, ref, S):
        x.setflags(write=False)
    return a, b, ref, S


def four_value_row(K=128, N=5):
    """One row of A with 1, 2^100, 1, -2^100 in four different K tiles (of
    either depth) and B all ones: the exact product is 2."""
    a = np.zeros((1, K), dtype=np.float64)
    a[0, 0], a[0, 32], a[0, 64], a[0, 96] = 1.0, BIG, 1.0, -BIG
    return a, np.ones((K, N), dtype=np.float64)


def model_gemm(a, b, T, level):
    """op(A) @ op(B) as the kernel computes it, for all outputs at once."""
    M, K = a.shape
    N = b.shape[1]
    bk = BK[T]
    a64, b64 = a.astype(T).astype(np.float64), b.astype(T).astype(np.float64)
    acc = np.zeros((M, N), dtype=T)
    s = np.zeros((M, N), dtype=T)
    comp = np.zeros((M, N), dtype=T)
    for k0 in range(0, K, bk):
        for k in range(k0, min(K, k0 + bk)):
            # product exact in float64 (operands of <= 24 bits, or float64
            # operands of 21 bits), then one rounding to T: an fma
            p = a64[:, k, None] * b64[None, k, :]
            acc = (acc.astype(np.float64) + p).astype(T)
        if level == 0:
            continue
        x = acc
        if level == 1:      # Kahan
            y = x - comp
            u = s + y
            comp = (u - s) - y
            s = u
        else:               # TwoSum (Neumaier)
            u = s + x
            bp = u - s
            comp = comp + ((s - (u - bp)) + (x - bp))
            s = u
        acc = np.zeros((M, N), dtype=T)
    if level == 0:
        return acc
    return s if level == 1 else s + comp


def error_in_us(got, ref, S, T):
    """max over the outputs of |got - ref| / (u * S)."""
    return float((np.abs(got.astype(np.float64) - ref) / (U[T] * S)).max())


K_MODEL = 1 << 14


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_compensated_levels_stay_inside_the_bound(T, level):
    a, b, ref, S = long_k_case(K_MODEL)
    got = model_gemm(a, b, T, level)
    err = np.abs(got.astype(np.float64) - ref)
    bound = (BK[T] + 4) * U[T] * S
    print("level %d %s: max error %.2f u*S, bound %d u*S" %
          (level, T.__name__, error_in_us(got, ref, S, T), BK[T] + 4))
    assert (err <= bound).all()


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_plain_level_exceeds_the_bound(T):
    a, b, ref, S = long_k_case(K_MODEL)
    got = model_gemm(a, b, T, 0)
    err = np.abs(got.astype(np.float64) - ref)
    bound = (BK[T] + 4) * U[T] * S
    print("level 0 %s: max error %.2f u*S, bound %d u*S" %
          (T.__name__, error_in_us(got, ref, S, T), BK[T] + 4))
    assert (err > bound).any()


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_four_value_row(T):
    a, b = four_value_row()
    assert (model_gemm(a, b, T, 2) == 2.0).all()
    assert (model_gemm(a, b, T, 0) == 0.0).all()


def test_fsum_ref_is_exact_on_integers():
    rs = np.random.RandomState(0)
    a = rs.randint(-8, 9, size=(3, 500)).astype(np.float64)
    b = rs.randint(-8, 9, size=(500, 4)).astype(np.float64)
    assert np.array_equal(fsum_ref(a, b),
                          (a.astype(np.int64) @ b.astype(np.int64)))
