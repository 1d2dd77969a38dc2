"""ALS Gramians and half-sweeps on inputs whose sums do not depend on the order of addition (tests/exact_sums.py; bounds and
preconditions checked on the host by test_exact_sums_host.py).

Gramians: X holds multiples of 1/8 in [-1, 1], so every product is a multiple of 1/64 and every partial sum of up to 2048 of
them is exact in fp32: the MFMA Gramian must equal the int64 Gramian and the oracle's bit for bit, and be bit-symmetric.

Diagonal systems: row i of X is x_i e_(i mod k) with x_i in {+-1/2, +-1}.  Every Gramian -- the implicit model's base Gramian
over all rows included -- is then diagonal and exact, every right-hand side is exact, the solution is y_c = b_c / A_cc and
exactly 0 where b_c = 0.  Each element is compared with the fp64 quotient; cap 64 ulp.  The cap is derived, not tuned: the
solve is a square root (or v_rsq) and two divisions or reciprocal multiplies, each within 1-2 ulp plus a rounding, under 16 ulp
together; the cap leaves 4x.  Dropping any single entry of the longest segment moves its coordinate by at least 256 ulp
(exact_sums.check_sensitivity), so a Gramian that loses or doubles an entry across its splits, or a reducer that drops a
partial, cannot stay under the cap.  Segments of 0 .. 20 000 entries: unsplit, split in two and three, and ten chunks.

A block subspace sweep from a warm start y0 computes y0 - (A y0 - b) / A: its rounding is relative to max(|y0|, |y|), so the
warm-start cases measure the 64 ulp at max(|y0_c|, |y_c|); from zero they are measured at y_c.

Measured maxima (MI355X, printed by the tests as `exact-measured` lines):
    als_half variant 1 (MFMA Gramian + Cholesky solve), k = 5 .. 128:      3.52 ulp
    als_half variant 0 (as written, bit-equal to the oracle):             2.99 ulp
    ials_half, k = 5 .. 128, alpha 0 / 1 / 0.5:                            4.68 ulp
    ials_block_half from zero, k = 64 .. 1024, d = 16 / 64 / 128:          4.13 ulp
    ials_block_half from the warm start (at max(|y0|, |y|)):              7.11 ulp
    (the same figures for every d at a given k and alpha: the off-diagonal blocks are zero, each coordinate is solved alone)
"""
import numpy as np
import pytest

import exact_sums as ex
from exact_sums import bits

pytestmark = pytest.mark.gpu

LAM = ex.ALS_LAMBDA


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1
    return m


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def tables():
    """k -> (X, x, ptr, idx, val) of the one-hot table and its segments: one data set per k for the whole module"""
    cache = {}

    def get(k):
        if k not in cache:
            X, x = ex.one_hot_table(ex.DIAGONAL_ROWS, k, k)
            cache[k] = (X, x) + ex.diagonal_segments(ex.DIAGONAL_ROWS, ex.DIAGONAL_SIZES, 100 + k)
        return cache[k]
    return get


# ------------------------------------------------------------------ Gramians
@pytest.mark.parametrize("k", ex.GRAMIAN_KS)
def test_gramian_bit_exact(mfx, orc, k):
    rng = np.random.default_rng(1000 + k)
    X = ex.dyadic_table(300, k, k)
    for count in ex.GRAMIAN_COUNTS:
        idx = rng.integers(0, 300, count).astype(np.uint32)
        want = ex.int_gramian(idx, X)
        assert np.array_equal(bits(orc.gramian(idx, X, k)), bits(want)), (k, count)
        A = mfx.als_gramian(idx, X, k)
        assert np.array_equal(bits(A), bits(A.T)), (k, count)
        nz = want != 0
        bad = np.argwhere(bits(A) != bits(want))
        assert np.array_equal(bits(A[nz]), bits(want[nz])) and np.all(A[~nz] == 0), (k, count, bad[:10])


# ------------------------------------------------------------------ diagonal systems
def _check_solution(Y, ptr, idx, val, x, k, alpha, what, Y0=None):
    A, b, y = ex.diagonal_solution(ptr, idx, val, x, k, LAM, alpha)
    n = np.diff(ptr.astype(np.int64))
    assert not np.any(Y[n == 0]), what  # an empty segment gives exactly 0
    if Y0 is None:
        assert np.all(Y[b == 0] == 0), (what, "b = 0 must give exactly 0", np.argwhere((b == 0) & (Y != 0))[:10])
        err = ex.ulps(Y, y)
    else:
        at = np.maximum(np.abs(y), np.abs(Y0.astype(np.float64)))
        err = np.abs(Y.astype(np.float64) - y) / np.spacing(at.astype(np.float32)).astype(np.float64)
        err[n == 0] = 0
    worst = float(err.max())
    s, c = np.unravel_index(int(np.argmax(err)), err.shape)
    print(f"exact-measured {what} max_ulp={worst:.2f} (segment of {int(n[s])} entries, coordinate {c})")
    assert worst <= ex.ULP_CAP, (what, worst, "segment", int(s), "entries", int(n[s]), "coordinate", int(c), float(Y[s, c]), float(y[s, c]))
    return worst


@pytest.mark.parametrize("k", ex.HALF_KS)
def test_als_half_diagonal_systems(mfx, orc, tables, k):
    X, x, ptr, idx, val = tables(k)
    assert ex.check_sensitivity(ptr, idx, val, x, k, LAM) >= ex.ULP_SENSITIVITY
    Y = mfx.als_half(ptr, idx, val, X, k, LAM, variant=1)
    _check_solution(Y, ptr, idx, val, x, k, None, f"als_half k={k} variant=1")
    Y0 = mfx.als_half(ptr, idx, val, X, k, LAM, variant=0)
    assert np.array_equal(bits(Y0), bits(orc.als_half(ptr, idx, val, X, k, LAM, orc.max_threads()))), k
    _check_solution(Y0, ptr, idx, val, x, k, None, f"als_half k={k} variant=0")


@pytest.mark.parametrize("alpha", ex.IALS_ALPHAS)
@pytest.mark.parametrize("k", ex.HALF_KS)
def test_ials_half_diagonal_systems(mfx, tables, k, alpha):
    X, x, ptr, idx, val = tables(k)
    assert ex.check_sensitivity(ptr, idx, val, x, k, LAM, alpha) >= ex.ULP_SENSITIVITY
    Y = mfx.ials_half(ptr, idx, val, X, k, LAM, alpha)
    _check_solution(Y, ptr, idx, val, x, k, alpha, f"ials_half k={k} alpha={alpha}")


@pytest.mark.parametrize("d", ex.BLOCK_DS)
@pytest.mark.parametrize("k", ex.BLOCK_KS)
def test_ials_block_half_diagonal_systems(mfx, tables, k, d):
    """off-diagonal blocks are zero, so ONE sweep gives the solution, from zero and from a dyadic warm start"""
    X, x, ptr, idx, val = tables(k)
    rng = np.random.default_rng(2000 + k)
    Y_in = (rng.integers(-16, 17, (len(ex.DIAGONAL_SIZES), k)).astype(np.float32) / np.float32(64))
    for alpha in ex.IALS_ALPHAS:
        assert ex.check_sensitivity(ptr, idx, val, x, k, LAM, alpha) >= ex.ULP_SENSITIVITY
        Y = mfx.ials_block_half(ptr, idx, val, X, k, LAM, alpha, d)
        _check_solution(Y, ptr, idx, val, x, k, alpha, f"ials_block_half k={k} d={d} alpha={alpha} start=zero")
        Y = mfx.ials_block_half(ptr, idx, val, X, k, LAM, alpha, d, Y_in=Y_in)
        _check_solution(Y, ptr, idx, val, x, k, alpha, f"ials_block_half k={k} d={d} alpha={alpha} start=Y0", Y0=Y_in)
