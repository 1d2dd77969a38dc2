"""GPU tests of the device inverse of a symmetric positive definite matrix (mfx_spd_inverse, csrc/spd_inverse.hip): the
preconditioner of implicit ALS by conjugate gradients.

Matrices, for every k (the blocks are 32 wide: 63 / 64 / 65, 127 .. 130 sit on their edges, 37 / 63 / 65 / 127 / 129 / 130 /
1000 are no multiple of 4 or of 32):
    well conditioned   G = H^T H + 0.1 I with H = foldin_cg_ref.inputs(k)[3] (6000 rows ~ N(0, 1/k)): condition number 1.0 .. 5.5
    ill conditioned    the same with column j of H scaled by 10^(-2 j / (k - 1)) and lambda = 3e-4 * 6000 / k, which puts the
                       condition number of the fp32 matrix at 2.5e3 .. 2.9e3 (asserted to lie in [1e3, 1e5]; k >= 2: a 1 x 1
                       matrix has condition number 1)
Bound: |I - A X|_F, evaluated in fp64, at most k 2^-24 cond_2(A), the first-order bound of an inverse through a Cholesky
factorisation; an indexing error is O(1) against it.  The result must be exactly symmetric and the same bits on every call.

Measured on the MI355X (printed as `spdinv-measured` lines; profiles/r22_ials_cg_accuracy.txt holds every line), residual
of mfx_spd_inverse / of np.linalg.inv on the same fp32 matrix / share of the bound the former uses:
    well conditioned  k =    1: 1.6e-09 / 1.6e-09 / 0.03      k =  128: 3.3e-06 / 2.8e-07 / 0.24
                      k =    2: 5.0e-08 / 5.0e-08 / 0.41      k =  160: 3.8e-06 / 2.8e-07 / 0.21
                      k =   37: 7.4e-07 / 1.3e-07 / 0.25      k =  256: 6.4e-06 / 4.4e-07 / 0.18
                      k =   64: 1.6e-06 / 2.1e-07 / 0.28      k = 1024: 3.3e-05 / 9.9e-07 / 0.10
    ill conditioned   k = 2 ... 1024: 2.3e-08 ... 8.4e-05 / 2.3e-08 ... 3.2e-06 / below 0.001
Up to k = 32 the whole inverse is formed in fp64 and rounded once (numpy's figure); above, the fp32 fused multiply-add chains of
the 32 x 32 tiles leave 5 to 33 times the residual of LAPACK's fp32 inverse, a quarter of the bound at most.
"""
import functools

import numpy as np
import pytest

import foldin_cg_ref as ref

pytestmark = pytest.mark.gpu

MFX_ERR_INVALID = -1  # include/mfx.h
KS = [1, 2, 37, 63, 64, 65, 127, 128, 129, 130, 160, 256, 1000, 1024]


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1, m.lib().mfx_last_error()
    return m


@functools.lru_cache(maxsize=None)
def matrix(k, ill):
    """(A fp32, cond_2 of the fp32 matrix from its fp64 eigenvalues)."""
    H = ref.inputs(k)[3].astype(np.float64)
    lam = 0.1
    if ill:
        H = H * (10.0 ** (-2.0 * np.arange(k) / (k - 1)))[None, :]
        lam = 3e-4 * ref.COLS / k
    A = (H.T @ H + lam * np.eye(k)).astype(np.float32)
    ev = np.linalg.eigvalsh(A.astype(np.float64))
    assert ev[0] > 0
    return A, float(ev[-1] / ev[0])


def residual(A, X):
    return float(np.linalg.norm(np.eye(A.shape[0]) - A.astype(np.float64) @ X.astype(np.float64)))


# (k = 1 has no ill-conditioned case: a 1 x 1 matrix has condition number 1 whatever its entry)
@pytest.mark.parametrize("k,ill", [(k, ill) for k in KS for ill in (False, True) if not (ill and k == 1)])
def test_inverse_within_the_first_order_bound(mfx, k, ill):
    A, cond = matrix(k, ill)
    if ill:
        assert 1e3 <= cond <= 1e5, (k, cond)
    else:
        assert cond <= 6.0, (k, cond)
    X = mfx.spd_inverse(A)
    assert X.shape == (k, k) and X.dtype == np.float32 and np.isfinite(X).all()
    assert np.array_equal(X.view(np.uint32), X.T.view(np.uint32)), k  # exactly symmetric
    again = mfx.spd_inverse(A.copy())
    assert np.array_equal(X.view(np.uint32), again.view(np.uint32)), k  # the same bits on every call
    got, bound = residual(A, X), k * 2.0 ** -24 * cond
    numpy32 = residual(A, np.linalg.inv(A))
    print(f"spdinv-measured k={k} {'ill' if ill else 'well'} cond={cond:.4g} residual={got:.3e} bound={bound:.3e} "
          f"numpy_fp32_inverse={numpy32:.3e} max_abs={float(np.max(np.abs(np.eye(k) - A.astype(np.float64) @ X.astype(np.float64)))):.3e}")
    assert got <= bound, (k, ill, got, bound)


@pytest.mark.parametrize("k", [20, 65, 160])
def test_a_matrix_that_is_not_positive_definite_is_refused(mfx, k):
    from mfx.api import _f32
    A, _ = matrix(k, False)
    ev, V = np.linalg.eigh(A.astype(np.float64))
    ev[k // 2] = -0.5  # one negative eigenvalue
    neg = ((V * ev[None, :]) @ V.T).astype(np.float32)
    neg = ((neg + neg.T) / 2).astype(np.float32)
    nan = A.copy()
    nan[k - 1, k - 1] = np.nan
    for bad, what in ((neg, "negative eigenvalue"), (nan, "NaN entry")):
        out = np.empty_like(bad)
        rc = mfx.lib().mfx_spd_inverse(k, _f32(np.ascontiguousarray(bad)), _f32(out), 0)
        assert rc == MFX_ERR_INVALID, (k, what, rc)
        assert "positive definite" in mfx.lib().mfx_last_error().decode()
    X = mfx.spd_inverse(A)  # ... and the next call is served
    assert residual(A, X) <= k * 2.0 ** -24 * matrix(k, False)[1]
