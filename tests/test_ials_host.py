"""CPU tests of implicit-feedback ALS: the fp64 reference (tests/ials_ref.py) against itself, the C ABI surface
and the argument checks that must fail on the host, before any device is touched."""
import ctypes as C
import math

import numpy as np
import pytest

import ials_ref

MFX_ERR_INVALID = -1  # include/mfx.h


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    return m


def _matrix(seed=0, rows=40, cols=30, density=0.2):
    from mfx import dataset as ds
    rng = np.random.default_rng(seed)
    mask = rng.random((rows, cols)) < density
    r, c = np.nonzero(mask)
    v = rng.integers(0, 6, r.size).astype(np.float32)  # strengths 0..5: explicit zeros included
    return ds.from_coo(rows, cols, r, c, v)


def test_shortcut_system_equals_dense_form():
    R = _matrix(1)
    rng = np.random.default_rng(2)
    H = rng.standard_normal((R.cols, 6))
    for alpha in (0.0, 1.0, 40.0):
        for s in range(R.rows):
            A, b = ials_ref.dense_system(R.csr_row_ptr, R.csr_col_idx, R.csr_val, s, H, 0.1, alpha)
            A2, b2 = ials_ref.shortcut_system(R.csr_row_ptr, R.csr_col_idx, R.csr_val, s, H, 0.1, alpha)
            np.testing.assert_allclose(A2, A, rtol=1e-12, atol=1e-10)
            np.testing.assert_allclose(b2, b, rtol=1e-12, atol=1e-10)


def test_loss_formula_equals_dense_loss():
    R = _matrix(3)
    rng = np.random.default_rng(4)
    W = rng.standard_normal((R.rows, 5)) * 0.3
    H = rng.standard_normal((R.cols, 5)) * 0.3
    for alpha in (0.0, 2.5, 40.0):
        d = ials_ref.dense_loss(R, W, H, 0.05, alpha)
        s = ials_ref.shortcut_loss(R, W, H, 0.05, alpha)
        assert abs(d - s) <= 1e-10 * abs(d), (d, s)


def test_reference_iteration_never_increases_the_loss():
    R = _matrix(5)
    H = np.random.default_rng(6).standard_normal((R.cols, 4)) * 0.1
    W = np.zeros((R.rows, 4))
    prev = ials_ref.dense_loss(R, W, H, 0.1, 10.0)
    for _ in range(4):
        W, H = ials_ref.iteration(R, H, 0.1, 10.0)
        cur = ials_ref.dense_loss(R, W, H, 0.1, 10.0)
        assert cur <= prev * (1 + 1e-12)
        prev = cur


def test_new_symbols_are_exported_and_bound(mfx):
    from mfx import _lib as L
    lib = mfx.lib()
    for name in ("mfx_ials_create", "mfx_ials_loss", "mfx_ials_half"):
        assert name in L.SIGNATURES
        assert hasattr(lib, name)
    assert lib.mfx_version() == L.MFX_VERSION == 2
    assert hasattr(mfx, "ImplicitAlsSolver") and hasattr(mfx, "ials_half")


def _create(mfx, R, k=8, alpha=1.0, schedule=1, out=True, p_null=False, r_null=False):
    from mfx import _lib as L
    from mfx.api import _csx
    p = mfx.parameter()
    p.k = k
    cp = p.to_c()
    cp.schedule = schedule
    h = C.c_void_p()
    csx = _csx(R)
    rc = mfx.lib().mfx_ials_create(C.byref(h) if out else None, None if r_null else C.byref(csx),
                                   None if p_null else C.byref(cp), alpha, L.MFX_HOST)
    return rc, mfx.lib().mfx_last_error().decode()


@pytest.mark.parametrize("alpha", [-1.0, -1e-30, math.nan, math.inf, -math.inf])
def test_create_rejects_bad_alpha_on_the_host(mfx, alpha):
    rc, msg = _create(mfx, _matrix(7), alpha=alpha)
    assert rc == MFX_ERR_INVALID, (rc, msg)  # not MFX_ERR_NO_DEVICE: nothing reached the device
    assert "alpha" in msg


@pytest.mark.parametrize("k", [0, 129, 1000])
def test_create_rejects_bad_rank_on_the_host(mfx, k):
    rc, msg = _create(mfx, _matrix(7), k=k)
    assert rc == MFX_ERR_INVALID, (rc, msg)
    assert "rank" in msg


def test_create_rejects_as_written_schedule_on_the_host(mfx):
    rc, msg = _create(mfx, _matrix(7), schedule=0)
    assert rc == MFX_ERR_INVALID, (rc, msg)
    assert "schedule" in msg


def test_create_rejects_null_arguments_on_the_host(mfx):
    R = _matrix(7)
    for kw in ({"out": False}, {"p_null": True}, {"r_null": True}):
        rc, msg = _create(mfx, R, **kw)
        assert rc == MFX_ERR_INVALID, (kw, rc, msg)


def test_loss_and_half_reject_bad_arguments_on_the_host(mfx):
    lib = mfx.lib()
    out = C.c_double(0.0)
    assert lib.mfx_ials_loss(None, C.byref(out)) == MFX_ERR_INVALID
    ptr = np.array([0, 1], np.uint32)
    idx = np.array([0], np.uint32)
    val = np.array([1.0], np.float32)
    X = np.ones((2, 4), np.float32)
    for bad_alpha in (-0.5, math.nan, math.inf):
        with pytest.raises(mfx.MfxError, match="alpha"):
            mfx.ials_half(ptr, idx, val, X, 4, 0.1, bad_alpha)
    for bad_k in (0, 129):
        Xk = np.ones((2, max(bad_k, 1)), np.float32)
        with pytest.raises(mfx.MfxError, match="rank"):
            mfx.ials_half(ptr, idx, val, Xk, bad_k, 0.1, 1.0)
