"""CPU tests of implicit ALS by block subspace sweeps: the fp64 reference (tests/ialsb_ref.py) against the dense
reference of the exact method, the C ABI surface, and the argument checks that must fail on the host, before any
device is touched."""
import ctypes as C
import math

import numpy as np
import pytest

import ials_ref
import ialsb_ref

MFX_ERR_INVALID, MFX_ERR_NO_DEVICE = -1, -2  # include/mfx.h


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    return m


def _matrix(seed=0, rows=40, cols=30, density=0.2):
    from mfx import dataset as ds
    rng = np.random.default_rng(seed)
    mask = rng.random((rows, cols)) < density
    mask[3, :] = False  # an empty user
    r, c = np.nonzero(mask)
    v = rng.integers(0, 6, r.size).astype(np.float32)  # strengths 0..5: explicit zeros included
    return ds.from_coo(rows, cols, r, c, v)


def test_single_block_from_zero_is_the_exact_half():
    R = _matrix(1)
    H = np.random.default_rng(2).standard_normal((R.cols, 6))
    for alpha in (0.0, 1.0, 40.0):
        want = ials_ref.half(R.csr_row_ptr, R.csr_col_idx, R.csr_val, H, 0.1, alpha)
        for d in (6, 7, 128):
            got = ialsb_ref.block_sweep(R.csr_row_ptr, R.csr_col_idx, R.csr_val, H, np.zeros((R.rows, 6)), 0.1, alpha, d)
            assert np.linalg.norm(got - want) <= 1e-12 * np.linalg.norm(want), (alpha, d)
            assert not np.any(got[3])


def test_more_sweeps_come_closer_to_the_exact_half():
    R = _matrix(3)
    k = 12
    H = np.random.default_rng(4).standard_normal((R.cols, k)) / np.sqrt(k)
    want = ials_ref.half(R.csr_row_ptr, R.csr_col_idx, R.csr_val, H, 0.1, 10.0)
    Y = np.zeros((R.rows, k))
    err = []
    for _ in range(4):
        Y = ialsb_ref.block_sweep(R.csr_row_ptr, R.csr_col_idx, R.csr_val, H, Y, 0.1, 10.0, 4)
        err.append(np.linalg.norm(Y - want))
    assert err[3] < err[0], err
    assert all(b <= a * (1 + 1e-12) for a, b in zip(err, err[1:])), err


def test_reference_sweeps_never_increase_the_loss():
    R = _matrix(5)
    k = 8
    H = np.random.default_rng(6).standard_normal((R.cols, k)) * 0.1
    W = np.zeros((R.rows, k))
    prev = ials_ref.dense_loss(R, W, H, 0.1, 10.0)
    for _ in range(4):
        W, H = ialsb_ref.iteration(R, H, W, 0.1, 10.0, 3)
        cur = ials_ref.dense_loss(R, W, H, 0.1, 10.0)
        assert cur <= prev * (1 + 1e-12)
        prev = cur


def test_new_symbols_are_exported_and_bound(mfx):
    from mfx import _lib as L
    lib = mfx.lib()
    for name in ("mfx_ials_block_create", "mfx_ials_block_half"):
        assert name in L.SIGNATURES
        assert hasattr(lib, name)
    assert lib.mfx_version() == L.MFX_VERSION == 2
    assert hasattr(mfx, "ials_block_half")
    import inspect
    assert "block" in inspect.signature(mfx.ImplicitAlsSolver.__init__).parameters


def _create(mfx, R, k=8, alpha=1.0, block=0, schedule=1, out=True, p_null=False, r_null=False):
    from mfx import _lib as L
    from mfx.api import _csx
    p = mfx.parameter()
    p.k = k
    cp = p.to_c()
    cp.schedule = schedule
    h = C.c_void_p()
    csx = _csx(R)
    rc = mfx.lib().mfx_ials_block_create(C.byref(h) if out else None, None if r_null else C.byref(csx),
                                         None if p_null else C.byref(cp), alpha, block, L.MFX_HOST)
    msg = mfx.lib().mfx_last_error().decode()
    if rc == 0:
        mfx.lib().mfx_als_destroy(h)
    return rc, msg


@pytest.mark.parametrize("alpha", [-1.0, -1e-30, math.nan, math.inf, -math.inf])
def test_create_rejects_bad_alpha_on_the_host(mfx, alpha):
    rc, msg = _create(mfx, _matrix(7), alpha=alpha)
    assert rc == MFX_ERR_INVALID, (rc, msg)  # not MFX_ERR_NO_DEVICE: nothing reached the device
    assert "alpha" in msg


@pytest.mark.parametrize("k", [0, 1025, 4096])
def test_create_rejects_bad_rank_on_the_host(mfx, k):
    rc, msg = _create(mfx, _matrix(7), k=k)
    assert rc == MFX_ERR_INVALID, (rc, msg)
    assert "rank" in msg


@pytest.mark.parametrize("block", [-1, 129, 1024])
def test_create_rejects_bad_block_on_the_host(mfx, block):
    rc, msg = _create(mfx, _matrix(7), k=256, block=block)
    assert rc == MFX_ERR_INVALID, (rc, msg)
    assert "block" in msg


def test_create_rejects_as_written_schedule_on_the_host(mfx):
    rc, msg = _create(mfx, _matrix(7), schedule=0)
    assert rc == MFX_ERR_INVALID, (rc, msg)
    assert "schedule" in msg


def test_create_rejects_null_arguments_on_the_host(mfx):
    R = _matrix(7)
    for kw in ({"out": False}, {"p_null": True}, {"r_null": True}):
        rc, msg = _create(mfx, R, **kw)
        assert rc == MFX_ERR_INVALID, (kw, rc, msg)


@pytest.mark.parametrize("k,block", [(129, 0), (256, 64), (1024, 128), (129, 1)])
def test_ranks_above_128_pass_the_argument_checks(mfx, k, block):
    rc, msg = _create(mfx, _matrix(7), k=k, block=block)
    if mfx.device_count() >= 1:
        assert rc == 0, (rc, msg)
    else:
        assert rc == MFX_ERR_NO_DEVICE, (rc, msg)


def test_half_rejects_bad_arguments_on_the_host(mfx):
    ptr = np.array([0, 1], np.uint32)
    idx = np.array([0], np.uint32)
    val = np.array([1.0], np.float32)
    X = np.ones((2, 4), np.float32)
    for bad_alpha in (-0.5, math.nan, math.inf):
        with pytest.raises(mfx.MfxError, match="alpha"):
            mfx.ials_block_half(ptr, idx, val, X, 4, 0.1, bad_alpha, 2)
    for bad_block in (-1, 129):
        with pytest.raises(mfx.MfxError, match="block"):
            mfx.ials_block_half(ptr, idx, val, X, 4, 0.1, 1.0, bad_block)
    for bad_k in (0, 1025):
        Xk = np.ones((2, max(bad_k, 1)), np.float32)
        with pytest.raises(mfx.MfxError, match="rank"):
            mfx.ials_block_half(ptr, idx, val, Xk, bad_k, 0.1, 1.0, 0)
    for k in (129, 256, 1024):  # valid: past the argument checks
        Xk = np.ones((2, k), np.float32)
        lib = mfx.lib()
        Y = np.empty((1, k), np.float32)
        from mfx.api import _f32, _u32
        rc = lib.mfx_ials_block_half(1, 1, _u32(ptr), _u32(idx), _f32(val), 2, _f32(Xk), None, _f32(Y), k, 64, 0.1, 1.0, 0)
        assert rc == (0 if mfx.device_count() >= 1 else MFX_ERR_NO_DEVICE), (k, rc, lib.mfx_last_error())
