"""CPU tests of explicit ALS by block subspace sweeps: the fp64 reference (tests/alsb_ref.py) against the dense solve, the
C ABI surface, and the argument checks that must fail on the host, before any device is touched (a refusal is
MFX_ERR_INVALID, never MFX_ERR_NO_DEVICE, and names the offending argument)."""
import ctypes as C
import inspect
import math

import numpy as np
import pytest

import alsb_ref

MFX_ERR_INVALID, MFX_ERR_NO_DEVICE = -1, -2  # include/mfx.h
NEW = ("mfx_als_block_create", "mfx_als_block_half", "mfx_rec_fold_in_block_setup_als")


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
    v = rng.integers(-2, 6, r.size).astype(np.float32)  # explicit zeros and negative values included
    return ds.from_coo(rows, cols, r, c, v)


# ------------------------------------------------------------------------------------------------ the fp64 reference
@pytest.mark.parametrize("reg", [0, 1])
def test_single_block_from_any_start_is_the_dense_solve(reg):
    R = _matrix(1)
    k = 6
    H = np.random.default_rng(2).standard_normal((R.cols, k))
    want = np.zeros((R.rows, k))
    for s in range(R.rows):
        if R.csr_row_ptr[s + 1] > R.csr_row_ptr[s]:
            A, b = alsb_ref.dense_system(R.csr_row_ptr, R.csr_col_idx, R.csr_val, s, H, 0.1, reg)
            want[s] = np.linalg.solve(A, b)
    for start in (np.zeros((R.rows, k)), np.random.default_rng(3).standard_normal((R.rows, k))):
        for d in (6, 7, 128):
            got = alsb_ref.block_sweep(R.csr_row_ptr, R.csr_col_idx, R.csr_val, H, start, 0.1, d, reg)
            assert np.linalg.norm(got - want) <= 1e-12 * np.linalg.norm(want), (reg, d)
            assert not np.any(got[3])


@pytest.mark.parametrize("reg", [0, 1])
def test_more_sweeps_come_closer_and_never_increase_the_objective(reg):
    R = _matrix(3)
    k = 12
    H = np.random.default_rng(4).standard_normal((R.cols, k)) / np.sqrt(k)
    want = alsb_ref.block_sweep(R.csr_row_ptr, R.csr_col_idx, R.csr_val, H, np.zeros((R.rows, k)), 0.1, k, reg)
    Y, err = np.zeros((R.rows, k)), []
    for _ in range(4):
        Y = alsb_ref.block_sweep(R.csr_row_ptr, R.csr_col_idx, R.csr_val, H, Y, 0.1, 4, reg)
        err.append(np.linalg.norm(Y - want))
    assert err[3] < err[0] and all(b <= a * (1 + 1e-12) for a, b in zip(err, err[1:])), err
    W, H = np.zeros((R.rows, k)), H * 0.3
    prev = alsb_ref.objective(R, W, H, 0.1, reg)
    for _ in range(4):
        W, H = alsb_ref.iteration(R, H, W, 0.1, 5, reg)
        cur = alsb_ref.objective(R, W, H, 0.1, reg)
        assert cur <= prev * (1 + 1e-12), (reg, prev, cur)
        prev = cur


# ------------------------------------------------------------------------------------------------ the surface
def test_header_library_and_bindings_agree(mfx):
    import os
    from mfx import _lib as L
    raw = C.CDLL(L.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mfx.h")).read()
    for name, nargs in zip(NEW, (7, 14, 6)):
        assert hasattr(raw, name), name
        assert name in L.SIGNATURES, name
        res, args = L.SIGNATURES[name]
        fn = getattr(mfx.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == list(args) and len(args) == nargs, name
        decl = header[header.index("int " + name + "("):]
        decl = decl[:decl.index(";")]
        assert decl.count(",") + 1 == nargs, (name, decl)
    assert mfx.lib().mfx_version() == L.MFX_VERSION == 2


def test_the_python_surface(mfx):
    init = inspect.signature(mfx.AlsSolver.__init__).parameters
    assert init["block"].default is None and init["count_reg"].default is False
    half = inspect.signature(mfx.als_block_half).parameters
    assert list(half)[:7] == ["ptr", "idx", "val", "X", "k", "lam", "block"]
    assert half["Y_in"].default is None and half["count_reg"].default is False
    setup = inspect.signature(mfx.Recommender.fold_in_block_setup_als).parameters
    assert list(setup) == ["self", "lam", "block", "sweeps", "tol", "count_reg"]
    assert (setup["block"].default, setup["sweeps"].default, setup["tol"].default, setup["count_reg"].default) == (0, 8, 0.0, False)


# ------------------------------------------------------------------------------------------------ mfx_als_block_create
def _create(mfx, R, k=8, lam=0.1, block=0, reg=0, schedule=1, out=True, p_null=False, r_null=False):
    from mfx import _lib as L
    from mfx.api import _coo, _csx
    p = mfx.parameter()
    p.k, p.lambda_ = k, lam
    cp = p.to_c()
    cp.schedule = schedule
    h = C.c_void_p()
    csx, coo = _csx(R), _coo(None)
    rc = mfx.lib().mfx_als_block_create(C.byref(h) if out else None, None if r_null else C.byref(csx), C.byref(coo),
                                        None if p_null else C.byref(cp), block, reg, L.MFX_HOST)
    msg = mfx.lib().mfx_last_error().decode()
    if rc == 0:
        mfx.lib().mfx_als_destroy(h)
    return rc, msg


@pytest.mark.parametrize("kw,word", [({"k": 0}, "rank"), ({"k": 1025}, "rank"), ({"k": 4096}, "rank"),
                                     ({"k": 256, "block": -1}, "block"), ({"k": 256, "block": 129}, "block"),
                                     ({"k": 256, "block": 1024}, "block"), ({"reg": -1}, "reg"), ({"reg": 2}, "reg"),
                                     ({"lam": 0.0}, "lambda"), ({"lam": -0.1}, "lambda"), ({"lam": math.nan}, "lambda"),
                                     ({"lam": math.inf}, "lambda"), ({"schedule": 0}, "schedule")])
def test_create_rejects_bad_arguments_on_the_host(mfx, kw, word):
    rc, msg = _create(mfx, _matrix(7), **kw)
    assert rc == MFX_ERR_INVALID, (kw, rc, msg)  # not MFX_ERR_NO_DEVICE: nothing reached the device
    assert word in msg, (kw, msg)


def test_create_rejects_null_arguments_on_the_host(mfx):
    R = _matrix(7)
    for kw in ({"out": False}, {"p_null": True}, {"r_null": True}):
        rc, msg = _create(mfx, R, **kw)
        assert rc == MFX_ERR_INVALID, (kw, rc, msg)


@pytest.mark.parametrize("k,block,reg", [(129, 0, 0), (256, 64, 1), (1024, 128, 0), (129, 1, 1)])
def test_ranks_above_128_pass_the_argument_checks(mfx, k, block, reg):
    rc, msg = _create(mfx, _matrix(7), k=k, block=block, reg=reg)
    assert rc == (0 if mfx.device_count() >= 1 else MFX_ERR_NO_DEVICE), (rc, msg)


def test_the_python_solver_refuses_on_the_host(mfx):
    R = _matrix(7)
    p = mfx.parameter()
    for k, block, word in ((1025, 0, "rank"), (0, 0, "rank"), (256, 129, "block"), (256, -1, "block")):
        p.k, p.lambda_ = k, 0.1
        with pytest.raises(mfx.MfxError, match=word):
            mfx.AlsSolver(R, None, p, block=block)
    p.k, p.lambda_ = 16, -1.0
    with pytest.raises(mfx.MfxError, match="lambda"):
        mfx.AlsSolver(R, None, p, block=0, count_reg=True)
    p.lambda_ = 0.1
    with pytest.raises(ValueError, match="comm"):
        mfx.AlsSolver(R, None, p, comm=object(), block=0)
    with pytest.raises(ValueError, match="block"):
        mfx.AlsSolver(R, None, p, count_reg=True)


# ------------------------------------------------------------------------------------------------ mfx_als_block_half
def test_half_rejects_bad_arguments_on_the_host(mfx):
    from mfx.api import _f32, _u32
    ptr = np.array([0, 1], np.uint32)
    idx = np.array([0], np.uint32)
    val = np.array([1.0], np.float32)
    X = np.ones((2, 4), np.float32)
    for bad_lam in (0.0, -0.5, math.nan, math.inf):
        with pytest.raises(mfx.MfxError, match="lambda"):
            mfx.als_block_half(ptr, idx, val, X, 4, bad_lam, 2)
    for bad_block in (-1, 129):
        with pytest.raises(mfx.MfxError, match="block"):
            mfx.als_block_half(ptr, idx, val, X, 4, 0.1, bad_block)
    for bad_k in (0, 1025):
        Xk = np.ones((2, max(bad_k, 1)), np.float32)
        with pytest.raises(mfx.MfxError, match="rank"):
            mfx.als_block_half(ptr, idx, val, Xk, bad_k, 0.1, 0)
    lib = mfx.lib()
    Y = np.empty((1, 4), np.float32)
    for bad_reg in (-1, 2):
        assert lib.mfx_als_block_half(1, 1, _u32(ptr), _u32(idx), _f32(val), 2, _f32(X), None, _f32(Y), 4, 2, 0.1, bad_reg, 0) == MFX_ERR_INVALID
        assert "reg" in lib.mfx_last_error().decode()
    for null in ("ptr", "X", "Y", "idx"):
        a = {"ptr": _u32(ptr), "X": _f32(X), "Y": _f32(Y), "idx": _u32(idx)}
        a[null] = None
        assert lib.mfx_als_block_half(1, 1, a["ptr"], a["idx"], _f32(val), 2, a["X"], None, a["Y"], 4, 2, 0.1, 0, 0) == MFX_ERR_INVALID, null
    for k in (129, 256, 1024):  # valid: past the argument checks
        Xk = np.ones((2, k), np.float32)
        Yk = np.empty((1, k), np.float32)
        rc = lib.mfx_als_block_half(1, 1, _u32(ptr), _u32(idx), _f32(val), 2, _f32(Xk), None, _f32(Yk), k, 64, 0.1, 1, 0)
        assert rc == (0 if mfx.device_count() >= 1 else MFX_ERR_NO_DEVICE), (k, rc, lib.mfx_last_error())


# ------------------------------------------------------------------------------------------------ fold-in setup
def test_fold_in_setup_refuses_a_null_handle(mfx):
    lib = mfx.lib()
    assert lib.mfx_rec_fold_in_block_setup_als(None, 0.1, 0, 0, 8, 0.0) == MFX_ERR_INVALID
    assert "null recommender" in lib.mfx_last_error().decode()


def test_the_exact_entry_points_still_stop_at_128(mfx):
    R = _matrix(7)
    p = mfx.parameter()
    p.k, p.lambda_ = 129, 0.1
    with pytest.raises(mfx.MfxError, match="not supported"):
        mfx.AlsSolver(R, None, p)
