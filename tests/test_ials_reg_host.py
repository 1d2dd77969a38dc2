"""CPU tests of implicit ALS with an unobserved weight and a frequency-scaled regulariser: the fp64 reference
(tests/ials_reg_ref.py) against tests/ials_ref.py / ialsb_ref.py and against itself, the C ABI surface, the argument
checks that must fail on the host before any device is touched, and the conditioning gate of tests/test_gpu_ials_reg.py."""
import ctypes as C
import math

import numpy as np
import pytest

import ials_ref
import ials_reg_ref as ref
import ialsb_ref
from solve_sweep import segments

MFX_ERR_INVALID = -1  # include/mfx.h
SIZES = [0, 1, 3, 0, 17, 250, 2048, 2049, 2100, 5000, 1]  # tests/test_gpu_ials.py (a GPU module: not imported here)
PARAMS = [(0.3, 0.5, 0.1), (2.0, 1.0, 0.002), (1.0, 0.25, 0.1)]  # (alpha0, nu, lambda)
LAM32 = float(np.float32(0.1))  # the lambda the C ABI receives for 0.1


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    return m


def _matrix(seed=0, rows=40, cols=30, density=0.2):
    from mfx import dataset as ds
    rng = np.random.default_rng(seed)
    mask = rng.random((rows, cols)) < density
    mask[3, :] = False
    mask[:, 5] = False
    r, c = np.nonzero(mask)
    v = rng.integers(0, 6, r.size).astype(np.float32)  # strengths 0..5: explicit zeros included
    return ds.from_coo(rows, cols, r, c, v)


def test_rho_formula():
    ptr = np.array([0, 3, 3, 5], np.uint32)
    val = np.array([1, 0, 2, 0, 0], np.float32)
    r = ref.rho(ptr, val, 100, 0.1, 0.3, 0.5)
    lam, a0 = float(np.float32(0.1)), float(np.float32(0.3))
    want = [np.float32(lam * math.sqrt(n + a0 * 100)) for n in (2, 0, 0)]
    assert list(r) == [float(w) for w in want]
    assert np.all(ref.rho(ptr, val, 100, 0.1, 0.3, 0.0) == lam)  # nu = 0: lambda exactly
    r1 = ref.rho(ptr, val, 100, 0.1, 1e-12, 1.0)                 # nu = 1, tiny alpha0: fp32(lambda n)
    assert r1[0] == float(np.float32(lam * (2 + float(np.float32(1e-12)) * 100)))
    assert abs(r1[0] - float(np.float32(0.1) * np.float32(2))) <= 1e-7


def test_reduces_to_the_plain_references_at_alpha0_1_nu_0():
    R = _matrix(1)
    rng = np.random.default_rng(2)
    H = rng.standard_normal((R.cols, 6))
    W0 = rng.standard_normal((R.rows, 6)) * 0.1
    for alpha in (0.0, 1.0, 40.0):
        for s in range(R.rows):
            A, b = ref.dense_system(R.csr_row_ptr, R.csr_col_idx, R.csr_val, s, H, LAM32, alpha, 1.0, 0.0)
            A2, b2 = ials_ref.dense_system(R.csr_row_ptr, R.csr_col_idx, R.csr_val, s, H, LAM32, alpha)
            np.testing.assert_allclose(A, A2, rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(b, b2, rtol=1e-12, atol=1e-12)
        Y = ref.half(R.csr_row_ptr, R.csr_col_idx, R.csr_val, H, LAM32, alpha, 1.0, 0.0)
        np.testing.assert_allclose(Y, ials_ref.half(R.csr_row_ptr, R.csr_col_idx, R.csr_val, H, LAM32, alpha), rtol=1e-12, atol=1e-12)
        for d in (2, 4, 6):
            B = ref.block_sweep(R.csr_row_ptr, R.csr_col_idx, R.csr_val, H, W0, LAM32, alpha, 1.0, 0.0, d)
            B2 = ialsb_ref.block_sweep(R.csr_row_ptr, R.csr_col_idx, R.csr_val, H, W0, LAM32, alpha, d)
            np.testing.assert_allclose(B, B2, rtol=1e-12, atol=1e-12)
        Wn, Hn = ref.iteration(R, H, LAM32, alpha, 1.0, 0.0)
        Wp, Hp = ials_ref.iteration(R, H, LAM32, alpha)
        np.testing.assert_allclose(Wn, Wp, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(Hn, Hp, rtol=1e-12, atol=1e-12)
        for f in (ref.dense_loss, ref.shortcut_loss):
            got, want = f(R, Wn, Hn, LAM32, alpha, 1.0, 0.0), ials_ref.dense_loss(R, Wp, Hp, LAM32, alpha)
            assert abs(got - want) <= 1e-12 * abs(want), (f.__name__, got, want)


@pytest.mark.parametrize("alpha0,nu,lam", PARAMS + [(0.3, 0.0, 0.1)])
def test_loss_formula_equals_dense_loss(alpha0, nu, lam):
    R = _matrix(3)
    rng = np.random.default_rng(4)
    W = rng.standard_normal((R.rows, 5)) * 0.3
    H = rng.standard_normal((R.cols, 5)) * 0.3
    for alpha in (0.0, 2.5, 40.0):
        d = ref.dense_loss(R, W, H, lam, alpha, alpha0, nu)
        s = ref.shortcut_loss(R, W, H, lam, alpha, alpha0, nu)
        assert abs(d - s) <= 1e-10 * abs(d), (d, s)


@pytest.mark.parametrize("alpha0,nu,lam", PARAMS)
def test_half_zeroes_the_gradient_of_the_dense_loss(alpha0, nu, lam):
    """W = half(H) minimises dense_loss over W: a central difference of the loss along random directions vanishes, and
    the loss does not fall for any perturbed W.  The same for the H-half."""
    R = _matrix(5)
    rng = np.random.default_rng(6)
    k, alpha = 4, 3.0
    H = rng.standard_normal((R.cols, k)) * 0.3
    W = ref.half(R.csr_row_ptr, R.csr_col_idx, R.csr_val, H, lam, alpha, alpha0, nu)
    assert not np.any(W[3])  # the empty user
    base = ref.dense_loss(R, W, H, lam, alpha, alpha0, nu)
    for _ in range(5):
        D = rng.standard_normal(W.shape)
        D[3] = 0
        eps = 1e-4
        up = ref.dense_loss(R, W + eps * D, H, lam, alpha, alpha0, nu)
        dn = ref.dense_loss(R, W - eps * D, H, lam, alpha, alpha0, nu)
        curv = (up + dn - 2 * base) / eps ** 2  # the loss is quadratic in W: (up - dn) / 2 eps is the exact slope
        assert abs(up - dn) / (2 * eps) <= 1e-7 * max(curv, 1.0), (up, dn, base)
        assert up >= base and dn >= base
    Hn = ref.half(R.csc_col_ptr, R.csc_row_idx, R.csc_val, W, lam, alpha, alpha0, nu)
    base = ref.dense_loss(R, W, Hn, lam, alpha, alpha0, nu)
    for _ in range(5):
        D = rng.standard_normal(Hn.shape)
        D[5] = 0
        up = ref.dense_loss(R, W, Hn + 1e-4 * D, lam, alpha, alpha0, nu)
        dn = ref.dense_loss(R, W, Hn - 1e-4 * D, lam, alpha, alpha0, nu)
        curv = (up + dn - 2 * base) / 1e-8
        assert abs(up - dn) / 2e-4 <= 1e-7 * max(curv, 1.0)
        assert up >= base and dn >= base


@pytest.mark.parametrize("alpha0,nu,lam", PARAMS)
def test_block_sweep_never_increases_the_segment_objective(alpha0, nu, lam):
    R = _matrix(7)
    rng = np.random.default_rng(8)
    k = 7
    H = rng.standard_normal((R.cols, k)) * 0.4
    args = (R.csr_row_ptr, R.csr_col_idx, R.csr_val)
    for alpha in (0.0, 1.0, 40.0):
        exact = ref.half(*args, H, lam, alpha, alpha0, nu)
        for d in (1, 3, 7, 128):
            Y = rng.standard_normal((R.rows, k)) * 0.2
            prev = [ref.segment_objective(*args, s, H, Y[s] * (R.csr_row_ptr[s + 1] > R.csr_row_ptr[s]), lam, alpha, alpha0, nu)
                    for s in range(R.rows)]
            for sweep in range(4):
                Y = ref.block_sweep(*args, H, Y, lam, alpha, alpha0, nu, d)
                cur = [ref.segment_objective(*args, s, H, Y[s], lam, alpha, alpha0, nu) for s in range(R.rows)]
                for s in range(R.rows):
                    assert cur[s] <= prev[s] + 1e-10 * abs(prev[s]), (alpha, d, sweep, s, prev[s], cur[s])
                prev = cur
            if d >= k:  # a single block is the solve
                np.testing.assert_allclose(Y, exact, rtol=1e-9, atol=1e-11)


def test_reference_iteration_never_increases_the_loss():
    R = _matrix(9)
    for alpha0, nu, lam in PARAMS:
        for d in (None, 2):
            H = np.random.default_rng(10).standard_normal((R.cols, 4)) * 0.1
            W = np.zeros((R.rows, 4))
            prev = ref.dense_loss(R, W, H, lam, 10.0, alpha0, nu)
            for _ in range(4):
                W, H = ref.iteration(R, H, lam, 10.0, alpha0, nu, W=W, d=d)
                cur = ref.dense_loss(R, W, H, lam, 10.0, alpha0, nu)
                assert cur <= prev * (1 + 1e-12)
                prev = cur


# ------------------------------------------------------------------------------------------------ the C ABI surface
NEW = ("mfx_ials_create_reg", "mfx_ials_block_create_reg", "mfx_ials_half_reg", "mfx_ials_block_half_reg",
       "mfx_rec_fold_in_setup_reg", "mfx_rec_fold_in_block_setup_reg")


def test_new_symbols_are_exported_and_bound(mfx):
    from mfx import _lib as L
    lib = mfx.lib()
    for name in NEW:
        assert name in L.SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.mfx_version() == L.MFX_VERSION == 2


def test_header_declares_the_new_entry_points():
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mfx.h")) as f:
        h = f.read()
    for name in NEW:
        assert f"int {name}(" in h, name
    assert "#define MFX_VERSION 2" in h


def _create(mfx, R, block=None, k=8, alpha=1.0, alpha0=1.0, nu=0.0, lam=0.1, schedule=1, out=True, p_null=False, r_null=False):
    from mfx import _lib as L
    from mfx.api import _csx
    p = mfx.parameter()
    p.k, p.lambda_ = k, lam
    cp = p.to_c()
    cp.schedule = schedule
    h = C.c_void_p()
    csx = _csx(R)
    o, r, pp = (C.byref(h) if out else None), (None if r_null else C.byref(csx)), (None if p_null else C.byref(cp))
    if block is None:
        rc = mfx.lib().mfx_ials_create_reg(o, r, pp, alpha, alpha0, nu, L.MFX_HOST)
    else:
        rc = mfx.lib().mfx_ials_block_create_reg(o, r, pp, alpha, alpha0, nu, block, L.MFX_HOST)
    return rc, mfx.lib().mfx_last_error().decode()


BLOCKS = [None, 0, 4]


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("alpha0", [0.0, -0.0, -1.0, -1e-30, math.nan, math.inf, -math.inf])
def test_create_rejects_bad_alpha0_on_the_host(mfx, block, alpha0):
    rc, msg = _create(mfx, _matrix(7), block=block, alpha0=alpha0)
    assert rc == MFX_ERR_INVALID, (rc, msg)  # not MFX_ERR_NO_DEVICE: nothing reached the device
    assert "alpha0" in msg


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("nu", [-0.01, 1.01, 2.0, math.nan, math.inf, -math.inf])
def test_create_rejects_bad_nu_on_the_host(mfx, block, nu):
    rc, msg = _create(mfx, _matrix(7), block=block, nu=nu)
    assert rc == MFX_ERR_INVALID, (rc, msg)
    assert "nu =" in msg


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("lam,alpha0,nu", [(3e38, 1.0, 1.0), (1e30, 1e30, 0.5), (math.inf, 1.0, 0.0), (math.nan, 1.0, 0.5)])
def test_create_rejects_an_overflowing_regulariser_on_the_host(mfx, block, lam, alpha0, nu):
    rc, msg = _create(mfx, _matrix(7), block=block, lam=lam, alpha0=alpha0, nu=nu)
    assert rc == MFX_ERR_INVALID, (rc, msg)
    assert "regulariser" in msg


@pytest.mark.parametrize("block", BLOCKS)
def test_create_still_rejects_what_the_plain_entry_points_reject(mfx, block):
    R = _matrix(7)
    for alpha in (-1.0, math.nan, math.inf):
        rc, msg = _create(mfx, R, block=block, alpha=alpha)
        assert rc == MFX_ERR_INVALID and "alpha" in msg and "alpha0" not in msg, (rc, msg)
    for k in ((0, 129) if block is None else (0, 1025)):
        rc, msg = _create(mfx, R, block=block, k=k)
        assert rc == MFX_ERR_INVALID and "rank" in msg, (rc, msg)
    rc, msg = _create(mfx, R, block=block, schedule=0)
    assert rc == MFX_ERR_INVALID and "schedule" in msg, (rc, msg)
    for kw in ({"out": False}, {"p_null": True}, {"r_null": True}):
        rc, msg = _create(mfx, R, block=block, **kw)
        assert rc == MFX_ERR_INVALID, (kw, rc, msg)
    if block is not None:
        for b in (-1, 129):
            rc, msg = _create(mfx, R, block=b)
            assert rc == MFX_ERR_INVALID and "block" in msg, (rc, msg)


def test_half_operators_reject_bad_arguments_on_the_host(mfx):
    ptr = np.array([0, 1], np.uint32)
    idx = np.array([0], np.uint32)
    val = np.array([1.0], np.float32)
    X = np.ones((2, 4), np.float32)
    calls = (lambda **kw: mfx.ials_half(ptr, idx, val, X, 4, kw.pop("lam", 0.1), kw.pop("alpha", 1.0), **kw),
             lambda **kw: mfx.ials_block_half(ptr, idx, val, X, 4, kw.pop("lam", 0.1), kw.pop("alpha", 1.0), 2, **kw))
    for call in calls:
        for a0 in (0.0, -1.0, math.nan, math.inf):
            with pytest.raises(mfx.MfxError, match="alpha0"):
                call(alpha0=a0, nu=0.5)
            with pytest.raises(mfx.MfxError, match="alpha0"):
                call(alpha0=a0)  # a lone alpha0 means nu = 0: still the _reg entry point
        for nu in (-0.5, 1.5, math.nan):
            with pytest.raises(mfx.MfxError, match="nu"):
                call(alpha0=1.0, nu=nu)
            with pytest.raises(mfx.MfxError, match="nu"):
                call(nu=nu)  # a lone nu means alpha0 = 1
        with pytest.raises(mfx.MfxError, match="regulariser"):
            call(lam=3e38, alpha0=1.0, nu=1.0)
        for bad_alpha in (-0.5, math.nan, math.inf):
            with pytest.raises(mfx.MfxError, match="alpha"):
                call(alpha=bad_alpha, alpha0=1.0, nu=0.0)
    for bad_k in (0, 129):
        with pytest.raises(mfx.MfxError, match="rank"):
            mfx.ials_half(ptr, idx, val, np.ones((2, max(bad_k, 1)), np.float32), bad_k, 0.1, 1.0, alpha0=1.0, nu=0.0)
    with pytest.raises(mfx.MfxError, match="rank"):
        mfx.ials_block_half(ptr, idx, val, np.ones((2, 1025), np.float32), 1025, 0.1, 1.0, 64, alpha0=1.0, nu=0.0)
    with pytest.raises(mfx.MfxError, match="block"):
        mfx.ials_block_half(ptr, idx, val, X, 4, 0.1, 1.0, 129, alpha0=1.0, nu=0.0)


def test_fold_in_setups_reject_a_null_handle(mfx):
    lib = mfx.lib()
    assert lib.mfx_rec_fold_in_setup_reg(None, 0.1, 1.0, 1.0, 0.0) == MFX_ERR_INVALID
    assert lib.mfx_rec_fold_in_block_setup_reg(None, 0.1, 1.0, 1.0, 0.0, 0, 4, 0.0) == MFX_ERR_INVALID


# ------------------------------------------------------------------------------------------------ the conditioning gate
def _conds(k, params):
    """Largest condition number of the systems tests/test_gpu_ials_reg.py gates on, at rank k: the segments of
    segments(100 + k, 6000, SIZES), X ~ N(0, 1/k) seeded by k, alpha in {0, 1, 40}.  A is formed as alpha0 X^T X + rho I +
    sum_j w_j x_j x_j^T (equal to the dense form: test_reduces_to... and test_shortcut_equals_dense_form below)."""
    nrows_x = 6000
    ptr, idx, val = segments(100 + k, nrows_x, SIZES)
    X = (np.random.default_rng(k).standard_normal((nrows_x, k)) / np.sqrt(k)).astype(np.float32).astype(np.float64)
    S = X.T @ X
    worst = 0.0
    for alpha0, nu, lam in params:
        rh = ref.rho(ptr, val, nrows_x, lam, alpha0, nu)
        for s, n in enumerate(SIZES):
            if n == 0:
                continue
            lo, hi = int(ptr[s]), int(ptr[s + 1])
            Xj = X[idx[lo:hi].astype(np.int64)]
            for alpha in (0.0, 1.0, 40.0):
                w = ials_ref.weights(val[lo:hi], alpha)
                A = float(np.float32(alpha0)) * S + rh[s] * np.eye(k) + (Xj * w[:, None]).T @ Xj
                ev = np.linalg.eigvalsh(A)
                worst = max(worst, float(ev[-1] / ev[0]) if ev[0] > 0 else float("inf"))
    return worst


def test_shortcut_equals_dense_form():
    ptr, idx, val = segments(105, 300, [0, 1, 7, 40])
    X = np.random.default_rng(5).standard_normal((300, 5))
    S = X.T @ X
    for alpha0, nu, lam in PARAMS:
        rh = ref.rho(ptr, val, 300, lam, alpha0, nu)
        for s in (1, 2, 3):
            lo, hi = int(ptr[s]), int(ptr[s + 1])
            Xj = X[idx[lo:hi].astype(np.int64)]
            w = ials_ref.weights(val[lo:hi], 3.0)
            A = float(np.float32(alpha0)) * S + rh[s] * np.eye(5) + (Xj * w[:, None]).T @ Xj
            Ad, _ = ref.dense_system(ptr, idx, val, s, X, lam, 3.0, alpha0, nu)
            np.testing.assert_allclose(A, Ad, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("lo,hi", [(1, 33), (33, 65), (65, 97), (97, 129)])
def test_conditioning_gate_skips_no_segment_up_to_rank_128(lo, hi):
    worst = max(_conds(k, PARAMS) for k in range(lo, hi))
    print(f"ialsr-host largest condition number, k = {lo}..{hi - 1}: {worst:.1f}")
    assert worst <= 1e3, worst


@pytest.mark.parametrize("k", [160, 256, 1024])
def test_conditioning_gate_skips_no_segment_above_rank_128(k):
    worst = _conds(k, PARAMS)
    plain = _conds(k, [(1.0, 0.0, 0.1)])  # the objective of mfx_ials_block_create: what tests/test_gpu_ialsb.py quotes
    print(f"ialsr-host largest condition number, k = {k}: {worst:.1f} (alpha0 = 1, nu = 0: {plain:.1f})")
    assert worst <= 1e3 and plain <= 1e3, (worst, plain)
    assert abs(plain - {160: 18.7, 256: 29.1, 1024: 144.1}[k]) <= 0.06, plain
