"""CPU tests of implicit ALS by preconditioned conjugate gradients: the fp64 reference (tests/ials_cg_ref.py) against the dense
reference of the exact method, the C ABI surface, and the argument checks that must fail on the host, before any device is
touched.

The reference alone, one iteration at k = 160 against ials_ref.iteration (largest-entry relative; the bound is 1e-3):
    steps = 64, tol = 1e-5, both halves cold: W 1.5e-05, H 7.4e-05, at most 13 steps
    steps = 64, tol = 1e-4, both halves cold: W 1.5e-04, H 6.8e-04, at most 11 steps
(the H-half warm from H0, as the trainer runs it, is printed by the test)."""
import ctypes as C
import math

import numpy as np
import pytest

import ials_cg_ref
import ials_ref
from test_gpu_ials import _random_matrix

MFX_ERR_INVALID, MFX_ERR_NO_DEVICE = -1, -2  # include/mfx.h


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    return m


def _rel(A, B):
    return float(np.max(np.abs(A - B)) / np.max(np.abs(B)))


def test_reference_iteration_is_within_the_bound_of_the_exact_iteration():
    R = _random_matrix(1)
    k, lam, alpha, steps, tol = 160, 0.1, 5.0, 64, 1e-5
    H0 = (np.random.default_rng(2).standard_normal((R.cols, k)) * 0.1).astype(np.float32).astype(np.float64)
    Wr, Hr = ials_ref.iteration(R, H0, lam, alpha)
    W, H, (cw, ch) = ials_cg_ref.iteration(R, H0, None, lam, alpha, steps, tol)
    print(f"ialscg-reference iteration k={k} tol={tol:g} cold W, warm H: W={_rel(W, Wr):.3e} H={_rel(H, Hr):.3e} "
          f"max_steps={int(cw.max())}/{int(ch.max())}")
    assert _rel(W, Wr) <= 1e-3 and _rel(H, Hr) <= 1e-3
    assert not np.any(W[7]) and not np.any(H[11])
    assert cw[7] == 0 and ch[11] == 0
    W0 = np.random.default_rng(3).standard_normal((R.rows, k)) * 0.1  # the warm start of test_gpu_ialsb.py
    W2, H2, (cw2, ch2) = ials_cg_ref.iteration(R, H0, W0, lam, alpha, steps, tol)
    print(f"ialscg-reference iteration k={k} tol={tol:g} warm W, warm H: W={_rel(W2, Wr):.3e} H={_rel(H2, Hr):.3e} "
          f"max_steps={int(cw2.max())}/{int(ch2.max())}")
    assert _rel(W2, Wr) <= 1e-3 and _rel(H2, Hr) <= 1e-3
    assert not np.any(W2[7]) and not np.any(H2[11])  # a row without entries is zero whatever the start held


def test_reference_never_increases_the_loss_with_two_steps_per_half():
    R = _random_matrix(3)
    k, lam, alpha = 16, 0.05, 10.0
    H = (np.random.default_rng(4).standard_normal((R.cols, k)) * 0.1).astype(np.float32).astype(np.float64)
    W = None
    prev = ials_ref.dense_loss(R, np.zeros((R.rows, k)), H, lam, alpha)
    for it in range(8):
        W, H, _ = ials_cg_ref.iteration(R, H, W, lam, alpha, 2, 0.0)
        cur = ials_ref.dense_loss(R, W, H, lam, alpha)
        assert cur <= prev * (1 + 1e-12), (it, prev, cur)
        prev = cur


def test_new_symbols_are_exported_and_bound(mfx):
    from mfx import _lib as L
    lib = mfx.lib()
    for name in ("mfx_ials_cg_create", "mfx_ials_cg_stats", "mfx_ials_cg_half", "mfx_spd_inverse"):
        assert name in L.SIGNATURES
        assert hasattr(lib, name)
    assert lib.mfx_version() == L.MFX_VERSION == 2
    assert hasattr(mfx, "ials_cg_half") and hasattr(mfx, "spd_inverse")
    assert hasattr(mfx.ImplicitAlsSolver, "cg_stats")
    import inspect
    assert "cg" in inspect.signature(mfx.ImplicitAlsSolver.__init__).parameters


def _create(mfx, R, k=8, alpha=1.0, steps=3, tol=1e-4):
    from mfx import _lib as L
    from mfx.api import _csx
    p = mfx.parameter()
    p.k = k
    cp = p.to_c()
    h = C.c_void_p()
    csx = _csx(R)
    rc = mfx.lib().mfx_ials_cg_create(C.byref(h), C.byref(csx), C.byref(cp), alpha, steps, tol, L.MFX_HOST)
    msg = mfx.lib().mfx_last_error().decode()
    if rc == 0:
        mfx.lib().mfx_als_destroy(h)
    return rc, msg


@pytest.mark.parametrize("kw,word", [({"k": 0}, "rank"), ({"k": 1025}, "rank"), ({"steps": 0}, "steps"), ({"tol": -1e-6}, "tol"),
                                     ({"tol": math.nan}, "tol")])
def test_create_rejects_bad_arguments_on_the_host(mfx, kw, word):
    rc, msg = _create(mfx, _random_matrix(7, rows=40, cols=30, density=0.2), **kw)
    assert rc == MFX_ERR_INVALID, (rc, msg)  # not MFX_ERR_NO_DEVICE: nothing reached the device
    assert word in msg


@pytest.mark.parametrize("k", [129, 1024])
def test_ranks_above_128_pass_the_argument_checks(mfx, k):
    rc, msg = _create(mfx, _random_matrix(7, rows=40, cols=30, density=0.2), k=k)
    assert rc == (0 if mfx.device_count() >= 1 else MFX_ERR_NO_DEVICE), (rc, msg)


@pytest.mark.parametrize("k", [0, 1025])
def test_spd_inverse_rejects_bad_sizes_on_the_host(mfx, k):
    from mfx.api import _f32
    A = np.eye(max(k, 1), dtype=np.float32)
    out = np.empty_like(A)
    rc = mfx.lib().mfx_spd_inverse(k, _f32(A), _f32(out), 0)
    assert rc == MFX_ERR_INVALID, (rc, mfx.lib().mfx_last_error())
    assert "k" in mfx.lib().mfx_last_error().decode()


def test_cg_excludes_the_other_methods(mfx):
    R = _random_matrix(7, rows=40, cols=30, density=0.2)
    p = mfx.parameter()
    p.k = 8
    for kw in ({"block": 0}, {"block": 64}, {"alpha0": 0.5}, {"nu": 0.5}):
        with pytest.raises(ValueError, match="cg="):
            mfx.ImplicitAlsSolver(R, p, 1.0, cg=(3, 1e-4), **kw)
