"""GPU tests of implicit-feedback ALS (mfx_ials_create / mfx_ials_loss / mfx_ials_half) against the dense fp64
reference of tests/ials_ref.py.

Tolerances: every system is checked by its normwise backward error in fp64 against the DENSE system (fp32 Gramians
over up to 6 000 rows and an fp32 Cholesky: a few 1e-6; bound 3e-5), and by its relative error where the condition
number is at most 1e3 (bound 1e-3)."""
import ctypes as C

import numpy as np
import pytest

import ials_ref
from solve_sweep import segments as _segments  # (test_gpu_alsb.py and test_gpu_ialsb.py import it from here)

pytestmark = pytest.mark.gpu

MFX_ERR_INVALID = -1  # include/mfx.h


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1
    return m


SIZES = [0, 1, 3, 0, 17, 250, 2048, 2049, 2100, 5000, 1]  # 0, 1, 2 and 3 chunks of 2048 entries


@pytest.mark.parametrize("k", [1, 5, 16, 32, 36, 60, 64, 68, 100, 128])
def test_ials_half_against_dense_reference(mfx, k):
    nrows_x = 6000
    ptr, idx, val = _segments(100 + k, nrows_x, SIZES)
    X = (np.random.default_rng(k).standard_normal((nrows_x, k)) / np.sqrt(k)).astype(np.float32)
    lam = 0.1
    for alpha in (0.0, 1.0, 40.0):
        Y = mfx.ials_half(ptr, idx, val, X, k, lam, alpha)
        for s, n in enumerate(SIZES):
            if n == 0:
                assert not np.any(Y[s]), (k, alpha, s)  # b = 0: exactly zero
                continue
            A, b = ials_ref.dense_system(ptr, idx, val, s, X, lam, alpha)
            be = ials_ref.backward_error(A, Y[s], b)
            assert be <= 3e-5, (k, alpha, s, n, be)
            if np.linalg.cond(A) <= 1e3:
                y = np.linalg.solve(A, b)
                rel = np.linalg.norm(Y[s] - y) / max(np.linalg.norm(y), 1e-30)
                assert rel <= 1e-3, (k, alpha, s, n, rel)


def _random_matrix(seed, rows=300, cols=200, density=0.06):
    from mfx import dataset as ds
    rng = np.random.default_rng(seed)
    mask = rng.random((rows, cols)) < density
    mask[7, :] = False  # an empty user
    mask[:, 11] = False  # an empty item
    r, c = np.nonzero(mask)
    v = rng.integers(0, 6, r.size).astype(np.float32)
    return ds.from_coo(rows, cols, r, c, v)


def _params(mfx, k, lam):
    p = mfx.parameter()
    p.k, p.lambda_ = k, lam
    return p


def test_one_iteration_matches_fp64_reference(mfx):
    R = _random_matrix(1)
    k, lam, alpha = 16, 0.1, 5.0
    H0 = (np.random.default_rng(2).standard_normal((R.cols, k)) * 0.1).astype(np.float32)
    s = mfx.ImplicitAlsSolver(R, _params(mfx, k, lam), alpha)
    s.set_factors(H0)
    rep = s.iterate(1)
    assert rep[0].update_time > 0 and rep[0].rmse == 0
    W, H = s.get_factors()
    kt = s.kernel_times()
    s.close()
    Wr, Hr = ials_ref.iteration(R, H0.astype(np.float64), lam, alpha)
    assert np.max(np.abs(W - Wr)) <= 1e-3 * np.max(np.abs(Wr))
    assert np.max(np.abs(H - Hr)) <= 1e-3 * np.max(np.abs(Hr))
    assert not np.any(W[7]) and not np.any(H[11])
    assert set(kt) == {"ials_half_rows(W over H)", "ials_half_cols(H over W)", "ials_base_gram(H)", "ials_base_gram(W)"}


def test_loss_matches_dense_loss_and_decreases(mfx):
    R = _random_matrix(3)
    k, lam, alpha = 8, 0.05, 10.0
    H0 = (np.random.default_rng(4).standard_normal((R.cols, k)) * 0.1).astype(np.float32)
    s = mfx.ImplicitAlsSolver(R, _params(mfx, k, lam), alpha)
    s.set_factors(H0)
    prev = None
    for it in range(8):
        s.iterate(1)
        got = s.loss()
        W, H = s.get_factors()
        want = ials_ref.dense_loss(R, W, H, lam, alpha)
        assert abs(got - want) <= 1e-6 * abs(want), (it, got, want)
        if prev is not None:
            assert got <= prev * (1 + 1e-6), (it, prev, got)
        prev = got
    s.close()


def _device_arrays(R):
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a)).to(dev)
    return {"rows": R.rows, "cols": R.cols, "csr_row_ptr": t(R.csr_row_ptr), "csr_col_idx": t(R.csr_col_idx),
            "csr_val": t(R.csr_val), "csc_col_ptr": t(R.csc_col_ptr), "csc_row_idx": t(R.csc_row_idx), "csc_val": t(R.csc_val)}


def _train(mfx, R, k, lam, alpha, H0, n, device_arrays=None):
    s = mfx.ImplicitAlsSolver(R if device_arrays is None else None, _params(mfx, k, lam), alpha, device_arrays=device_arrays)
    s.set_factors(H0)
    s.iterate(n)
    W, H = s.get_factors()
    s.close()
    return W, H


def _explicit(mfx, R, k, lam, H0, n):
    s = mfx.AlsSolver(R, None, _params(mfx, k, lam))
    s.set_factors(H0)
    s.iterate(n, with_rmse=False)
    W, H = s.get_factors()
    s.close()
    return W, H


def test_determinism_across_handles_memspaces_and_explicit_als(mfx):
    import torch  # noqa: F401  (device-resident inputs)
    R = _random_matrix(5, rows=2500, cols=400, density=0.03)
    R.csr_val[:5] = 0.0  # explicit zeros in both orientations
    from mfx import dataset as ds
    r = np.repeat(np.arange(R.rows), np.diff(R.csr_row_ptr.astype(np.int64)))
    R = ds.from_coo(R.rows, R.cols, r, R.csr_col_idx, R.csr_val)
    for k in (32, 64):
        H0 = (np.random.default_rng(k).standard_normal((R.cols, k)) * 0.1).astype(np.float32)
        E1 = _explicit(mfx, R, k, 0.1, H0, 2)
        a = _train(mfx, R, k, 0.1, 2.0, H0, 3)
        b = _train(mfx, R, k, 0.1, 2.0, H0, 3)
        c = _train(mfx, R, k, 0.1, 2.0, H0, 3, device_arrays=_device_arrays(R))
        E2 = _explicit(mfx, R, k, 0.1, H0, 2)
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        for x, y in zip(a, c):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        for x, y in zip(E1, E2):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf")])
def test_bad_strengths_rejected_at_create(mfx, bad):
    R = _random_matrix(7, rows=50, cols=40, density=0.2)
    from mfx import dataset as ds
    r = np.repeat(np.arange(R.rows), np.diff(R.csr_row_ptr.astype(np.int64)))
    v = R.csr_val.copy()
    v[len(v) // 2] = bad
    Rb = ds.from_coo(R.rows, R.cols, r, R.csr_col_idx, v)
    with pytest.raises(mfx.MfxError, match="implicit ALS"):
        mfx.ImplicitAlsSolver(Rb, _params(mfx, 8, 0.1), 1.0)
    # alpha * r overflowing fp32 is rejected too
    with pytest.raises(mfx.MfxError, match="implicit ALS"):
        mfx.ImplicitAlsSolver(ds.from_coo(R.rows, R.cols, r, R.csr_col_idx, R.csr_val * np.float32(1e37)), _params(mfx, 8, 0.1), 100.0)


def test_loss_on_explicit_handle_is_invalid(mfx):
    R = _random_matrix(8, rows=50, cols=40, density=0.2)
    s = mfx.AlsSolver(R, None, _params(mfx, 8, 0.1))
    s.set_factors(np.zeros((R.cols, 8), np.float32))
    out = C.c_double(0.0)
    assert mfx.lib().mfx_ials_loss(s.handle, C.byref(out)) == MFX_ERR_INVALID
    s.close()


def test_planted_clusters_recommend_end_to_end(mfx):
    """20 clusters of 30 items, 2 000 users: 25 training items of the user's own cluster plus 2 random ones, one more
    in-cluster item held out.  Trained for 10 iterations at k = 32, the top-10 lists (training items excluded) must
    find the held-out item for at least 90 % of the users (random lists: about 1.7 %)."""
    from mfx import dataset as ds
    rng = np.random.default_rng(11)
    nc, per, users = 20, 30, 2000
    items = nc * per
    tr_r, tr_c, te_r, te_c = [], [], [], []
    for u in range(users):
        cl = u % nc
        own = cl * per + rng.permutation(per)[:26]
        others = np.setdiff1d(np.arange(items), cl * per + np.arange(per))
        extra = rng.choice(others, 2, replace=False)
        tr = np.concatenate([own[:25], extra])
        tr_r += [u] * tr.size
        tr_c += list(tr)
        te_r.append(u)
        te_c.append(own[25])
    R = ds.from_coo(users, items, np.array(tr_r), np.array(tr_c), np.ones(len(tr_r), np.float32),
                    np.array(te_r), np.array(te_c), np.ones(len(te_r), np.float32))
    k = 32
    H0 = (rng.standard_normal((items, k)) * 0.1).astype(np.float32)
    W, H = _train(mfx, R, k, 0.1, 40.0, H0, 10)
    top, _ = mfx.recommend(W, H, 1, 10, exclude=R)
    m = mfx.topn_metrics(top, mfx.test_data_of(R))
    assert m["users"] == users
    assert m["hr"] >= 0.9, m
