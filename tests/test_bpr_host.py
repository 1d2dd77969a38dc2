"""BPR training without a GPU: the host sampler (mfx_bpr_triples) against the Python-integer sampler of tests/bpr_exact.py,
the self-checks of that exact reference, the condition the GPU end-to-end test relies on (the reference learns the planted
clusters), and the argument refusals that never reach the device."""
import ctypes as C

import numpy as np
import pytest

import bpr_exact as bx
from rec_exact import fmaf32

MFX_ERR_INVALID = -1  # include/mfx.h
F = np.float32


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    return m


@pytest.fixture(autouse=True)
def _library_has_bpr(mfx):
    """tests/bpr_exact.py restates the contract of the library's BPR entry points: without them its self-checks have no subject."""
    assert all(hasattr(mfx.lib(), name) for name in ("mfx_bpr_create", "mfx_bpr_triples", "mfx_bpr_apply"))


@pytest.fixture(scope="module")
def R():
    return bx.small_matrix()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the sampler
SEEDS = [0, 1, 12345, (1 << 63) + 5, (1 << 64) - 1]
RANGES = [(0, 300), (12345, 200), ((1 << 32) - 100, 200), (1 << 40, 50), ((1 << 62) - 7, 20)]


@pytest.mark.parametrize("seed", SEEDS)
def test_triples_equal_the_python_sampler(mfx, R, seed):
    assert R.rows == 60 and R.cols == 40 and R.nnz == 503
    for first, count in RANGES:
        got = mfx.bpr_triples(R, seed, first, count)
        for want in (bx.triples(R, seed, first, count), bx.triples_np(R, seed, first, count)):
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and np.array_equal(g, w), (seed, first)
    u, i, j, s = mfx.bpr_triples(R, seed, 5, 0)
    assert u.size == i.size == j.size == s.size == 0


def test_slots_are_a_function_of_seed_and_number_alone(mfx, R):
    a = mfx.bpr_triples(R, 9, 100, 400)
    b = mfx.bpr_triples(R, 9, 300, 200)
    for x, y in zip(a, b):
        assert np.array_equal(x[200:], y)
    c = mfx.bpr_triples(R, 10, 100, 400)
    assert not np.array_equal(a[2], c[2]) and not np.array_equal(a[1], c[1])


def test_every_entry_and_item_is_drawn_as_often_as_expected(mfx, R):
    """10^5 slots: an entry is drawn with p = 1 / nnz, an item with p = 1 / cols; every count must lie within five standard
    deviations sqrt(N p (1 - p)) of N p (503 + 40 counts: a fair sampler fails this once in about 3 000 000 seeds)."""
    n = 100_000
    u, i, j, s = mfx.bpr_triples(R, 2024, 0, n)
    ptr = R.csr_row_ptr.astype(np.int64)
    key = np.repeat(np.arange(R.rows), np.diff(ptr)) * R.cols + R.csr_col_idx
    assert np.all(np.diff(key) > 0)
    entry = np.searchsorted(key, u.astype(np.int64) * R.cols + i)
    assert np.array_equal(key[entry], u.astype(np.int64) * R.cols + i)  # (u, i) is a stored entry
    for counts, p in ((np.bincount(entry, minlength=R.nnz), 1.0 / R.nnz), (np.bincount(j, minlength=R.cols), 1.0 / R.cols)):
        sd = np.sqrt(n * p * (1 - p))
        assert np.all(np.abs(counts - n * p) <= 5 * sd), (counts.min(), counts.max(), n * p, sd)
    member = np.zeros((R.rows, R.cols), bool)
    member[np.repeat(np.arange(R.rows), np.diff(ptr)), R.csr_col_idx] = True
    assert np.array_equal(s, member[u, j])
    assert 0 < s.sum() < n


# ------------------------------------------------------------------------------------------------ the reference itself
def _sgd_textbook(W, H, u, i, j, skipped, lr, lam):
    """Classical BPR-SGD, one triple after the other, written on scalars: x = <w_u, h_i - h_j>, g = 1 / (1 + e^x),
    w_u += lr (g (h_i - h_j) - lam w_u), h_i += lr (g w_u - lam h_i), h_j += lr (-g w_u - lam h_j), all from the values of
    before the triple.  The two things the contract adds to the textbook are written out: a gradient term is cut to a
    multiple of 2^-36 (q), and a row that a triple touches twice (i == j) sees lam twice."""
    W, H = W.copy(), H.copy()
    lr, lam = F(lr), F(lam)
    q = lambda t: F(np.trunc(np.float64(t) * 2.0 ** 36) * 2.0 ** -36)
    for t in range(len(u)):
        if skipped[t]:
            continue
        wu, hi, hj = W[u[t]].copy(), H[i[t]].copy(), H[j[t]].copy()
        d = hi - hj
        x = np.zeros(1, F)
        for c in range(len(wu)):
            x = fmaf32(wu[c:c + 1], d[c:c + 1], x)
        g = bx.sigmoid_neg(x)[0]
        assert i[t] != j[t]
        for c in range(len(wu)):
            W[u[t], c] = wu[c] + lr * (q(g * d[c]) - lam * wu[c])
            H[i[t], c] = hi[c] + lr * (q(g * wu[c]) - lam * hi[c])
            H[j[t], c] = hj[c] + lr * (-q(g * wu[c]) - lam * hj[c])
    return W, H


def test_batch_of_one_is_textbook_sgd(R):
    k = 7
    W, H = bx.initial_factors(R.rows, R.cols, k, 1)
    u, i, j, s = bx.triples(R, 4, 0, 120)
    Wt, Ht = _sgd_textbook(W, H, u, i, j, s, 0.05, 0.01)
    for t in range(len(u)):
        W, H, st = bx.step(W, H, u[t:t + 1], i[t:t + 1], j[t:t + 1], s[t:t + 1], 0.05, 0.01)
        assert st[0] == 1 and st[1] == int(s[t]) and st[2] == 0
    assert np.array_equal(bits(W), bits(Wt)) and np.array_equal(bits(H), bits(Ht))


def test_permuting_a_batch_changes_no_bit(R):
    k = 9
    W, H = bx.initial_factors(R.rows, R.cols, k, 2)
    u, i, j, s = bx.triples(R, 5, 0, 400)
    a = bx.step(W, H, u, i, j, s, 0.05, 0.01)
    o = np.random.default_rng(0).permutation(400)
    b = bx.step(W, H, u[o], i[o], j[o], s[o], 0.05, 0.01)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])) and a[2] == b[2]
    assert not np.array_equal(bits(a[0]), bits(W))
    touched = np.zeros(R.rows, bool)
    touched[u[~s]] = True
    assert np.array_equal(bits(a[0][~touched]), bits(W[~touched]))


def test_sigmoid_recipe():
    x = np.linspace(-30, 30, 1_000_001).astype(F)
    g = bx.sigmoid_neg(x).astype(np.float64)
    ref = 1.0 / (1.0 + np.exp(x.astype(np.float64)))
    assert np.max(np.abs(g - ref) / ref) <= 1e-6
    x = np.linspace(-200, 200, 2_000_001).astype(F)
    g = bx.sigmoid_neg(x)
    assert np.all(np.isfinite(g)) and np.all(g > 0) and np.all(g <= 1)
    assert np.all(np.diff(g) <= 0)  # non-increasing along the grid
    far = bx.sigmoid_neg(np.array([-np.inf, -1e30, -200, 200, 1e30, np.inf], F))
    assert np.all(far[:3] == 1) and np.all(far[3:] == far[3]) and far[3] == bx.sigmoid_neg(F(80))[()] > 0
    assert bx.sigmoid_neg(F(0))[()] == F(0.5)


def test_bad_slots_and_untouched_rows():
    rows, cols, k = 6, 5, 3
    W, H = bx.initial_factors(rows, cols, k, 3)
    W[0, 0] = 200.0
    H[0, 0] = H[1, 0]            # slot 0: d_0 = 0, x small, g about 1/2: the term g * W[0][0] is about 100
    H[4, 2] = np.nan             # slot 1: a NaN factor
    u = np.array([0, 1, 2, 2]); i = np.array([0, 2, 3, 2]); j = np.array([1, 4, 2, 3])
    W2, H2, st = bx.step(W, H, u, i, j, None, 0.05, 0.01)
    assert st == [4, 0, 2, st[3]]
    for X, X2, same in ((W, W2, [0, 1, 3, 4, 5]), (H, H2, [0, 1, 4])):
        assert np.array_equal(bits(X[same]), bits(X2[same]))
    assert not np.array_equal(bits(W[2]), bits(W2[2])) and not np.array_equal(bits(H[2]), bits(H2[2]))


def test_reference_learns_the_planted_clusters(mfx):
    """What tests/test_gpu_bpr.py relies on: the exact reference, fed by the library's sampler, puts the held-out item
    into the top 10 of at least 90 % of the users (4 epochs here; the GPU test runs the 10 of the issue)."""
    P = bx.planted_clusters()
    assert (P.rows, P.cols, P.nnz) == (2000, 600, 54000)
    W, H = bx.initial_factors(P.rows, P.cols, 32, 5)
    W, H, stats, pos = bx.train(P, W, H, 0.05, 0.01, 1024, 7, 4, sampler=mfx.bpr_triples)
    assert pos == 4 * P.nnz and np.all(stats[:, 0] == P.nnz) and np.all(stats[:, 2] == 0)
    auc = stats[:, 3] / (stats[:, 0] - stats[:, 1] - stats[:, 2])
    assert auc[-1] > auc[0]
    S = W.astype(np.float64) @ H.astype(np.float64).T
    S[np.repeat(np.arange(P.rows), np.diff(P.csr_row_ptr.astype(np.int64))), P.csr_col_idx] = -np.inf
    top = np.argsort(-S, axis=1, kind="stable")[:, :10]
    hit = np.any(top[P.test_row] == P.test_col[:, None].astype(np.int64), axis=1)
    assert hit.mean() >= 0.9, hit.mean()


# ------------------------------------------------------------------------------------------------ refusals without a device
def _create(mfx, R, k=8, lam=0.01, lr=0.05, batch=64, csx=None):
    from mfx import api
    p = mfx.parameter()
    p.k, p.lambda_ = k, lam
    cp = p.to_c()
    cp.k = k & 0xFFFFFFFF
    h = C.c_void_p()
    csx = api._csx(R) if csx is None else csx
    rc = mfx.lib().mfx_bpr_create(C.byref(h), C.byref(csx), C.byref(cp), lr, batch, 0, 0)
    assert not h.value
    return rc


@pytest.mark.parametrize("kw", [dict(k=0), dict(k=1025), dict(batch=0), dict(batch=(1 << 20) + 1), dict(batch=-1), dict(lr=-0.1),
                                dict(lr=float("nan")), dict(lr=float("inf")), dict(lam=-1.0), dict(lam=float("nan")),
                                dict(lam=float("inf"))])
def test_create_refuses_bad_arguments_before_the_device(mfx, R, kw):
    assert _create(mfx, R, **kw) == MFX_ERR_INVALID, mfx.lib().mfx_last_error()


def test_create_refuses_degenerate_matrices_and_nulls(mfx, R):
    from mfx import api
    lib = mfx.lib()
    empty = api._csx(R)
    empty.nnz = 0
    assert _create(mfx, R, csx=empty) == MFX_ERR_INVALID
    one_col = api._csx(R)
    one_col.cols = 1
    assert _create(mfx, R, csx=one_col) == MFX_ERR_INVALID
    no_csr = api._csx(R)
    no_csr.csr_col_idx = None
    assert _create(mfx, R, csx=no_csr) == MFX_ERR_INVALID
    cp, csx, h = mfx.parameter().to_c(), api._csx(R), C.c_void_p()
    assert lib.mfx_bpr_create(None, C.byref(csx), C.byref(cp), 0.05, 64, 0, 0) == MFX_ERR_INVALID
    assert lib.mfx_bpr_create(C.byref(h), None, C.byref(cp), 0.05, 64, 0, 0) == MFX_ERR_INVALID
    assert lib.mfx_bpr_create(C.byref(h), C.byref(csx), None, 0.05, 64, 0, 0) == MFX_ERR_INVALID
    assert lib.mfx_bpr_create(C.byref(h), C.byref(csx), C.byref(cp), 0.05, 64, 0, 7) == MFX_ERR_INVALID  # memory space
    for fn in (lib.mfx_bpr_set_factors, lib.mfx_bpr_get_factors):
        assert fn(None, None, None, 0) == MFX_ERR_INVALID
    assert lib.mfx_bpr_steps(None, 1, None, None) == MFX_ERR_INVALID
    assert lib.mfx_bpr_epochs(None, 1, None, None) == MFX_ERR_INVALID
    assert lib.mfx_bpr_position(None, None) == MFX_ERR_INVALID
    assert lib.mfx_bpr_destroy(None) == 0


def test_apply_and_triples_refuse_bad_arguments_before_the_device(mfx, R):
    W, H = bx.initial_factors(4, 5, 3, 0)
    z = np.zeros(2, np.uint32)
    for kw in (dict(lr=-1.0), dict(lr=float("nan")), dict(lam=-1.0), dict(lam=float("inf"))):
        with pytest.raises(mfx.MfxError, match="mfx_bpr_apply"):
            mfx.bpr_apply(W, H, z, z, z, **{"lr": 0.05, "lam": 0.01, **kw})
    with pytest.raises(mfx.MfxError, match="2\\^20"):
        big = np.zeros((1 << 20) + 1, np.uint32)
        mfx.bpr_apply(W, H, big, big, big, 0.05, 0.01)
    with pytest.raises(mfx.MfxError, match="k must be"):
        mfx.bpr_apply(np.zeros((4, 1025), F), np.zeros((5, 1025), F), z, z, z, 0.05, 0.01)
    with pytest.raises(mfx.MfxError, match="mfx_bpr_triples"):
        mfx.bpr_triples(R, 0, -1, 4)
    bad = R.copy()
    bad.csr_row_ptr[3], bad.csr_row_ptr[4] = bad.csr_row_ptr[4] + 1, bad.csr_row_ptr[3]
    with pytest.raises(mfx.MfxError, match="csr_row_ptr"):
        mfx.bpr_triples(bad, 0, 0, 4)
