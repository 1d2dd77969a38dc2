"""SLIM without a GPU: the exported symbols, the self-checks of the exact reference tests/slim_exact.py (its Gram against a
separately written dense integer X^T X, its solve against an fp64 coordinate descent, the descent of its objective, the
all-zero solution under a large l1), the condition the GPU end-to-end test relies on (the reference finds the held-out items
of the planted clusters), and the argument refusals that never reach the device."""
import ctypes as C

import numpy as np
import pytest

import bpr_exact as bx
import knn_exact as kx
import slim_exact as sx

MFX_ERR_INVALID = -1  # include/mfx.h
F = np.float32
PAD = sx.PAD
SLIM_SYMBOLS = ("mfx_slim_train", "mfx_slim_gram", "mfx_slim_solve", "mfx_slim_create_from_lists", "mfx_slim_weights",
                "mfx_slim_recommend", "mfx_slim_times", "mfx_slim_destroy")


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    return m


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def random_matrix(mfx, rows, cols, nnz, seed, values="ratings"):
    rng = np.random.default_rng(seed)
    cells = rng.choice(rows * cols, nnz, replace=False)
    v = rng.integers(1, 6, nnz).astype(F) if values == "ratings" else rng.integers(-3, 4, nnz).astype(F)
    return mfx.dataset.from_coo(rows, cols, cells // cols, cells % cols, v)


def random_support(cols, K, seed, pads=True):
    """Distinct ids that are not the item itself; with pads: lists of every length 0 .. K."""
    rng = np.random.default_rng(seed)
    S = np.full((cols, K), PAD, np.uint32)
    for j in range(cols):
        n = int(rng.integers(0, K + 1)) if pads else K
        S[j, :n] = rng.permutation(np.setdiff1d(np.arange(cols), [j]))[:n]
    return S


# ------------------------------------------------------------------------------------------------ symbols
def test_symbols_are_exported_and_bound(mfx):
    from mfx import _lib
    lib = mfx.lib()
    for name in SLIM_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.mfx_version() == 2
    assert mfx.MFX_SLIM_SIGNED == 1
    assert callable(mfx.slim_gram) and callable(mfx.slim_solve) and hasattr(mfx.Slim, "from_lists")
    for m in ("weights", "recommend", "sweeps_used", "times", "close", "__enter__", "__exit__"):
        assert hasattr(mfx.Slim, m), m


# ------------------------------------------------------------------------------------------------ the reference itself
def test_reference_gram_equals_dense_integer_gram_on_small_integers(mfx):
    """Small-integer values: every term is an integer, exact on the 2^-36 grid, so every block entry is an entry of the dense
    X^T X, the diagonal included."""
    X = random_matrix(mfx, 37, 29, 400, 5, "small_int")
    ptr = X.csr_row_ptr.astype(np.int64)
    D = np.zeros((X.rows, X.cols), np.int64)
    for u in range(X.rows):
        for e in range(ptr[u], ptr[u + 1]):
            D[u, X.csr_col_idx[e]] = int(X.csr_val[e])
    G = D.T @ D
    assert np.array_equal(sx.gram_sums(X), G * (1 << 36))
    K = 6
    S = random_support(X.cols, K, 3)
    B = sx.gram_blocks(X, S)
    assert B.shape == (X.cols, K + 1, K) and B.dtype == F
    n = sx.real_slots(S)
    assert set(n) == set(range(K + 1))
    for j in range(X.cols):
        for p in range(K):
            for t in range(K):
                want = float(G[S[j, p], S[j, t]]) if p < n[j] and t < n[j] else 0.0
                assert float(B[j, p, t]) == want
            assert float(B[j, K, p]) == (float(G[j, S[j, p]]) if p < n[j] else 0.0)


def test_reference_gram_is_symmetric_in_bits_and_its_last_row_is_the_knn_similarity(mfx):
    X = mfx.knn_weights(random_matrix(mfx, 37, 29, 400, 6), "cosine")
    K = 9
    ids, sims = kx.build(X, K)
    B = sx.gram_blocks(X, ids)
    assert np.array_equal(bits(B[:, :K, :]), bits(np.ascontiguousarray(B[:, :K, :].transpose(0, 2, 1))))
    real = ids != PAD
    assert np.array_equal(bits(B[:, K, :][real]), bits(sims[real])) and np.all(B[:, K, :][~real] == 0)
    d = np.array([B[j, p, p] for j in range(X.cols) for p in range(K) if real[j, p]])
    assert np.all(np.abs(d - 1.0) < 1e-5)  # unit columns


def without_column(mfx, X, c):
    r = np.repeat(np.arange(X.rows), np.diff(X.csr_row_ptr.astype(np.int64)))
    keep = X.csr_col_idx != c
    return mfx.dataset.from_coo(X.rows, X.cols, r[keep], X.csr_col_idx[keep], X.csr_val[keep])


def test_sparse_reference_gram_equals_the_dense_one_in_bits(mfx):
    """gram_blocks_sparse (pair by pair, for catalogues too wide for gram_sums) against gram_blocks: ratings, small integers
    of both signs that cancel (and explicit zeros), an empty column; lists with pads, one all pads, full lists at K = 1, 6
    and 28; and the 50 x 700 matrix of the GPU suite with its hub item, unused item and empty column."""
    from test_gpu_slim import _hub_matrix, _hub_support
    cases = []
    for values, seed in (("ratings", 6), ("small_int", 5)):
        X = random_matrix(mfx, 37, 29, 400, seed, values)
        for K in (1, 6, 28):
            S = random_support(29, K, 30 + K)
            S[7, :] = PAD
            cases += [(X, S), (X, random_support(29, K, 40 + K, pads=False))]
        E = without_column(mfx, X, 5)
        assert E.csc_col_ptr[5] == E.csc_col_ptr[6]
        S = random_support(29, 6, 50, pads=False)
        assert np.any(S == 5)
        cases.append((E, S))
    small_int = sx.gram_sums(cases[-1][0])
    assert (small_int[~np.eye(29, dtype=bool)] == 0).sum() > 0  # pairs that meet and cancel, or never meet
    H = _hub_matrix(mfx)
    assert H.cols == 700 and H.csc_col_ptr[5] == H.csc_col_ptr[6]
    cases.append((H, _hub_support()))
    for X, S in cases:
        want = sx.gram_blocks(X, S)
        got = sx.gram_blocks_sparse(X, S)
        assert got.shape == want.shape and got.dtype == want.dtype == F and np.array_equal(bits(got), bits(want))
        assert want.any()
    X, S = cases[0]
    a, b = np.divmod(np.arange(29 * 29), 29)
    assert np.array_equal(sx.pair_sums(X, a, b, chunk=100).reshape(29, 29), sx.gram_sums(X))  # every pair, in many chunks
    c = X.copy()
    e = int(c.csc_col_ptr[4])
    u = int(c.csc_row_idx[e])
    c.csc_val[e] = 9.0  # 81 on the diagonal of item 4 alone
    r0, r1 = int(c.csr_row_ptr[u]), int(c.csr_row_ptr[u + 1])
    c.csr_val[r0 + int(np.nonzero(c.csr_col_idx[r0:r1] == 4)[0][0])] = 9.0
    with pytest.raises(kx.BadTerm) as err:
        sx.gram_blocks_sparse(c, S)
    assert err.value.item == 4
    c.csc_val[e] = c.csr_val[r0 + int(np.nonzero(c.csr_col_idx[r0:r1] == 4)[0][0])] = 70.0  # and 70 * rating >= 64 with every pair
    with pytest.raises(kx.BadTerm) as err:
        sx.pair_sums(c, a, b)
    with pytest.raises(kx.BadTerm) as dense:
        sx.gram_sums(c)
    assert err.value.item == dense.value.item


def psd_blocks(N, K, seed, rows=40):
    """N random blocks: G = A^T A of a rows x K matrix of small entries, g = A^T y."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((N, rows, K)) * 0.5
    y = rng.standard_normal((N, rows)) * 0.5 + A[:, :, : max(1, K // 3)].sum(axis=2)
    B = np.zeros((N, K + 1, K), F)
    B[:, :K, :] = np.einsum("nrk,nrl->nkl", A, A).astype(F)
    B[:, :K, :] = 0.5 * (B[:, :K, :] + B[:, :K, :].transpose(0, 2, 1))  # (exact: a sum of two fp32 halved)
    B[:, K, :] = np.einsum("nrk,nr->nk", A, y).astype(F)
    return B


def cd64(block, l1, l2, sweeps, signed):
    """The same coordinate descent in fp64 on the direct form of the update."""
    K = block.shape[1]
    G = block[:K].astype(np.float64)
    g = block[K].astype(np.float64)
    w = np.zeros(K)
    for _ in range(sweeps):
        for a in range(K):
            z = g[a] - G[a] @ w + G[a, a] * w[a]
            t = np.sign(z) * max(abs(z) - l1, 0.0) if signed else max(z - l1, 0.0)
            w[a] = t / (G[a, a] + l2)
    return w


def slim_solve_distance(seed):
    """The worst distance over items, modes and shapes of the reference solve from the fp64 descent, relative to the largest
    fp64 weight of the item."""
    worst = 0.0
    for K, signed, l1, l2 in ((5, False, 0.5, 1.0), (20, True, 0.25, 2.0), (64, False, 0.1, 5.0), (100, True, 0.0, 10.0)):
        B = psd_blocks(6, K, seed + K)
        w32, used, failed = sx.solve(B, None, l1, l2, 8, 0.0, signed)
        assert failed == 0 and np.all((used >= 1) & (used <= 8))  # (tol = 0: an item stops early only when a sweep changes nothing)
        for n in range(B.shape[0]):
            w64 = cd64(B[n], l1, l2, 8, signed)
            assert np.abs(w64).max() > 0
            worst = max(worst, float(np.abs(w32[n] - w64).max() / np.abs(w64).max()))
    return worst


def test_reference_solve_follows_an_fp64_coordinate_descent():
    """Random PSD blocks at K = 5, 20, 64, 100, both modes, 8 sweeps: the fp32 covariance-update form against the direct form
    in fp64.  Measured on the CPU with the seed 1000: worst relative distance 1.4e-6; the bound is four times that, for the
    fp32 rounding of another seed (2000, used here)."""
    d = slim_solve_distance(2000)
    print("worst relative distance", d)
    assert d <= 4 * 1.4e-6, d


def test_reference_objective_never_increases():
    """The objective of the fp32 iterates after every sweep, evaluated in fp64.  An exact coordinate step never raises it; the
    fp32 step lands within one rounding of each of its K coordinates, so a sweep may raise the objective by at most about
    K * 2^-23 of its magnitude near the minimum, which is the slack allowed."""
    for K, signed, l1, l2 in ((5, False, 0.5, 1.0), (20, True, 0.25, 2.0), (64, False, 0.1, 5.0)):
        B = psd_blocks(4, K, 77 + K)
        trace = []
        sx.solve(B, None, l1, l2, 12, 0.0, signed, trace=trace)
        assert 2 <= len(trace) <= 12  # (it ends with the last item; a stopped item keeps its weights)
        for n in range(B.shape[0]):
            f = [0.0] + [sx.objective(B[n], K, w[n], l1, l2) for w in trace]
            slack = K * 2.0 ** -23 * max(abs(x) for x in f)
            assert all(b <= a + slack for a, b in zip(f, f[1:])), f
            assert f[1] < 0 and f[-1] <= f[1]


def test_large_l1_gives_all_zero_weights():
    B = psd_blocks(5, 12, 91)
    l1 = float(np.abs(B[:, 12, :]).max())
    for signed in (False, True):
        w, used, failed = sx.solve(B, None, l1, 1.0, 5, 0.0, signed)
        assert failed == 0 and not w.any() and np.all(used == 1)  # the first sweep changes nothing: m = 0 <= tol
    w, _, _ = sx.solve(B, None, 0.5 * l1, 1.0, 5, 0.0, True)
    assert w.any()


def test_reference_skips_zero_diagonals_and_counts_failures():
    B = psd_blocks(3, 4, 92)
    B[1, 2, :] = 0
    B[1, :, 2] = 0  # coordinate 2 of item 1: d = 0, g = 0
    w, used, failed = sx.solve(B, None, 0.0, 0.0, 3, 0.0, True)
    assert failed == 0 and w[1, 2] == 0 and np.all(used == 3)
    B[2, 4, 0] = np.inf
    w2, used2, failed2 = sx.solve(B, None, 0.0, 0.0, 3, 0.0, True)
    assert failed2 == 1 and not w2[2].any() and used2[2] == 0
    assert np.array_equal(bits(w2[:2]), bits(w[:2])) and np.array_equal(used2[:2], used[:2])


def test_reference_refuses_bad_supports_and_bad_terms(mfx):
    X = random_matrix(mfx, 20, 12, 100, 8)
    S = random_support(12, 4, 9, pads=False)
    for item, slot, ident in ((5, 1, 5), (5, 2, None), (3, 0, 12), (7, 1, PAD)):
        T = S.copy()
        T[9, 0] = 9  # a later bad item: the first one is named
        T[item, slot] = T[item, 0] if ident is None else ident
        with pytest.raises(sx.BadSupport) as err:
            sx.gram_blocks(X, T)
        assert err.value.item == item
    c = X.copy()
    e = int(c.csc_col_ptr[4])
    u = int(c.csc_row_idx[e])
    c.csc_val[e] = 9.0  # 81 on the diagonal of item 4 alone: every pair stays below 64
    r0, r1 = int(c.csr_row_ptr[u]), int(c.csr_row_ptr[u + 1])
    c.csr_val[r0 + int(np.nonzero(c.csr_col_idx[r0:r1] == 4)[0][0])] = 9.0
    with pytest.raises(kx.BadTerm) as err:
        sx.gram_blocks(c, S)
    assert err.value.item == 4


def test_transpose_holds_every_weight_once_with_ascending_targets():
    S = random_support(30, 5, 10)
    w = np.random.default_rng(11).standard_normal(S.shape).astype(F)
    iptr, tj, tw = sx.transpose(S, w)
    assert iptr[-1] == (S != PAD).sum()
    for i in range(30):
        t = tj[iptr[i]:iptr[i + 1]]
        assert np.all(np.diff(t.astype(np.int64)) > 0)
        for j, x in zip(t, tw[iptr[i]:iptr[i + 1]]):
            p = int(np.nonzero(S[j] == i)[0][0])
            assert bits(w[j, p:p + 1])[0] == bits(np.array([x], F))[0]
    ids, vals = sx.transposed_lists(S, w)
    ptr = np.array([0, 3], np.uint32)
    idx = np.array([2, 7, 19], np.uint32)
    val = np.array([1.0, -0.5, 2.0], F)
    a = sx.recommend(S, w, ptr, idx, val, 8)
    b = kx.recommend(ids, vals, ptr, idx, val, 8)
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and a[2] == b[2] == 0


# ------------------------------------------------------------------------------------------------ the model learns
@pytest.fixture(scope="module")
def planted(mfx):
    P = bx.planted_clusters()
    ids, _ = kx.build(mfx.knn_weights(P, "cosine"), 20)
    return P, ids, sx.gram_sums(P)


def test_reference_finds_the_held_out_items_of_the_planted_clusters(planted):
    """Raw values, the support of the cosine kNN reference at K = 20, l1 = 1, l2 = 10, 10 sweeps, tol = 0: the held-out item
    is in the top 10 for >= 90 % of the users."""
    P, ids, sums = planted
    w, used, failed = sx.train(P, ids, 1.0, 10.0, 10, 0.0, sums=sums)
    assert failed == 0 and used.max() <= 10
    items, scores, bad = sx.recommend(ids, w, P.csr_row_ptr, P.csr_col_idx, P.csr_val, 10)
    assert bad == 0
    hits = np.any(items == P.test_col[np.argsort(P.test_row)][:, None], axis=1)
    assert hits.shape == (P.rows,)
    print("HR@10", hits.mean())
    assert hits.mean() >= 0.9, hits.mean()


def test_reference_items_stop_after_different_sweep_counts(planted):
    """l1 = 0, l2 = 200, tol = 1e-4: the items stop on their own, not all after the same sweep."""
    P, ids, sums = planted
    w, used, failed = sx.train(P, ids, 0.0, 200.0, 50, 1e-4, sums=sums)
    print("sweep counts", np.unique(used))
    assert failed == 0 and used.max() < 50 and len(np.unique(used)) >= 2


# ------------------------------------------------------------------------------------------------ refusals
def _train(mfx, X, S, K=4, l1=1.0, l2=10.0, sweeps=10, tol=0.0, flags=0, tile=0, space=0, csx=None, null_support=False):
    from mfx import api
    h = C.c_void_p(0x1)
    failed = C.c_int64(0)
    csx = csx if csx is not None else api._csx(X)
    ps = None if null_support else S.ctypes.data_as(C.c_void_p)
    rc = mfx.lib().mfx_slim_train(C.byref(h), C.byref(csx), K, ps, l1, l2, sweeps, tol, flags, tile, C.byref(failed), space, 0)
    return rc, h


BAD_PARAMS = [dict(l1=-1.0), dict(l1=float("nan")), dict(l2=-0.5), dict(l2=float("nan")), dict(tol=-1e-3), dict(tol=float("nan")),
              dict(sweeps=0), dict(flags=2), dict(flags=-1)]


@pytest.mark.parametrize("kw", [dict(K=0), dict(K=129), dict(space=7), dict(tile=-64), dict(tile=32), dict(tile=100), dict(tile=8256),
                                dict(null_support=True)] + BAD_PARAMS)
def test_train_refuses_bad_arguments_before_the_device(mfx, kw):
    X = bx.small_matrix()
    S = np.full((X.cols, 129), PAD, np.uint32)  # (wide enough for every K tried; never read)
    rc, h = _train(mfx, X, S, **kw)
    assert rc == MFX_ERR_INVALID, mfx.lib().mfx_last_error()
    assert not h.value  # the handle pointer is left null


def test_train_and_gram_refuse_degenerate_matrices_and_nulls(mfx):
    from mfx import _lib, api
    X = bx.small_matrix()
    S = random_support(X.cols, 4, 13)
    lib = mfx.lib()
    full = api._csx(X)
    fields = [f for f, _ in _lib.mfx_csx._fields_]
    out = np.zeros((X.cols, 5, 4), F)
    ps, po = S.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)

    def variant(**kw):
        c = _lib.mfx_csx(*[getattr(full, f) for f in fields])
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    variants = [variant(nnz=0), variant(cols=1), variant(rows=0)] + [variant(**{f: None}) for f in fields[3:]]
    for c in variants:
        rc, h = _train(mfx, X, S, csx=c)
        assert rc == MFX_ERR_INVALID and not h.value
        assert lib.mfx_slim_gram(C.byref(c), 4, ps, 0, po, 0, 0) == MFX_ERR_INVALID
    failed = C.c_int64(0)
    assert lib.mfx_slim_train(None, C.byref(full), 4, ps, 1.0, 10.0, 10, 0.0, 0, 0, C.byref(failed), 0, 0) == MFX_ERR_INVALID
    h = C.c_void_p(0x1)
    assert lib.mfx_slim_train(C.byref(h), None, 4, ps, 1.0, 10.0, 10, 0.0, 0, 0, C.byref(failed), 0, 0) == MFX_ERR_INVALID and not h.value
    for args in ((None, 4, ps, 0, po, 0), (C.byref(full), 4, None, 0, po, 0), (C.byref(full), 4, ps, 0, None, 0), (C.byref(full), 0, ps, 0, po, 0),
                 (C.byref(full), 129, ps, 0, po, 0), (C.byref(full), 4, ps, 32, po, 0), (C.byref(full), 4, ps, 0, po, 5)):
        assert lib.mfx_slim_gram(*args, 0) == MFX_ERR_INVALID, args


def test_solve_refuses_bad_arguments_before_the_device(mfx):
    lib = mfx.lib()
    B = psd_blocks(2, 3, 14)
    w = np.zeros((2, 3), F)
    used = np.zeros(2, np.int32)
    failed = C.c_int64(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(n=2, K=3, blocks=p(B), l1=1.0, l2=10.0, sweeps=10, tol=0.0, flags=0, pw=p(w), pu=p(used), space=0):
        return lib.mfx_slim_solve(n, K, blocks, None, l1, l2, sweeps, tol, flags, pw, pu, C.byref(failed), space, 0)
    for kw in [dict(K=0), dict(K=129), dict(n=-1), dict(n=1 << 32), dict(space=3), dict(blocks=None), dict(pw=None), dict(pu=None)] + BAD_PARAMS:
        assert call(**kw) == MFX_ERR_INVALID, kw
    assert call(n=0, blocks=None, pw=None, pu=None) == 0  # nothing to do


def test_from_lists_and_handle_calls_refuse_before_the_device(mfx):
    lib = mfx.lib()
    S = np.zeros((4, 3), np.uint32)
    w = np.zeros((4, 3), F)
    ps, pw = S.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p)
    for args in ((4, 0, ps, pw, 0), (4, 129, ps, pw, 0), (1, 3, ps, pw, 0), (4, 3, None, pw, 0), (4, 3, ps, None, 0), (4, 3, ps, pw, 5),
                 (1 << 32, 3, ps, pw, 0)):
        h = C.c_void_p(0x1)
        assert lib.mfx_slim_create_from_lists(C.byref(h), *args, 0) == MFX_ERR_INVALID, args
        assert not h.value
    assert lib.mfx_slim_create_from_lists(None, 4, 3, ps, pw, 0, 0) == MFX_ERR_INVALID
    out = (C.c_double * 5)()
    bad = C.c_int64(0)
    assert lib.mfx_slim_weights(None, ps, pw, None, 0) == MFX_ERR_INVALID
    assert lib.mfx_slim_recommend(None, 1, 0, ps, None, None, 1, 0, 0, ps, pw, C.byref(bad), 0) == MFX_ERR_INVALID
    assert lib.mfx_slim_times(None, out) == MFX_ERR_INVALID
    assert lib.mfx_slim_destroy(None) == 0


def test_python_front_end_refuses_malformed_input(mfx):
    with pytest.raises(ValueError):
        mfx.Slim.from_lists(np.zeros((4, 3), np.uint32), np.zeros((4, 2), F))
    with pytest.raises(ValueError):
        mfx.Slim(None, 5, weighting="cosine", device_arrays={"rows": 1, "cols": 2})
    with pytest.raises(ValueError):
        mfx.Slim(None, 5, device_arrays={"rows": 1, "cols": 2})  # device arrays need a support
    with pytest.raises(ValueError):
        mfx.slim_solve(np.zeros((2, 3, 3), F))
    with pytest.raises(ValueError):
        mfx.slim_gram(bx.small_matrix(), 4, np.zeros((3, 4), np.uint32))
