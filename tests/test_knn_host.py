"""Item-kNN without a GPU: the exported symbols, the self-checks of the exact reference tests/knn_exact.py (against a
separately written dense integer X^T X, the symmetry of the similarities), mfx.knn_weights against separately written
loops, the condition the GPU end-to-end test relies on (the reference finds the held-out items of the planted clusters),
and the argument refusals that never reach the device."""
import ctypes as C
import math

import numpy as np
import pytest

import bpr_exact as bx
import knn_exact as kx

MFX_ERR_INVALID = -1  # include/mfx.h
F = np.float32
KNN_SYMBOLS = ("mfx_knn_build", "mfx_knn_create_from_lists", "mfx_knn_lists", "mfx_knn_neighbours", "mfx_knn_recommend",
               "mfx_knn_times", "mfx_knn_destroy")


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    return m


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def random_matrix(mfx, rows, cols, nnz, seed, values="ratings"):
    rng = np.random.default_rng(seed)
    cells = rng.choice(rows * cols, nnz, replace=False)
    if values == "ratings":
        v = rng.integers(1, 6, nnz).astype(F)
    elif values == "small_int":
        v = rng.integers(-3, 4, nnz).astype(F)
    else:
        v = rng.standard_normal(nnz).astype(F)
    return mfx.dataset.from_coo(rows, cols, cells // cols, cells % cols, v)


# ------------------------------------------------------------------------------------------------ symbols
def test_symbols_are_exported_and_bound(mfx):
    from mfx import _lib
    lib = mfx.lib()
    for name in KNN_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.mfx_version() == 2
    assert mfx.MFX_KNN_KEEP_SEEN == 1
    assert callable(mfx.knn_weights) and hasattr(mfx.ItemKnn, "from_lists")
    for m in ("neighbours", "recommend", "lists", "times", "close", "__enter__", "__exit__"):
        assert hasattr(mfx.ItemKnn, m), m


# ------------------------------------------------------------------------------------------------ the reference itself
def test_reference_equals_dense_integer_gram_on_small_integers(mfx):
    """Small-integer values: every term is an integer, exact on the 2^-36 grid, so the sums are those of the dense X^T X."""
    X = random_matrix(mfx, 37, 29, 400, 5, "small_int")
    ptr = X.csr_row_ptr.astype(np.int64)
    D = np.zeros((X.rows, X.cols), np.int64)
    for u in range(X.rows):
        for e in range(ptr[u], ptr[u + 1]):
            D[u, X.csr_col_idx[e]] = int(X.csr_val[e])
    G = D.T @ D
    np.fill_diagonal(G, 0)
    S = kx.similarities(X)
    assert np.array_equal(S, G * (1 << 36))
    assert (G == 0).sum() > X.cols  # some pairs cancel or never meet
    K = 7
    ids, sims = kx.build(X, K)
    for i in range(X.cols):  # the order, written as a Python sort on tuples
        want = sorted(((-int(G[i, j]), j) for j in range(X.cols) if G[i, j] != 0))[:K]
        n = len(want)
        assert [int(x) for x in ids[i, :n]] == [j for _, j in want]
        assert [float(x) for x in sims[i, :n]] == [float(-g) for g, _ in want]
        assert np.all(ids[i, n:] == kx.PAD) and np.all(np.isneginf(sims[i, n:]))


def test_similarity_is_symmetric_in_bits(mfx):
    X = mfx.knn_weights(random_matrix(mfx, 37, 29, 400, 6), "cosine")
    S = kx.similarities(X)
    assert np.array_equal(S, S.T)
    s = kx.from_fixed(S)
    assert np.array_equal(bits(s), bits(s.T.copy()))
    X2 = random_matrix(mfx, 37, 29, 400, 7, "normal")  # terms that are NOT on the grid: truncation is still symmetric
    S2 = kx.similarities(X2)
    assert np.array_equal(S2, S2.T) and np.any(S2 % (1 << 20) != 0)


def test_fixed_point_truncates_toward_zero():
    t = np.array([1.0, -1.0, 2.0 ** -36, -2.0 ** -36, 2.0 ** -37, -2.0 ** -37, 1.5 * 2.0 ** -36, -1.5 * 2.0 ** -36, 63.999996], F)
    assert list(kx.to_fixed(t)) == [1 << 36, -(1 << 36), 1, -1, 0, 0, 1, -1, int(np.float64(F(63.999996)) * 2.0 ** 36)]
    assert np.array_equal(kx.from_fixed(np.array([1 << 36, -3, (1 << 60) + 1], np.int64)), np.array([1.0, -3 * 2.0 ** -36, 2.0 ** 24], F))


def test_reference_refuses_what_the_contract_refuses(mfx):
    X = random_matrix(mfx, 20, 12, 100, 8)
    c = X.copy()
    u = int(np.argmax(np.diff(c.csr_row_ptr.astype(np.int64)) >= 2))
    e = int(c.csr_row_ptr[u])
    c.csr_val[e] = 50.0
    c.csr_val[e + 1] = 2.0  # the term 100 for the pair of the row's first two items
    with pytest.raises(kx.BadTerm) as err:
        kx.similarities(c)
    assert err.value.item == int(c.csr_col_idx[e])
    c.csr_val[e] = np.nan
    with pytest.raises(kx.BadTerm) as err:
        kx.similarities(c)
    assert err.value.item == int(c.csr_col_idx[e])  # (the row's smallest item: every pair with the NaN is bad)


def _with_holes_and_signs(mfx):
    """+-1 values (pairs that meet and cancel), column 3 and row 5 empty."""
    rng = np.random.default_rng(31)
    cells = rng.choice(30 * 14, 200, replace=False)
    r, c = cells // 14, cells % 14
    keep = (r != 5) & (c != 3)
    v = (2 * rng.integers(0, 2, 200) - 1).astype(F)
    return mfx.dataset.from_coo(30, 14, r[keep], c[keep], v[keep])


@pytest.mark.parametrize("name", ["small_int", "ratings", "normal", "cosine", "signs"])
def test_similarity_rows_equal_the_dense_reference(mfx, name):
    """similarity_rows (the sparse reference of the wide catalogues) against similarities, the reference pinned above: every
    item at once, a subset in an order of its own with an item twice, one item, and no item."""
    if name == "signs":
        X = _with_holes_and_signs(mfx)
        assert X.csc_col_ptr[3] == X.csc_col_ptr[4]  # an empty column: a row of zeros
    elif name == "cosine":
        X = mfx.knn_weights(random_matrix(mfx, 37, 29, 400, 6), "cosine")
    else:
        X = random_matrix(mfx, 37, 29, 400, 5, name)
    S = kx.similarities(X)
    assert np.array_equal(kx.similarity_rows(X, np.arange(X.cols)), S)
    sub = np.array([X.cols - 1, 3, 0, 7, 3])
    got = kx.similarity_rows(X, sub)
    assert got.dtype == np.int64 and got.shape == (5, X.cols) and np.array_equal(got, S[sub])
    assert np.array_equal(kx.similarity_rows(X, [3]), S[3:4])
    assert kx.similarity_rows(X, []).shape == (0, X.cols)
    if name == "signs":
        D = np.zeros((X.rows, X.cols), np.int64)
        D[np.repeat(np.arange(X.rows), np.diff(X.csr_row_ptr.astype(np.int64))), X.csr_col_idx] = 1
        co = D.T @ D
        np.fill_diagonal(co, 0)
        assert np.any((S == 0) & (co > 0))  # pairs that meet but whose terms cancel
        assert not S[3].any() and not S[:, 3].any()
    ids, sims = kx.top_lists(kx.similarity_rows(X, sub), 6)
    want = kx.build(X, 6)
    assert np.array_equal(ids, want[0][sub]) and np.array_equal(bits(sims), bits(want[1][sub]))


def test_similarity_rows_refuse_with_the_same_item(mfx):
    X = random_matrix(mfx, 20, 12, 100, 8)
    u = int(np.argmax(np.diff(X.csr_row_ptr.astype(np.int64)) >= 3))
    e = int(X.csr_row_ptr[u])
    first, second, third = (int(X.csr_col_idx[e + q]) for q in range(3))

    def put(Y, item, value):  # on both sides
        Y.csr_val[int(Y.csr_row_ptr[u]) + int(np.nonzero(Y.csr_col_idx[Y.csr_row_ptr[u]:Y.csr_row_ptr[u + 1]] == item)[0][0])] = value
        c0, c1 = int(Y.csc_col_ptr[item]), int(Y.csc_col_ptr[item + 1])
        Y.csc_val[c0 + int(np.nonzero(Y.csc_row_idx[c0:c1] == u)[0][0])] = value

    c = X.copy()
    put(c, second, 9.0)
    put(c, third, 8.0)  # the term 72 for the pair (second, third) only: with ratings up to 5 every other term stays below 64
    with pytest.raises(kx.BadTerm) as want:
        kx.similarities(c)
    assert want.value.item == second
    with pytest.raises(kx.BadTerm) as err:
        kx.similarity_rows(c, np.arange(c.cols))
    assert err.value.item == want.value.item
    with pytest.raises(kx.BadTerm) as err:
        kx.similarity_rows(c, [third, second])  # whatever the order of the items
    assert err.value.item == second
    with pytest.raises(kx.BadTerm) as err:
        kx.similarity_rows(c, [third])  # of the items asked for, the smallest bad one
    assert err.value.item == third
    clean = [i for i in range(c.cols) if i not in (second, third)]
    assert np.array_equal(kx.similarity_rows(c, clean)[:, clean], kx.similarities(X)[np.ix_(clean, clean)])  # the others are served
    c = X.copy()
    put(c, second, np.nan)
    with pytest.raises(kx.BadTerm) as want:
        kx.similarities(c)
    with pytest.raises(kx.BadTerm) as err:
        kx.similarity_rows(c, np.arange(c.cols))
    assert err.value.item == want.value.item == first  # (the row's smallest item: every pair with the NaN is bad)


# ------------------------------------------------------------------------------------------------ the weights
def _weights_by_loops(R, scheme, k1, b):
    """Entry by entry in Python floats: {(u, i): x}."""
    ptr = R.csr_row_ptr.astype(np.int64)
    entries = {}
    for u in range(R.rows):
        for e in range(ptr[u], ptr[u + 1]):
            entries[(u, int(R.csr_col_idx[e]))] = float(R.csr_val[e])
    c = [0] * R.cols
    n_u = [0] * R.rows
    for (u, i) in entries:
        c[i] += 1
        n_u[u] += 1
    nbar = sum(n_u) / R.rows
    idf = [math.log(R.rows) - math.log(1 + ci) for ci in c]
    out = {}
    if scheme == "bm25":
        for (u, i), r in entries.items():
            out[(u, i)] = r * (k1 + 1) / (k1 * (1 - b + b * n_u[u] / nbar) + r) * idf[i]
        return out
    y = {k: (r if scheme == "cosine" else math.sqrt(r) * idf[k[1]]) for k, r in entries.items()}
    sq = [0.0] * R.cols
    for (u, i), v in y.items():
        sq[i] += v * v
    return {(u, i): v / math.sqrt(sq[i]) for (u, i), v in y.items()}


@pytest.mark.parametrize("scheme,k1,b", [("cosine", 1.2, 0.75), ("tfidf", 1.2, 0.75), ("bm25", 1.2, 0.75), ("bm25", 2.0, 0.3)])
def test_weights_match_loops(mfx, scheme, k1, b):
    """Both sides compute in fp64 (relative error ~1e-15, the order of the norm's sum and the libm differ) and round to fp32
    once, so two results differ by at most one fp32 unit in the last place, |a - b| <= 2^-23 |b|, and nearly all are equal."""
    R = random_matrix(mfx, 37, 29, 400, 9)  # (no column is empty here; the empty column is the next test)
    X = mfx.knn_weights(R, scheme, k1=k1, b=b)
    want = _weights_by_loops(R, scheme, k1, b)
    assert X.csr_val.dtype == F and X.csc_val.dtype == F
    assert np.array_equal(X.csr_col_idx, R.csr_col_idx) and np.array_equal(X.csc_row_idx, R.csc_row_idx)
    rows_of = np.repeat(np.arange(R.rows), np.diff(R.csr_row_ptr.astype(np.int64)))
    cols_of = np.repeat(np.arange(R.cols), np.diff(R.csc_col_ptr.astype(np.int64)))
    w_csr = np.array([want[(int(u), int(i))] for u, i in zip(rows_of, R.csr_col_idx)])
    w_csc = np.array([want[(int(u), int(i))] for u, i in zip(R.csc_row_idx, cols_of)])
    for got, w in ((X.csr_val, w_csr), (X.csc_val, w_csc)):
        w32 = w.astype(F)
        assert np.all(np.abs(got.astype(np.float64) - w32) <= 2.0 ** -23 * np.abs(w32))
        assert np.mean(bits(got) == bits(w32)) > 0.95
    ref_csr, ref_csc = kx.weights(R, scheme, k1, b)
    for got, w32 in ((X.csr_val, ref_csr), (X.csc_val, ref_csc)):
        assert np.all(np.abs(got.astype(np.float64) - w32) <= 2.0 ** -23 * np.abs(w32))
    if scheme != "bm25":  # unit columns
        sq = np.bincount(cols_of, weights=X.csc_val.astype(np.float64) ** 2, minlength=R.cols)
        assert np.allclose(sq, 1.0, atol=1e-6)


def test_weights_keep_empty_columns_and_both_sides_agree(mfx):
    R = mfx.dataset.from_coo(5, 4, [0, 0, 1, 3, 4, 4], [0, 3, 0, 3, 0, 1], np.array([1, 2, 3, 4, 5, 1], F))  # column 2, row 2 empty
    for scheme in ("cosine", "tfidf", "bm25", None):
        X = mfx.knn_weights(R, scheme)
        assert np.array_equal(X.csc_col_ptr, R.csc_col_ptr) and np.array_equal(X.csr_row_ptr, R.csr_row_ptr)
        dense_r = np.zeros((5, 4), F)
        dense_c = np.zeros((5, 4), F)
        dense_r[np.repeat(np.arange(5), np.diff(X.csr_row_ptr.astype(np.int64))), X.csr_col_idx] = X.csr_val
        dense_c[X.csc_row_idx, np.repeat(np.arange(4), np.diff(X.csc_col_ptr.astype(np.int64)))] = X.csc_val
        assert np.array_equal(bits(dense_r), bits(dense_c))
        assert np.all(np.isfinite(X.csr_val))
    assert np.array_equal(mfx.knn_weights(R, None).csr_val, R.csr_val)
    with pytest.raises(ValueError):
        mfx.knn_weights(R, "jaccard")


# ------------------------------------------------------------------------------------------------ the model learns
def test_reference_finds_the_held_out_items_of_the_planted_clusters(mfx):
    """Cosine weights, K = 100, every training user's own row: the held-out item is in the top 10 for >= 90 % of the users."""
    P = bx.planted_clusters()
    X = mfx.knn_weights(P, "cosine")
    ids, sims = kx.build(X, 100)
    items, scores, bad = kx.recommend(ids, sims, X.csr_row_ptr, X.csr_col_idx, X.csr_val, 10)
    assert bad == 0
    hits = np.any(items == P.test_col[np.argsort(P.test_row)][:, None], axis=1)
    assert hits.shape == (P.rows,)
    assert hits.mean() >= 0.9, hits.mean()


# ------------------------------------------------------------------------------------------------ refusals
def _build(mfx, X, K=5, tile=0, space=0, csx=None):
    from mfx import api
    h = C.c_void_p(0x1)
    csx = csx if csx is not None else api._csx(X)
    rc = mfx.lib().mfx_knn_build(C.byref(h), C.byref(csx), K, tile, space, 0)
    return rc, h


@pytest.mark.parametrize("kw", [dict(K=0), dict(K=-1), dict(K=1025), dict(space=7), dict(tile=-64), dict(tile=32), dict(tile=100),
                                dict(tile=8256), dict(K=600, tile=8192)])
def test_build_refuses_bad_arguments_before_the_device(mfx, kw):
    X = bx.small_matrix()
    rc, h = _build(mfx, X, **kw)
    assert rc == MFX_ERR_INVALID, mfx.lib().mfx_last_error()
    assert not h.value  # the handle pointer is left null


def test_build_refuses_degenerate_matrices_and_nulls(mfx):
    from mfx import _lib, api
    X = bx.small_matrix()
    lib = mfx.lib()
    full = api._csx(X)
    fields = [f for f, _ in _lib.mfx_csx._fields_]

    def variant(**kw):
        c = _lib.mfx_csx(*[getattr(full, f) for f in fields])
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    assert _build(mfx, X, csx=variant(nnz=0))[0] == MFX_ERR_INVALID
    assert _build(mfx, X, csx=variant(cols=1))[0] == MFX_ERR_INVALID
    assert _build(mfx, X, csx=variant(rows=0))[0] == MFX_ERR_INVALID
    for f in fields[3:]:  # each of the six arrays: both orientations are needed
        rc, h = _build(mfx, X, csx=variant(**{f: None}))
        assert rc == MFX_ERR_INVALID and not h.value, f
    h = C.c_void_p()
    assert lib.mfx_knn_build(None, C.byref(full), 5, 0, 0, 0) == MFX_ERR_INVALID
    assert lib.mfx_knn_build(C.byref(h), None, 5, 0, 0, 0) == MFX_ERR_INVALID


def test_from_lists_and_handle_calls_refuse_before_the_device(mfx):
    lib = mfx.lib()
    idx = np.zeros((4, 3), np.uint32)
    sim = np.zeros((4, 3), F)
    pi, ps = idx.ctypes.data_as(C.c_void_p), sim.ctypes.data_as(C.c_void_p)
    for args in ((4, 0, pi, ps, 0), (4, 1025, pi, ps, 0), (1, 3, pi, ps, 0), (4, 3, None, ps, 0), (4, 3, pi, None, 0), (4, 3, pi, ps, 5),
                 (1 << 32, 3, pi, ps, 0)):
        h = C.c_void_p(0x1)
        assert lib.mfx_knn_create_from_lists(C.byref(h), *args, 0) == MFX_ERR_INVALID, args
        assert not h.value
    assert lib.mfx_knn_create_from_lists(None, 4, 3, pi, ps, 0, 0) == MFX_ERR_INVALID
    out = (C.c_double * 4)()
    bad = C.c_int64(0)
    assert lib.mfx_knn_lists(None, pi, ps, 0) == MFX_ERR_INVALID
    assert lib.mfx_knn_neighbours(None, 1, None, 1, pi, ps, 0) == MFX_ERR_INVALID
    assert lib.mfx_knn_recommend(None, 1, 0, pi, None, None, 1, 0, 0, pi, ps, C.byref(bad), 0) == MFX_ERR_INVALID
    assert lib.mfx_knn_times(None, out) == MFX_ERR_INVALID
    assert lib.mfx_knn_destroy(None) == 0


def test_python_front_end_refuses_malformed_input(mfx):
    with pytest.raises(ValueError):
        mfx.ItemKnn.from_lists(np.zeros((4, 3), np.uint32), np.zeros((4, 2), F))
    with pytest.raises(ValueError):
        mfx.ItemKnn(None, 5, "cosine", device_arrays={"rows": 1, "cols": 2})
