"""GPU tests of EASE (mfx_ease_*, csrc/ease.hip and csrc/ease_inverse.hip) against the exact reference tests/ease_exact.py.

Gram matrix, weights and recommendations are compared bit for bit.  The inverse has two schedules (grouped LDS-staged kernels,
and one wavefront per block) that must agree in bits with each other for every n and with mfx_spd_inverse for n <= 1024; above
1024 the result is also held to the bound of tests/test_gpu_spd_inverse.py, |I - A X|_F in fp64 at most n 2^-24 cond_2(A), on
G = X^T X + lambda I of a random binary X with skewed item popularity (5000 x 1025, 6000 x 1300, 8000 x 2100; printed as
`easeinv-measured` lines with numpy's fp32 inverse beside it)."""
import functools

import numpy as np
import pytest

import bpr_exact as bx
import ease_exact as ex
import knn_exact as kx

pytestmark = pytest.mark.gpu

F = np.float32
PAD = ex.PAD


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1, m.lib().mfx_last_error()
    return m


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(bits(got), bits(want))


def random_matrix(mfx, rows, cols, nnz, seed, values="normal"):
    rng = np.random.default_rng(seed)
    cells = rng.choice(rows * cols, nnz, replace=False)
    if values == "normal":
        v = rng.standard_normal(nnz).astype(F)
    elif values == "ratings":
        v = rng.integers(1, 6, nnz).astype(F)
    else:  # +-small integers: pairs that meet and cancel
        v = (rng.integers(1, 3, nnz) * (2 * rng.integers(0, 2, nnz) - 1)).astype(F)
    return mfx.dataset.from_coo(rows, cols, cells // cols, cells % cols, v)


def device_dict(X):
    import torch
    dev = torch.device("cuda", 0)
    d = {"rows": X.rows, "cols": X.cols}
    for k in ("csr_row_ptr", "csr_col_idx", "csc_col_ptr", "csc_row_idx"):
        d[k] = torch.from_numpy(getattr(X, k).view(np.int32)).to(dev)
    for k in ("csr_val", "csc_val"):
        d[k] = torch.from_numpy(getattr(X, k)).to(dev)
    return d


# ------------------------------------------------------------------------------------------------ Gram
@pytest.mark.parametrize("data", ["ones", "normal", "ratings", "cancel"])
def test_gram_small_matrices_and_two_lambdas(mfx, data):
    X = bx.small_matrix() if data == "ones" else random_matrix(mfx, 37, 29, 400, 21, data)
    for lam in (0.5, 37.25):
        want = ex.gram(X, lam)
        got = mfx.ease_gram(X, lam)
        assert same(got, want)
        assert same(got, np.ascontiguousarray(got.T))  # symmetric in bits
    assert not same(mfx.ease_gram(X, 0.5), mfx.ease_gram(X, 37.25))


@pytest.mark.parametrize("tile", [0, 64])
@pytest.mark.parametrize("cols", [63, 64, 65, 130, 300])
def test_gram_at_the_tile_edges(mfx, cols, tile):
    X = random_matrix(mfx, 50, cols, 12 * cols, 30 + cols, "normal")
    assert same(mfx.ease_gram(X, 2.0, tile_items=tile), ex.gram(X, 2.0))


def _without_column(mfx, X, c):
    r = np.repeat(np.arange(X.rows), np.diff(X.csr_row_ptr.astype(np.int64)))
    keep = X.csr_col_idx != c
    return mfx.dataset.from_coo(X.rows, X.cols, r[keep], X.csr_col_idx[keep], X.csr_val[keep])


@pytest.mark.parametrize("tile", [0, 64])
def test_gram_empty_column_long_column_and_long_row(mfx, tile):
    """200 x 300: item 0 is held by all 200 users (four waves' worth of column entries), user 0 holds all 300 items (a row of
    more than one batch of 64 x 4 entries), column 5 is empty."""
    rng = np.random.default_rng(44)
    D = (rng.random((200, 300)) < 0.04) * rng.integers(1, 6, (200, 300))
    D[:, 0] = rng.integers(1, 6, 200)
    D[0, :] = rng.integers(1, 6, 300)
    D[:, 5] = 0
    r, c = np.nonzero(D)
    X = mfx.dataset.from_coo(200, 300, r, c, D[r, c].astype(F))
    assert X.csc_col_ptr[1] == 200 and X.csr_row_ptr[1] == 299 and X.csc_col_ptr[5] == X.csc_col_ptr[6]
    got = mfx.ease_gram(X, 1.5, tile_items=tile)
    assert same(got, ex.gram(X, 1.5))
    assert got[5, 5] == F(1.5) and not np.delete(got[5], 5).any() and not np.delete(got[:, 5], 5).any()


def test_gram_takes_device_arrays_a_weighting_and_meets_item_knn(mfx):
    R = random_matrix(mfx, 70, 300, 3600, 51, "ratings")
    X = mfx.knn_weights(R, "bm25")
    want = ex.gram(X, 3.0)
    a = mfx.ease_gram(R, 3.0, weighting="bm25")
    b = mfx.ease_gram(X, 3.0)
    c = mfx.ease_gram(None, 3.0, device_arrays=device_dict(X))
    assert same(a, want) and same(b, want) and same(c.cpu().numpy(), want)
    ids, sims = kx.build(X, 25)  # the item-kNN reference: its similarities are the off-diagonal entries
    real = ids != PAD
    rows = np.repeat(np.arange(300)[:, None], 25, axis=1)
    assert real.sum() > 3000 and same(a[rows[real], ids[real].astype(np.int64)], sims[real])


def test_gram_names_the_item_of_a_bad_term(mfx):
    X = random_matrix(mfx, 37, 29, 400, 6, "ratings")
    u = int(np.argmax(np.diff(X.csr_row_ptr.astype(np.int64)) >= 3))

    def with_value(Y, pos, value):
        Y = Y.copy()
        e = int(Y.csr_row_ptr[u]) + pos
        item = int(Y.csr_col_idx[e])
        Y.csr_val[e] = value
        lo, hi = int(Y.csc_col_ptr[item]), int(Y.csc_col_ptr[item + 1])
        Y.csc_val[lo + int(np.nonzero(Y.csc_row_idx[lo:hi] == u)[0][0])] = value
        return Y
    pair = with_value(with_value(X, 1, 50.0), 2, 2.0)  # a pair's term of 100
    nan = with_value(X, 1, np.nan)
    diag = with_value(X, 2, 9.0)  # 81 on one diagonal alone: ratings up to 5 keep every pair below 64
    for bad in (pair, nan, diag):
        with pytest.raises(kx.BadTerm) as err:
            ex.gram(bad, 1.0)
        with pytest.raises(mfx.MfxError, match=f"item {err.value.item}:"):
            mfx.ease_gram(bad, 1.0)
        with pytest.raises(mfx.MfxError, match=f"item {err.value.item}:"):
            mfx.Ease(bad, 1.0)
    assert same(mfx.ease_gram(X, 1.0), ex.gram(X, 1.0))  # the same call on clean data is served


# ------------------------------------------------------------------------------------------------ inverse, n <= 1024
def _spd_cases():
    from test_gpu_spd_inverse import KS
    return [(k, ill) for k in KS for ill in (False, True) if not (ill and k == 1)]


@pytest.mark.parametrize("k,ill", _spd_cases())
def test_inverse_up_to_1024_has_the_bits_of_spd_inverse_on_both_paths(mfx, k, ill):
    from test_gpu_spd_inverse import matrix
    A, _ = matrix(k, ill)
    want = mfx.spd_inverse(A)
    assert same(mfx.ease_inverse(A), want), "grouped"
    assert same(mfx.ease_inverse(A, simple=True), want), "simple"


# ------------------------------------------------------------------------------------------------ inverse, n > 1024
BIG = {1025: 5000, 1300: 6000, 2100: 8000}  # n -> users


@functools.lru_cache(maxsize=None)
def binary_gram(n):
    """X^T X (fp32, exact integers) of a random binary users x n matrix whose item j is held with probability
    0.3 (j + 1)^-0.5: a skewed catalogue."""
    rng = np.random.default_rng(1000 + n)
    p = 0.3 * (np.arange(n) + 1.0) ** -0.5
    X = (rng.random((BIG[n], n)) < p[None, :]).astype(F)
    G = X.T @ X
    assert float(G.max()) < 2 ** 24 and np.array_equal(G, G.T)
    return G


@functools.lru_cache(maxsize=None)
def big_matrix(n, lam):
    """(A fp32 = X^T X + lambda I, cond_2 of A from its fp64 eigenvalues)."""
    A = binary_gram(n) + F(lam) * np.eye(n, dtype=F)
    ev = np.linalg.eigvalsh(A.astype(np.float64))
    assert ev[0] > 0
    return A, float(ev[-1] / ev[0])


def residual(A, X):
    return float(np.linalg.norm(np.eye(A.shape[0]) - A.astype(np.float64) @ X.astype(np.float64)))


@pytest.mark.parametrize("lam", [0.5, 100.0])
@pytest.mark.parametrize("n", [1025, 1300, 2100])
def test_inverse_above_1024_paths_agree_and_meet_the_bound(mfx, n, lam):
    A, cond = big_matrix(n, lam)
    X = mfx.ease_inverse(A)
    assert X.shape == (n, n) and X.dtype == F and np.isfinite(X).all()
    assert same(mfx.ease_inverse(A, simple=True), X)  # grouped equals simple in bits
    assert same(X, np.ascontiguousarray(X.T))  # exactly symmetric
    assert same(mfx.ease_inverse(A.copy()), X)  # the same bits on a second call
    got, bound = residual(A, X), n * 2.0 ** -24 * cond
    numpy32 = residual(A, np.linalg.inv(A))
    print(f"easeinv-measured n={n} lambda={lam} cond={cond:.4g} residual={got:.3e} bound={bound:.3e} share={got / bound:.4f} "
          f"numpy_fp32_inverse={numpy32:.3e} numpy_share={numpy32 / bound:.5f}")
    assert got <= bound, (n, lam, got, bound)


def test_inverse_of_a_block_diagonal_matrix_is_the_inverses_of_its_blocks(mfx):
    """704 + 601 rows; 704 is a multiple of 32, so the second block starts on a block edge.  The cross blocks of L, M and T are
    exact zeros and add nothing to any chain, so each diagonal block of the result has the values of mfx_spd_inverse of the
    block alone (np.array_equal on floats: -0 and +0 tie) and both off-diagonal blocks are all zero."""
    G = big_matrix(2100, 100.0)[0]
    A1, A2 = np.ascontiguousarray(G[:704, :704]), np.ascontiguousarray(G[704:1305, 704:1305])
    A = np.zeros((1305, 1305), F)
    A[:704, :704], A[704:, 704:] = A1, A2
    want1, want2 = mfx.spd_inverse(A1), mfx.spd_inverse(A2)
    for simple in (False, True):
        X = mfx.ease_inverse(A, simple=simple)
        assert np.array_equal(X[:704, :704], want1) and np.array_equal(X[704:, 704:], want2), simple
        assert not X[:704, 704:].any() and not X[704:, :704].any(), simple


def test_inverse_refuses_matrices_that_are_not_positive_definite(mfx):
    A = big_matrix(1300, 100.0)[0]
    neg = A.copy()
    neg[700, 700] = -5.0  # a negative diagonal entry: not positive definite
    nan = A.copy()
    nan[1299, 1299] = np.nan
    for bad in (neg, nan):
        for simple in (False, True):
            with pytest.raises(mfx.MfxError, match="not positive definite"):
                mfx.ease_inverse(bad, simple=simple)
    small = A[:40, :40].copy()
    small[3, 3] = -1.0
    with pytest.raises(mfx.MfxError, match="not positive definite"):
        mfx.ease_inverse(small)
    X = mfx.ease_inverse(A)  # ... and the next call is served
    assert residual(A, X) <= 1300 * 2.0 ** -24 * big_matrix(1300, 100.0)[1]


def test_inverse_takes_and_returns_device_tensors(mfx):
    import torch
    A = big_matrix(1025, 100.0)[0]
    X = mfx.ease_inverse(torch.from_numpy(A).cuda())
    assert X.is_cuda and same(X.cpu().numpy(), mfx.ease_inverse(A))


# ------------------------------------------------------------------------------------------------ weights
@pytest.mark.parametrize("n", [65, 300, 1300])
def test_weights_from_the_library_inverse_bit_for_bit(mfx, n):
    if n == 1300:
        G = big_matrix(1300, 100.0)[0]
    else:
        G = ex.gram(random_matrix(mfx, 50, n, 12 * n, 30 + n, "ratings"), 5.0)
    P = mfx.ease_inverse(G)
    B = mfx.ease_weights_from_inverse(P)
    assert same(B, ex.weights_from_inverse(P))
    assert not np.diagonal(B).any() and not np.signbit(np.diagonal(B)).any()


def test_weights_refuse_a_diagonal_that_is_not_positive(mfx):
    P = np.eye(6, dtype=F)
    for v in (0.0, -1.0, np.nan, np.inf):
        Q = P.copy()
        Q[4, 4] = v
        Q[5, 5] = v  # the smallest item is named
        with pytest.raises(mfx.MfxError, match="item 4:"):
            mfx.ease_weights_from_inverse(Q)
    B = mfx.ease_weights_from_inverse(P)  # (-0) / 1 off the diagonal, +0 on it
    assert same(B, ex.weights_from_inverse(P)) and not B.any() and not np.signbit(np.diagonal(B)).any()


@pytest.fixture(scope="module")
def trained(mfx):
    X = random_matrix(mfx, 70, 300, 3600, 51, "ratings")
    m = mfx.Ease(X, 20.0)
    yield m, X, m.weights()
    m.close()


def test_train_is_the_composition_of_the_three_steps(mfx, trained):
    m, X, B = trained
    G = mfx.ease_gram(X, 20.0)
    for simple in (False, True):
        want = mfx.ease_weights_from_inverse(mfx.ease_inverse(G, simple=simple))
        assert same(B, want)
        with mfx.Ease(X, 20.0, simple_inverse=simple, tile_items=64) as h:
            assert same(h.weights(), want)
        with mfx.Ease(None, 20.0, device_arrays=device_dict(X), simple_inverse=simple) as d:
            assert same(d.weights(), want)
    Xc = mfx.knn_weights(X, "cosine")
    with mfx.Ease(X, 0.5, weighting="cosine") as c:  # the values under a weighting
        assert same(c.weights(), mfx.ease_weights_from_inverse(mfx.ease_inverse(ex.gram(Xc, 0.5))))
    t = m.times()
    assert set(t) == {"train_checks", "gram_pass", "inverse", "weights", "recommend_checks", "recommend_pass"}
    assert t["gram_pass"] > 0 and t["inverse"] > 0 and t["weights"] > 0


def test_weights_slices_and_round_trip_through_from_weights(mfx, trained):
    import torch
    m, X, B = trained
    assert B.shape == (300, 300) and B.dtype == F
    assert same(m.weights(17, 40), B[17:57]) and same(m.weights(299), B[299:]) and m.weights(300).shape == (0, 300)
    for first, count in ((-1, 2), (0, 301), (300, 1), (5, -1)):
        with pytest.raises(mfx.MfxError):
            m.weights(first, count)
    rows = (X.csr_row_ptr, X.csr_col_idx, X.csr_val)
    want = m.recommend(rows, 10)
    for src in (B, torch.from_numpy(B).cuda()):
        with mfx.Ease.from_weights(src) as c:
            assert same(c.weights(), B)
            got = c.recommend(rows, 10)
            assert same(got[0], want[0]) and same(got[1], want[1])


def test_from_weights_refuses_a_non_zero_diagonal_and_a_nan(mfx):
    B = np.random.default_rng(5).standard_normal((40, 40)).astype(F)
    np.fill_diagonal(B, 0)
    for i, j, v in ((7, 7, 0.5), (9, 3, np.nan), (12, 30, np.inf)):
        C = B.copy()
        C[i, j] = v
        C[20, 20] = 1.0  # a later bad row: the first one is named
        with pytest.raises(mfx.MfxError, match=f"row {i}:"):
            mfx.Ease.from_weights(C)
    with mfx.Ease.from_weights(B) as c:
        assert same(c.weights(), B)


# ------------------------------------------------------------------------------------------------ recommend
@functools.lru_cache(maxsize=None)
def hand_made(cols):
    """B [cols][cols]: normal values; a third of the entries exact zeros; every seventh column negative; columns 3 and 10, 4
    and cols - 1 duplicated off the diagonal and rows 3, 10, 4, cols - 1 zeroed, so that their scores tie and the item id
    decides; the diagonal zero."""
    rng = np.random.default_rng(cols)
    B = rng.standard_normal((cols, cols)).astype(F)
    B[rng.random((cols, cols)) < 0.33] = 0
    B[:, ::7] = -np.abs(B[:, ::7])
    B[:, 10] = B[:, 3]
    B[:, cols - 1] = B[:, 4]
    B[[3, 10, 4, cols - 1], :] = 0
    np.fill_diagonal(B, 0)
    return B


def queries(cols, n, seed, bad_at=None):
    """n CSR rows: row 1 empty, row 2 names every item, row 3 has min(300, cols - 5) entries, the others 1 .. 12 entries with
    normal values; bad_at: a row with an infinite value."""
    rng = np.random.default_rng(seed)
    idx, val, ptr = [], [], [0]
    for r in range(n):
        k = 0 if r == 1 else cols if r == 2 else min(300, cols - 5) if r == 3 else int(rng.integers(1, 13))
        i = np.sort(rng.choice(cols, min(k, cols), replace=False))
        x = rng.standard_normal(len(i)).astype(F)
        if r == bad_at:
            x[len(x) // 2] = np.inf
        idx.append(i)
        val.append(x)
        ptr.append(ptr[-1] + len(i))
    return np.array(ptr, np.uint32), np.concatenate(idx).astype(np.uint32), np.concatenate(val).astype(F)


def check_recommend(m, B, rows, n_top, bad=0, **kw):
    want = ex.recommend(B, *rows, n_top, keep_seen=kw.get("keep_seen", False))
    got = m.recommend(rows, n_top, **kw)
    assert want[2] == bad and m.bad_rows == bad
    assert same(got[0], want[0]) and same(got[1], want[1])
    return got


@pytest.mark.parametrize("tile", [0, 64])
@pytest.mark.parametrize("cols", [63, 64, 65, 130, 300, 1300])
def test_recommend_at_the_tile_edges(mfx, cols, tile):
    B = hand_made(cols)
    rows = queries(cols, 24, 7 + cols, bad_at=6)
    with mfx.Ease.from_weights(B) as m:
        items, scores = check_recommend(m, B, rows, 10, bad=1, tile_items=tile)
        assert np.all(items[1] == PAD) and np.all(items[2] == PAD) and np.all(items[6] == PAD)  # empty, every item seen, bad
        assert np.all(scores[6] == -np.inf) and not np.any(items[5] == PAD) and not np.any(items[7] == PAD)
        items, _ = check_recommend(m, B, rows, 10, bad=1, tile_items=tile, keep_seen=True)
        assert np.all(items[1] == PAD) and not np.any(items[2] == PAD)
        assert (scores <= 0).any() and (scores > 0).any()  # zero and negative scores are candidates


@pytest.mark.parametrize("n_top", [1, 10, 1024])
def test_recommend_list_lengths_and_fewer_eligible_items_than_asked_for(mfx, n_top):
    for cols in (300, 1300):
        B = hand_made(cols)
        rows = queries(cols, 12, 90 + cols)
        with mfx.Ease.from_weights(B) as m:
            items, _ = check_recommend(m, B, rows, n_top)
            check_recommend(m, B, rows, n_top, tile_items=128)
            if n_top == 1024 and cols == 300:
                n = np.diff(rows[0].astype(np.int64))
                assert np.array_equal((items != PAD).sum(axis=1), np.where(n == 0, 0, 300 - n))  # every eligible item, then pads


@pytest.mark.parametrize("n", [1, 7, 300])
def test_recommend_rows_do_not_depend_on_the_batch(mfx, n):
    B = hand_made(130)
    rows = queries(130, 300, 5)
    ptr = rows[0]
    part = (ptr[:n + 1], rows[1][:ptr[n]], rows[2][:ptr[n]])
    with mfx.Ease.from_weights(B) as m:
        got = check_recommend(m, B, part, 10)
        full = m.recommend(rows, 10)
        assert same(full[0][:n], got[0]) and same(full[1][:n], got[1])


def test_recommend_more_rows_than_workgroups(mfx):
    """8 * CUs + 3 rows: the grid's stride loop takes every workgroup to a second row."""
    import torch
    n = 8 * torch.cuda.get_device_properties(0).multi_processor_count + 3
    B = hand_made(64)
    rng = np.random.default_rng(3)
    k = rng.integers(0, 4, n)
    ptr = np.concatenate([[0], np.cumsum(k)]).astype(np.uint32)
    idx = np.concatenate([np.sort(rng.choice(64, c, replace=False)) for c in k]).astype(np.uint32)
    val = rng.standard_normal(len(idx)).astype(F)
    with mfx.Ease.from_weights(B) as m:
        check_recommend(m, B, (ptr, idx, val), 5)


def test_recommend_tensors_in_tensors_out_and_bad_queries(mfx):
    import torch
    B = hand_made(300)
    rows = queries(300, 20, 77, bad_at=9)
    with mfx.Ease.from_weights(B) as m:
        want = check_recommend(m, B, rows, 10, bad=1)
        t = [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda() for a in rows]
        items, scores = m.recommend(tuple(t), 10)
        assert items.is_cuda and scores.is_cuda and m.bad_rows == 1
        assert same(items.cpu().numpy().view(np.uint32), want[0]) and same(scores.cpu().numpy(), want[1])
        items, scores = m.recommend(rows, 10, on_device=True)
        assert same(items.cpu().numpy().view(np.uint32), want[0]) and same(scores.cpu().numpy(), want[1])
        for kw in (dict(n_top=0), dict(n_top=1025), dict(n_top=5, tile_items=32)):
            with pytest.raises(mfx.MfxError):
                m.recommend(rows, **kw)
        d = rows[1].copy()
        d[rows[0][4]] = 300  # an id that is out of range
        with pytest.raises(mfx.MfxError, match="row 4:"):
            m.recommend((rows[0], d, rows[2]), 4)
        after = m.recommend(rows, 10)
        assert same(after[0], want[0]) and same(after[1], want[1])


# ------------------------------------------------------------------------------------------------ end to end
def test_planted_clusters_end_to_end(mfx):
    """Raw values, lambda = 100: the held-out item is in the top 10 for >= 90 % of the users (the reference alone reaches
    1.000, tests/test_ease_host.py), and for the first 200 users the top 10 are those of the reference on the library's B."""
    P = bx.planted_clusters()
    with mfx.Ease(P, 100.0) as m:
        items, scores = m.recommend(P, 10)
        assert m.bad_rows == 0
        hits = np.any(items == P.test_col[np.argsort(P.test_row)][:, None], axis=1)
        print("HR@10", hits.mean())
        assert hits.shape == (P.rows,) and hits.mean() >= 0.9, hits.mean()
        ptr = P.csr_row_ptr[:201]
        want = ex.recommend(m.weights(), ptr, P.csr_col_idx[:ptr[200]], P.csr_val[:ptr[200]], 10)
        assert np.array_equal(items[:200], want[0]) and same(scores[:200], want[1])
