"""GPU tests of SLIM on given supports (mfx_slim_*) against the exact reference of tests/slim_exact.py.  Every comparison is
on the uint32 views of the Gram blocks, the weights, the ids and the scores: the contract of include/mfx.h fixes each fp32
operation and every sum is an integer sum, so there is nothing to tolerate."""
import numpy as np
import pytest

import bpr_exact as bx
import knn_exact as kx
import slim_exact as sx

pytestmark = pytest.mark.gpu

F = np.float32
PAD = sx.PAD


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1
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


def random_support(cols, K, seed, pads=True, among=None):
    """Distinct ids (of `among`, default every item) that are not the item itself; with pads: lists of every length 0 .. K."""
    rng = np.random.default_rng(seed)
    among = np.arange(cols) if among is None else np.asarray(among)
    S = np.full((cols, K), PAD, np.uint32)
    for j in range(cols):
        pool = np.setdiff1d(among, [j])
        n = min(len(pool), int(rng.integers(0, K + 1)) if pads else K)
        S[j, :n] = rng.permutation(pool)[:n]
    return S


def knn_support(sums, K):
    """The kNN lists of the integer sums (the diagonal set aside)."""
    Z = sums.copy()
    np.fill_diagonal(Z, 0)
    return kx.top_lists(Z, K)[0]


_DATA = {}


def data_of(name, make):
    """The matrix `name` and the reference's integer Gram sums of it, computed once for the module."""
    if name not in _DATA:
        X = make()
        _DATA[name] = (X, sx.gram_sums(X))
    return _DATA[name]


def check_gram(mfx, name, make, S, tile=0):
    X, sums = data_of(name, make)
    want = sx.gram_blocks(X, S, sums)
    got = mfx.slim_gram(X, S.shape[1], S, tile_items=tile)
    assert same(got, want), (name, S.shape[1], tile, int((bits(got) != bits(want)).sum()))
    return X, want


# ------------------------------------------------------------------------------------------------ Gram
def _small(mfx, kind):
    if kind == "ones":
        return bx.small_matrix
    if kind == "cosine":
        return lambda: mfx.knn_weights(random_matrix(mfx, 37, 29, 400, 21, "ratings"), "cosine")
    return lambda: random_matrix(mfx, 37, 29, 400, 21, kind)


@pytest.mark.parametrize("K", [1, 3, 28])
@pytest.mark.parametrize("data", ["ones", "ratings", "cancel", "cosine"])
def test_gram_bit_for_bit(mfx, data, K):
    """60 x 40 all ones and 37 x 29 in three kinds of values; the kNN lists of the matrix, full random lists, and random
    lists with pads of which one is all pads."""
    make = _small(mfx, data)
    X, sums = data_of(data, make)
    check_gram(mfx, data, make, knn_support(sums, K))
    check_gram(mfx, data, make, random_support(X.cols, K, 5 + K, pads=False))
    S = random_support(X.cols, K, 6 + K)
    S[7, :] = PAD
    X, want = check_gram(mfx, data, make, S)
    assert not want[7].any()
    if data == "cancel":
        off = sums.copy()
        np.fill_diagonal(off, 0)
        assert (off == 0).sum() > 0 and np.all(np.diag(sums) > 0)


@pytest.mark.parametrize("cols", [63, 64, 65, 130, 300])
def test_gram_across_tile_boundaries(mfx, cols):
    """One tile (automatic) and tiles of 64, with supports that straddle them: the same bits, the reference's."""
    make = lambda: random_matrix(mfx, 70, cols, 12 * cols, 100 + cols)
    S = random_support(cols, 10, cols)
    for tile in (0, 64):
        check_gram(mfx, f"tiles{cols}", make, S, tile)


def _hub_support(cols=700):
    """K = 3: item 0 is in every other list (an inverse list wider than a workgroup), item cols - 1 in none."""
    S = random_support(cols, 3, 41, pads=False, among=np.arange(1, cols - 1))
    S[1:, 0] = 0
    if 5 not in S[10]:
        S[10, 1] = 5  # (the item whose column _hub_matrix leaves empty is in a list)
    return S


def _hub_matrix(mfx):
    X = random_matrix(mfx, 50, 700, 5000, 42, "ratings")
    r = np.repeat(np.arange(X.rows), np.diff(X.csr_row_ptr.astype(np.int64)))
    keep = X.csr_col_idx != 5  # column 5 is empty
    return mfx.dataset.from_coo(X.rows, X.cols, r[keep], X.csr_col_idx[keep], X.csr_val[keep])


@pytest.mark.parametrize("tile", [0, 64])
def test_gram_hub_item_unused_item_and_empty_column(mfx, tile):
    S = _hub_support()
    assert np.all(S[1:, 0] == 0) and not np.any(S == 699) and np.any(S == 5)
    X, want = check_gram(mfx, "hub", lambda: _hub_matrix(mfx), S, tile)
    assert X.csc_col_ptr[5] == X.csc_col_ptr[6]
    j, p = np.argwhere(S == 5)[0]
    assert not want[j, p, :].any() and not want[j, :, p].any()  # the empty column: zeros, its diagonal included


def test_gram_widest_support(mfx):
    """K = 128 at 130 items: every list holds all but one of the other items."""
    make = lambda: random_matrix(mfx, 40, 130, 1500, 43)
    check_gram(mfx, "wide", make, random_support(130, 128, 44, pads=False))


def _full_lines(mfx):
    """200 x 300: column 2 is held by every row and row 4 holds every column."""
    X = random_matrix(mfx, 200, 300, 3000, 45)
    D = np.zeros((X.rows, X.cols), F)
    D[np.repeat(np.arange(X.rows), np.diff(X.csr_row_ptr.astype(np.int64))), X.csr_col_idx] = X.csr_val
    rng = np.random.default_rng(46)
    D[:, 2] = rng.standard_normal(X.rows).astype(F) * F(0.25) + F(1.0)
    D[4, :] = rng.standard_normal(X.cols).astype(F) * F(0.25) + F(1.0)
    rr, cc = np.nonzero(D)
    return mfx.dataset.from_coo(X.rows, X.cols, rr, cc, D[rr, cc])


def test_gram_full_column_and_full_row(mfx):
    X, _ = check_gram(mfx, "full", lambda: _full_lines(mfx), random_support(300, 5, 47))
    assert np.diff(X.csc_col_ptr.astype(np.int64))[2] == 200 and np.diff(X.csr_row_ptr.astype(np.int64))[4] == 300


def _device_dict(X):
    import torch
    dev = torch.device("cuda", 0)
    d = {"rows": X.rows, "cols": X.cols}
    for k in ("csr_row_ptr", "csr_col_idx", "csc_col_ptr", "csc_row_idx"):
        d[k] = torch.from_numpy(getattr(X, k).view(np.int32)).to(dev)
    for k in ("csr_val", "csc_val"):
        d[k] = torch.from_numpy(getattr(X, k)).to(dev)
    return d


def test_gram_is_reproducible_takes_device_arrays_and_meets_item_knn(mfx):
    import torch
    X = mfx.knn_weights(random_matrix(mfx, 70, 300, 3600, 51, "ratings"), "bm25")
    with mfx.ItemKnn(X, 20, None) as nn:
        ids, sims = nn.lists()
        a = mfx.slim_gram(X, 20, ids)
        b = mfx.slim_gram(X, 20, nn)  # the handle itself as the support
        c = mfx.slim_gram(None, 20, nn, device_arrays=_device_dict(X))
        d = mfx.slim_gram(None, 20, torch.from_numpy(ids.view(np.int32)).cuda(), device_arrays=_device_dict(X))
    assert same(a, b) and same(c.cpu().numpy(), a) and same(d.cpu().numpy(), a)
    real = ids != PAD
    assert same(a[:, 20, :][real], sims[real]) and np.all(a[:, 20, :][~real] == 0)  # row K is nbr_sim
    assert same(a[:, :20, :], np.ascontiguousarray(a[:, :20, :].transpose(0, 2, 1)))  # symmetric in bits


def _set(X, u, pos, value):
    """X with the value of the pos-th entry of row u replaced, on both sides."""
    Y = X.copy()
    e = int(Y.csr_row_ptr[u]) + pos
    item = int(Y.csr_col_idx[e])
    Y.csr_val[e] = value
    c0, c1 = int(Y.csc_col_ptr[item]), int(Y.csc_col_ptr[item + 1])
    Y.csc_val[c0 + int(np.nonzero(Y.csc_row_idx[c0:c1] == u)[0][0])] = value
    return Y, item


def test_gram_refuses_bad_terms_and_names_the_item(mfx):
    X = random_matrix(mfx, 37, 29, 400, 61, "ratings")
    S = random_support(29, 4, 62)
    u = int(np.argmax(np.diff(X.csr_row_ptr.astype(np.int64)) >= 3))
    Y, _ = _set(X, u, 1, 50.0)
    Y, _ = _set(Y, u, 2, 2.0)  # the pair's term is 100 (and 50 * 50 on a diagonal)
    Z, _ = _set(X, u, 1, np.nan)
    W, item9 = _set(X, u, 2, 9.0)  # 81 on one diagonal alone: ratings up to 5 keep every pair below 64
    for bad in (Y, Z, W):
        with pytest.raises(kx.BadTerm) as err:
            sx.gram_blocks(bad, S)
        with pytest.raises(mfx.MfxError, match=f"item {err.value.item}:"):
            mfx.slim_gram(bad, 4, S)
        with pytest.raises(mfx.MfxError, match=f"item {err.value.item}:"):
            mfx.Slim(bad, 4, support=S)
    assert err.value.item == item9
    assert mfx.slim_gram(X, 4, S).shape == (29, 5, 4)  # the same call on clean data succeeds


def test_refuses_bad_supports_and_names_the_item(mfx):
    X = random_matrix(mfx, 37, 29, 400, 61, "ratings")
    S = random_support(29, 4, 63, pads=False)
    w = np.ones(S.shape, F)
    for item, slot, ident in ((5, 1, 5), (5, 2, None), (3, 0, 29), (7, 1, PAD)):  # itself, a duplicate, >= cols, a pad in the middle
        T = S.copy()
        T[9, 0] = 9  # a later bad item: the smallest one is named
        T[item, slot] = T[item, 0] if ident is None else ident
        with pytest.raises(sx.BadSupport) as err:
            sx.gram_blocks(X, T)
        assert err.value.item == item
        for call in (lambda: mfx.slim_gram(X, 4, T), lambda: mfx.Slim(X, 4, support=T), lambda: mfx.Slim.from_lists(T, w)):
            with pytest.raises(mfx.MfxError, match=f"item {item}:"):
                call()
    v = w.copy()
    v[11, 2] = np.inf
    with pytest.raises(mfx.MfxError, match="item 11:"):
        mfx.Slim.from_lists(S, v)


# ------------------------------------------------------------------------------------------------ solve
def psd_blocks(N, K, seed, rows=40):
    """N random blocks: G = A^T A of a rows x K matrix (symmetric in bits), g = A^T y."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((N, rows, K)) * 0.5
    y = rng.standard_normal((N, rows)) * 0.5 + A[:, :, : max(1, K // 3)].sum(axis=2)
    B = np.zeros((N, K + 1, K), F)
    B[:, :K, :] = np.einsum("nrk,nrl->nkl", A, A).astype(F)
    B[:, :K, :] = 0.5 * (B[:, :K, :] + B[:, :K, :].transpose(0, 2, 1))
    B[:, K, :] = np.einsum("nrk,nr->nk", A, y).astype(F)
    return B


def check_solve(mfx, B, n_real, **kw):
    want = sx.solve(B, n_real, **kw)
    got = mfx.slim_solve(B, n_real, **kw)
    assert got[0].dtype == F and got[1].dtype == np.int32
    assert same(got[0], want[0]), (kw, int((bits(got[0]) != bits(want[0])).sum()))
    assert np.array_equal(got[1], want[1]) and got[2] == want[2]
    return want


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 127, 128])
def test_solve_bit_for_bit(mfx, K, signed):
    """Hand-made blocks at every K where the lanes' ownership changes, with real-slot counts 0 .. K (beyond them the blocks
    hold values that must not be read), with and without l2."""
    B = psd_blocks(7, K, 200 + K)
    n_real = np.array([K, K - 1, 0, K // 2, max(K - 2, 0), 1, K], np.uint32)
    for l1, l2 in ((0.25, 2.0), (0.0, 0.0)):
        w, used, failed = check_solve(mfx, B, n_real, l1=l1, l2=l2, sweeps=4, tol=0.0, signed=signed)
        assert failed == 0 and (K < 63 or w[0].any())
        for n in range(7):
            assert not w[n, n_real[n]:].any()
    check_solve(mfx, B, None, l1=0.25, l2=2.0, sweeps=4, tol=0.0, signed=signed)
    if signed and K > 2:
        assert (sx.solve(B, None, 0.0, 2.0, 4, 0.0, True)[0] < 0).any()


@pytest.mark.parametrize("K", [4, 65])
def test_solve_skips_a_zero_diagonal(mfx, K):
    B = psd_blocks(3, K, 300 + K)
    B[1, 2, :] = 0
    B[1, :K, 2] = 0
    B[1, K, 2] = 0.75  # d = 0 with l2 = 0: den is not > 0, the coordinate is never visited
    w, used, failed = check_solve(mfx, B, None, l1=0.0, l2=0.0, sweeps=3, tol=0.0, signed=True)
    assert failed == 0 and w[1, 2] == 0 and w[1, 1] != 0 and w[0, 2] != 0


def test_solve_one_sweep_and_per_item_stopping(mfx):
    B = psd_blocks(40, 20, 400)
    w, used, _ = check_solve(mfx, B, None, l1=0.1, l2=1.0, sweeps=1, tol=0.0)
    assert np.all(used == 1)
    w, used, _ = check_solve(mfx, B, None, l1=0.1, l2=1.0, sweeps=60, tol=1e-3)
    assert len(np.unique(used)) >= 2 and used.max() < 60  # the items stop on their own, after different counts
    w, used, _ = check_solve(mfx, B, None, l1=1e6, l2=1.0, sweeps=5, tol=0.0)
    assert not w.any() and np.all(used == 1)


def test_solve_more_items_than_waves(mfx):
    """8 * CUs * 8 + 3 items: the grid's stride loop takes every wave to a second item, three to a third."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N = 8 * cus * 8 + 3
    B = psd_blocks(N, 4, 500, rows=8)
    n_real = (np.arange(N) % 5).astype(np.uint32)
    w, used, failed = check_solve(mfx, B, n_real, l1=0.05, l2=0.5, sweeps=3, tol=0.0)
    assert failed == 0 and not w[n_real == 0].any() and w[N - 3:].any()


@pytest.mark.parametrize("K", [5, 70])
def test_solve_counts_a_block_with_an_infinity(mfx, K):
    B = psd_blocks(5, K, 600 + K)
    clean = check_solve(mfx, B, None, l1=0.1, l2=1.0, sweeps=3, tol=0.0)
    B[2, K, 0] = np.inf
    w, used, failed = check_solve(mfx, B, None, l1=0.1, l2=1.0, sweeps=3, tol=0.0)
    assert failed == 1 and not w[2].any() and used[2] == 0
    keep = np.arange(5) != 2
    assert same(w[keep], clean[0][keep]) and np.array_equal(used[keep], clean[1][keep])


# ------------------------------------------------------------------------------------------------ train and model
@pytest.fixture(scope="module")
def trained(mfx):
    """37 x 29 ratings, the cosine kNN support at K = 5, signed weights: the model and the reference's."""
    X = random_matrix(mfx, 37, 29, 400, 21, "ratings")
    m = mfx.Slim(X, 5, l1=0.5, l2=2.0, sweeps=6, signed=True)
    S, w = m.weights()
    yield m, X, S, w
    m.close()


def test_train_equals_gram_solve_and_transpose_of_the_reference(mfx, trained):
    m, X, S, w = trained
    ids = kx.build(mfx.knn_weights(X, "cosine"), 5)[0]
    assert same(S, ids)  # the default support: the ids of ItemKnn(R, K, "cosine")
    want_w, want_used, failed = sx.train(X, S, 0.5, 2.0, 6, 0.0, True)
    assert same(w, want_w) and np.array_equal(m.sweeps_used, want_used) and m.failed == failed == 0
    assert (w < 0).any() and (w > 0).any()
    t = m.times()
    assert t["train_checks"] > 0 and t["gram_pass"] > 0 and t["solve"] > 0 and t["recommend_pass"] == 0
    for tile in (0, 64):
        with mfx.Slim(X, 5, l1=0.5, l2=2.0, sweeps=6, signed=True, support=S, tile_items=tile) as again:
            assert same(again.weights()[1], w)
    with mfx.Slim(None, 5, l1=0.5, l2=2.0, sweeps=6, signed=True, support=S, device_arrays=_device_dict(X)) as dev:
        assert same(dev.weights()[1], w) and same(dev.weights()[0], S)
    Xc = mfx.knn_weights(X, "cosine")
    with mfx.Slim(X, 5, l1=0.01, l2=0.1, sweeps=4, weighting="cosine", support=S) as c:  # the values under a weighting
        assert same(c.weights()[1], sx.train(Xc, S, 0.01, 0.1, 4, 0.0, False)[0])
    rows = (X.csr_row_ptr, X.csr_col_idx, X.csr_val)
    check_recommend(m, (S, w), rows, 10)


def test_weights_round_trip_through_from_lists(mfx, trained):
    import torch
    m, X, S, w = trained
    with mfx.Slim.from_lists(S, w) as c:
        assert same(c.weights()[0], S) and same(c.weights()[1], w) and not c.sweeps_used.any()
        assert c.cols == 29 and c.K == 5
    with mfx.Slim.from_lists(torch.from_numpy(S.view(np.int32)).cuda(), torch.from_numpy(w).cuda()) as c:
        assert same(c.weights()[0], S) and same(c.weights()[1], w)


# ------------------------------------------------------------------------------------------------ recommend
def random_rows(cols, n, seed, max_len=12):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, n)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    idx = np.concatenate([np.sort(rng.choice(cols, k, replace=False)) for k in lens] + [np.zeros(0, np.int64)]).astype(np.uint32)
    val = rng.standard_normal(idx.size).astype(F)
    return ptr, idx, val


def check_recommend(m, model, rows, n_top, keep_seen=False, tile=0, bad=0):
    want = sx.recommend(model[0], model[1], *rows, n_top, keep_seen)
    got = m.recommend(rows, n_top, keep_seen=keep_seen, tile_items=tile)
    assert got[0].dtype == np.uint32 and got[1].dtype == F
    assert same(got[0], want[0]) and same(got[1], want[1]), (n_top, keep_seen, tile, int((bits(got[0]) != bits(want[0])).sum()))
    assert m.bad_rows == want[2] == bad
    return want


@pytest.fixture(scope="module")
def handmade(mfx):
    """50 items, K = 6, random lists with pads and random weights of both signs; items 1 and 49 are in no list."""
    S = random_support(50, 6, 71, among=np.arange(2, 49))
    S[3, :] = PAD
    w = np.where(S != PAD, np.random.default_rng(72).standard_normal(S.shape), 0).astype(F)
    m = mfx.Slim.from_lists(S, w)
    yield m, (S, w)
    m.close()


@pytest.mark.parametrize("keep_seen", [False, True])
@pytest.mark.parametrize("n_top", [1, 10, 1024])
def test_recommend_on_a_trained_model(mfx, trained, n_top, keep_seen):
    m, X, S, w = trained
    rows = (X.csr_row_ptr, X.csr_col_idx, X.csr_val)
    want = check_recommend(m, (S, w), rows, n_top, keep_seen)
    if n_top == 1024:
        assert np.all(want[0][:, 29:] == PAD)
    got_rd = m.recommend(X, n_top, keep_seen=keep_seen)  # a RatingData is its CSR side
    assert same(got_rd[0], want[0]) and same(got_rd[1], want[1])
    if not keep_seen:
        for u in range(X.rows):
            assert not np.intersect1d(want[0][u], X.csr_col_idx[X.csr_row_ptr[u]:X.csr_row_ptr[u + 1]]).size


@pytest.mark.parametrize("keep_seen", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_recommend_on_handmade_weights_in_batches(mfx, handmade, n, keep_seen):
    m, model = handmade
    ptr, idx, val = random_rows(50, 300, 81)
    rows = (ptr[:n + 1], idx[:ptr[n]], val[:ptr[n]])
    for n_top in (1, 10):
        check_recommend(m, model, rows, n_top, keep_seen)


def test_recommend_rows_alone_on_the_device_and_as_item_knn(mfx, handmade):
    import torch
    m, model = handmade
    ptr, idx, val = random_rows(50, 40, 82)
    want = check_recommend(m, model, (ptr, idx, val), 10)
    for u in (0, 17, 39):
        one = (np.array([0, ptr[u + 1] - ptr[u]], np.uint32), idx[ptr[u]:ptr[u + 1]], val[ptr[u]:ptr[u + 1]])
        got = m.recommend(one, 10)
        assert same(got[0], want[0][u:u + 1]) and same(got[1], want[1][u:u + 1])
    t = [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda() for a in (ptr, idx, val)]
    gi, gs = m.recommend(tuple(t), 10)
    assert same(gi.cpu().numpy().view(np.uint32), want[0]) and same(gs.cpu().numpy(), want[1])
    t0 = m.times()
    assert t0["recommend_pass"] > 0 and t0["recommend_checks"] > 0
    lists = sx.transposed_lists(*model)  # the transpose as neighbour lists: the same sums through item-kNN
    assert lists[0].shape[1] <= 1024
    with mfx.ItemKnn.from_lists(*lists) as nn:
        for keep_seen in (False, True):
            a = nn.recommend((ptr, idx, val), 10, keep_seen=keep_seen)
            b = m.recommend((ptr, idx, val), 10, keep_seen=keep_seen)
            assert same(a[0], b[0]) and same(a[1], b[1])


def test_recommend_empty_rows_and_sources_without_targets(mfx, handmade):
    m, (S, w) = handmade
    assert not np.any(S == 1) and not np.any(S == 49)
    ptr = np.array([0, 0, 2, 2, 5], np.uint32)  # empty, two items that are in no list, empty, an ordinary row
    idx = np.array([1, 49, 2, 4, 30], np.uint32)
    val = np.array([1, 2, 0.5, -1, 3], F)
    want = check_recommend(m, (S, w), (ptr, idx, val), 10)
    assert np.all(want[0][:3] == PAD) and np.all(np.isneginf(want[1][:3])) and want[0][3, 0] != PAD
    only_empty = (np.array([0, 0], np.uint32), np.zeros(0, np.uint32), np.zeros(0, F))
    got = m.recommend(only_empty, 3)
    assert np.all(got[0] == PAD) and np.all(np.isneginf(got[1])) and got[0].shape == (1, 3)


def test_recommend_bad_row_between_good_ones(mfx, handmade):
    m, (S, w) = handmade
    ptr, idx, val = random_rows(50, 9, 83)
    good = check_recommend(m, (S, w), (ptr, idx, val), 10)
    iptr, tj, tw = sx.transpose(S, w)
    u = 4
    src = idx[ptr[u]:ptr[u + 1]]
    has = np.nonzero(iptr[src.astype(np.int64) + 1] > iptr[src.astype(np.int64)])[0]
    assert has.size
    e = int(ptr[u]) + int(has[0])
    first = tw[iptr[idx[e]]]
    assert first != 0
    v = val.copy()
    v[e] = F(65.0) / np.abs(first)  # the term with the source's first target has magnitude >= 64
    want = check_recommend(m, (S, w), (ptr, idx, v), 10, bad=1)
    assert np.all(want[0][u] == PAD) and np.all(np.isneginf(want[1][u]))
    keep = np.arange(9) != u
    assert same(want[0][keep], good[0][keep]) and same(want[1][keep], good[1][keep])
    v[e] = np.nan
    check_recommend(m, (S, w), (ptr, idx, v), 10, bad=1)
    check_recommend(m, (S, w), (ptr, idx, val), 10)  # and the handle is as before


@pytest.mark.parametrize("n_top", [10, 1024])
def test_recommend_across_tiles_with_a_source_of_many_targets(mfx, n_top):
    """700 items, item 0 in 699 lists (a source list of several rounds of a wave), tiles of 64 and automatic."""
    S = _hub_support()
    w = np.random.default_rng(91).standard_normal(S.shape).astype(F)
    ptr, idx, val = random_rows(700, 30, 92, max_len=20)
    idx[ptr[3]] = 0  # (rows are sorted: the first entry may become item 0)
    assert ptr[4] > ptr[3] and sx.transpose(S, w)[0][1] == 699
    with mfx.Slim.from_lists(S, w) as m:
        for keep_seen in (False, True):
            a = check_recommend(m, (S, w), (ptr, idx, val), n_top, keep_seen, tile=0)
            b = check_recommend(m, (S, w), (ptr, idx, val), n_top, keep_seen, tile=64)
            assert same(a[0], b[0]) and same(a[1], b[1])


def test_recommend_refusals_leave_the_handle_usable(mfx, handmade):
    m, model = handmade
    ptr, idx, val = random_rows(50, 5, 84)
    before = m.recommend((ptr, idx, val), 4)
    for kw in (dict(n_top=0), dict(n_top=1025), dict(n_top=4, tile_items=32), dict(n_top=4, tile_items=8256), dict(n_top=600, tile_items=8192)):
        with pytest.raises(mfx.MfxError):
            m.recommend((ptr, idx, val), **kw)
    assert ptr[3] - ptr[2] >= 2
    d = idx.copy()
    d[ptr[2]:ptr[3]] = idx[ptr[2]:ptr[3]][::-1]
    with pytest.raises(mfx.MfxError, match="row 2:"):
        m.recommend((ptr, d, val), 4)
    after = m.recommend((ptr, idx, val), 4)
    assert same(after[0], before[0]) and same(after[1], before[1])


# ------------------------------------------------------------------------------------------------ end to end
def test_planted_clusters_end_to_end(mfx):
    """Raw values, the default support (cosine kNN at K = 20), l1 = 1, l2 = 10, 10 sweeps, tol = 0."""
    P = bx.planted_clusters()
    with mfx.Slim(P, 20, l1=1.0, l2=10.0, sweeps=10, tol=0.0) as m:
        items, scores = m.recommend(P, 10)
        assert m.bad_rows == 0 and m.failed == 0
        S, w = m.weights()
    assert np.all(w >= 0) and w.any()
    met = mfx.topn_metrics(items, P)
    assert met["users"] == P.rows
    print("HR@10", met["hr"])
    assert met["hr"] >= 0.9, met
