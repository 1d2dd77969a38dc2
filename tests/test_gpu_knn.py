"""GPU tests of the item-kNN model (mfx_knn_*) against the exact reference of tests/knn_exact.py.  Every comparison is on
the uint32 views of ids and similarities or scores: the contract of include/mfx.h fixes each fp32 operation and every sum is
an integer sum, so there is nothing to tolerate."""
import ctypes as C

import numpy as np
import pytest

import bpr_exact as bx
import knn_exact as kx

pytestmark = pytest.mark.gpu

MFX_ERR_INVALID = -1  # include/mfx.h
F = np.float32
PAD = kx.PAD


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1
    return m


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want):
    """(ids, values) pairs equal in every bit."""
    return all(g.shape == w.shape and np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


def random_matrix(mfx, rows, cols, nnz, seed, values="normal"):
    rng = np.random.default_rng(seed)
    cells = rng.choice(rows * cols, nnz, replace=False)
    if values == "normal":
        v = rng.standard_normal(nnz).astype(F)
    elif values == "ratings":
        v = rng.integers(1, 6, nnz).astype(F)
    elif values == "signs":
        v = (2 * rng.integers(0, 2, nnz) - 1).astype(F)
    else:
        v = np.ones(nnz, F)
    return mfx.dataset.from_coo(rows, cols, cells // cols, cells % cols, v)


_SUMS = {}


def sums_of(name, make):
    """The matrix `name` and the reference's integer sums of it, computed once for the module."""
    if name not in _SUMS:
        X = make()
        _SUMS[name] = (X, kx.similarities(X))
    return _SUMS[name]


def check_build(mfx, name, make, K, tile=0):
    X, S = sums_of(name, make)
    want = kx.top_lists(S, K)
    with mfx.ItemKnn(X, K, None, tile_items=tile) as m:
        got = m.lists()
    assert got[0].dtype == np.uint32 and got[1].dtype == F
    assert same(got, want), (name, K, tile, int((bits(got[0]) != bits(want[0])).sum()), int((bits(got[1]) != bits(want[1])).sum()))
    return X, want


# ------------------------------------------------------------------------------------------------ build
def _weighted(mfx, scheme):
    return lambda: mfx.knn_weights(random_matrix(mfx, 37, 29, 400, 21, "ratings"), scheme)


@pytest.mark.parametrize("K", [1, 3, 20, 28, 64])
@pytest.mark.parametrize("data", ["ones", "cosine", "tfidf", "bm25"])
def test_build_bit_for_bit(mfx, data, K):
    """60 x 40 all ones: massive ties, the item order decides.  37 x 29 in the three weightings.  K = 64 > cols - 1: pads."""
    make = bx.small_matrix if data == "ones" else _weighted(mfx, data)
    X, want = check_build(mfx, data, make, K)
    if K == 64:
        assert np.all(want[0][:, X.cols - 1:] == PAD) and np.all(np.isneginf(want[1][:, X.cols - 1:]))
    if data == "ones":
        ties = (want[1][:, :-1] == want[1][:, 1:]) & (want[0][:, 1:] != PAD)
        assert K == 1 or (ties.any() and np.all(want[0][:, :-1][ties] < want[0][:, 1:][ties]))


@pytest.mark.parametrize("cols", [63, 64, 65, 130, 300])
def test_build_across_tile_boundaries(mfx, cols):
    """One tile (automatic) and tiles of 64: the same bits, the reference's."""
    make = lambda: random_matrix(mfx, 70, cols, 12 * cols, 100 + cols)
    for tile in (0, 64):
        check_build(mfx, f"tiles{cols}", make, 10, tile)


def _holes(mfx):
    """+-1 values, column 3 and row 5 empty."""
    X = random_matrix(mfx, 30, 14, 200, 31, "signs")
    r = np.repeat(np.arange(X.rows), np.diff(X.csr_row_ptr.astype(np.int64)))
    keep = (r != 5) & (X.csr_col_idx != 3)
    return mfx.dataset.from_coo(X.rows, X.cols, r[keep], X.csr_col_idx[keep], X.csr_val[keep])


def _full_lines(mfx):
    """Column 2 is held by every row and row 4 holds every column."""
    X = random_matrix(mfx, 30, 14, 150, 32)
    D = np.zeros((X.rows, X.cols), F)
    r = np.repeat(np.arange(X.rows), np.diff(X.csr_row_ptr.astype(np.int64)))
    D[r, X.csr_col_idx] = X.csr_val
    rng = np.random.default_rng(33)
    D[:, 2] = rng.standard_normal(X.rows).astype(F) + F(3.0)
    D[4, :] = rng.standard_normal(X.cols).astype(F) + F(3.0)
    rr, cc = np.nonzero(D)
    return mfx.dataset.from_coo(X.rows, X.cols, rr, cc, D[rr, cc])


@pytest.mark.parametrize("K", [4, 13])
def test_build_edge_shapes(mfx, K):
    X, want = check_build(mfx, "holes", lambda: _holes(mfx), K)
    assert np.all(want[0][3] == PAD) and not np.any(want[0] == 3)  # the empty column has no neighbours and is nobody's
    S = _SUMS["holes"][1]
    co = (np.abs(_dense(X)).T @ np.abs(_dense(X))).astype(np.int64)
    np.fill_diagonal(co, 0)
    cancelled = (S == 0) & (co > 0)
    assert cancelled.any()  # pairs that meet but whose +-1 terms cancel: not neighbours
    i, j = np.argwhere(cancelled)[0]
    assert j not in want[0][i]
    X2, want2 = check_build(mfx, "full", lambda: _full_lines(mfx), K)
    assert np.all(np.diff(X2.csc_col_ptr.astype(np.int64))[2] == X2.rows) and np.diff(X2.csr_row_ptr.astype(np.int64))[4] == X2.cols
    assert not np.any(want2[0][:, 0] == PAD)  # through row 4 every item meets every other


def _dense(X):
    D = np.zeros((X.rows, X.cols), np.float64)
    D[np.repeat(np.arange(X.rows), np.diff(X.csr_row_ptr.astype(np.int64))), X.csr_col_idx] = X.csr_val
    return D


@pytest.mark.parametrize("tile", [0, 64])
def test_build_maximal_tied_lists(mfx, tile):
    """8 x 1 100 all ones, K = 1024: 1 099 neighbours of one similarity per item, kept by ascending id."""
    make = lambda: mfx.dataset.from_coo(8, 1100, np.repeat(np.arange(8), 1100), np.tile(np.arange(1100), 8), np.ones(8800, F))
    X, want = check_build(mfx, "tied", make, 1024, tile)
    assert np.all(want[1] == 8.0)
    assert np.array_equal(want[0][0], np.arange(1, 1025)) and np.array_equal(want[0][1099], np.arange(0, 1024))


@pytest.mark.parametrize("K", [5, 1024])
def test_build_merges_when_the_candidate_area_fills(mfx, K):
    """3 x 2 600, values 1..3: every item has 2 599 candidates, more than the candidate area holds (1 024 / 2 048 slots), so
    list and candidates are merged several times on the way."""
    def make():
        rng = np.random.default_rng(41)
        return mfx.dataset.from_coo(3, 2600, np.repeat(np.arange(3), 2600), np.tile(np.arange(2600), 3), rng.integers(1, 4, 7800).astype(F))
    check_build(mfx, "merges", make, K)


def test_build_is_reproducible_and_takes_device_arrays(mfx):
    import torch
    X = mfx.knn_weights(random_matrix(mfx, 70, 300, 3600, 51, "ratings"), "bm25")
    with mfx.ItemKnn(X, 20, None) as a, mfx.ItemKnn(X, 20, None) as b:
        la, lb = a.lists(), b.lists()
        t = a.times()
    assert same(la, lb)
    assert t["build_pass"] > 0 and t["build_checks"] > 0 and t["recommend_pass"] == 0
    dev = torch.device("cuda", 0)
    d = {"rows": X.rows, "cols": X.cols}
    for k in ("csr_row_ptr", "csr_col_idx", "csc_col_ptr", "csc_row_idx"):
        d[k] = torch.from_numpy(getattr(X, k).view(np.int32)).to(dev)
    for k in ("csr_val", "csc_val"):
        d[k] = torch.from_numpy(getattr(X, k)).to(dev)
    with mfx.ItemKnn(None, 20, None, device_arrays=d) as c:
        assert same(c.lists(), la)


def _raw_build(mfx, X, K=5):
    from mfx import api
    h = C.c_void_p(0x1)
    csx = api._csx(X)
    rc = mfx.lib().mfx_knn_build(C.byref(h), C.byref(csx), K, 0, 0, 0)
    return rc, h, mfx.lib().mfx_last_error().decode()


def _set(X, u, pos, value):
    """X with the value of the pos-th entry of row u replaced, on both sides."""
    Y = X.copy()
    e = int(Y.csr_row_ptr[u]) + pos
    item = int(Y.csr_col_idx[e])
    Y.csr_val[e] = value
    c0, c1 = int(Y.csc_col_ptr[item]), int(Y.csc_col_ptr[item + 1])
    Y.csc_val[c0 + int(np.nonzero(Y.csc_row_idx[c0:c1] == u)[0][0])] = value
    return Y, item


def test_build_refuses_bad_terms_and_names_the_item(mfx):
    X = random_matrix(mfx, 37, 29, 400, 61, "ratings")
    u = int(np.argmax(np.diff(X.csr_row_ptr.astype(np.int64)) >= 3))
    Y, first = _set(X, u, 1, 50.0)
    Y, second = _set(Y, u, 2, 2.0)  # the pair's term is 100
    with pytest.raises(kx.BadTerm) as err:
        kx.similarities(Y)
    rc, h, msg = _raw_build(mfx, Y)
    assert rc == MFX_ERR_INVALID and not h.value
    assert f"item {err.value.item}:" in msg, msg
    Z, item = _set(X, u, 1, np.nan)
    with pytest.raises(kx.BadTerm) as err:
        kx.similarities(Z)
    rc, h, msg = _raw_build(mfx, Z)
    assert rc == MFX_ERR_INVALID and not h.value
    assert f"item {err.value.item}:" in msg and err.value.item == int(X.csr_col_idx[X.csr_row_ptr[u]]), msg
    rc, h, msg = _raw_build(mfx, X)  # the same call on clean data succeeds
    assert rc == 0 and h.value
    assert mfx.lib().mfx_knn_destroy(h) == 0


def test_build_refuses_descending_ids_and_names_the_row(mfx):
    X = random_matrix(mfx, 37, 29, 400, 62, "ratings")
    u = 11
    e = int(X.csr_row_ptr[u])
    assert X.csr_row_ptr[u + 1] - e >= 2
    Y = X.copy()
    Y.csr_col_idx[e], Y.csr_col_idx[e + 1] = X.csr_col_idx[e + 1], X.csr_col_idx[e]
    rc, h, msg = _raw_build(mfx, Y)
    assert rc == MFX_ERR_INVALID and not h.value and f"row {u} " in msg, msg
    Y = X.copy()
    Y.csr_col_idx[e] = 29  # an id >= cols
    rc, h, msg = _raw_build(mfx, Y)
    assert rc == MFX_ERR_INVALID and not h.value and "row " in msg, msg


# ------------------------------------------------------------------------------------------------ lists
def random_lists(cols, K, seed):
    """Hand-made lists: unsorted, the same j under several i (and twice under one), pads at the tail, two items without any."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, cols, (cols, K)).astype(np.uint32)
    sim = rng.standard_normal((cols, K)).astype(F)
    fill = rng.integers(0, K + 1, cols)
    fill[[1, cols - 1]] = 0
    fill[2] = K
    for i in range(cols):
        idx[i, fill[i]:] = PAD
        sim[i, fill[i]:] = -np.inf
    return idx, sim


def test_lists_round_trip_and_neighbours_are_their_prefix(mfx):
    X = mfx.knn_weights(random_matrix(mfx, 37, 29, 400, 21, "ratings"), "cosine")
    with mfx.ItemKnn(X, 9, None) as m:
        idx, sim = m.lists()
        with mfx.ItemKnn.from_lists(idx, sim) as c:
            assert same(c.lists(), (idx, sim))
            assert c.cols == 29 and c.K == 9
        for n_top in (1, 4, 9):
            assert same(m.neighbours(n_top), (idx[:, :n_top], sim[:, :n_top]))
        q = np.array([28, 0, 7, 7, 13])
        assert same(m.neighbours(3, q), (idx[q, :3], sim[q, :3]))
        import torch
        ti, ts = m.neighbours(3, torch.from_numpy(q.astype(np.int32)).cuda())
        assert same((ti.cpu().numpy().view(np.uint32), ts.cpu().numpy()), (idx[q, :3], sim[q, :3]))
        with pytest.raises(mfx.MfxError, match="query 1 "):
            m.neighbours(3, np.array([0, 29, 30]))
        with pytest.raises(mfx.MfxError, match="n_top"):
            m.neighbours(10)
    hi, hs = random_lists(50, 6, 71)
    with mfx.ItemKnn.from_lists(hi, hs) as c:  # no order is required
        assert same(c.lists(), (hi, hs))
    import torch
    with mfx.ItemKnn.from_lists(torch.from_numpy(hi.view(np.int32)).cuda(), torch.from_numpy(hs).cuda()) as c:
        assert same(c.lists(), (hi, hs))


def test_from_lists_refuses_and_names_the_item(mfx):
    hi, hs = random_lists(50, 6, 72)
    assert hi[2, 5] != PAD
    for item, slot, ident, value in ((2, 3, PAD, 0.5), (7, 0, 50, 0.5), (2, 1, 4, np.inf), (2, 1, 4, np.nan)):
        bi, bs = hi.copy(), hs.copy()
        bi[40, 0], bs[40, 0] = PAD, 1.0  # a later bad item: the first one is named
        bi[40, 1] = 3
        bi[item, slot], bs[item, slot] = ident, value
        if item == 7:
            bi[7, :], bs[7, :] = 1, 0.25
            bi[7, 0] = 50
        with pytest.raises(mfx.MfxError, match=f"item {item}:"):
            mfx.ItemKnn.from_lists(bi, bs)


# ------------------------------------------------------------------------------------------------ recommend
def random_rows(cols, n, seed, max_len=12):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, n)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    idx = np.concatenate([np.sort(rng.choice(cols, k, replace=False)) for k in lens] + [np.zeros(0, np.int64)]).astype(np.uint32)
    val = rng.standard_normal(idx.size).astype(F)
    return ptr, idx, val


def check_recommend(m, lists, rows, n_top, keep_seen=False, tile=0, bad=0):
    want = kx.recommend(lists[0], lists[1], *rows, n_top, keep_seen)
    got = m.recommend(rows, n_top, keep_seen=keep_seen, tile_items=tile)
    assert got[0].dtype == np.uint32 and got[1].dtype == F
    assert same(got, want[:2]), (n_top, keep_seen, tile, int((bits(got[0]) != bits(want[0])).sum()))
    assert m.bad_rows == want[2] == bad
    return want


@pytest.fixture(scope="module")
def built(mfx):
    X = mfx.knn_weights(random_matrix(mfx, 37, 29, 400, 21, "ratings"), "cosine")
    m = mfx.ItemKnn(X, 5, None)
    yield m, m.lists(), X
    m.close()


@pytest.fixture(scope="module")
def handmade(mfx):
    lists = random_lists(50, 6, 71)
    m = mfx.ItemKnn.from_lists(*lists)
    yield m, lists
    m.close()


@pytest.mark.parametrize("keep_seen", [False, True])
@pytest.mark.parametrize("n_top", [1, 10, 1024])
def test_recommend_on_a_built_model(mfx, built, n_top, keep_seen):
    m, lists, X = built
    rows = (X.csr_row_ptr, X.csr_col_idx, X.csr_val)
    want = check_recommend(m, lists, rows, n_top, keep_seen)
    if n_top == 1024:
        assert np.all(want[0][:, 29:] == PAD)  # more slots than eligible items: pads
    got_rd = m.recommend(X, n_top, keep_seen=keep_seen)  # a RatingData is its CSR side
    assert same(got_rd, want[:2])
    if not keep_seen:
        for u in range(X.rows):
            assert not np.intersect1d(want[0][u], X.csr_col_idx[X.csr_row_ptr[u]:X.csr_row_ptr[u + 1]]).size


@pytest.mark.parametrize("keep_seen", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_recommend_on_handmade_lists_in_batches(mfx, handmade, n, keep_seen):
    m, lists = handmade
    ptr, idx, val = random_rows(50, 300, 81)
    rows = (ptr[:n + 1], idx[:ptr[n]], val[:ptr[n]])
    for n_top in (1, 10):
        check_recommend(m, lists, rows, n_top, keep_seen)


def test_recommend_rows_alone_and_on_the_device(mfx, handmade):
    import torch
    m, lists = handmade
    ptr, idx, val = random_rows(50, 40, 82)
    want = check_recommend(m, lists, (ptr, idx, val), 10)
    for u in (0, 17, 39):
        one = (np.array([0, ptr[u + 1] - ptr[u]], np.uint32), idx[ptr[u]:ptr[u + 1]], val[ptr[u]:ptr[u + 1]])
        got = m.recommend(one, 10)
        assert same(got, (want[0][u:u + 1], want[1][u:u + 1]))
    t = [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda() for a in (ptr, idx, val)]
    gi, gs = m.recommend(tuple(t), 10)
    assert same((gi.cpu().numpy().view(np.uint32), gs.cpu().numpy()), want[:2])
    t0 = m.times()
    assert t0["recommend_pass"] > 0 and t0["recommend_checks"] > 0


def test_recommend_empty_rows_and_rows_without_neighbours(mfx, handmade):
    m, lists = handmade
    assert np.all(lists[0][1] == PAD) and np.all(lists[0][49] == PAD)
    ptr = np.array([0, 0, 2, 2, 5], np.uint32)  # empty, two items without neighbours, empty, an ordinary row
    idx = np.array([1, 49, 2, 3, 30], np.uint32)
    val = np.array([1, 2, 0.5, -1, 3], F)
    want = check_recommend(m, lists, (ptr, idx, val), 10)
    assert np.all(want[0][:3] == PAD) and np.all(np.isneginf(want[1][:3])) and want[0][3, 0] != PAD
    only_empty = (np.array([0, 0], np.uint32), np.zeros(0, np.uint32), np.zeros(0, F))
    got = m.recommend(only_empty, 3)
    assert np.all(got[0] == PAD) and np.all(np.isneginf(got[1])) and got[0].shape == (1, 3)


def test_recommend_bad_row_between_good_ones(mfx, handmade):
    m, lists = handmade
    ptr, idx, val = random_rows(50, 9, 83)
    good = check_recommend(m, lists, (ptr, idx, val), 10)
    u = 4
    assert ptr[u + 1] - ptr[u] >= 1
    e = int(ptr[u]) + int(np.argmax(lists[0][idx[ptr[u]:ptr[u + 1]], 0] != PAD))
    i = int(idx[e])
    assert lists[0][i, 0] != PAD
    v = val.copy()
    v[e] = F(65.0) / np.abs(lists[1][i, 0])  # the term with the first neighbour has magnitude >= 64
    assert abs(F(v[e]) * lists[1][i, 0]) >= 64
    want = check_recommend(m, lists, (ptr, idx, v), 10, bad=1)
    assert np.all(want[0][u] == PAD) and np.all(np.isneginf(want[1][u]))
    keep = np.arange(9) != u
    assert same((want[0][keep], want[1][keep]), (good[0][keep], good[1][keep]))
    v[e] = np.nan
    check_recommend(m, lists, (ptr, idx, v), 10, bad=1)
    check_recommend(m, lists, (ptr, idx, val), 10)  # and the handle is as before


@pytest.mark.parametrize("n_top", [10, 1024])
def test_recommend_across_tiles(mfx, n_top):
    X, S = sums_of("tiles300", lambda: random_matrix(mfx, 70, 300, 3600, 400))
    lists = kx.top_lists(S, 10)
    rows = (X.csr_row_ptr, X.csr_col_idx, X.csr_val)
    with mfx.ItemKnn.from_lists(*lists) as m:
        for keep_seen in (False, True):
            a = check_recommend(m, lists, rows, n_top, keep_seen, tile=0)
            b = check_recommend(m, lists, rows, n_top, keep_seen, tile=64)
            assert same(a[:2], b[:2])


def test_recommend_refusals_leave_the_handle_usable(mfx, handmade):
    m, lists = handmade
    ptr, idx, val = random_rows(50, 5, 84)
    before = m.recommend((ptr, idx, val), 4)
    for kw in (dict(n_top=0), dict(n_top=1025), dict(n_top=4, tile_items=32), dict(n_top=4, tile_items=8256), dict(n_top=600, tile_items=8192)):
        with pytest.raises(mfx.MfxError):
            m.recommend((ptr, idx, val), **kw)
    lib = mfx.lib()
    out_i, out_s = np.empty((5, 4), np.uint32), np.empty((5, 4), F)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    bad = C.c_int64(0)
    args = lambda flags, space: (m.handle, 5, int(idx.size), p(ptr), p(idx), p(val), 4, flags, 0, p(out_i), p(out_s), C.byref(bad), space)
    assert lib.mfx_knn_recommend(*args(2, 0)) == MFX_ERR_INVALID  # an unknown flag
    assert lib.mfx_knn_recommend(*args(0, 9)) == MFX_ERR_INVALID  # an unknown memory space
    assert ptr[3] - ptr[2] >= 2
    d = idx.copy()
    d[ptr[2]:ptr[3]] = idx[ptr[2]:ptr[3]][::-1]
    with pytest.raises(mfx.MfxError, match="row 2:"):
        m.recommend((ptr, d, val), 4)
    assert same(m.recommend((ptr, idx, val), 4), before)


# ------------------------------------------------------------------------------------------------ end to end
def test_planted_clusters_end_to_end(mfx):
    P = bx.planted_clusters()
    with mfx.ItemKnn(P, 100, "cosine") as m:
        X = mfx.knn_weights(P, "cosine")
        items, scores = m.recommend(X, 10)
        assert m.bad_rows == 0
        sims = m.lists()[1]
    assert np.all(sims[:, 0] > 0) and np.all(sims[np.isfinite(sims)] <= 1.0 + 1e-6)  # cosines
    met = mfx.topn_metrics(items, P)
    assert met["users"] == P.rows
    assert met["hr"] >= 0.9, met
