"""Item-kNN (csrc/knn.hip, mfx_knn_*) where its wave, batch and workgroup loops take more than one turn, against the exact
reference of tests/knn_exact.py.  As in tests/test_gpu_knn.py every comparison is on the uint32 views of ids and values:
there are no tolerances.  Every input is one the reference accepts (terms below 64, ids strictly ascending); the reference
call not raising is the check.

tests/test_gpu_knn.py pins the contract at ties, pads, tile boundaries, a full candidate area and bad terms, but on matrices
of 3 to 70 rows, rows of at most 66 entries and at most 300 users.  Read beside the kernels that leaves (BEFORE):

    loop / switch                             run before                         never run before
    BuildSrc::add_terms, e0 += 512            wave 0, one batch, nb < 64         waves 1 .. 7, nb = 64, a second batch, the
                                                                                 lower-bound search of base > 0 in waves 1 .. 7
    BuildSrc::add_terms, r0 += 256            one round (rows up to 300 only     a row of exactly 256 and of 257 entries on
                                              on one tile in wave 0)             tiles of 64, in every wave
    RecSrc::add_terms, p0 += 2048             batch slot b = 0 and, up to 660    b = 2, 3; a second, third, fourth round;
                                              pairs (rows of 66 entries at       p / K with quotients above 65
                                              K = 10, across tiles only), b = 1
    RecSrc::drop_seen, e += 512               one entry per thread               a second entry
    k_knn_recommend, r += gridDim.x           the first row of a workgroup       a second row: after a heavy, a bad, an empty one
    knn_area at keep 512 / 513                keep <= 100 and 1024               both sides of the switch
    the area holding NC and NC + 1            2 599 candidates: several merges   exactly full without a merge; one merge for one
    T = 8192 / 8128, LDS above 64 KiB         (tools/knn_bench.py, timed only)   any bit of it; a second tile at automatic width
    the 2^21 entries of a column / a row      the numpy reference only           the device's refusal, and the limit itself

AFTER (this module):

    build, 1 200 x 300                        columns of 64, 65, 128, 511, 512, 513, 1 025 and 1 200 users, rows of 256, 257 and
                                              300 entries, K = 10 and 299, one tile and five tiles of 64, twice
    recommend, 700 items, K = 7 and 64        n_u * K = 511, 512, 518, 2 044, 2 048, 2 051, 4 200, 6 400, 38 400; a row of 600
                                              entries; both keep_seen; one tile and eleven; n_top 10, 512, 513, 1 024
    recommend, 8 CUs + 301 rows               every workgroup's second row for 301 of them, empty / neighbourless / heavy / bad
                                              rows at r and r + 8 CUs in both orders, the good rows alone
    8 261 items                               recommend at T = 8192 + 69, 8128 + 133, 64 x 130; build at K = 20 and 600
    the area's edges                          1 024 / 1 025 candidates at K = 5 and 2 048 / 2 049 at K = 600, tied and distinct;
                                              2 599 candidates at K = 512 and 513
    the limits                                a column of 2^21 + 1 refused, one of 2^21 built; a query row of 2^21 + 1 all pads

What the sweep found: nothing.  All 35 cases pass on the MI355X against the library as it stood, bit for bit, so knn.hip is
unchanged.  The loop turns listed under "never run before" ran here for the first time against a reference.  That the cases
would notice was tried on three scratch builds of knn.hip that each only skip terms (never committed), tests/test_gpu_knn.py
and this module once each per build:
    waves 1 .. 7 return at once from BuildSrc::add_terms    test_gpu_knn.py passes; here test_build_long_columns (4 of 4) and
                                                            test_build_at_the_limit fail
    RecSrc::add_terms ignores the batch slots b >= 1        test_gpu_knn.py fails in test_recommend_across_tiles (2 of 2: its
                                                            rows reach slot b = 1, see above); here
                                                            test_recommend_many_pairs_per_row fails (8 of 8)
    k_knn_recommend skips the scan-and-clear of the first   test_gpu_knn.py passes; here
    tile for rows that are not the workgroup's first        test_recommend_more_rows_than_workgroups fails (2 of 2)

Wall time of every test on the MI355X (pytest --durations=0, this module after tests/test_gpu_knn.py as in the suite; the
reference of a matrix is computed once, in the first case that needs it, and its time is in that case):
    test_build_long_columns                                 0.11 s the first case, 0.01 s each of the other three
    test_recommend_many_pairs_per_row                       below 0.005 s each of the 8
    test_recommend_more_rows_than_workgroups                0.08 s, 0.05 s (12.3 s for the first when the module runs alone: the
                                                            import of torch and its start on the device, which the suite has
                                                            paid for before this module)
    test_recommend_on_the_widest_tile                       0.01 s of set-up, below 0.005 s each of the 5
    test_build_on_the_widest_tile                           0.50 s (K = 20: with the reference at both K), 0.01 s, 0.01 s
    test_build_with_the_area_exactly_full_and_one_over      0.04 - 0.05 s at 1 025 / 1 026 columns, 0.19 - 0.27 s at 2 049 / 2 050
    test_build_merges_on_both_sides_of_the_area_switch      0.35 s, 0.15 s
    test_build_refuses_a_column_one_past_the_limit          0.35 s
    test_build_at_the_limit                                 0.59 s
    test_recommend_refuses_a_row_one_past_the_limit         0.38 s
"""
import numpy as np
import pytest

import knn_exact as kx
from test_gpu_knn import bits, check_recommend, random_lists, random_matrix, random_rows, same

pytestmark = pytest.mark.gpu

F = np.float32
PAD = kx.PAD
LIMIT = kx.MAX_ENTRIES  # 2^21


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1
    return m


def lens_of(ptr):
    return np.diff(np.asarray(ptr).astype(np.int64))


def from_mask(mfx, M, values):
    """The matrix with an entry wherever M is set, the values in row-major order of the entries."""
    r, c = np.nonzero(M)
    return mfx.dataset.from_coo(M.shape[0], M.shape[1], r, c, np.asarray(values, F))


def rows_from(parts):
    """(ptr, idx, val) of the rows given as (ids, values) pairs."""
    ptr = np.concatenate([[0], np.cumsum([len(i) for i, _ in parts])]).astype(np.uint32)
    idx = np.concatenate([np.asarray(i, np.uint32) for i, _ in parts] + [np.zeros(0, np.uint32)])
    val = np.concatenate([np.asarray(v, F) for _, v in parts] + [np.zeros(0, F)])
    return ptr, idx, val


def row_of(rows, r):
    ptr, idx, val = rows
    return np.array([0, ptr[r + 1] - ptr[r]], np.uint32), idx[ptr[r]:ptr[r + 1]], val[ptr[r]:ptr[r + 1]]


_ONCE = {}


def once(name, make):
    """What `make` returns, computed once for the module and left unchanged."""
    if name not in _ONCE:
        _ONCE[name] = make()
    return _ONCE[name]


def check_build_twice(mfx, X, want, K, tile=0):
    with mfx.ItemKnn(X, K, None, tile_items=tile) as a, mfx.ItemKnn(X, K, None, tile_items=tile) as b:
        got, again = a.lists(), b.lists()
    assert same(got, want), (K, tile, int((bits(got[0]) != bits(want[0])).sum()), int((bits(got[1]) != bits(want[1])).sum()))
    assert same(again, got)


# ------------------------------------------------------------------------------------------------ build: long columns
COLUMN_LENGTHS = (64, 65, 128, 511, 512, 513, 1025, 1200)
FULL_ROWS = (3, 500, 777, 1199)
ROWS_OF = {10: 256, 600: 256, 11: 257, 601: 257}


def long_columns(mfx):
    """1 200 x 300, standard-normal values: the first columns have the lengths of COLUMN_LENGTHS, the others about 12 random rows
    and what the special rows add; FULL_ROWS hold every column, ROWS_OF[u] columns the rows u."""
    rng = np.random.default_rng(2101)
    rows, cols = 1200, 300
    M = np.zeros((rows, cols), bool)
    M[list(FULL_ROWS), :] = True
    M[:, 7] = True
    for u, n in ROWS_OF.items():
        free = np.nonzero(~M[u])[0]
        M[u, rng.choice(free, n - int(M[u].sum()), replace=False)] = True
    special = np.zeros(rows, bool)
    special[list(FULL_ROWS) + list(ROWS_OF)] = True
    for c in range(cols):
        n = COLUMN_LENGTHS[c] - int(M[:, c].sum()) if c < len(COLUMN_LENGTHS) else 12
        free = np.nonzero(~M[:, c] & ~special)[0]
        M[rng.choice(free, n, replace=False), c] = True
    X = from_mask(mfx, M, rng.standard_normal(int(M.sum())))
    return X, kx.similarities(X)


@pytest.mark.parametrize("tile", [0, 64])
@pytest.mark.parametrize("K", [10, 299])
def test_build_long_columns(mfx, K, tile):
    """Columns of 64 .. 1 200 users: every wave adds terms, whole batches of 64 users, a second and a third batch per wave; with
    tiles of 64 (five, the last of 44) the lower-bound search in every wave.  Rows of 256 / 257 / 300 entries: one round of
    64 * kKnnBatch and two.  K = 299 keeps every neighbour.  Built twice."""
    X, S = once("long", lambda: long_columns(mfx))
    assert tuple(lens_of(X.csc_col_ptr)[:len(COLUMN_LENGTHS)]) == COLUMN_LENGTHS
    row_lens = lens_of(X.csr_row_ptr)
    assert all(row_lens[u] == 300 for u in FULL_ROWS) and all(row_lens[u] == n for u, n in ROWS_OF.items())
    assert X.rows == 1200 and X.cols == 300 and lens_of(X.csc_col_ptr)[8:].min() >= 12
    want = kx.top_lists(S, K)
    if K == 299:
        assert not np.any(want[0][7] == PAD)  # column 7 meets every other item: a full list, nothing cut
    check_build_twice(mfx, X, want, K, tile)


# ------------------------------------------------------------------------------------------------ recommend: many pairs per row
PAIR_ROWS = (73, 74, 292, 293, 8, 32, 100, 600, 0, 1)  # x 7: 511 518 2044 2051 56 224 700 4200; x 64: .. 512 2048 6400 38400


def pair_rows():
    rng = np.random.default_rng(2201)
    return rows_from([(np.sort(rng.choice(700, n, replace=False)), rng.standard_normal(n)) for n in PAIR_ROWS])


@pytest.fixture(scope="module", params=[7, 64])
def lists700(mfx, request):
    K = request.param
    lists = random_lists(700, K, 2200 + K)
    m = mfx.ItemKnn.from_lists(*lists)
    yield m, lists, K
    m.close()


@pytest.mark.parametrize("tile", [0, 64])
@pytest.mark.parametrize("keep_seen", [False, True])
def test_recommend_many_pairs_per_row(mfx, lists700, keep_seen, tile):
    """n_u * K on both sides of 512 (one pair per thread), of 2 048 (the four batch slots of one round) and beyond 3 x 2 048
    (further rounds); K = 7 divides by a multiplication, K = 64 by a shift; 600 entries: drop_seen's second turn."""
    m, lists, K = lists700
    rows = once("pairs", pair_rows)
    pairs = set(int(n) * K for n in lens_of(rows[0]))
    assert pairs >= ({511, 518, 2044, 2051, 4200} if K == 7 else {512, 2048, 6400, 38400})
    assert lens_of(rows[0]).max() == 600
    for n_top in (10, 512, 513, 1024):
        want = check_recommend(m, lists, rows, n_top, keep_seen, tile)
        assert want[0][7, 0] != PAD and np.all(want[0][8] == PAD)  # (the row of 600 scores, the empty one does not)


# ------------------------------------------------------------------------------------------------ recommend: rows per workgroup
def crowd(lists, G):
    """8 CUs + 301 short rows on the 50-item lists; special rows at r and r + G, which one workgroup computes one after the other."""
    n = G + 301
    ptr, idx, val = random_rows(50, n, 2301)
    parts = [(idx[ptr[r]:ptr[r + 1]], val[ptr[r]:ptr[r + 1]]) for r in range(n)]
    rng = np.random.default_rng(2302)
    empty = (np.zeros(0, np.uint32), np.zeros(0, F))
    lonely = (np.array([1, 49], np.uint32), np.array([1.5, -2.0], F))  # items without neighbours
    heavy = lambda: (np.arange(50, dtype=np.uint32), rng.standard_normal(50).astype(F))
    i = 2  # item 2 has a full list
    big = (np.array([0, i, 30], np.uint32), np.array([0.5, F(65.0) / np.abs(lists[1][i, 0]), -1.0], F))
    assert abs(big[1][1] * lists[1][i, 0]) >= 64
    nan = (np.array([i, 7, 20], np.uint32), np.array([np.nan, 1.0, 2.0], F))
    special = {10: empty, 10 + G: heavy(), 11: heavy(), 11 + G: empty, 12: big, 12 + G: heavy(), 13: heavy(), 13 + G: nan,
               14: lonely, 14 + G: heavy(), 15: heavy(), 15 + G: lonely, 16: empty, 16 + G: empty, 17: lonely, 17 + G: lonely,
               18: nan, 19 + G: big}
    for r, part in special.items():
        parts[r] = part
    bad = [r for r, part in special.items() if part is big or part is nan]
    return rows_from(parts), sorted(special), bad


@pytest.mark.parametrize("keep_seen", [False, True])
def test_recommend_more_rows_than_workgroups(mfx, keep_seen):
    """A workgroup's second row (r + 8 CUs) after an empty, a neighbourless, a heavy and a bad first row, and the reverse: the
    accumulators are all zero again whatever the row before was."""
    import torch
    G = 8 * torch.cuda.get_device_properties(0).multi_processor_count
    lists = random_lists(50, 6, 71)
    rows, special, bad = crowd(lists, G)
    nusers = len(rows[0]) - 1
    assert nusers == G + 301 and nusers > min(nusers, G)  # the grid of k_knn_recommend: min(nusers, 8 CUs) workgroups
    with mfx.ItemKnn.from_lists(*lists) as m:
        want = check_recommend(m, lists, rows, 10, keep_seen, bad=len(bad))
        assert len(bad) == 4
        for r in bad:
            assert np.all(want[0][r] == PAD) and np.all(np.isneginf(want[1][r]))
        good = [r for r in special + [0, G - 1, G, G + 300] if r not in bad]
        for r in good:  # the same rows alone
            got = m.recommend(row_of(rows, r), 10, keep_seen=keep_seen)
            assert m.bad_rows == 0 and same(got, (want[0][r:r + 1], want[1][r:r + 1])), r
        ptr, idx, val = rows  # every second row as the first row of its workgroup
        tail = ((ptr[G:] - ptr[G]).astype(np.uint32), idx[ptr[G]:], val[ptr[G]:])
        got = m.recommend(tail, 10, keep_seen=keep_seen)
        assert m.bad_rows == sum(r >= G for r in bad)
        assert same(got, (want[0][G:], want[1][G:]))


# ------------------------------------------------------------------------------------------------ the widest tile
WIDE = 8261  # automatic T = 8192 and a second tile of 69; above keep = 512 T = 8128 and 133


@pytest.fixture(scope="module")
def wide_lists(mfx):
    lists = random_lists(WIDE, 8, 2401)
    m = mfx.ItemKnn.from_lists(*lists)
    yield m, lists, random_rows(WIDE, 60, 2402, max_len=40)
    m.close()


@pytest.mark.parametrize("n_top,tile", [(10, 0), (10, 8192), (10, 64), (600, 0), (600, 8128)])
def test_recommend_on_the_widest_tile(mfx, wide_lists, n_top, tile):
    """The launches with 73 792 (T = 8192, 1 024 slots) and 81 472 bytes (T = 8128, 2 048 slots) of LDS, automatic and asked for,
    each with a second tile; tiles of 64 must give the same."""
    m, lists, rows = wide_lists
    assert lens_of(rows[0]).max() == 40 and (lists[0][lists[0] != PAD] >= 8192).any()  # neighbours in the second tile
    for keep_seen in (False, True):
        check_recommend(m, lists, rows, n_top, keep_seen, tile)


def wide_matrix(mfx):
    """400 x 8 261 with 25 entries per row on average, and the reference's lists at K = 600 and 20, computed in slices."""
    X = random_matrix(mfx, 400, WIDE, 10000, 2403)
    want = {}
    for K in (20, 600):
        parts = [kx.top_lists(kx.similarity_rows(X, np.arange(lo, min(lo + 1024, WIDE))), K) for lo in range(0, WIDE, 1024)]
        want[K] = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
    return X, want


@pytest.mark.parametrize("K,tile", [(20, 0), (600, 0), (20, 64)])
def test_build_on_the_widest_tile(mfx, K, tile):
    X, want = once("wide", lambda: wide_matrix(mfx))
    assert want[K][0].shape == (WIDE, K) and (want[K][0][:, 0] != PAD).sum() > WIDE // 2
    check_build_twice(mfx, X, want[K], K, tile)


# ------------------------------------------------------------------------------------------------ the area's edges
def dense_rows(mfx, rows, cols, values):
    """Every cell filled: all ones, or integers 1 .. 3."""
    rng = np.random.default_rng(2500 + cols)
    v = np.ones(rows * cols, F) if values == "ones" else rng.integers(1, 4, rows * cols).astype(F)
    X = mfx.dataset.from_coo(rows, cols, np.repeat(np.arange(rows), cols), np.tile(np.arange(cols), rows), v)
    return X, kx.similarities(X)


@pytest.mark.parametrize("values", ["ones", "distinct"])
@pytest.mark.parametrize("cols,K", [(1025, 5), (1026, 5), (2049, 600), (2050, 600)])
def test_build_with_the_area_exactly_full_and_one_over(mfx, cols, K, values):
    """cols - 1 candidates per item on one tile: 1 024 (2 048) fill the area of K = 5 (600) exactly and are sorted once at the
    end; one more stays in its accumulator, list and area are merged once, and the tile is scanned again for that one."""
    X, S = once(f"dense{cols}{values}", lambda: dense_rows(mfx, 4, cols, values))
    want = kx.top_lists(S, K)
    assert np.count_nonzero(S[0]) == cols - 1 and not np.any(want[0] == PAD)
    if values == "ones":
        assert np.all(want[1] == 4.0) and np.array_equal(want[0][0], np.arange(1, K + 1))
    check_build_twice(mfx, X, want, K)


@pytest.mark.parametrize("K", [512, 513])
def test_build_merges_on_both_sides_of_the_area_switch(mfx, K):
    """The 3 x 2 600 matrix of test_build_merges_when_the_candidate_area_fills: 2 599 candidates against 1 024 slots at K = 512
    and against 2 048 at K = 513."""
    def make():
        rng = np.random.default_rng(41)
        X = mfx.dataset.from_coo(3, 2600, np.repeat(np.arange(3), 2600), np.tile(np.arange(2600), 3), rng.integers(1, 4, 7800).astype(F))
        return X, kx.similarities(X)
    X, S = once("merges", make)
    check_build_twice(mfx, X, kx.top_lists(S, K), K)


# ------------------------------------------------------------------------------------------------ the 2^21 limits
def two_columns(mfx, n, x0, x1_rows, x1):
    """n rows x 2 columns: column 0 held by every row (values x0), column 1 by the first x1_rows rows (values x1)."""
    from mfx.dataset import RatingData
    lens = np.ones(n, np.int64)
    lens[:x1_rows] = 2
    ptr = np.concatenate([[0], np.cumsum(lens)])
    idx = np.zeros(ptr[-1], np.uint32)
    val = np.empty(ptr[-1], F)
    val[ptr[:-1]] = x0
    idx[ptr[:x1_rows] + 1] = 1
    val[ptr[:x1_rows] + 1] = x1
    return RatingData(n, 2, ptr.astype(np.uint32), idx, val, np.array([0, n, n + x1_rows], np.uint32),
                      np.concatenate([np.arange(n), np.arange(x1_rows)]).astype(np.uint32), np.concatenate([x0, x1]).astype(F))


def test_build_refuses_a_column_one_past_the_limit(mfx):
    """2^21 + 1 users in column 0 (the reference is not called: it walks the rows in Python)."""
    n = LIMIT + 1
    X = two_columns(mfx, n, np.ones(n, F), 2, np.ones(2, F))
    X.validate()
    assert tuple(lens_of(X.csc_col_ptr)) == (LIMIT + 1, 2)
    with pytest.raises(mfx.MfxError, match="item 0:"):
        mfx.ItemKnn(X, 1, None)


def test_build_at_the_limit(mfx):
    """2^21 users in both columns: 4 096 batches of 64 users per wave, and a sum of 2^21 terms."""
    rng = np.random.default_rng(2601)
    x0, x1 = rng.standard_normal(LIMIT).astype(F), rng.standard_normal(LIMIT).astype(F)
    X = two_columns(mfx, LIMIT, x0, LIMIT, x1)
    X.validate()
    assert tuple(lens_of(X.csc_col_ptr)) == (LIMIT, LIMIT)
    t = x0 * x1
    assert t.dtype == F and np.abs(t).max() < 64
    value = kx.from_fixed(kx.to_fixed(t).sum())
    assert value != 0
    want = (np.array([[1], [0]], np.uint32), np.array([[value], [value]], F))
    with mfx.ItemKnn(X, 1, None) as m:
        got = m.lists()
    assert same(got, want), (got, want)


def test_recommend_refuses_a_row_one_past_the_limit(mfx):
    """A query row of 2^21 + 1 entries between two short ones: all pads and counted, its neighbours as in the reference."""
    cols = LIMIT + 64
    idx = np.full((cols, 1), PAD, np.uint32)
    sim = np.full((cols, 1), -np.inf, F)
    for i, (j, s) in {0: (7, 0.5), 5: (LIMIT + 10, -1.25), 7: (0, 2.0), LIMIT: (5, 3.0), LIMIT + 10: (8200, 0.75)}.items():
        idx[i, 0], sim[i, 0] = j, s
    rows = rows_from([(np.array([0, 5]), np.array([1.0, 2.0])), (np.arange(LIMIT + 1), np.ones(LIMIT + 1)),
                      (np.array([5, 7, LIMIT, LIMIT + 10]), np.array([-1.0, 0.5, 1.5, 2.0]))])
    assert tuple(lens_of(rows[0])) == (2, LIMIT + 1, 4)
    with mfx.ItemKnn.from_lists(idx, sim) as m:
        want = check_recommend(m, (idx, sim), rows, 4, bad=1)
    assert np.all(want[0][1] == PAD) and np.all(np.isneginf(want[1][1]))
    assert list(want[0][0][:2]) == [7, LIMIT + 10] and list(want[0][2][:2]) == [8200, 0]
