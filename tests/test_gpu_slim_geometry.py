"""SLIM (csrc/slim.hip, mfx_slim_*) where its wave, tile, batch and workgroup loops take more than one turn, against the exact
reference of tests/slim_exact.py.  As in tests/test_gpu_slim.py every comparison is on the uint32 views of blocks, weights, ids
and scores: there are no tolerances.  Every input is one the reference accepts (standard-normal values keep every term below
64); the reference call not raising is the check.

tests/test_gpu_slim.py pins the contract on matrices of 37 to 200 rows, query rows of at most 29 entries, at most 300 users
and at most 700 items.  Read beside the kernels that leaves (BEFORE):

    loop / switch                             run before                         never run against a reference before
    SlimRecSrc::add_terms, e0 += 512          wave 0, lanes 0 .. 28, nb < 64     waves 1 .. 7; nb = 64; a wave's second batch (a row
                                                                                 above 512 entries); the lower-bound search of
                                                                                 base > 0 outside wave 0
    SlimRecSrc::add_terms, r0 += 256          one source of 699 targets, always  lists of exactly 256 / 257 targets; long lists whose
                                              in wave 0                          source sits in another wave or in the second batch;
                                                                                 the early break there
    SlimRecSrc::drop_seen, e += 512           one entry per thread               a second entry
    k_slim_recommend, r += gridDim.x          a workgroup's first row only       any second row: after a heavy, a bad, an empty row,
    (grid = min(users, 8 CUs))                                                   with the area and ctl[3] left by the row before
    k_slim_solve, waves per workgroup         4 (K <= 71) and 1 (K >= 102)       3 (K = 72 .. 82) and 2 (K = 83 .. 101): blockDim
    = min(4, 81920 / (4 stride))                                                 192 / 128, the item blockIdx.x * waves + wave
    k_slim_solve, item stride loop            K = 4 only                         a wave's second item with the LDS slice staged again
                                                                                 at K > 64 (c1 / w1), with fewer than 4 waves, with
                                                                                 another n_real than the item before
    BuildSrc::add_terms as compiled into      columns up to 200 users, rows up   columns of 511 .. 1 200 users (every wave, second
    k_slim_gram                               to 300                             and third batch), rows of 256 / 257 entries on
                                                                                 tiles of 64
    k_slim_gram pair loop, p / K              K = 3 (699 lists), K = 128 on one  K = 128 across tiles; a K that is no power of two
                                              tile                               with thousands of pairs
    T = 8192, LDS above 64 KiB (allow_lds)    nothing (k_slim_gram needs 65 600  both kernels; a second tile at automatic width
                                              bytes there, k_slim_recommend
                                              73 792 / 81 472)
    k_slim_diag, stride over items            first turn                         a second turn (cols > 262 144)
    (65 536 blocks x 4 waves)
    the 2^21 limits                           nowhere for SLIM                   the refusal of a column of 2^21 + 1 by mfx_slim_gram
                                                                                 and mfx_slim_train; a column of exactly 2^21; a
                                                                                 query row of 2^21 + 1

AFTER (this module):

    recommend, 1 300 items, K = 8             sources with inverse lists of 64, 65, 255, 256, 257, 513 and 1 299 targets, in six
                                              waves and three batches of the longest row; rows of 64, 65, 128, 511, 512, 513, 1 025
                                              and 1 200 entries, an empty one, one of a single entry (the source of 1 299 targets);
                                              both keep_seen; one tile and 21 of 64; n_top 10, 512, 513, 1 024
    recommend, 8 CUs + 301 rows               every workgroup's second row for 301 of them; empty / neighbourless / heavy / bad
                                              rows at r and r + 8 CUs in both orders; the good rows alone; the second rows as first
    solve, K = 71, 72, 82, 83, 101, 102       4, 3, 3, 2, 2, 1 waves per workgroup, seven blocks, both modes, with and without l2
    solve, 8 CUs x waves + 3 items            K = 65, 72, 83, 102, 128: three waves take a second item whose n_real differs; a block
                                              with an infinity among them
    gram, 1 200 x 300                         columns of 64 .. 1 200 users, rows of 256 / 257 / 300 entries; K = 10 with a hub item
                                              in some 270 lists (about 2 700 pairs, divided by 10) and K = 128 full (16 384 pairs
                                              and more per item, five tiles of 64); one tile and five; twice
    8 261 items                               gram at T = 8192 + 69 (65 600 bytes), 8192 asked for, 64 x 130; recommend at
                                              T = 8192 + 69, 8128 + 133 and 64 x 130
    262 147 items                             k_slim_diag's second turn (d of the last three items sits in the blocks of items
                                              0 .. 2); the Gram pass of 33 tiles per item; the solve with about 32 items per wave
    the limits                                a column of 2^21 + 1 refused by mfx_slim_gram and mfx_slim_train, two of 2^21 summed; a
                                              query row of 2^21 + 1 all pads and counted

What the sweep found: nothing.  All 44 cases pass on the MI355X against the library as it stood, bit for bit, so slim.hip and
knn_device.hpp are unchanged.  The loop turns listed under "never run against a reference before" ran here for the first time
against one.  The case of 262 147 items, whose time nobody had measured, takes 0.54 s of wall time, data and reference included.
That the cases would notice was tried on six scratch builds of slim.hip that each only skip work (never committed; none moves
a read or a write), tests/test_gpu_slim.py and this module once each per build:
    waves 1 .. 7 return at once from                        test_gpu_slim.py passes; here
    SlimRecSrc::add_terms                                   test_recommend_long_rows_and_long_lists fails (8 of 8)
    k_slim_solve computes its item index (start and         test_gpu_slim.py fails in test_solve_bit_for_bit at K = 127 and 128
    stride) with a hard-coded 4 in place of a.waves         (4 of 14: its seven blocks reach the class of one wave); here
                                                            test_solve_on_both_sides_of_every_wave_class fails at K = 72 .. 102
                                                            (10 of 12, all but the four-wave K = 71) and
                                                            test_solve_a_waves_second_item at K = 72, 83, 102, 128 (4 of 5)
    k_slim_recommend skips drop_seen for rows that are      test_gpu_slim.py passes; here
    not the workgroup's first                               test_recommend_more_rows_than_workgroups[False] fails (keep_seen
                                                            has nothing to drop)
    waves 1 .. 7 return at once from BuildSrc::add_terms    test_gpu_slim.py fails in test_gram_full_column_and_full_row (its
    as compiled into slim.hip                               column of 200 users reaches waves 1 .. 3); here
                                                            test_gram_long_columns_and_rows (4 of 4) and test_gram_at_the_limit
    k_slim_diag leaves out the items of its second turn     test_gpu_slim.py passes; here
                                                            test_gram_and_train_with_more_items_than_waves fails
    k_slim_solve leaves out the items of a wave's           test_gpu_slim.py fails in test_solve_more_items_than_waves; here
    second turn                                             test_solve_a_waves_second_item (5 of 5) and
                                                            test_gram_and_train_with_more_items_than_waves fail

Wall time of every test on the MI355X (pytest --durations=0, this module after tests/test_gpu_slim.py as in the suite; a
reference is computed once, in the first case that needs it, and its time is in that case; where numpy, not the device,
takes most of a case's time the line says so):
    test_long_lists_are_what_they_claim                     0.04 s (the model and its rows are made here)
    test_recommend_long_rows_and_long_lists                 below 0.005 s each of the 8
    test_recommend_more_rows_than_workgroups                0.05 s, 0.04 s
    test_solve_on_both_sides_of_every_wave_class            0.03 s at K = 71, 72; 0.04 s at 82, 83; 0.05 s at 101, 102 (the
                                                            reference's six solves)
    test_solve_a_waves_second_item                          0.04 s at K = 65, 0.08 - 0.09 s at the others (82 - 134 MiB of blocks
                                                            tiled on the host and copied to the device)
    test_gram_long_columns_and_rows                         0.05 s, 0.05 s, 0.05 s, below 0.005 s
    test_gram_on_the_widest_tile                            0.05 s (with the matrix, the support and the sparse reference), below
                                                            0.005 s each of the other two
    test_recommend_on_the_widest_tile                       0.01 s, below 0.005 s, 0.01 s, 0.01 s, below 0.005 s
    test_gram_and_train_with_more_items_than_waves          0.54 s (most of it numpy: the matrix, the support, the sparse
                                                            reference and the reference's solve of 262 147 blocks)
    test_gram_and_train_refuse_a_column_one_past_the_limit  0.68 s (a matrix of 2^21 + 3 entries, copied to the device twice)
    test_gram_at_the_limit                                  0.63 s
    test_recommend_refuses_a_row_one_past_the_limit         0.38 s
"""
import numpy as np
import pytest

import knn_exact as kx
import slim_exact as sx
from test_gpu_knn_geometry import lens_of, long_columns, once, row_of, rows_from, two_columns
from test_gpu_slim import bits, check_solve, handmade, psd_blocks, random_matrix, random_rows, random_support, same  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu

F = np.float32
PAD = sx.PAD
LIMIT = kx.MAX_ENTRIES  # 2^21


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1
    return m


def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def check_rec(m, want, rows, n_top, keep_seen, tile=0):
    """m.recommend against a reference computed before: (items, scores, bad_rows) of sx.recommend."""
    got = m.recommend(rows, n_top, keep_seen=keep_seen, tile_items=tile)
    assert got[0].dtype == np.uint32 and got[1].dtype == F
    assert same(got[0], want[0]) and same(got[1], want[1]), (n_top, keep_seen, tile, int((bits(got[0]) != bits(want[0])).sum()))
    assert m.bad_rows == want[2]
    return got


def weights_for(S, seed):
    """Standard-normal weights of both signs on the real slots, 0 on the pads."""
    return np.where(S != PAD, np.random.default_rng(seed).standard_normal(S.shape), 0).astype(F)


def neighbour_support(X, K, seed, pads=True):
    """A support whose Gram entries are not all zero: slot s of item c holds the item s + 1 places behind c (cyclically) in the
    row of one of c's users, a random id where that is c itself or in the list already or c has no user; with pads: the lists
    cut to random lengths 0 .. K."""
    rng = np.random.default_rng(seed)
    cols = X.cols
    ptr, cptr = X.csr_row_ptr.astype(np.int64), X.csc_col_ptr.astype(np.int64)
    keys = np.repeat(np.arange(X.rows, dtype=np.int64), np.diff(ptr)) * cols + X.csr_col_idx
    c = np.arange(cols, dtype=np.int64)
    clen = np.diff(cptr)
    C = rng.integers(0, cols, (cols, K))
    held = np.nonzero(clen > 0)[0]
    for s in range(K):
        u = X.csc_row_idx[cptr[held] + s % clen[held]].astype(np.int64)
        q = np.searchsorted(keys, u * cols + held) - ptr[u]
        C[held, s] = X.csr_col_idx[ptr[u] + (q + 1 + s) % (ptr[u + 1] - ptr[u])]
    ok = C != c[:, None]
    for s in range(1, K):
        ok[:, s] &= ~(C[:, :s] == C[:, s:s + 1]).any(axis=1)
    order = np.argsort(~ok, axis=1, kind="stable")  # the usable ids to the front, in their order
    C, ok = np.take_along_axis(C, order, axis=1), np.take_along_axis(ok, order, axis=1)
    n = ok.sum(axis=1)
    if pads:
        n = np.minimum(n, rng.integers(0, K + 1, cols))
    return np.where(np.arange(K)[None, :] < n[:, None], C, PAD).astype(np.uint32)


# ------------------------------------------------------------------------------------------------ recommend: long rows and lists
ITEMS = 1300
SOURCES = {5: 65, 100: 255, 300: 257, 450: 256, 640: 1299, 900: 513, 1250: 64}  # source item -> the targets of its inverse list
UNUSED = 1298
ROW_LENGTHS = (64, 65, 128, 511, 512, 513, 1025, 1200, 0, 1)


def long_lists():
    """1 300 items, K = 8: the lists hold the sources of SOURCES first (each in exactly as many lists as it says), then random
    ordinary items up to a random length; item UNUSED is in no list.  The rows of ROW_LENGTHS: the longest holds every source,
    the one of a single entry is the source of 1 299 targets."""
    rng = np.random.default_rng(3101)
    K = 8
    lists = [[] for _ in range(ITEMS)]
    for i, n in SOURCES.items():
        others = np.setdiff1d(np.arange(ITEMS), [i])
        for j in (others if n == ITEMS - 1 else rng.choice(others, n, replace=False)):
            lists[j].append(i)
    ordinary = np.setdiff1d(np.arange(ITEMS), list(SOURCES) + [UNUSED])
    S = np.full((ITEMS, K), PAD, np.uint32)
    for j in range(ITEMS):
        assert len(lists[j]) <= 7
        n = int(rng.integers(len(lists[j]), K + 1))
        fill = rng.permutation(np.setdiff1d(ordinary, [j]))[:n - len(lists[j])]
        S[j, :n] = np.concatenate([np.array(lists[j], np.int64), fill])
    w = weights_for(S, 3102)
    parts = []
    for n in ROW_LENGTHS:
        if n == 1:
            ids = np.array([640])
        elif n == 1200:
            rest = np.setdiff1d(np.arange(ITEMS), list(SOURCES))
            ids = np.sort(np.concatenate([list(SOURCES), rng.choice(rest, n - len(SOURCES), replace=False)]))
        else:
            ids = np.sort(rng.choice(ITEMS, n, replace=False))
        parts.append((ids, rng.standard_normal(n)))
    return S, w, rows_from(parts)


@pytest.fixture(scope="module")
def long_model(mfx):
    S, w, rows = once("slim_long_lists", long_lists)
    m = mfx.Slim.from_lists(S, w)
    yield m, S, w, rows
    m.close()


def test_long_lists_are_what_they_claim():
    S, w, rows = once("slim_long_lists", long_lists)
    sx.check_support(S, ITEMS, w)
    inverse = np.diff(sx.transpose(S, w)[0])
    assert all(inverse[i] == n for i, n in SOURCES.items()) and inverse[UNUSED] == 0
    assert sorted(SOURCES.values()) == [64, 65, 255, 256, 257, 513, 1299]
    assert (w < 0).any() and (w > 0).any() and (S == PAD).any()
    assert tuple(lens_of(rows[0])) == ROW_LENGTHS
    longest = row_of(rows, ROW_LENGTHS.index(1200))[1]
    at = np.searchsorted(longest, list(SOURCES))  # the entry index of every source in the longest row
    assert np.array_equal(longest[at], list(SOURCES))
    waves = set(((at % 512) // 64).tolist())
    assert len(waves) >= 4 and (at >= 512).any() and (at >= 1024).any(), at
    long_ones = [a for a, i in zip(at, SOURCES) if SOURCES[i] >= 256]  # lists of a second round: outside wave 0, in a later batch
    assert any((a % 512) // 64 > 0 for a in long_ones) and any(a >= 512 for a in long_ones)


@pytest.mark.parametrize("n_top", [10, 512, 513, 1024])
@pytest.mark.parametrize("keep_seen", [False, True])
def test_recommend_long_rows_and_long_lists(mfx, long_model, keep_seen, n_top):
    """Rows on both sides of 64 entries (a full wave), of 512 (every wave, one entry per thread in drop_seen) and of 1 024 (a
    wave's second and third batch); lists on both sides of 64 targets (one lane each) and of 256 (one round of 64 * kKnnBatch),
    up to six rounds, read by waves 0 .. 6 and in later batches; with tiles of 64 the lower-bound search in every wave and the
    early break of a long list.  One tile and 21 give the same bits."""
    m, S, w, rows = long_model
    want = once(("slim_long_want", n_top, keep_seen), lambda: sx.recommend(S, w, *rows, n_top, keep_seen))
    assert want[2] == 0
    a = check_rec(m, want, rows, n_top, keep_seen, 0)
    b = check_rec(m, want, rows, n_top, keep_seen, 64)
    assert same(a[0], b[0]) and same(a[1], b[1])
    empty, single = ROW_LENGTHS.index(0), ROW_LENGTHS.index(1)
    assert np.all(want[0][empty] == PAD) and (want[0][single] != PAD).sum() == min(n_top, 1299)
    assert (want[0][ROW_LENGTHS.index(1200)] != PAD).sum() == min(n_top, 1299 if keep_seen else 100)


# ------------------------------------------------------------------------------------------------ recommend: rows per workgroup
def crowd(model, G):
    """8 CUs + 301 short rows on the 50-item model; special rows at r and r + G, which one workgroup computes one after the
    other (the crowd() of tests/test_gpu_knn_geometry.py on a SLIM model: a bad term is x_i times the first stored weight of
    source i)."""
    S, w = model
    n = G + 301
    ptr, idx, val = random_rows(50, n, 3201)
    parts = [(idx[ptr[r]:ptr[r + 1]], val[ptr[r]:ptr[r + 1]]) for r in range(n)]
    rng = np.random.default_rng(3202)
    iptr, tj, tw = sx.transpose(S, w)
    assert iptr[2] == iptr[1] and iptr[50] == iptr[49]  # items 1 and 49 are in no list
    i = int(np.nonzero((np.diff(iptr) > 0) & (np.arange(50) > 1))[0][0])  # a source with targets
    first = tw[iptr[i]]
    assert first != 0
    empty = (np.zeros(0, np.uint32), np.zeros(0, F))
    lonely = (np.array([1, 49], np.uint32), np.array([1.5, -2.0], F))
    heavy = lambda: (np.arange(50, dtype=np.uint32), rng.standard_normal(50).astype(F))
    ids = np.array(sorted([i] + [j for j in (7, 20, 30) if j != i][:2]), np.uint32)
    big = (ids, np.where(ids == i, F(65.0) / np.abs(first), F(0.5)).astype(F))  # the term with the source's first target: >= 64
    assert np.abs(big[1][ids == i] * first) >= 64
    nan = (ids, np.where(ids == i, np.nan, 1.0).astype(F))
    special = {10: empty, 10 + G: heavy(), 11: heavy(), 11 + G: empty, 12: big, 12 + G: heavy(), 13: heavy(), 13 + G: nan,
               14: lonely, 14 + G: heavy(), 15: heavy(), 15 + G: lonely, 16: empty, 16 + G: empty, 17: lonely, 17 + G: lonely,
               18: nan, 19 + G: big}
    for r, part in special.items():
        parts[r] = part
    bad = [r for r, part in special.items() if part is big or part is nan]
    return rows_from(parts), sorted(special), bad


@pytest.mark.parametrize("keep_seen", [False, True])
def test_recommend_more_rows_than_workgroups(mfx, handmade, keep_seen):
    """A workgroup's second row (r + 8 CUs) after an empty, a neighbourless, a heavy and a bad first row, and the reverse: the
    accumulators are all zero again, the row's own items dropped again, the bad flag and the candidate area reset, whatever the
    row before was."""
    m, model = handmade
    G = 8 * cus()
    rows, special, bad = once(("slim_crowd", G), lambda: crowd(model, G))
    nusers = len(rows[0]) - 1
    assert nusers == G + 301 and nusers > min(nusers, G)  # the grid of k_slim_recommend: min(nusers, 8 CUs) workgroups
    want = once(("slim_crowd_want", G, keep_seen), lambda: sx.recommend(*model, *rows, 10, keep_seen))
    assert want[2] == len(bad) == 4
    check_rec(m, want, rows, 10, keep_seen)
    for r in bad:
        assert np.all(want[0][r] == PAD) and np.all(np.isneginf(want[1][r]))
    assert (want[0][12 + G, 0] != PAD) == keep_seen  # a heavy row behind a bad one: every item scored, every item its own
    good = [r for r in special + [0, G - 1, G, G + 300] if r not in bad]
    for r in good:  # the same rows alone
        got = m.recommend(row_of(rows, r), 10, keep_seen=keep_seen)
        assert m.bad_rows == 0 and same(got[0], want[0][r:r + 1]) and same(got[1], want[1][r:r + 1]), r
    ptr, idx, val = rows  # every second row as the first row of its workgroup
    tail = ((ptr[G:] - ptr[G]).astype(np.uint32), idx[ptr[G]:], val[ptr[G]:])
    got = m.recommend(tail, 10, keep_seen=keep_seen)
    assert m.bad_rows == sum(r >= G for r in bad)
    assert same(got[0], want[0][G:]) and same(got[1], want[1][G:])


# ------------------------------------------------------------------------------------------------ solve: waves per workgroup
def solve_waves(K):
    """The waves (items) per workgroup of k_slim_solve: the Gram rows of an item take K^2 floats of LDS, rounded up to a
    multiple of four, and a workgroup has 81 920 bytes."""
    stride = (K * K + 3) // 4 * 4
    return max(1, min(4, 81920 // (4 * stride)))


WAVE_CLASS_K = (71, 72, 82, 83, 101, 102)


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("K", WAVE_CLASS_K)
def test_solve_on_both_sides_of_every_wave_class(mfx, K, signed):
    """K on both sides of each switch 4 -> 3 -> 2 -> 1 waves per workgroup: seven blocks in 2, 3, 4 or 7 workgroups of 256, 192,
    128 or 64 threads, real-slot counts 0 .. K."""
    assert [solve_waves(k) for k in WAVE_CLASS_K] == [4, 3, 3, 2, 2, 1] and solve_waves(65) == 4 and solve_waves(128) == 1
    B = psd_blocks(7, K, 3300 + K)
    n_real = np.array([K, K - 1, 0, K // 2, K - 2, 1, K], np.uint32)
    for l1, l2 in ((0.25, 2.0), (0.0, 0.0)):
        w, used, failed = check_solve(mfx, B, n_real, l1=l1, l2=l2, sweeps=4, tol=0.0, signed=signed)
        assert failed == 0 and w[0].any() and w[3].any() and w[6].any()
        for n in range(7):
            assert not w[n, n_real[n]:].any()
    check_solve(mfx, B, None, l1=0.25, l2=2.0, sweeps=4, tol=0.0, signed=signed)


@pytest.mark.parametrize("K", [65, 72, 83, 102, 128])
def test_solve_a_waves_second_item(mfx, K):
    """8 CUs * waves(K) + 3 items: the first three waves of the grid take a second item, at K > 64 (two coefficients per lane),
    with 4, 3, 2 and 1 waves per workgroup.  61 distinct blocks and real-slot counts tiled with period 61 (a prime: it divides no
    grid geometry, so a wave's second item differs from its first in n_real); the reference solves the 61 and the planted block
    with an infinity, which is the second of the second turn."""
    G, waves = 8 * cus(), solve_waves(K)
    N = G * waves + 3
    planted = G * waves + 1
    U = psd_blocks(61, K, 3400 + K, rows=8)
    inf = U[planted % 61].copy()
    inf[K, 0] = np.inf
    blocks = np.concatenate([U, inf[None]])
    counts = np.concatenate([np.round(np.linspace(0, K, 61)), [K]]).astype(np.uint32)
    assert counts[0] == 0 and counts[60] == K and len(np.unique(counts[:61])) == 61
    kw = dict(l1=0.05, l2=0.5, sweeps=2, tol=0.0, signed=True)
    w, used, failed = sx.solve(blocks, counts, **kw)
    assert failed == 1 and not w[61].any() and used[61] == 0 and np.all(used[:61] >= 1) and (w[:61] < 0).any()
    pick = np.arange(N) % 61
    pick[planted] = 61
    for it in range(G * waves, N):
        assert counts[pick[it]] != counts[pick[it - G * waves]]  # (the item the same wave solved before)
    got = mfx.slim_solve(blocks[pick], counts[pick], **kw)
    assert same(got[0], w[pick]), int((bits(got[0]) != bits(w[pick])).any(axis=1).sum())
    assert np.array_equal(got[1], used[pick]) and got[2] == 1
    assert not got[0][planted].any() and got[1][planted] == 0 and got[0][N - 1].any()


# ------------------------------------------------------------------------------------------------ gram: long columns and rows
def long_gram(mfx):
    X, _ = once("long", lambda: long_columns(mfx))  # (shared with tests/test_gpu_knn_geometry.py)
    return X, sx.gram_sums(X)


def long_support(K):
    if K == 128:
        return random_support(300, 128, 3501, pads=False)
    S = random_support(300, K, 3502, among=np.setdiff1d(np.arange(300), [7]))
    S[(S[:, 0] != PAD) & (np.arange(300) != 7), 0] = 7  # the column that every user holds, in every list that is not empty
    return S


@pytest.mark.parametrize("tile", [0, 64])
@pytest.mark.parametrize("K", [10, 128])
def test_gram_long_columns_and_rows(mfx, K, tile):
    """The 1 200 x 300 matrix of tests/test_gpu_knn_geometry.py: columns of 64 .. 1 200 users (every wave adds terms, whole
    batches of 64 users, a second and a third batch per wave), rows of 256 / 257 / 300 entries (one round of 64 * kKnnBatch
    and two), with tiles of 64 the lower-bound search in every wave.  K = 10: lists with pads and a hub item whose pairs
    (inverse-list entry, slot) number thousands and are divided by 10; K = 128: full lists across five tiles.  Run twice."""
    X, sums = once("slim_long_gram", lambda: long_gram(mfx))
    assert lens_of(X.csc_col_ptr)[:8].tolist() == [64, 65, 128, 511, 512, 513, 1025, 1200]
    assert {256, 257, 300} <= set(lens_of(X.csr_row_ptr).tolist())
    S = once(("slim_long_support", K), lambda: long_support(K))
    inverse = np.diff(sx.transpose(S, np.zeros(S.shape, F))[0])
    assert inverse.max() * K >= (2048 if K == 10 else 16384) and ((S == PAD).any() == (K == 10))
    want = once(("slim_long_blocks", K), lambda: sx.gram_blocks(X, S, sums))
    got, again = mfx.slim_gram(X, K, S, tile_items=tile), mfx.slim_gram(X, K, S, tile_items=tile)
    assert same(got, want), (K, tile, int((bits(got) != bits(want)).sum()))
    assert same(again, got)
    if K == 128:
        assert same(got[:, :K, :], np.ascontiguousarray(got[:, :K, :].transpose(0, 2, 1))) and np.count_nonzero(got) > got.size // 2


# ------------------------------------------------------------------------------------------------ the widest tile
WIDE = 8261  # automatic T = 8192 and a second tile of 69; above n_top = 512 T = 8128 and 133


def wide_data(mfx):
    """400 x 8 261 with 25 entries per row on average, a support at K = 8 of items that share users, the reference's blocks
    (pair by pair: the dense 8 261 x 8 261 sums are not built), weights and 60 query rows of up to 40 entries."""
    X = random_matrix(mfx, 400, WIDE, 10000, 3601)
    S = neighbour_support(X, 8, 3602)
    return X, S, sx.gram_blocks_sparse(X, S), weights_for(S, 3603), random_rows(WIDE, 60, 3606, max_len=40)


@pytest.mark.parametrize("tile", [0, 8192, 64])
def test_gram_on_the_widest_tile(mfx, tile):
    """The launch with 65 600 bytes of LDS (T = 8192), automatic and asked for, with a second tile of 69; tiles of 64 give the
    same."""
    X, S, want, w, rows = once("slim_wide", lambda: wide_data(mfx))
    real = S != PAD
    assert (S[real] >= 8192).any() and real[8192:].any() and (~real).any() and set(real.sum(axis=1)) == set(range(9))
    assert np.count_nonzero(want[8192:]) > 0 and np.count_nonzero(want[:, 8, :]) > real.sum() // 2
    got = mfx.slim_gram(X, 8, S, tile_items=tile)
    assert same(got, want), (tile, int((bits(got) != bits(want)).sum()))


@pytest.fixture(scope="module")
def wide_model(mfx):
    X, S, blocks, w, rows = once("slim_wide", lambda: wide_data(mfx))
    m = mfx.Slim.from_lists(S, w)
    yield m, S, w, rows
    m.close()


@pytest.mark.parametrize("n_top,tile", [(10, 0), (10, 8192), (10, 64), (600, 0), (600, 8128)])
def test_recommend_on_the_widest_tile(mfx, wide_model, n_top, tile):
    """The launches with 73 792 (T = 8192, 1 024 slots) and 81 472 bytes (T = 8128, 2 048 slots) of LDS, automatic and asked for,
    each with a second tile; tiles of 64 must give the same."""
    m, S, w, rows = wide_model
    targets = sx.transpose(S, w)[1]
    assert lens_of(rows[0]).max() == 40 and (S[S != PAD] >= 8192).any() and (targets >= 8192).any()
    for keep_seen in (False, True):
        want = once(("slim_wide_want", n_top, keep_seen), lambda: sx.recommend(S, w, *rows, n_top, keep_seen))
        assert want[2] == 0 and (want[0] >= 8192).any() and (want[0] == PAD).any()
        check_rec(m, want, rows, n_top, keep_seen, tile)


# ------------------------------------------------------------------------------------------------ the item stride
MANY = 262144 + 3  # k_slim_diag and k_knn_work launch at most 65 536 workgroups of four waves


def many_items(mfx):
    """2 000 x 262 147, two entries per column in different rows (rows of some 262 entries), a support at K = 2 of items of
    the same row with pads; items 0 .. 2 name the last three items first, whose d k_slim_diag computes in its second turn."""
    rng = np.random.default_rng(3701)
    first = rng.integers(0, 2000, MANY)
    second = (first + rng.integers(1, 2000, MANY)) % 2000
    X = mfx.dataset.from_coo(2000, MANY, np.concatenate([first, second]), np.tile(np.arange(MANY), 2), rng.standard_normal(2 * MANY).astype(F))
    S = neighbour_support(X, 2, 3702)
    for j in range(3):
        S[j] = (MANY - 1 - j, S[j, 0] if S[j, 0] not in (PAD, MANY - 1 - j) else 100 + j)
    return X, S, sx.gram_blocks_sparse(X, S)


def test_gram_and_train_with_more_items_than_waves(mfx):
    """262 147 items: the wave-per-item kernels (k_slim_diag, k_knn_work) take a second turn for the last three items, the
    Gram pass walks 33 tiles of 8192 per item, every wave of the solve takes about 32 items (K = 2: four waves, 2 048
    workgroups)."""
    X, S, want = once("slim_many", lambda: many_items(mfx))
    assert X.cols == MANY > 65536 * 4 and np.all(lens_of(X.csc_col_ptr) == 2) and set(sx.real_slots(S)) == {0, 1, 2}
    d = kx.from_fixed(sx.diagonal(X)[0])
    assert np.all(d[-3:] != 0) and [want[j, 0, 0] for j in range(3)] == [d[MANY - 1], d[MANY - 2], d[MANY - 3]]
    assert np.count_nonzero(want[:, 2, :]) > MANY // 2 and np.count_nonzero(want[-3:]) > 0
    got = mfx.slim_gram(X, 2, S)
    assert same(got, want), int((bits(got) != bits(want)).sum())
    kw = dict(l1=0.01, l2=0.1, sweeps=2, tol=0.0, signed=True)
    w, used, failed = sx.solve(want, sx.real_slots(S), **kw)
    assert failed == 0 and w[-3:].any() and (w < 0).any() and (w > 0).any() and MANY // (4 * 8 * cus()) >= 31
    with mfx.Slim(X, 2, support=S, **kw) as m:
        got_S, got_w = m.weights()
        assert m.failed == 0 and np.array_equal(m.sweeps_used, used)
    assert same(got_S, S) and same(got_w, w), int((bits(got_w) != bits(w)).sum())


# ------------------------------------------------------------------------------------------------ the 2^21 limits
ONE_EACH = np.array([[1], [0]], np.uint32)  # cols = 2, K = 1: each item's support is the other


def test_gram_and_train_refuse_a_column_one_past_the_limit(mfx):
    """2^21 + 1 users in column 0 (the reference is not called)."""
    n = LIMIT + 1
    X = two_columns(mfx, n, np.ones(n, F), 2, np.ones(2, F))
    X.validate()
    assert tuple(lens_of(X.csc_col_ptr)) == (LIMIT + 1, 2)
    with pytest.raises(mfx.MfxError, match="item 0:"):
        mfx.slim_gram(X, 1, ONE_EACH)
    with pytest.raises(mfx.MfxError, match="item 0:"):
        mfx.Slim(X, 1, support=ONE_EACH)


def test_gram_at_the_limit(mfx):
    """2^21 users in both columns: 4 096 batches of 64 users per wave and sums of 2^21 terms, off and on the diagonal, computed
    here directly."""
    rng = np.random.default_rng(3801)
    x0, x1 = rng.standard_normal(LIMIT).astype(F), rng.standard_normal(LIMIT).astype(F)
    X = two_columns(mfx, LIMIT, x0, LIMIT, x1)
    X.validate()
    assert tuple(lens_of(X.csc_col_ptr)) == (LIMIT, LIMIT)
    t = x0 * x1
    assert t.dtype == F and np.abs(t).max() < 64
    g = kx.from_fixed(kx.to_fixed(t).sum())
    d, bad = sx.diagonal(X)
    assert bad is None and g != 0 and d[0] == kx.to_fixed(x0 * x0).sum() and d[1] == kx.to_fixed(x1 * x1).sum()
    d = kx.from_fixed(d)
    want = np.array([[[d[1]], [g]], [[d[0]], [g]]], F)  # block j: d of its one support item, then the pair
    got = mfx.slim_gram(X, 1, ONE_EACH)
    assert same(got, want), (got, want)


def test_recommend_refuses_a_row_one_past_the_limit(mfx):
    """A query row of 2^21 + 1 entries between two short ones: all pads and counted, its neighbours as in the reference."""
    cols = LIMIT + 64
    S = np.full((cols, 1), PAD, np.uint32)
    w = np.zeros((cols, 1), F)
    for j, (i, x) in {0: (7, 0.5), 5: (LIMIT + 10, -1.25), 7: (0, 2.0), LIMIT: (5, 3.0), LIMIT + 10: (8200, 0.75)}.items():
        S[j, 0], w[j, 0] = i, x  # (target j takes x_i * x from source i)
    rows = rows_from([(np.array([0, 5]), np.array([1.0, 2.0])), (np.arange(LIMIT + 1), np.ones(LIMIT + 1)),
                      (np.array([5, 7, LIMIT, LIMIT + 10]), np.array([-1.0, 0.5, 1.5, 2.0]))])
    assert tuple(lens_of(rows[0])) == (2, LIMIT + 1, 4)
    want = sx.recommend(S, w, *rows, 4)
    assert want[2] == 1 and np.all(want[0][1] == PAD) and np.all(np.isneginf(want[1][1]))
    assert list(want[0][0]) == [LIMIT, 7, PAD, PAD] and list(want[1][0][:2]) == [6.0, 2.0]  # 2 * 3 from item 5, 1 * 2 from item 0
    assert list(want[0][2]) == [0, PAD, PAD, PAD] and want[1][2][0] == 0.25  # 0.5 * 0.5 from item 7; items 5 and LIMIT are its own
    with mfx.Slim.from_lists(S, w) as m:
        check_rec(m, want, rows, 4, False)
