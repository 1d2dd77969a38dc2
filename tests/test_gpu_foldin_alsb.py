"""Fold-in by block subspace sweeps on the explicit objectives (mfx_rec_fold_in_block_setup_als / mfx_rec_fold_in_warm,
Recommender.fold_in_block_setup_als): S sweeps against S chained mfx.als_block_half calls bit for bit, the stop rule per
row, a single block against the direct models MFX_FOLD_ALS / MFX_FOLD_CCD, the lists against the exact fp32 reference of
tests/rec_exact.py, and the three kinds of setup replacing each other.  Bits are compared as uint32, -0 included.

Data: 6000 columns, the segment sizes of the operator tests (0, 1, 2 and 3 chunks of 2048 entries, empty rows),
H ~ N(0, 1/k), lambda = 0.1.  Measured figures are printed as `alsb-measured` lines (profiles/r12_alsb_accuracy.txt)."""
import numpy as np
import pytest

import alsb_ref
from rec_exact import chain_scores, eligible_mask, expected_topn
from test_gpu_foldin import F32, MFX_ERR_INVALID, SIZES, factors, handle, same, segments, select

pytestmark = pytest.mark.gpu

COLS, LAM = 6000, 0.1
CASES = [(130, 128), (160, 64), (192, 32), (512, 96), (1024, 128), (100, 128), (37, 5)]  # last block 2, 32, 96 wide; d > k; k <= 128


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1, m.lib().mfx_last_error()
    return m


def data(k, zero_frac=0.15):
    ptr, idx, val = segments(100 + k, COLS, SIZES, zero_frac=zero_frac)
    _, H = factors(k, COLS, k)
    return ptr, idx, val, H


def bad_rows(a, b):
    return np.nonzero((a.view(np.uint32) != b.view(np.uint32)).any(axis=1))[0].tolist()


# ------------------------------------------------------------------------------------------------ 1. chained operator
@pytest.mark.parametrize("k,d", CASES)
def test_sweeps_equal_chained_block_halves(mfx, k, d):
    ptr, idx, val, H = data(k)
    layout = CASES.index((k, d)) % 2
    W0 = (0.1 * np.random.default_rng(1000 + k).standard_normal((len(SIZES), k))).astype(F32)
    with handle(mfx, np.zeros((3, k), F32), H, layout) as r:
        for reg in (0, 1):
            firsts = []
            for start in (None, W0):
                want, Y = {}, start
                for s in (1, 2, 3):
                    Y = mfx.als_block_half(ptr, idx, val, H, k, LAM, d, Y_in=Y, count_reg=bool(reg))
                    want[s] = Y
                firsts.append(want[1])
                for S in (1, 3):
                    r.fold_in_block_setup_als(LAM, block=d, sweeps=S, count_reg=bool(reg))
                    _, _, got, done = r.fold_in((ptr, idx, val), W_init=start, return_sweeps=True)
                    assert bad_rows(got, want[S]) == [], (k, d, layout, reg, S, start is not None)
                    assert done.dtype == np.int32 and done.tolist() == [S if n else 0 for n in SIZES]
                    for s, n in enumerate(SIZES):
                        if n == 0:  # whatever W_init held
                            assert same(got[s], np.zeros(k, F32)), (k, d, S, s)
                    if start is None:  # mfx_rec_fold_in after this setup: the warm call without a start row and counts
                        assert same(r.fold_in((ptr, idx, val))[2], got)
            if d < k:  # W_init is honoured: more than one block, so the start shows in the result
                assert not same(firsts[0], firsts[1]), (k, d, reg)


@pytest.mark.parametrize("k,default", [(160, 64), (37, 37)])
def test_block_zero_is_the_default_block(mfx, k, default):
    ptr, idx, val, H = data(k)
    want = mfx.als_block_half(ptr, idx, val, H, k, LAM, default)
    assert same(want, mfx.als_block_half(ptr, idx, val, H, k, LAM, 0))
    with handle(mfx, np.zeros((3, k), F32), H, 1) as r:
        r.fold_in_block_setup_als(LAM, sweeps=1)
        assert same(r.fold_in((ptr, idx, val))[2], want)


# ------------------------------------------------------------------------------------------------ 2. per-row stop
@pytest.mark.parametrize("reg", [0, 1])
def test_rows_stop_on_their_own(mfx, reg):
    k, d, tol, sweeps = 160, 64, 1e-3, 64
    ptr, idx, val, H = data(k)
    nonempty = np.array(SIZES) > 0
    with handle(mfx, np.zeros((3, k), F32), H, 1) as r:
        r.fold_in_block_setup_als(LAM, block=d, sweeps=sweeps, tol=tol, count_reg=bool(reg))
        bi, bs, got, cnt = r.fold_in((ptr, idx, val), 10, return_sweeps=True)
        dist = []
        for s in np.nonzero(nonempty)[0]:
            want = np.linalg.solve(*alsb_ref.dense_system(ptr, idx, val, s, H, LAM, reg))
            dist.append(float(np.linalg.norm(got[s] - want) / np.linalg.norm(want)))
        print(f"alsb-measured per-row-stop k={k} d={d} reg={reg} tol={tol} counts={cnt.tolist()} worst_distance={max(dist):.3e}")
        assert cnt.dtype == np.int32
        assert not cnt[~nonempty].any() and not got[~nonempty].any()
        assert cnt[nonempty].min() >= 1 and cnt[nonempty].max() <= sweeps, cnt.tolist()
        assert cnt[nonempty].min() < sweeps and len(set(cnt[nonempty].tolist())) >= 2, cnt.tolist()  # the rule did stop rows, at different times
        # a row alone, and in a shuffled batch with repeats: the same bits, the same count, the same list
        rng = np.random.default_rng(4)
        sel = np.concatenate([rng.permutation(len(SIZES)), [2, 5, 5, 0, 9]])
        gi, gs, gw, gc = r.fold_in(select(ptr, idx, val, sel), 10, return_sweeps=True)
        assert same(gw, got[sel]) and np.array_equal(gc, cnt[sel]) and same(gi, bi[sel]) and same(gs, bs[sel])
        for s in (0, 1, 5, 9):
            ai, as_, aw, ac = r.fold_in(select(ptr, idx, val, [s]), 10, return_sweeps=True)
            assert same(aw[0], got[s]) and ac[0] == cnt[s] and same(ai[0], bi[s]) and same(as_[0], bs[s]), s
        # a frozen row's bits never change: it is the row after exactly that many sweeps
        for c in sorted(set(cnt[nonempty].tolist())):
            r.fold_in_block_setup_als(LAM, block=d, sweeps=c, count_reg=bool(reg))
            fixed = r.fold_in((ptr, idx, val))[2]
            rows = np.nonzero(cnt == c)[0]
            assert same(fixed[rows], got[rows]), (c, rows.tolist())


# ------------------------------------------------------------------------------------------------ 3. the direct models
@pytest.mark.parametrize("k", [16, 64, 100, 128])
def test_a_single_block_agrees_with_the_direct_models(mfx, k):
    ptr, idx, val, H = data(k)
    with handle(mfx, np.zeros((3, k), F32), H, k % 2) as r:
        for reg, model in ((0, mfx.MFX_FOLD_ALS), (1, mfx.MFX_FOLD_CCD)):
            r.fold_in_setup(model, LAM)
            want = r.fold_in((ptr, idx, val))[2]
            r.fold_in_block_setup_als(LAM, block=128, sweeps=1, count_reg=bool(reg))
            got = r.fold_in((ptr, idx, val))[2]
            rel = []
            for s, n in enumerate(SIZES):
                if n == 0:
                    assert same(got[s], np.zeros(k, F32)) and same(want[s], np.zeros(k, F32))
                    continue
                rel.append(float(np.linalg.norm(got[s].astype(np.float64) - want[s]) / np.linalg.norm(want[s])))
            print(f"alsb-measured direct-model k={k} reg={reg} max_rel={max(rel):.3e}")
            assert max(rel) <= 1e-3, (k, reg, rel)


# ------------------------------------------------------------------------------------------------ 4. lists
@pytest.mark.parametrize("layout", [0, 1])
def test_lists_equal_query_and_the_exact_reference_on_the_solved_rows(mfx, layout):
    cols, k, d, n_top = 3001, 160, 64, 10
    rng = np.random.default_rng(50 + layout)
    sizes = list(rng.integers(0, 400, 40))
    sizes[::11] = [0] * len(sizes[::11])
    sizes += [cols - 5, cols, 2500]  # fewer than n_top eligible items: padded lists
    ptr, idx, val = segments(60 + layout, cols, sizes)
    W, H = factors(60 + layout, cols, k)
    H[2000:2100] = H[10:110]  # ties across tiles: ordered by item
    n = len(sizes)
    ex = mfx.dataset.from_coo(n, cols, np.repeat(np.arange(n), np.diff(ptr.astype(np.int64))), idx, val)
    assert np.array_equal(ex.csr_row_ptr, ptr) and np.array_equal(ex.csr_col_idx, idx)
    with handle(mfx, W, H, layout) as r:
        r.fold_in_block_setup_als(LAM, block=d, sweeps=2, count_reg=bool(layout))
        items, scores, Wq = r.fold_in((ptr, idx, val), n_top)
        assert same(Wq, r.fold_in((ptr, idx, val))[2])
    with mfx.Recommender(Wq, H, 1, exclude=ex) as r2:
        qi, qs = r2.query(n_top)
    assert same(items, qi) and same(scores, qs), layout
    wi, ws = expected_topn(chain_scores(Wq, H, np.arange(n)), eligible_mask(ex, np.arange(n), cols), n_top)
    assert same(items, wi) and same(scores, ws), layout
    assert (items[-2] == 0xFFFFFFFF).all() and (items[-3, 5:] == 0xFFFFFFFF).all()


# ------------------------------------------------------------------------------------------------ 5. setups, refusals
def _warm(mfx, r, ptr, idx, val, n_top=5, W_init=None):
    from mfx.api import _vp
    n = len(ptr) - 1
    W, items, done = np.empty((n, r.k), F32), np.empty((n, n_top), np.uint32), np.empty(n, np.int32)
    rc = mfx.lib().mfx_rec_fold_in_warm(r.handle, n, idx.size, _vp(ptr), _vp(idx), _vp(val), _vp(W_init), _vp(W), _vp(done),
                                        n_top, _vp(items), None, 0)
    return rc, mfx.lib().mfx_last_error().decode()


def test_refusals_leave_the_handle_usable(mfx):
    cols, k = 500, 160
    ptr, idx, val = segments(7, cols, [3, 0, 10, 25])  # rows 0..3 at positions [0, 3), [3, 3), [3, 13), [13, 38)
    W, H = factors(7, cols, k)
    nan, inf = float("nan"), float("inf")
    with mfx.Recommender(W, H, 1) as r:
        r.fold_in_block_setup_als(LAM, block=64, sweeps=3, tol=1e-3)
        good = r.fold_in((ptr, idx, val), 5, return_sweeps=True)
        again = lambda: all(same(a, b) for a, b in zip(r.fold_in((ptr, idx, val), 5, return_sweeps=True), good))
        # (lambda, reg, block, sweeps, tol)
        for bad, word in (((LAM, 0, -1, 3, 0.0), "block"), ((LAM, 0, 129, 3, 0.0), "block"), ((LAM, 0, 64, 0, 0.0), "sweeps"),
                          ((LAM, 0, 64, 1025, 0.0), "sweeps"), ((LAM, 0, 64, 3, -1.0), "tol"), ((LAM, 0, 64, 3, nan), "tol"),
                          ((LAM, 0, 64, 3, inf), "tol"), ((0.0, 0, 64, 3, 0.0), "lambda"), ((nan, 0, 64, 3, 0.0), "lambda"),
                          ((inf, 1, 64, 3, 0.0), "lambda"), ((LAM, 2, 64, 3, 0.0), "reg"), ((LAM, -1, 64, 3, 0.0), "reg")):
            assert mfx.lib().mfx_rec_fold_in_block_setup_als(r.handle, *bad) == MFX_ERR_INVALID, bad
            assert word in mfx.lib().mfx_last_error().decode(), bad
            assert again(), bad
        cases = []
        i = idx.copy(); i[20] = cols; cases.append(("index >= cols", ptr, i, val))
        i = idx.copy(); i[[5, 6]] = i[[6, 5]]; cases.append(("decreasing ids", ptr, i, val))
        p = ptr.copy(); p[2] = 14; cases.append(("ptr not monotone", p, idx, val))
        p = ptr.copy(); p[-1] = 37; cases.append(("ptr[U] != nnz", p, idx, val))
        for bad in (nan, inf, -inf):
            v = val.copy(); v[17] = bad; cases.append((f"value {bad}", ptr, idx, v))
        for what, p, i, v in cases:
            rc, msg = _warm(mfx, r, p, i, v)
            assert rc == MFX_ERR_INVALID, (what, rc, msg)
            assert again(), what
        v = val.copy(); v[17] = -2.0  # a negative value is an entry like any other
        assert _warm(mfx, r, ptr, idx, v)[0] == 0


def test_the_three_setups_replace_each_other(mfx):
    cols, k = 500, 64
    ptr, idx, val = segments(7, cols, [3, 0, 10, 25])
    W, H = factors(8, cols, k)
    direct = mfx.als_half(ptr, idx, val, H, k, LAM)
    implicit = mfx.ials_block_half(ptr, idx, val, H, k, LAM, 2.0, 16)
    explicit = mfx.als_block_half(ptr, idx, val, H, k, LAM, 16)
    explicit_n = mfx.als_block_half(ptr, idx, val, H, k, LAM, 16, count_reg=True)
    assert not same(direct, explicit) and not same(implicit, explicit) and not same(explicit, explicit_n)
    with mfx.Recommender(W, H, 1) as r:
        rc, msg = _warm(mfx, r, ptr, idx, val)
        assert rc == MFX_ERR_INVALID and "mfx_rec_fold_in_block_setup_als" in msg
        for _ in range(2):
            r.fold_in_block_setup_als(LAM, block=16, sweeps=1)
            assert same(r.fold_in((ptr, idx, val))[2], explicit)
            assert _warm(mfx, r, ptr, idx, val)[0] == 0
            r.fold_in_block_setup(LAM, 2.0, block=16, sweeps=1)
            assert same(r.fold_in((ptr, idx, val))[2], implicit)
            r.fold_in_block_setup_als(LAM, block=16, sweeps=1, count_reg=True)
            assert same(r.fold_in((ptr, idx, val))[2], explicit_n)
            r.fold_in_setup(mfx.MFX_FOLD_ALS, LAM)
            assert same(r.fold_in((ptr, idx, val))[2], direct)
            rc, msg = _warm(mfx, r, ptr, idx, val)
            assert rc == MFX_ERR_INVALID and "mfx_rec_fold_in_block_setup_als" in msg
            assert same(r.fold_in((ptr, idx, val))[2], direct)
