"""Fold-in on the implicit objective with an unobserved weight and a frequency-scaled regulariser
(mfx_rec_fold_in_setup_reg / mfx_rec_fold_in_block_setup_reg; Recommender.fold_in_setup with alpha0= / nu=,
Recommender.fold_in_block_setup_reg) checked bit for bit against the paths it reuses: the direct solve against mfx.ials_half(alpha0=, nu=) of the
same rows over the handle's H, S sweeps against S chained mfx.ials_block_half(alpha0=, nu=) calls, one sweep from the
trainer's factors against the trainer's next user half, a row stopped by the rule against the same row in another batch,
the lists against mfx_rec_query on the solved rows.  Bits are compared as uint32, -0 included.  A query row has N = cols
and n_u = its entries with r > 0.  Data: that of tests/test_gpu_foldin.py and test_gpu_foldin_block.py."""
import numpy as np
import pytest

from test_gpu_foldin import F32, MFX_ERR_INVALID, SIZES, _matrix, factors, handle, same, segments, select

pytestmark = pytest.mark.gpu

COLS = 6000
PARAMS = [(0.3, 0.5, 0.1), (2.0, 1.0, 0.002), (1.0, 0.25, 0.1)]  # (alpha0, nu, lambda)


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


# ------------------------------------------------------------------------------------------------ 1. single operators
@pytest.mark.parametrize("k", [1, 5, 16, 36, 60, 64, 68, 100, 128])
def test_fold_in_equals_ials_half_reg(mfx, k):
    ptr, idx, val, H = data(k)
    layout = k % 2
    alpha0, nu, lam = PARAMS[k % 3]
    with handle(mfx, np.zeros((3, k), F32), H, layout) as r:
        for alpha in (0.0, 2.0, 40.0):
            want = mfx.ials_half(ptr, idx, val, H, k, lam, alpha, alpha0=alpha0, nu=nu)
            r.fold_in_setup(mfx.MFX_FOLD_IMPLICIT, lam, alpha, alpha0=alpha0, nu=nu)
            items, scores, got = r.fold_in((ptr, idx, val), 0)
            assert items is None and scores is None
            assert bad_rows(got, want) == [], (k, layout, alpha)
            for s, n in enumerate(SIZES):
                if n == 0:
                    assert same(got[s], np.zeros(k, F32))
        # rho_u comes from the row's own entries: any sub-batch, in any order, gives the same bits
        rows = [9, 1, 4, 4, 0, 8]
        sub = r.fold_in(select(ptr, idx, val, rows), 0)[2]
        assert same(sub, got[rows]), k
        # (alpha0, nu) = (1, 0) is the plain implicit fold-in
        r.fold_in_setup(mfx.MFX_FOLD_IMPLICIT, lam, 2.0, alpha0=1.0, nu=0.0)
        a = r.fold_in((ptr, idx, val), 0)[2]
        r.fold_in_setup(mfx.MFX_FOLD_IMPLICIT, lam, 2.0)
        assert same(a, r.fold_in((ptr, idx, val), 0)[2]), k


@pytest.mark.parametrize("k,d", [(130, 128), (160, 64), (1024, 128), (100, 128), (37, 5)])
def test_sweeps_equal_chained_block_halves_reg(mfx, k, d):
    ptr, idx, val, H = data(k)
    cases = [(130, 128), (160, 64), (1024, 128), (100, 128), (37, 5)]
    alpha, layout = 2.0, cases.index((k, d)) % 2
    alpha0, nu, lam = PARAMS[cases.index((k, d)) % 3]
    W0 = (0.1 * np.random.default_rng(1000 + k).standard_normal((len(SIZES), k))).astype(F32)
    with handle(mfx, np.zeros((3, k), F32), H, layout) as r:
        for start in (None, W0):
            want, Y = {}, start
            for s in (1, 2, 3):
                Y = mfx.ials_block_half(ptr, idx, val, H, k, lam, alpha, d, Y_in=Y, alpha0=alpha0, nu=nu)
                want[s] = Y
            for S in (1, 3):
                r.fold_in_block_setup_reg(lam, alpha, alpha0, nu, block=d, sweeps=S, tol=0.0)
                _, _, got, done = r.fold_in((ptr, idx, val), W_init=start, return_sweeps=True)
                assert bad_rows(got, want[S]) == [], (k, d, layout, S, start is not None)
                assert done.dtype == np.int32 and done.tolist() == [S if n else 0 for n in SIZES]
                for s, n in enumerate(SIZES):
                    if n == 0:
                        assert same(got[s], np.zeros(k, F32)), (k, d, S, s)
                if start is None:
                    assert same(r.fold_in((ptr, idx, val))[2], got)


# ------------------------------------------------------------------------------------------------ 2. training step
@pytest.mark.parametrize("k,d", [(16, None), (64, None), (100, None), (160, 64)])
def test_fold_in_of_training_rows_is_the_next_user_half(mfx, k, d):
    R = _matrix(10 + k)
    alpha0, nu, lam = PARAMS[0]
    alpha = 3.0
    p = mfx.parameter()
    p.k, p.lambda_ = k, lam
    kw = dict(alpha0=alpha0, nu=nu) if d is None else dict(alpha0=alpha0, nu=nu, block=d)
    s = mfx.ImplicitAlsSolver(R, p, alpha, **kw)
    s.set_factors((np.random.default_rng(k).standard_normal((R.cols, k)) * 0.1).astype(F32))
    s.iterate(2)
    W0, H0 = s.get_factors()
    s.iterate(1)
    W1, _ = s.get_factors()
    s.close()
    with mfx.Recommender(W0, H0, 1) as r:
        if d is None:
            r.fold_in_setup(mfx.MFX_FOLD_IMPLICIT, lam, alpha, alpha0=alpha0, nu=nu)
            items, scores, W = r.fold_in(R)
        else:
            r.fold_in_block_setup_reg(lam, alpha, alpha0, nu, block=d, sweeps=1)
            items, scores, W = r.fold_in(R, W_init=W0)
    assert items is None and scores is None
    assert bad_rows(W, W1) == []
    assert not W[[3, 77, 250]].any()


# ------------------------------------------------------------------------------------------------ 3. per-row stop
def test_rows_stop_on_their_own_whatever_the_batch(mfx):
    """k = 160, d = 64, alpha = 40, (alpha0, nu, lambda) = (0.3, 0.5, 0.1), tol = 1e-4: the rule in fp64 (tests/ials_reg_ref.py
    block_sweep, computed on the CPU) stops the nine non-empty rows after 13, 21, 21, 23, 7, 7, 7, 5 and 19 sweeps: the rows
    stop at different sweeps, all within the 32 allowed."""
    k, d, alpha, tol, sweeps = 160, 64, 40.0, 1e-4, 32
    alpha0, nu, lam = PARAMS[0]
    ptr, idx, val, H = data(k, 0.0)
    with handle(mfx, np.zeros((3, k), F32), H, 1) as r:
        r.fold_in_block_setup_reg(lam, alpha, alpha0, nu, block=d, sweeps=sweeps, tol=tol)
        _, _, got, cnt = r.fold_in((ptr, idx, val), return_sweeps=True)
        nonempty = np.array([n > 0 for n in SIZES])
        print(f"ialsr-measured per-row-stop k={k} d={d} alpha={alpha} alpha0={alpha0} nu={nu} tol={tol} counts={cnt.tolist()}")
        assert (cnt[~nonempty] == 0).all() and cnt[nonempty].min() >= 1 and cnt[nonempty].max() <= sweeps, cnt.tolist()
        assert len(set(cnt[nonempty].tolist())) >= 2, cnt.tolist()  # the rows do stop at different sweeps
        # two batches that share rows: a row's bits and its count are those of the full batch
        for rows in ([1, 2, 4, 5, 9], [9, 5, 0, 10, 10, 6, 2]):
            _, _, g, c = r.fold_in(select(ptr, idx, val, rows), return_sweeps=True)
            assert same(g, got[rows]), rows
            assert c.tolist() == cnt[rows].tolist(), (rows, c.tolist())
        # a row stopped after c sweeps holds the bits of exactly c sweeps with tol = 0
        for c in sorted(set(cnt[nonempty].tolist())):
            rows = np.nonzero(cnt == c)[0]
            r.fold_in_block_setup_reg(lam, alpha, alpha0, nu, block=d, sweeps=int(c), tol=0.0)
            fixed = r.fold_in((ptr, idx, val))[2]
            assert same(fixed[rows], got[rows]), (c, rows.tolist())


# ------------------------------------------------------------------------------------------------ 4. lists and the filter
@pytest.mark.parametrize("block", [None, 64])
def test_lists_exclusion_and_item_filter(mfx, block):
    cols, k, n_top = 3001, 64 if block is None else 160, 10
    alpha0, nu, lam = PARAMS[2]
    rng = np.random.default_rng(50)
    sizes = list(rng.integers(0, 400, 40))
    sizes[::11] = [0] * len(sizes[::11])
    sizes += [cols - 5, cols, 2500]  # fewer than n_top eligible items: padded lists
    ptr, idx, val = segments(60, cols, sizes)
    W, H = factors(60, cols, k)
    n = len(sizes)
    ex = mfx.dataset.from_coo(n, cols, np.repeat(np.arange(n), np.diff(ptr.astype(np.int64))), idx, val)
    keep = rng.random(cols) < 0.5
    with handle(mfx, W, H, 1) as r:
        if block is None:
            r.fold_in_setup(mfx.MFX_FOLD_IMPLICIT, lam, 2.0, alpha0=alpha0, nu=nu)
        else:
            r.fold_in_block_setup_reg(lam, 2.0, alpha0, nu, block=block, sweeps=2)
        items, scores, Wq = r.fold_in((ptr, idx, val), n_top)
        assert same(Wq, r.fold_in((ptr, idx, val))[2])
        r.set_item_filter(keep)
        fitems, fscores, Wf = r.fold_in((ptr, idx, val), n_top)
        r.set_item_filter(None)
        assert same(Wf, Wq)  # the filter does not touch the solve
    with mfx.Recommender(Wq, H, 1, exclude=ex) as r2:
        qi, qs = r2.query(n_top)
        r2.set_item_filter(keep)
        fi, fs = r2.query(n_top)
    assert same(items, qi) and same(scores, qs)
    assert same(fitems, fi) and same(fscores, fs)
    assert (items[-2] == 0xFFFFFFFF).all() and (items[-3, 5:] == 0xFFFFFFFF).all()
    for u in range(n):  # the row's own items are excluded, the filtered lists hold kept items only
        own = set(idx[ptr[u]:ptr[u + 1]].tolist())
        assert not own & set(items[u].tolist()), u
        assert all(i == 0xFFFFFFFF or keep[i] for i in fitems[u].tolist()), u


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_leave_the_handle_usable(mfx):
    cols, k = 500, 64
    ptr, idx, val = segments(7, cols, [3, 0, 10, 25])
    W, H = factors(7, cols, k)
    nan, inf = float("nan"), float("inf")
    lib = mfx.lib()
    alpha0, nu, lam = PARAMS[0]
    direct = mfx.ials_half(ptr, idx, val, H, k, lam, 2.0, alpha0=alpha0, nu=nu)
    block = mfx.ials_block_half(ptr, idx, val, H, k, lam, 2.0, 16, alpha0=alpha0, nu=nu)
    plain = mfx.ials_half(ptr, idx, val, H, k, lam, 2.0)
    assert not same(direct, block) and not same(direct, plain)
    with mfx.Recommender(W, H, 1) as r:
        r.fold_in_setup(mfx.MFX_FOLD_IMPLICIT, lam, 2.0, alpha0=alpha0, nu=nu)
        good = r.fold_in((ptr, idx, val), 5)
        assert same(good[2], direct)
        again = lambda: all(same(a, b) for a, b in zip(r.fold_in((ptr, idx, val), 5), good))
        for bad, word in (((lam, 2.0, 0.0, nu), "alpha0"), ((lam, 2.0, -1.0, nu), "alpha0"), ((lam, 2.0, nan, nu), "alpha0"),
                          ((lam, 2.0, inf, nu), "alpha0"), ((lam, 2.0, alpha0, -0.1), "nu"), ((lam, 2.0, alpha0, 1.1), "nu"),
                          ((lam, 2.0, alpha0, nan), "nu"), ((3e38, 2.0, 1.0, 1.0), "regulariser"), ((0.0, 2.0, alpha0, nu), "lambda"),
                          ((nan, 2.0, alpha0, nu), "lambda"), ((lam, -1.0, alpha0, nu), "alpha"), ((lam, inf, alpha0, nu), "alpha")):
            assert lib.mfx_rec_fold_in_setup_reg(r.handle, *bad) == MFX_ERR_INVALID, bad
            assert word in lib.mfx_last_error().decode(), (bad, lib.mfx_last_error())
            assert again(), bad
            assert lib.mfx_rec_fold_in_block_setup_reg(r.handle, *bad, 16, 3, 0.0) == MFX_ERR_INVALID, bad
            assert word in lib.mfx_last_error().decode(), (bad, lib.mfx_last_error())
            assert again(), bad
        for bad in ((-1, 3, 0.0), (129, 3, 0.0), (16, 0, 0.0), (16, 1025, 0.0), (16, 3, -1.0), (16, 3, nan)):
            assert lib.mfx_rec_fold_in_block_setup_reg(r.handle, lam, 2.0, alpha0, nu, *bad) == MFX_ERR_INVALID, bad
            assert again(), bad
        # device-checked refusals of a query: bad strengths, ids, pointers, and a bad memory space
        from mfx.api import _vp
        def query(p, i, v, space=0):
            Wo, it = np.empty((len(p) - 1, k), F32), np.empty((len(p) - 1, 5), np.uint32)
            return lib.mfx_rec_fold_in(r.handle, len(p) - 1, i.size, _vp(p), _vp(i), _vp(v), _vp(Wo), 5, _vp(it), None, space)
        assert query(ptr, idx, val) == 0
        cases = []
        i = idx.copy(); i[20] = cols; cases.append(("index >= cols", ptr, i, val))
        i = idx.copy(); i[[5, 6]] = i[[6, 5]]; cases.append(("decreasing ids", ptr, i, val))
        p = ptr.copy(); p[-1] = 37; cases.append(("ptr[U] != nnz", p, idx, val))
        for b in (-1.0, nan, inf, 3e38):
            v = val.copy(); v[17] = b; cases.append((f"strength {b}", ptr, idx, v))
        for what, p, i, v in cases:
            assert query(p, i, v) == MFX_ERR_INVALID, what
            assert again(), what
        assert query(ptr, idx, val, space=7) == MFX_ERR_INVALID
        assert "memory space" in lib.mfx_last_error().decode()
        assert again()
        # the last successful setup decides, of whatever kind
        for _ in range(2):
            r.fold_in_block_setup_reg(lam, 2.0, alpha0, nu, block=16, sweeps=1)
            assert same(r.fold_in((ptr, idx, val))[2], block)
            r.fold_in_setup(mfx.MFX_FOLD_IMPLICIT, lam, 2.0)
            assert same(r.fold_in((ptr, idx, val))[2], plain)
            r.fold_in_setup(mfx.MFX_FOLD_IMPLICIT, lam, 2.0, alpha0=alpha0, nu=nu)
            assert same(r.fold_in((ptr, idx, val))[2], direct)
            r.fold_in_block_setup(lam, 2.0, block=16, sweeps=1)
            assert same(r.fold_in((ptr, idx, val))[2], mfx.ials_block_half(ptr, idx, val, H, k, lam, 2.0, 16))
            r.fold_in_setup(mfx.MFX_FOLD_IMPLICIT, lam, 2.0, alpha0=alpha0, nu=nu)
            assert same(r.fold_in((ptr, idx, val))[2], direct)
        with pytest.raises(ValueError):
            r.fold_in_setup(mfx.MFX_FOLD_ALS, lam, 0.0, alpha0=alpha0)
