"""Fold-in recommendation (mfx_rec_fold_in_setup / mfx_rec_fold_in, mfx.Recommender.fold_in) checked bit for bit:
the solved rows against the training step and the single operators they reuse (mfx.als_half variants 1 / 0,
mfx.ials_half), the CCD++ row minimiser against mfx.als_half with lambda * n_u, and the lists against mfx_rec_query on
the solved rows and the exact fp32 reference of tests/rec_exact.py.  Bits are compared as uint32, -0 included."""
import ctypes as C

import numpy as np
import pytest

import ials_ref
from rec_exact import chain_scores, eligible_mask, expected_topn

pytestmark = pytest.mark.gpu

F32 = np.float32
MFX_ERR_INVALID = -1  # include/mfx.h
SIZES = [0, 1, 3, 0, 17, 250, 2048, 2049, 2100, 5000, 1]  # 0, 1, 2 and 3 chunks of 2048 entries (test_gpu_ials.py)
KS = [1, 5, 16, 36, 60, 64, 68, 100, 128]                  # k_als_gram<1..4>, k_als_gram16 (full and not), the k > 64 tails


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1, m.lib().mfx_last_error()
    return m


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def host(a):
    """numpy view of a device result (int32 items become their uint32 bits)."""
    a = a.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def segments(seed, cols, sizes, zero_frac=0.0):
    """CSR rows of the given sizes over distinct columns (ascending), values 1..5 with a share of explicit zeros."""
    rng = np.random.default_rng(seed)
    ptr = np.zeros(len(sizes) + 1, np.uint32)
    ptr[1:] = np.cumsum(sizes)
    idx = np.concatenate([np.sort(rng.choice(cols, n, replace=False)) for n in sizes]).astype(np.uint32)
    val = rng.integers(1, 6, idx.size).astype(F32)
    val[rng.random(idx.size) < zero_frac] = 0.0
    return ptr, idx, val


def select(ptr, idx, val, rows):
    """The CSR of the given rows (any order, repeats allowed)."""
    lo, hi = ptr[rows].astype(np.int64), ptr[np.asarray(rows) + 1].astype(np.int64)
    p = np.zeros(len(rows) + 1, np.uint32)
    p[1:] = np.cumsum(hi - lo)
    pos = np.concatenate([np.arange(a, b) for a, b in zip(lo, hi)] + [np.zeros(0, np.int64)])
    return p, np.ascontiguousarray(idx[pos]), np.ascontiguousarray(val[pos])


def factors(seed, cols, k, rows=3):
    rng = np.random.default_rng(seed)
    H = (rng.standard_normal((cols, k)) / np.sqrt(k)).astype(F32)
    W = rng.standard_normal((rows, k)).astype(F32)
    return W, H


def handle(mfx, W, H, layout):
    """A recommender over ALS-layout factors, stored in `layout`."""
    if layout == 0:
        return mfx.Recommender(np.ascontiguousarray(W.T), np.ascontiguousarray(H.T), 0)
    return mfx.Recommender(W, H, 1)


# ------------------------------------------------------------------------------------------------ 1. training step
def _matrix(seed, rows=400, cols=300, density=0.05):
    from mfx import dataset as ds
    rng = np.random.default_rng(seed)
    mask = rng.random((rows, cols)) < density
    mask[[3, 77, 250]] = False  # empty users
    mask[:, 5] = False          # an empty item
    r, c = np.nonzero(mask)
    return ds.from_coo(rows, cols, r, c, rng.integers(1, 6, r.size).astype(F32))


@pytest.mark.parametrize("k", [16, 64, 100])
@pytest.mark.parametrize("implicit", [False, True])
def test_fold_in_of_training_rows_is_the_next_user_half(mfx, implicit, k):
    R = _matrix(10 + k)
    lam, alpha = 0.1, 3.0
    p = mfx.parameter()
    p.k, p.lambda_ = k, lam
    assert p.schedule == 1
    s = mfx.ImplicitAlsSolver(R, p, alpha) if implicit else mfx.AlsSolver(R, None, p)
    s.set_factors((np.random.default_rng(k).standard_normal((R.cols, k)) * 0.1).astype(F32))
    s.iterate(2) if implicit else s.iterate(2, with_rmse=False)
    W0, H0 = s.get_factors()
    s.iterate(1) if implicit else s.iterate(1, with_rmse=False)
    W1, _ = s.get_factors()
    s.close()
    with mfx.Recommender(W0, H0, 1) as r:
        r.fold_in_setup(mfx.MFX_FOLD_IMPLICIT if implicit else mfx.MFX_FOLD_ALS, lam, alpha if implicit else 0.0)
        items, scores, W = r.fold_in(R)
    assert items is None and scores is None
    assert same(W, W1), np.nonzero((W.view(np.uint32) != W1.view(np.uint32)).any(axis=1))[0][:10]
    assert not W[[3, 77, 250]].any()


# ------------------------------------------------------------------------------------------------ 2. single operators
@pytest.mark.parametrize("k", KS)
def test_fold_in_equals_the_single_operators(mfx, k):
    cols = 6000
    ptr, idx, val = segments(200 + k, cols, SIZES, zero_frac=0.15)
    W, H = factors(k, cols, k)
    lam, alpha = 0.1, 2.0
    layout = KS.index(k) % 2
    with handle(mfx, W, H, layout) as r:
        for model, want in ((mfx.MFX_FOLD_ALS, mfx.als_half(ptr, idx, val, H, k, lam, variant=1)),
                            (mfx.MFX_FOLD_ALS_EXACT, mfx.als_half(ptr, idx, val, H, k, lam, variant=0)),
                            (mfx.MFX_FOLD_IMPLICIT, mfx.ials_half(ptr, idx, val, H, k, lam, alpha))):
            r.fold_in_setup(model, lam, alpha)
            got = r.fold_in((ptr, idx, val))[2]
            bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]
            assert bad.size == 0, (k, layout, model, bad.tolist())
            for s, n in enumerate(SIZES):
                if n == 0:
                    assert same(got[s], np.zeros(k, F32)), (k, model, s)


# ------------------------------------------------------------------------------------------------ 3. lambda * n_u
@pytest.mark.parametrize("k", [1, 5, 36, 64, 100, 128])
def test_ccd_model_puts_lambda_times_count_on_the_diagonal(mfx, k):
    cols = 6000
    sizes = [0, 1, 3, 17, 250, 2048, 2049, 5000, 0, 40]
    ptr, idx, val = segments(300 + k, cols, sizes)
    W, H = factors(300 + k, cols, k)
    lam = 0.05
    with handle(mfx, W, H, k % 2) as r:
        r.fold_in_setup(mfx.MFX_FOLD_CCD, lam)
        got = r.fold_in((ptr, idx, val))[2]
    H64 = H.astype(np.float64)
    for s, n in enumerate(sizes):
        if n == 0:
            assert same(got[s], np.zeros(k, F32)), (k, s)
            continue
        lo, hi = int(ptr[s]), int(ptr[s + 1])
        lam_n = float(F32(lam) * F32(n))
        one = mfx.als_half(np.array([0, n], np.uint32), idx[lo:hi].copy(), val[lo:hi].copy(), H, k, lam_n, variant=1)
        assert same(got[s], one[0]), (k, s, n)
        Hs = H64[idx[lo:hi]]
        A = Hs.T @ Hs + lam_n * np.eye(k)
        b = Hs.T @ val[lo:hi].astype(np.float64)
        assert ials_ref.backward_error(A, got[s], b) <= 3e-5, (k, s, n)


# ------------------------------------------------------------------------------------------------ 4. batch independence
@pytest.mark.parametrize("k", [36, 64, 100])
@pytest.mark.parametrize("model", [0, 1, 2, 3])
def test_a_row_gives_the_same_bits_in_any_batch(mfx, model, k):
    cols, n_top = 3000, 10
    sizes = [0, 1, 5, 40, 300, 2100, 7, 0, 64, 2049]
    ptr, idx, val = segments(400 + k, cols, sizes, zero_frac=0.1)
    W, H = factors(400 + k, cols, k)
    rng = np.random.default_rng(model)
    with handle(mfx, W, H, 1) as r:
        r.fold_in_setup(model, 0.1, 4.0)
        bi, bs, bw = r.fold_in((ptr, idx, val), n_top)
        sel = np.concatenate([rng.permutation(len(sizes)), [2, 5, 5, 0, 9]])
        gi, gs, gw = r.fold_in(select(ptr, idx, val, sel), n_top)
        assert same(gw, bw[sel]) and same(gi, bi[sel]) and same(gs, bs[sel]), (model, k)
        for s in (0, 3, 5, 9):
            ai, as_, aw = r.fold_in(select(ptr, idx, val, [s]), n_top)
            assert same(aw[0], bw[s]) and same(ai[0], bi[s]) and same(as_[0], bs[s]), (model, k, s)


# ------------------------------------------------------------------------------------------------ 5. scoring
@pytest.mark.parametrize("layout", [0, 1])
def test_lists_equal_query_on_the_solved_rows_and_the_exact_reference(mfx, layout):
    cols, k = 3001, 24
    rng = np.random.default_rng(50 + layout)
    sizes = list(rng.integers(0, 400, 60))
    sizes[::11] = [0] * len(sizes[::11])
    sizes += [cols - 5, cols, 2500]  # fewer than n_top eligible items: padded lists
    ptr, idx, val = segments(60 + layout, cols, sizes)
    W, H = factors(60 + layout, cols, k)
    H[2000:2100] = H[10:110]  # ties across tiles: ordered by item
    n = len(sizes)
    r_ids = np.repeat(np.arange(n), np.diff(ptr.astype(np.int64)))
    ex = mfx.dataset.from_coo(n, cols, r_ids, idx, val)
    assert np.array_equal(ex.csr_row_ptr, ptr) and np.array_equal(ex.csr_col_idx, idx)
    with handle(mfx, W, H, layout) as r:
        r.fold_in_setup(mfx.MFX_FOLD_ALS, 0.1)
        Wq = r.fold_in((ptr, idx, val))[2]
        S = chain_scores(Wq, H, np.arange(n))
        elig = eligible_mask(ex, np.arange(n), cols)
        with mfx.Recommender(Wq, H, 1, exclude=ex) as r2:
            for n_top in (1, 10, 100, 1024):
                items, scores, Wn = r.fold_in((ptr, idx, val), n_top)
                assert same(Wn, Wq)
                qi, qs = r2.query(n_top)
                assert same(items, qi) and same(scores, qs), (layout, n_top)
                wi, ws = expected_topn(S, elig, n_top)
                assert same(items, wi) and same(scores, ws), (layout, n_top)


# ------------------------------------------------------------------------------------------------ 6. device arrays
def test_device_arrays_give_the_host_bits(mfx):
    import torch
    cols, k = 3000, 64
    ptr, idx, val = segments(6, cols, [0, 12, 300, 2049, 1, 77])
    W, H = factors(6, cols, k)
    t = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
    with mfx.Recommender(t(W), t(H), 1) as r:
        for model in (mfx.MFX_FOLD_ALS, mfx.MFX_FOLD_IMPLICIT):
            r.fold_in_setup(model, 0.1, 2.0)
            hi, hs, hw = r.fold_in((ptr, idx, val), 10)
            di, ds, dw = r.fold_in((t(ptr), t(idx), t(val)), 10)
            oi, os_, ow = r.fold_in((ptr, idx, val), 10, on_device=True)
            torch.cuda.synchronize()
            for got in ((di, ds, dw), (oi, os_, ow)):
                assert same(host(got[2]), hw) and same(host(got[0]), hi) and same(host(got[1]), hs), model
            sw = r.fold_in((t(ptr), t(idx), t(val)))[2]
            torch.cuda.synchronize()
            assert same(host(sw), hw)


# ------------------------------------------------------------------------------------------------ 7. refusals
def _raw(mfx, r, ptr, idx, val, n_top=5):
    from mfx.api import _vp
    n = len(ptr) - 1
    W = np.empty((n, r.k), F32)
    items = np.empty((n, n_top), np.uint32)
    rc = mfx.lib().mfx_rec_fold_in(r.handle, n, idx.size, _vp(ptr), _vp(idx), _vp(val), _vp(W), n_top, _vp(items), None,
                                   0)
    return rc, mfx.lib().mfx_last_error().decode()


def test_refusals_leave_the_handle_usable(mfx):
    cols, k = 500, 8
    ptr, idx, val = segments(7, cols, [3, 0, 10, 25])  # rows 0..3 at positions [0, 3), [3, 3), [3, 13), [13, 38)
    W, H = factors(7, cols, k)
    with mfx.Recommender(W, H, 1) as r:
        rc, msg = _raw(mfx, r, ptr, idx, val)
        assert rc == MFX_ERR_INVALID and "setup" in msg
        for bad in ((mfx.MFX_FOLD_ALS, 0.0, 0.0), (mfx.MFX_FOLD_ALS, -0.1, 0.0), (mfx.MFX_FOLD_ALS, float("nan"), 0.0),
                    (mfx.MFX_FOLD_IMPLICIT, 0.1, -1.0), (mfx.MFX_FOLD_IMPLICIT, 0.1, float("inf")), (4, 0.1, 0.0),
                    (-1, 0.1, 0.0)):
            assert mfx.lib().mfx_rec_fold_in_setup(r.handle, *bad) == MFX_ERR_INVALID, bad
        r.fold_in_setup(mfx.MFX_FOLD_IMPLICIT, 0.1, 2.0)
        good = r.fold_in((ptr, idx, val), 5)
        cases = []
        i = idx.copy(); i[20] = cols; cases.append(("index >= cols", ptr, i, val))
        i = idx.copy(); i[[5, 6]] = i[[6, 5]]; cases.append(("decreasing ids", ptr, i, val))
        p = ptr.copy(); p[2] = 14; cases.append(("ptr not monotone", p, idx, val))
        p = ptr.copy(); p[-1] = 37; cases.append(("ptr[U] != nnz", p, idx, val))
        for bad in (-1.0, float("nan"), float("inf"), 3e38):  # (3e38: alpha * r overflows fp32)
            v = val.copy(); v[17] = bad; cases.append((f"strength {bad}", ptr, idx, v))
        for what, p, i, v in cases:
            rc, msg = _raw(mfx, r, p, i, v)
            assert rc == MFX_ERR_INVALID, (what, rc, msg)
            again = r.fold_in((ptr, idx, val), 5)
            assert all(same(a, b) for a, b in zip(again, good)), what
    with mfx.Recommender(np.zeros((2, 129), F32), np.zeros((cols, 129), F32), 1) as r:
        assert mfx.lib().mfx_rec_fold_in_setup(r.handle, mfx.MFX_FOLD_ALS, 0.1, 0.0) == MFX_ERR_INVALID
        assert "k <= 128" in mfx.lib().mfx_last_error().decode()
