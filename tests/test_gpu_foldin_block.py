"""Fold-in by block subspace sweeps (mfx_rec_fold_in_block_setup / mfx_rec_fold_in_warm, Recommender.fold_in_block_setup)
checked bit for bit against the paths it reuses: S sweeps against S chained mfx.ials_block_half calls, one sweep from the
trainer's factors against the block trainer's next user half, a row stopped by the rule against a run of exactly that
many sweeps, the lists against mfx_rec_query on the solved rows.  Bits are compared as uint32, -0 included.

Data: 6000 columns, the segment sizes of the operator tests (0, 1, 2 and 3 chunks of 2048 entries, empty rows), H ~ N(0, 1/k),
lambda = 0.1.  Distances are |y - y*| / |y*| (2-norms) to the fp64 dense solve of tests/ials_ref.py; 1e-3 is the project's
standing tolerance for these rows (tests/test_gpu_ialsb.py).

What the fp64 reference does on this data (computed on the CPU, asserted below): 8 chained block sweeps from zero at alpha = 1
end 6.7e-9 (k = 160, d = 64) and 3.5e-12 (k = 130, d = 128) from the dense solve; at alpha = 40, k = 160, d = 64 the rule with
tol = 1e-4 stops the nine non-empty rows after 9, 13, 12, 15, 7, 7, 7, 5 and 11 sweeps, at most 1.4e-4 from the dense solve.

Measured on the MI355X (printed by the tests as `foldin-block-measured` lines; profiles/r11_foldin_block_accuracy.txt):
    convergence k=160 d=64  alpha=1 sweeps=8: worst distance 4.637e-07 (fp64 chain 6.650e-09)
    convergence k=130 d=128 alpha=1 sweeps=8: worst distance 6.336e-07 (fp64 chain 3.492e-12)
    per-row stop k=160 d=64 alpha=40 tol=1e-4: counts [0, 9, 13, 0, 12, 15, 7, 7, 7, 5, 11], the fp64 emulation's exactly;
        worst distance 1.398e-04 (emulation 1.399e-04)
"""

import numpy as np
import pytest

import ials_ref
import ialsb_ref
from test_gpu_foldin import F32, MFX_ERR_INVALID, SIZES, _matrix, factors, handle, host, same, segments, select

pytestmark = pytest.mark.gpu

COLS, LAM = 6000, 0.1
CASES = [(130, 128), (160, 64), (192, 32), (512, 96), (1024, 128), (100, 128), (37, 5)]  # last block 2, 32, 96 wide; d > k; k <= 128


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1, m.lib().mfx_last_error()
    return m


def data(k, zero_frac):
    """The rows and the H of the operator tests at rank k (tests/test_gpu_ials.py: the same seeds and draws)."""
    ptr, idx, val = segments(100 + k, COLS, SIZES, zero_frac=zero_frac)
    _, H = factors(k, COLS, k)
    return ptr, idx, val, H


def dense_rows(ptr, idx, val, H, alpha):
    return ials_ref.half(ptr, idx, val, H, LAM, alpha)


def distances(Y, D):
    return [float(np.linalg.norm(Y[s] - D[s]) / np.linalg.norm(D[s])) for s, n in enumerate(SIZES) if n]


def bad_rows(a, b):
    return np.nonzero((a.view(np.uint32) != b.view(np.uint32)).any(axis=1))[0].tolist()


# ------------------------------------------------------------------------------------------------ 1. chained operator
@pytest.mark.parametrize("k,d", CASES)
def test_sweeps_equal_chained_block_halves(mfx, k, d):
    ptr, idx, val, H = data(k, 0.15)
    alpha, layout = 2.0, CASES.index((k, d)) % 2
    W = np.zeros((3, k), F32)
    W0 = (0.1 * np.random.default_rng(1000 + k).standard_normal((len(SIZES), k))).astype(F32)
    with handle(mfx, W, H, layout) as r:
        for start in (None, W0):
            want, Y = {}, start
            for s in (1, 2, 3):
                Y = mfx.ials_block_half(ptr, idx, val, H, k, LAM, alpha, d, Y_in=Y)
                want[s] = Y
            for S in (1, 3):
                r.fold_in_block_setup(LAM, alpha, block=d, sweeps=S)
                _, _, got, done = r.fold_in((ptr, idx, val), W_init=start, return_sweeps=True)
                assert bad_rows(got, want[S]) == [], (k, d, layout, S, start is not None)
                assert done.dtype == np.int32 and done.tolist() == [S if n else 0 for n in SIZES]
                for s, n in enumerate(SIZES):
                    if n == 0:
                        assert same(got[s], np.zeros(k, F32)), (k, d, S, s)
                if start is None:  # mfx_rec_fold_in after a block setup: the warm call without a start row and counts
                    assert same(r.fold_in((ptr, idx, val))[2], got)


@pytest.mark.parametrize("k,default", [(160, 64), (37, 37)])
def test_block_zero_is_the_default_block(mfx, k, default):
    ptr, idx, val, H = data(k, 0.15)
    want = mfx.ials_block_half(ptr, idx, val, H, k, LAM, 2.0, default)
    assert same(want, mfx.ials_block_half(ptr, idx, val, H, k, LAM, 2.0, 0))
    with handle(mfx, np.zeros((3, k), F32), H, 1) as r:
        r.fold_in_block_setup(LAM, 2.0, sweeps=1)
        assert same(r.fold_in((ptr, idx, val))[2], want)


# ------------------------------------------------------------------------------------------------ 2. training step
def test_one_sweep_from_the_trained_rows_is_the_next_user_half(mfx):
    k, d, alpha = 160, 64, 3.0
    R = _matrix(10 + k)
    p = mfx.parameter()
    p.k, p.lambda_ = k, LAM
    s = mfx.ImplicitAlsSolver(R, p, alpha, block=d)
    s.set_factors((np.random.default_rng(k).standard_normal((R.cols, k)) * 0.1).astype(F32))
    s.iterate(2)
    W0, H0 = s.get_factors()
    s.iterate(1)
    W1, _ = s.get_factors()
    s.close()
    with mfx.Recommender(W0, H0, 1) as r:
        r.fold_in_block_setup(LAM, alpha, block=d, sweeps=1)
        items, scores, W = r.fold_in(R, W_init=W0)
    assert items is None and scores is None
    assert bad_rows(W, W1) == []
    assert not W[[3, 77, 250]].any()


# ------------------------------------------------------------------------------------------------ 3. convergence
@pytest.mark.parametrize("k,d", [(160, 64), (130, 128)])
def test_eight_sweeps_from_zero_reach_the_dense_solution(mfx, k, d):
    ptr, idx, val, H = data(k, 0.0)
    alpha, S = 1.0, 8
    D = dense_rows(ptr, idx, val, H, alpha)
    Yr = np.zeros((len(SIZES), k))
    for _ in range(S):
        Yr = ialsb_ref.block_sweep(ptr, idx, val, H, Yr, LAM, alpha, d)
    ref = max(distances(Yr, D))
    with handle(mfx, np.zeros((3, k), F32), H, 1) as r:
        r.fold_in_block_setup(LAM, alpha, block=d, sweeps=S)
        got = r.fold_in((ptr, idx, val))[2]
    dist = distances(got, D)
    print(f"foldin-block-measured convergence k={k} d={d} alpha={alpha} sweeps={S} worst={max(dist):.3e} fp64_chain={ref:.3e}")
    assert ref <= 1e-5, ref
    assert max(dist) <= 1e-3, dist
    for s, n in enumerate(SIZES):
        if n == 0:
            assert same(got[s], np.zeros(k, F32))


# ------------------------------------------------------------------------------------------------ 4. per-row stop
def emulated_stop(ptr, idx, val, H, alpha, d, tol, sweeps):
    """The rule in fp64: (rows, sweeps applied to each row)."""
    n = len(ptr) - 1
    Y, cnt = np.zeros((n, H.shape[1])), np.zeros(n, np.int64)
    frozen = np.diff(ptr.astype(np.int64)) == 0
    for _ in range(sweeps):
        Yn = ialsb_ref.block_sweep(ptr, idx, val, H, Y, LAM, alpha, d)
        for u in np.nonzero(~frozen)[0]:
            cnt[u] += 1
            frozen[u] = np.max(np.abs(Yn[u] - Y[u])) <= tol * np.max(np.abs(Yn[u]))
            Y[u] = Yn[u]
        if frozen.all():
            break
    return Y, cnt


def test_rows_stop_on_their_own(mfx):
    k, d, alpha, tol, sweeps = 160, 64, 40.0, 1e-4, 32
    ptr, idx, val, H = data(k, 0.0)
    D = dense_rows(ptr, idx, val, H, alpha)
    Ye, ce = emulated_stop(ptr, idx, val, H, alpha, d, tol, sweeps)
    assert ce.max() <= 16 and max(distances(Ye, D)) <= 1e-3, (ce.tolist(), distances(Ye, D))
    nonempty = np.array(SIZES) > 0
    with handle(mfx, np.zeros((3, k), F32), H, 1) as r:
        r.fold_in_block_setup(LAM, alpha, block=d, sweeps=sweeps, tol=tol)
        bi, bs, got, cnt = r.fold_in((ptr, idx, val), 10, return_sweeps=True)
        dist = distances(got, D)
        print(f"foldin-block-measured per-row-stop k={k} d={d} alpha={alpha} tol={tol} counts={cnt.tolist()} "
              f"emulated={ce.tolist()} worst={max(dist):.3e} emulated_worst={max(distances(Ye, D)):.3e}")
        assert not cnt[~nonempty].any() and not got[~nonempty].any()
        assert cnt[nonempty].min() >= 1 and cnt[nonempty].max() <= 31, cnt.tolist()
        assert len(set(cnt[nonempty].tolist())) >= 3, cnt.tolist()
        assert max(dist) <= 1e-3, dist
        # a row alone, and in a shuffled batch with repeats: the same bits, the same count, the same list
        rng = np.random.default_rng(4)
        sel = np.concatenate([rng.permutation(len(SIZES)), [2, 5, 5, 0, 9]])
        gi, gs, gw, gc = r.fold_in(select(ptr, idx, val, sel), 10, return_sweeps=True)
        assert same(gw, got[sel]) and np.array_equal(gc, cnt[sel]) and same(gi, bi[sel]) and same(gs, bs[sel])
        for s in (0, 1, 5, 9):
            ai, as_, aw, ac = r.fold_in(select(ptr, idx, val, [s]), 10, return_sweeps=True)
            assert same(aw[0], got[s]) and ac[0] == cnt[s] and same(ai[0], bi[s]) and same(as_[0], bs[s]), s
        # a stopped row is the row after exactly that many sweeps
        for c in sorted(set(cnt[nonempty].tolist())):
            r.fold_in_block_setup(LAM, alpha, block=d, sweeps=c)
            fixed = r.fold_in((ptr, idx, val))[2]
            rows = np.nonzero(cnt == c)[0]
            assert same(fixed[rows], got[rows]), (c, rows.tolist())


# ------------------------------------------------------------------------------------------------ 5. lists
@pytest.mark.parametrize("layout", [0, 1])
def test_lists_equal_query_on_the_solved_rows(mfx, layout):
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
        r.fold_in_block_setup(LAM, 2.0, block=d, sweeps=2)
        items, scores, Wq = r.fold_in((ptr, idx, val), n_top)
        assert same(Wq, r.fold_in((ptr, idx, val))[2])
    with mfx.Recommender(Wq, H, 1, exclude=ex) as r2:
        qi, qs = r2.query(n_top)
    assert same(items, qi) and same(scores, qs), layout
    assert (items[-2] == 0xFFFFFFFF).all() and (items[-3, 5:] == 0xFFFFFFFF).all()


# ------------------------------------------------------------------------------------------------ 6. device arrays
def test_device_arrays_give_the_host_bits(mfx):
    import torch
    cols, k = 3000, 160
    ptr, idx, val = segments(6, cols, [0, 12, 300, 2049, 1, 77])
    W, H = factors(6, cols, k)
    W0 = (0.1 * np.random.default_rng(8).standard_normal((6, k))).astype(F32)
    t = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
    with mfx.Recommender(t(W), t(H), 1) as r:
        for tol, start in ((0.0, W0), (1e-3, None), (1e-3, W0)):
            r.fold_in_block_setup(LAM, 2.0, block=64, sweeps=6, tol=tol)
            want = r.fold_in((ptr, idx, val), 10, W_init=start, return_sweeps=True)
            dev_start = t(start) if start is not None else None
            a = r.fold_in((t(ptr), t(idx), t(val)), 10, W_init=dev_start, return_sweeps=True)
            b = r.fold_in((ptr, idx, val), 10, on_device=True, W_init=start, return_sweeps=True)
            runs = [a, b]
            if start is not None:  # host rows, the start rows alone on the device
                runs.append(r.fold_in((ptr, idx, val), 10, W_init=dev_start, return_sweeps=True))
            torch.cuda.synchronize()
            for got in runs:
                assert all(same(host(g), w) for g, w in zip(got[:3], want[:3])), (tol, start is not None)
                assert got[3].dtype == torch.int32 and np.array_equal(host(got[3]).view(np.int32), want[3])
            assert want[3][0] == 0 and (want[3][1:] >= 1).all() and (tol > 0 or (want[3][1:] == 6).all())


# ------------------------------------------------------------------------------------------------ 7. refusals
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
        rc, msg = _warm(mfx, r, ptr, idx, val)
        assert rc == MFX_ERR_INVALID and "mfx_rec_fold_in_block_setup" in msg
        r.fold_in_block_setup(LAM, 2.0, block=64, sweeps=3, tol=1e-3)
        good = r.fold_in((ptr, idx, val), 5, return_sweeps=True)
        again = lambda: all(same(a, b) for a, b in zip(r.fold_in((ptr, idx, val), 5, return_sweeps=True), good))
        for bad in ((LAM, 2.0, -1, 3, 0.0), (LAM, 2.0, 129, 3, 0.0), (LAM, 2.0, 64, 0, 0.0), (LAM, 2.0, 64, -1, 0.0),
                    (LAM, 2.0, 64, 1025, 0.0), (LAM, 2.0, 64, 3, -1.0), (LAM, 2.0, 64, 3, nan), (LAM, 2.0, 64, 3, inf),
                    (0.0, 2.0, 64, 3, 0.0), (nan, 2.0, 64, 3, 0.0), (LAM, -1.0, 64, 3, 0.0), (LAM, inf, 64, 3, 0.0)):
            assert mfx.lib().mfx_rec_fold_in_block_setup(r.handle, *bad) == MFX_ERR_INVALID, bad
            assert again(), bad
        cases = []
        i = idx.copy(); i[20] = cols; cases.append(("index >= cols", ptr, i, val))
        i = idx.copy(); i[[5, 6]] = i[[6, 5]]; cases.append(("decreasing ids", ptr, i, val))
        p = ptr.copy(); p[2] = 14; cases.append(("ptr not monotone", p, idx, val))
        p = ptr.copy(); p[-1] = 37; cases.append(("ptr[U] != nnz", p, idx, val))
        for bad in (-1.0, nan, inf, 3e38):  # (3e38: alpha * r overflows fp32)
            v = val.copy(); v[17] = bad; cases.append((f"strength {bad}", ptr, idx, v))
        for what, p, i, v in cases:
            rc, msg = _warm(mfx, r, p, i, v)
            assert rc == MFX_ERR_INVALID, (what, rc, msg)
            assert again(), what
    # the setups replace each other (k = 64: both kinds apply)
    k = 64
    W, H = factors(8, cols, k)
    direct = mfx.ials_half(ptr, idx, val, H, k, LAM, 2.0)
    block = mfx.ials_block_half(ptr, idx, val, H, k, LAM, 2.0, 16)
    assert not same(direct, block)
    with mfx.Recommender(W, H, 1) as r:
        for _ in range(2):
            r.fold_in_block_setup(LAM, 2.0, block=16, sweeps=1)
            assert same(r.fold_in((ptr, idx, val))[2], block)
            assert _warm(mfx, r, ptr, idx, val)[0] == 0
            r.fold_in_setup(mfx.MFX_FOLD_IMPLICIT, LAM, 2.0)
            assert same(r.fold_in((ptr, idx, val))[2], direct)
            rc, msg = _warm(mfx, r, ptr, idx, val)
            assert rc == MFX_ERR_INVALID and "mfx_rec_fold_in_block_setup" in msg
            assert same(r.fold_in((ptr, idx, val))[2], direct)
