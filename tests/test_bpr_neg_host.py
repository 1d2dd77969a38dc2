"""Negative sampling by trials without a GPU: the host trial sampler (mfx_bpr_trials) and the default rank weights against
tests/bpr_neg_exact.py, the self-checks of that exact reference (a separately written sequential WARP, permutation of a batch,
M = 1), the condition the GPU end-to-end test relies on (the reference learns the planted clusters in both modes), and the
refusals that never reach the device."""
import ctypes as C

import numpy as np
import pytest

import bpr_exact as bx
import bpr_neg_exact as nx
from rec_exact import fmaf32

MFX_ERR_INVALID = -1  # include/mfx.h
F = np.float32


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    return m


@pytest.fixture(autouse=True)
def _library_has_the_trials(mfx):
    """tests/bpr_neg_exact.py restates the contract of these entry points: without them its self-checks have no subject."""
    names = ("mfx_bpr_create_neg", "mfx_bpr_trials", "mfx_bpr_rank_weights", "mfx_bpr_apply_neg", "mfx_bpr_trial_stats")
    assert all(hasattr(mfx.lib(), name) for name in names)


@pytest.fixture(scope="module")
def R():
    return bx.small_matrix()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ the trial sampler
SEEDS = [0, 1, 12345, (1 << 63) + 5, (1 << 64) - 1]
RANGES = [(0, 40), (12345, 30), ((1 << 32) - 20, 40), ((1 << 62) - 7, 20)]


@pytest.mark.parametrize("m", [1, 2, 17, 1024])
@pytest.mark.parametrize("seed", SEEDS)
def test_trials_equal_the_python_sampler(mfx, R, seed, m):
    for first, count in RANGES:
        got = mfx.bpr_trials(R, seed, first, count, m)
        assert got[2].shape == got[3].shape == (count, m)
        for want in (nx.trials(R, seed, first, count, m), nx.trials_np(R, seed, first, count, m)):
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and np.array_equal(g, w), (seed, first)
    u, i, items, member = mfx.bpr_trials(R, seed, 5, 0, m)
    assert u.size == i.size == items.size == member.size == 0


def test_trials_of_m_are_a_prefix_and_trial_one_is_the_triple(mfx, R):
    u5, i5, it5, mem5 = mfx.bpr_trials(R, 9, 100, 300, 5)
    u9, i9, it9, mem9 = mfx.bpr_trials(R, 9, 100, 300, 9)
    assert np.array_equal(u5, u9) and np.array_equal(i5, i9)
    assert np.array_equal(it5, it9[:, :5]) and np.array_equal(mem5, mem9[:, :5])
    u, i, j, s = mfx.bpr_triples(R, 9, 100, 300)
    assert np.array_equal(u, u9) and np.array_equal(i, i9) and np.array_equal(j, it9[:, 0]) and np.array_equal(s, mem9[:, 0])
    later = mfx.bpr_trials(R, 9, 250, 150, 9)  # a function of (seed, slot number) alone
    for x, y in zip((u9, i9, it9, mem9), later):
        assert np.array_equal(x[150:], y)
    assert not np.array_equal(mfx.bpr_trials(R, 10, 100, 300, 9)[2][:, 1:], it9[:, 1:])


def test_every_item_is_drawn_as_often_as_expected_and_flags_are_membership(mfx, R):
    """10^5 trials (12 500 slots of 8): an item is drawn with p = 1 / cols at every trial number; every count lies within five
    standard deviations of N p, over all trials and over the trials 2 .. 8 of the new stream alone."""
    u, i, items, member = mfx.bpr_trials(R, 2024, 0, 12_500, 8)
    p = 1.0 / R.cols
    for block in (items, items[:, 1:]):
        n = block.size
        sd = np.sqrt(n * p * (1 - p))
        cnt = np.bincount(block.ravel(), minlength=R.cols)
        assert cnt.size == R.cols and np.all(np.abs(cnt - n * p) <= 5 * sd), (cnt.min(), cnt.max(), n * p, sd)
    dense = np.zeros((R.rows, R.cols), bool)
    dense[np.repeat(np.arange(R.rows), np.diff(R.csr_row_ptr.astype(np.int64))), R.csr_col_idx] = True
    assert np.array_equal(member, dense[u[:, None], items])
    assert 0 < member.sum() < member.size


# ------------------------------------------------------------------------------------------------ the rank weights
@pytest.mark.parametrize("cols", [1, 2, 600, 17_770, (1 << 32) - 1])
def test_default_rank_weights(mfx, cols):
    m = 1024
    got = mfx.bpr_rank_weights(cols, m)
    assert got.dtype == F and got.shape == (m,)
    q = np.array([max(1, (cols - 1) // t) for t in range(1, m + 1)])
    want = nx.rank_weights(cols, m)
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp)  # (log is no single operation)
    assert np.all(np.diff(got) <= 0) and np.all(got >= 0)
    assert np.all(bits(got[q <= 1]) == 0)
    assert np.all(got[q > 1] > 0)
    for bad in (dict(cols=0), dict(m=0), dict(m=1025)):
        with pytest.raises(mfx.MfxError, match="mfx_bpr_rank_weights"):
            mfx.bpr_rank_weights(bad.get("cols", 5), bad.get("m", 4))


# ------------------------------------------------------------------------------------------------ the reference itself
def _warp_textbook(W, H, u, i, items, member, rw, lr, lam):
    """WARP one slot after the other on scalars: draw until a trial outside the row has s_i - s_t < 1, step by the weight of
    the number of draws: w_u += lr (g (h_i - h_j) - lam w_u), h_i += lr (g w_u - lam h_i), h_j += lr (-g w_u - lam h_j), with
    the terms cut to multiples of 2^-36 (q).  Returns (W, H, chosen trials)."""
    W, H = W.copy(), H.copy()
    lr, lam = F(lr), F(lam)
    q = lambda t: F(np.trunc(np.float64(t) * 2.0 ** 36) * 2.0 ** -36)

    def dot(a, b):
        x = np.zeros(1, F)
        for c in range(len(a)):
            x = fmaf32(a[c:c + 1], b[c:c + 1], x)
        return x[0]

    chosen = []
    for s in range(len(u)):
        wu, hi = W[u[s]].copy(), H[i[s]].copy()
        si = dot(wu, hi)
        t_hit = 0
        for t in range(1, items.shape[1] + 1):
            if member[s, t - 1]:
                continue
            if not (F(si - dot(wu, H[items[s, t - 1]])) >= F(1.0)):
                t_hit = t
                break
        chosen.append(t_hit)
        if not t_hit:
            continue
        jj = items[s, t_hit - 1]
        assert jj != i[s]
        hj, g = H[jj].copy(), rw[t_hit - 1]
        for c in range(len(wu)):
            W[u[s], c] = wu[c] + lr * (q(g * F(hi[c] - hj[c])) - lam * wu[c])
            H[i[s], c] = hi[c] + lr * (q(g * wu[c]) - lam * hi[c])
            H[jj, c] = hj[c] + lr * (-q(g * wu[c]) - lam * hj[c])
    return W, H, np.array(chosen)


def test_warp_batch_of_one_is_sequential_warp(R):
    k, m = 7, 6
    W, H = bx.initial_factors(R.rows, R.cols, k, 1)
    W *= F(6.0)
    H *= F(6.0)  # scores of a few units: margins on both sides of 1
    u, i, items, member = nx.trials(R, 4, 0, 150, m)
    keep = np.all(items != i[:, None], axis=1)  # (the textbook form above does not write out i == j)
    u, i, items, member = u[keep], i[keep], items[keep], member[keep]
    rw = np.array([2.0, 1.5, 1.0, 0.5, 0.25, 0.0], F)
    Wt, Ht, chosen = _warp_textbook(W, H, u, i, items, member, rw, 0.05, 0.01)
    ts = []
    for s in range(len(u)):
        W, H, st, j, t = nx.step_neg(W, H, u[s:s + 1], i[s:s + 1], items[s:s + 1], member[s:s + 1], nx.WARP, rw, 0.05, 0.01)
        assert st[0] == 1 and st[1] == int(t[0] == 0) and st[2] == 0
        ts.append(int(t[0]))
    assert ts == chosen.tolist() and len(set(ts)) >= 5
    assert same_bits(W, Wt) and same_bits(H, Ht)


@pytest.mark.parametrize("mode", [nx.HARDEST, nx.WARP])
def test_permuting_a_batch_changes_no_bit(R, mode):
    k, m, n = 9, 7, 400
    W, H = bx.initial_factors(R.rows, R.cols, k, 2)
    W *= F(5.0)
    H *= F(5.0)
    u, i, items, member = nx.trials_np(R, 5, 0, n, m)
    rw = nx.rank_weights(R.cols, m)
    a = nx.step_neg(W, H, u, i, items, member, mode, rw, 0.05, 0.01)
    o = np.random.default_rng(0).permutation(n)
    b = nx.step_neg(W, H, u[o], i[o], items[o], member[o], mode, rw, 0.05, 0.01)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and a[2] == b[2]
    assert np.array_equal(a[3][o], b[3]) and np.array_equal(a[4][o], b[4])
    assert not same_bits(a[0], W) and len(set(a[4].tolist())) >= 3


def test_hardest_of_one_is_the_uniform_step(R):
    k, n = 8, 300
    W, H = bx.initial_factors(R.rows, R.cols, k, 3)
    u, i, j, s = bx.triples_np(R, 6, 0, n)
    u2, i2, items, member = nx.trials_np(R, 6, 0, n, 1)
    assert np.array_equal(u, u2) and np.array_equal(i, i2) and np.array_equal(items[:, 0], j) and np.array_equal(member[:, 0], s)
    want = bx.step(W, H, u, i, j, s, 0.05, 0.01)
    got = nx.step_neg(W, H, u, i, items, member, nx.HARDEST, None, 0.05, 0.01)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and got[2] == want[2]
    assert np.array_equal(got[4], (~s).astype(np.int64))


def test_choices_on_crafted_scores():
    nan, inf = np.nan, np.inf
    sc = np.array([[1.0, 3.0, 3.0, 2.0], [nan, -inf, nan, -inf], [-0.0, 0.0, -1.0, -0.0], [nan, nan, nan, nan],
                   [inf, 5.0, inf, 1.0], [1.0, 2.0, 3.0, 4.0]], F)
    mem = np.zeros(sc.shape, bool)
    mem[5] = True
    mem[0, 1] = True
    assert nx.choose_hardest(sc, mem).tolist() == [3, 2, 1, 1, 1, 0]
    si = np.array([4.0, 4.0, 0.5, 1.0, 9.0, 0.0], F)
    # row 0: margins 3, (member), 1, 2: none below 1;  row 1: a NaN score violates;  row 2: 0.5 - (-0) < 1
    assert nx.choose_warp(si, sc, mem).tolist() == [0, 1, 1, 1, 1, 0]


def _hit_rate(P, W, H):
    S = W.astype(np.float64) @ H.astype(np.float64).T
    S[np.repeat(np.arange(P.rows), np.diff(P.csr_row_ptr.astype(np.int64))), P.csr_col_idx] = -np.inf
    top = np.argsort(-S, axis=1, kind="stable")[:, :10]
    return float(np.any(top[P.test_row] == P.test_col[:, None].astype(np.int64), axis=1).mean())


@pytest.mark.parametrize("mode,m,lr,epochs", [(nx.WARP, 16, 0.01, 10), (nx.HARDEST, 8, 0.05, 5)])
def test_reference_learns_the_planted_clusters(mfx, mode, m, lr, epochs):
    """What tests/test_gpu_bpr_neg.py relies on: the exact reference, fed by the library's trial sampler, puts the held-out
    item into the top 10 of at least 90 % of the users at k = 32, batch 1 024, lambda 0.01 with the default rank weights."""
    P = bx.planted_clusters()
    W, H = bx.initial_factors(P.rows, P.cols, 32, 5)
    rw = mfx.bpr_rank_weights(P.cols, m)
    W, H, stats, pos, ts = nx.train_neg(P, W, H, lr, 0.01, 1024, 7, epochs, m, mode, rank_weight=rw, sampler=mfx.bpr_trials)
    assert pos == epochs * P.nnz and np.all(stats[:, 0] == P.nnz) and np.all(stats[:, 2] == 0)
    hr = _hit_rate(P, W, H)
    print("mode", mode, "hit rate", hr, "stats", stats.tolist(), "trial stats", ts.tolist())
    assert hr >= 0.9, hr


# ------------------------------------------------------------------------------------------------ refusals without a device
def _create_neg(mfx, R, mode=1, m=4, rw=None, k=8, lam=0.01, lr=0.05, batch=64):
    from mfx import api
    p = mfx.parameter()
    p.k, p.lambda_ = k, lam
    cp = p.to_c()
    cp.k = k & 0xFFFFFFFF
    h = C.c_void_p()
    csx = api._csx(R)
    rw = None if rw is None else np.ascontiguousarray(rw, F)
    rc = mfx.lib().mfx_bpr_create_neg(C.byref(h), C.byref(csx), C.byref(cp), lr, batch, 0, mode, m, api._vp(rw), 0)
    assert not h.value
    return rc


@pytest.mark.parametrize("kw", [dict(mode=-1), dict(mode=3), dict(m=0), dict(m=1025), dict(m=-4), dict(mode=0, m=2),
                                dict(mode=2, rw=[1.0, -0.5, 0.0, 0.0]), dict(mode=2, rw=[1.0, float("nan"), 0.0, 0.0]),
                                dict(mode=2, rw=[float("inf"), 1.0, 0.0, 0.0]), dict(k=0), dict(k=1025), dict(batch=0),
                                dict(batch=(1 << 20) + 1), dict(lr=-0.1), dict(lr=float("nan")), dict(lam=-1.0),
                                dict(lam=float("inf"))])
def test_create_neg_refuses_bad_arguments_before_the_device(mfx, R, kw):
    assert _create_neg(mfx, R, **kw) == MFX_ERR_INVALID
    assert b"mfx_bpr_create_neg" in mfx.lib().mfx_last_error()


def test_the_other_entry_points_refuse_before_the_device(mfx, R):
    lib = mfx.lib()
    W, H = bx.initial_factors(4, 5, 3, 0)
    z, it = np.zeros(2, np.uint32), np.zeros((2, 3), np.uint32)
    for kw in (dict(lr=-1.0), dict(lr=float("nan")), dict(lam=-1.0), dict(lam=float("inf")), dict(rank_weight=[1.0, -1.0, 0.0], loss="warp"),
               dict(rank_weight=[1.0, float("inf"), 0.0], loss="warp")):
        with pytest.raises(mfx.MfxError, match="mfx_bpr_apply_neg"):
            mfx.bpr_apply_neg(W, H, z, z, it, **{"lr": 0.05, "lam": 0.01, **kw})
    with pytest.raises(mfx.MfxError, match="2\\^20"):
        big = np.zeros((1 << 20) + 1, np.uint32)
        mfx.bpr_apply_neg(W, H, big, big, big[:, None], 0.05, 0.01)
    with pytest.raises(mfx.MfxError, match="negatives"):
        mfx.bpr_apply_neg(W, H, z, z, np.zeros((2, 1025), np.uint32), 0.05, 0.01)
    with pytest.raises(mfx.MfxError, match="k must be"):
        mfx.bpr_apply_neg(np.zeros((4, 1025), F), np.zeros((5, 1025), F), z, z, it, 0.05, 0.01)
    stats = (C.c_int64 * 4)()
    args = (4, 5, 3, W.ctypes.data_as(lib.mfx_bpr_apply_neg.argtypes[3]), H.ctypes.data_as(lib.mfx_bpr_apply_neg.argtypes[4]), 2,
            z.ctypes.data_as(lib.mfx_bpr_apply_neg.argtypes[6]), z.ctypes.data_as(lib.mfx_bpr_apply_neg.argtypes[7]), 3,
            it.ctypes.data_as(lib.mfx_bpr_apply_neg.argtypes[9]), None)
    for mode in (0, 3, -1):  # (the uniform mode has mfx_bpr_apply)
        assert lib.mfx_bpr_apply_neg(*args, mode, None, 0.05, 0.01, stats, None, None, 0) == MFX_ERR_INVALID
    with pytest.raises(mfx.MfxError, match="mfx_bpr_trials"):
        mfx.bpr_trials(R, 0, -1, 4, 3)
    for m in (0, 1025):
        with pytest.raises(mfx.MfxError, match="mfx_bpr_trials"):
            mfx.bpr_trials(R, 0, 0, 4, m)
    bad = R.copy()
    bad.csr_row_ptr[3], bad.csr_row_ptr[4] = bad.csr_row_ptr[4] + 1, bad.csr_row_ptr[3]
    with pytest.raises(mfx.MfxError, match="csr_row_ptr"):
        mfx.bpr_trials(bad, 0, 0, 4, 3)
    assert lib.mfx_bpr_trial_stats(None, None) == MFX_ERR_INVALID
