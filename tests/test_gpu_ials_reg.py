"""GPU tests of implicit ALS with an unobserved weight alpha0 and a frequency-scaled regulariser (mfx_ials_create_reg,
mfx_ials_block_create_reg, mfx_ials_half_reg, mfx_ials_block_half_reg, mfx_ials_loss on those handles) against the
fp64 reference of tests/ials_reg_ref.py, and bit for bit against the un-suffixed entry points at alpha0 = 1, nu = 0.

Data: the shapes of tests/test_gpu_ials.py and test_gpu_ialsb.py (6 000 rows of X ~ N(0, 1/k), the eleven segments of
SIZES) plus one segment whose three entries are all explicit zeros; the trainers run on the 300 x 200 matrix with an
empty user and an empty item.  Parameter sets (alpha0, nu, lambda): (0.3, 0.5, 0.1), (2, 1, 0.002), (1, 0.25, 0.1).

Tolerances are those of tests/test_gpu_ials.py / test_gpu_ialsb.py for the same kernels plus one fp32 rounding (G0 =
fp32(alpha0 S), far below either bound): backward error against the dense system at most 3e-5, relative error at most
1e-3 where the condition number is at most 1e3 (the gate is asserted to skip no segment; tests/test_ials_reg_host.py
asserts the same on the CPU: at most 107.6), factors of one iteration within 1e-3 of the largest reference entry,
loss to 1e-6.  The tests print what they measure as `ialsr-measured` lines (profiles/r15_ials_reg_accuracy.txt)."""
import numpy as np
import pytest

import ials_ref
import ials_reg_ref as ref
from test_gpu_ials import SIZES, _device_arrays, _params, _random_matrix, _segments

pytestmark = pytest.mark.gpu

PARAMS = [(0.3, 0.5, 0.1), (2.0, 1.0, 0.002), (1.0, 0.25, 0.1)]  # (alpha0, nu, lambda)
KS = [1, 5, 16, 32, 36, 60, 64, 68, 100, 128]
ALPHAS = (0.0, 1.0, 40.0)
NROWS_X = 6000
ALL_SIZES = SIZES + [3]  # segment 11: three stored entries, all explicit zeros (n_s = 0, b = 0)


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1
    return m


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


_DATA = {}


def data(k, nrows_x=NROWS_X, sizes=None):
    """(ptr, idx, val, X) of the operator tests at rank k (read-only, shared): the segments of SIZES exactly as
    tests/test_gpu_ials.py draws them, then the all-explicit-zero segment."""
    key = (k, nrows_x, tuple(sizes) if sizes else None)
    if key not in _DATA:
        ptr, idx, val = _segments(100 + k, nrows_x, sizes if sizes else SIZES)
        zi = np.sort(np.random.default_rng(7000 + k).choice(nrows_x, 3, replace=False)).astype(np.uint32)
        ptr = np.concatenate([ptr, [ptr[-1] + 3]]).astype(np.uint32)
        idx, val = np.concatenate([idx, zi]), np.concatenate([val, np.zeros(3, np.float32)])
        X = (np.random.default_rng(k).standard_normal((nrows_x, k)) / np.sqrt(k)).astype(np.float32)
        for a in (ptr, idx, val, X):
            a.setflags(write=False)
        _DATA[key] = (ptr, idx, val, X)
    return _DATA[key]


def _cond(A):
    ev = np.linalg.eigvalsh(A)
    return float(ev[-1] / ev[0]) if ev[0] > 0 else float("inf")


# ------------------------------------------------------------------------------------------------ 1. alpha0 = 1, nu = 0
@pytest.mark.parametrize("k", KS)
def test_half_reg_at_alpha0_1_nu_0_is_ials_half_bit_for_bit(mfx, k):
    ptr, idx, val, X = data(k)
    for alpha in ALPHAS:
        want = mfx.ials_half(ptr, idx, val, X, k, 0.1, alpha)
        assert same(mfx.ials_half(ptr, idx, val, X, k, 0.1, alpha, alpha0=1.0, nu=0.0), want), (k, alpha)
        assert same(mfx.ials_half(ptr, idx, val, X, k, 0.1, alpha, alpha0=1.0), want), (k, alpha)  # a lone alpha0: nu = 0
        assert same(mfx.ials_half(ptr, idx, val, X, k, 0.1, alpha, nu=0.0), want), (k, alpha)      # a lone nu: alpha0 = 1


def _train(mfx, R, k, lam, alpha, H0, n, device_arrays=None, **kw):
    s = mfx.ImplicitAlsSolver(R if device_arrays is None else None, _params(mfx, k, lam), alpha, device_arrays=device_arrays, **kw)
    s.set_factors(H0)
    losses = []
    for _ in range(n):
        s.iterate(1)
        losses.append(s.loss())
    W, H = s.get_factors()
    kt = s.kernel_times()
    s.close()
    return W, H, losses, kt


@pytest.mark.parametrize("k", [24, 64, 100])
def test_trainer_at_alpha0_1_nu_0_is_the_plain_trainer_bit_for_bit(mfx, k):
    R = _random_matrix(1)
    H0 = (np.random.default_rng(2).standard_normal((R.cols, k)) * 0.1).astype(np.float32)
    W, H, losses, kt = _train(mfx, R, k, 0.1, 5.0, H0, 2)
    Wr, Hr, lr, ktr = _train(mfx, R, k, 0.1, 5.0, H0, 2, alpha0=1.0, nu=0.0)
    assert same(W, Wr) and same(H, Hr)
    assert np.array_equal(np.array(losses).view(np.uint64), np.array(lr).view(np.uint64)), (losses, lr)
    assert set(kt) == set(ktr)


# ------------------------------------------------------------------------------------------------ 2. the dense reference
@pytest.mark.parametrize("k", KS)
def test_half_reg_against_dense_reference(mfx, k):
    ptr, idx, val, X = data(k)
    worst_be, worst_rel, worst_cond = 0.0, 0.0, 0.0
    for alpha0, nu, lam in PARAMS:
        rh = ref.rho(ptr, val, NROWS_X, lam, alpha0, nu)
        for alpha in ALPHAS:
            Y = mfx.ials_half(ptr, idx, val, X, k, lam, alpha, alpha0=alpha0, nu=nu)
            for s, n in enumerate(ALL_SIZES):
                if n == 0 or s == 11:
                    assert not np.any(Y[s]), (k, alpha0, nu, alpha, s)  # b = 0: exactly zero
                if n == 0:
                    continue
                A, b = ref.dense_system(ptr, idx, val, s, X, lam, alpha, alpha0, nu, rh[s])
                c = _cond(A)
                worst_cond = max(worst_cond, c)
                assert c <= 1e3, (k, alpha0, nu, alpha, s, n, c)  # the gate skips nothing
                if s == 11:
                    assert not np.any(b)
                    continue
                be = ref.backward_error(A, Y[s], b)
                worst_be = max(worst_be, be)
                assert be <= 3e-5, (k, alpha0, nu, alpha, s, n, be)
                y = np.linalg.solve(A, b)
                rel = float(np.linalg.norm(Y[s] - y) / max(np.linalg.norm(y), 1e-30))
                worst_rel = max(worst_rel, rel)
                assert rel <= 1e-3, (k, alpha0, nu, alpha, s, n, rel)
    print(f"ialsr-measured half k={k} worst_backward_error={worst_be:.3e} worst_rel={worst_rel:.3e} worst_cond={worst_cond:.1f}")


# ------------------------------------------------------------------------------------------------ 3. block sweeps
def _rel_errors(Y, Yr, sizes):
    out = []
    for s, n in enumerate(sizes):
        if n == 0 or s == len(sizes) - 1:  # the last segment: explicit zeros only
            if n == 0:
                assert not np.any(Y[s]) and not np.any(Yr[s]), s
            continue
        out.append(float(np.linalg.norm(Y[s] - Yr[s]) / max(np.linalg.norm(Yr[s]), 1e-30)))
    return out


def _check_operator(mfx, k, d, pset, nrows_x=NROWS_X, sizes=None):
    ptr, idx, val, X = data(k, nrows_x, sizes)
    all_sizes = (list(sizes) if sizes else SIZES) + [3]
    alpha0, nu, lam = PARAMS[pset]
    S = X.astype(np.float64).T @ X.astype(np.float64)
    Y0 = (0.1 * np.random.default_rng(1000 + k).standard_normal((len(all_sizes), k))).astype(np.float32)
    worst = 0.0
    for alpha in ALPHAS:
        for Y_in in (Y0, None):
            Y = mfx.ials_block_half(ptr, idx, val, X, k, lam, alpha, d, Y_in=Y_in, alpha0=alpha0, nu=nu)
            Yr = ref.block_sweep(ptr, idx, val, X, Y0 if Y_in is not None else np.zeros_like(Y0), lam, alpha, alpha0, nu, d, S=S)
            rel = _rel_errors(Y, Yr, all_sizes)
            worst = max(worst, max(rel))
            assert max(rel) <= 1e-3, (k, d, pset, alpha, Y_in is None, rel)
            if Y_in is None:  # from zero the all-explicit-zero segment stays exactly zero (b = 0, P = 0)
                assert not np.any(Y[-1]), (k, d, pset, alpha)
            else:             # from a start it shrinks towards zero like the reference's row
                assert np.linalg.norm(Y[-1] - Yr[-1]) <= 1e-3 * np.linalg.norm(Y0[-1]), (k, d, pset, alpha)
    print(f"ialsr-measured operator k={k} d={d} alpha0={alpha0} nu={nu} lambda={lam} worst_rel={worst:.3e}")


@pytest.mark.parametrize("pset", [0, 1, 2])
@pytest.mark.parametrize("k,d", [(160, 64), (256, 128), (130, 128), (1024, 128), (64, 16), (37, 5)])
def test_block_half_reg_against_fp64_block_sweep(mfx, k, d, pset):
    _check_operator(mfx, k, d, pset)


@pytest.mark.parametrize("pset", [0, 1, 2])
def test_block_half_reg_on_a_segment_of_ten_chunks(mfx, pset):
    _check_operator(mfx, 256, 64, pset, 30000, [20000, 0, 5])


@pytest.mark.parametrize("k", [16, 64, 100, 128])
def test_single_block_from_zero_solves_the_dense_system(mfx, k):
    ptr, idx, val, X = data(k)
    worst = 0.0
    for alpha0, nu, lam in PARAMS:
        rh = ref.rho(ptr, val, NROWS_X, lam, alpha0, nu)
        for alpha in ALPHAS:
            Y = mfx.ials_block_half(ptr, idx, val, X, k, lam, alpha, 128, alpha0=alpha0, nu=nu)
            for s, n in enumerate(ALL_SIZES):
                if n == 0 or s == 11:
                    assert not np.any(Y[s]), (k, alpha0, nu, alpha, s)
                    continue
                A, b = ref.dense_system(ptr, idx, val, s, X, lam, alpha, alpha0, nu, rh[s])
                be = ref.backward_error(A, Y[s], b)
                worst = max(worst, be)
                assert be <= 3e-5, (k, alpha0, nu, alpha, s, n, be)
    print(f"ialsr-measured single-block k={k} worst_backward_error={worst:.3e}")


@pytest.mark.parametrize("pset", [0, 1, 2])
def test_four_chained_sweeps(mfx, pset):
    k, d, alpha = 256, 64, 40.0
    alpha0, nu, lam = PARAMS[pset]
    ptr, idx, val, X = data(k)
    S = X.astype(np.float64).T @ X.astype(np.float64)
    Y, Yr = None, np.zeros((len(ALL_SIZES), k))
    for _ in range(4):
        Y = mfx.ials_block_half(ptr, idx, val, X, k, lam, alpha, d, Y_in=Y, alpha0=alpha0, nu=nu)
        Yr = ref.block_sweep(ptr, idx, val, X, Yr, lam, alpha, alpha0, nu, d, S=S)
    rel = _rel_errors(Y, Yr, ALL_SIZES)
    print(f"ialsr-measured four-sweeps k={k} d={d} alpha0={alpha0} nu={nu} lambda={lam} max_rel={max(rel):.3e}")
    assert max(rel) <= 1e-3, rel
    assert not np.any(Y[-1])


# ------------------------------------------------------------------------------------------------ 4. the trainers
@pytest.mark.parametrize("pset", [0, 1, 2])
@pytest.mark.parametrize("k,d", [(24, None), (160, 64)])
def test_one_iteration_and_loss_match_the_fp64_reference(mfx, k, d, pset):
    alpha0, nu, lam = PARAMS[pset]
    R = _random_matrix(1)
    alpha = 5.0
    H0 = (np.random.default_rng(2).standard_normal((R.cols, k)) * 0.1).astype(np.float32)
    kw = dict(alpha0=alpha0, nu=nu) if d is None else dict(alpha0=alpha0, nu=nu, block=d)
    s = mfx.ImplicitAlsSolver(R, _params(mfx, k, lam), alpha, **kw)
    s.set_factors(H0)
    rep = s.iterate(1)
    assert rep[0].update_time > 0 and rep[0].rmse == 0
    W, H = s.get_factors()
    Wr, Hr = ref.iteration(R, H0.astype(np.float64), lam, alpha, alpha0, nu, d=d)
    eW, eH = np.max(np.abs(W - Wr)) / np.max(np.abs(Wr)), np.max(np.abs(H - Hr)) / np.max(np.abs(Hr))
    print(f"ialsr-measured iteration k={k} d={d} alpha0={alpha0} nu={nu} lambda={lam} W={eW:.3e} H={eH:.3e}")
    assert eW <= 1e-3 and eH <= 1e-3
    assert not np.any(W[7]) and not np.any(H[11])
    prev, worst = None, 0.0
    for it in range(5):
        if it:
            s.iterate(1)
            W, H = s.get_factors()
        got = s.loss()
        want = ref.dense_loss(R, W, H, lam, alpha, alpha0, nu)
        worst = max(worst, abs(got - want) / abs(want))
        assert abs(got - want) <= 1e-6 * abs(want), (it, got, want)
        if prev is not None:
            assert got <= prev * (1 + 1e-6), (it, prev, got)
        prev = got
    print(f"ialsr-measured loss k={k} d={d} alpha0={alpha0} nu={nu} lambda={lam} worst_rel={worst:.3e}")
    assert len(s.kernel_times()) == 4
    s.close()


def test_loss_at_nu_0_takes_the_trace_form(mfx):
    """nu = 0 with alpha0 != 1: the regulariser comes from the traces of the fp64 Gramians (the other branch of the loss)."""
    R = _random_matrix(3)
    k, lam, alpha, alpha0 = 8, 0.05, 10.0, 0.3
    H0 = (np.random.default_rng(4).standard_normal((R.cols, k)) * 0.1).astype(np.float32)
    W, H, losses, _ = _train(mfx, R, k, lam, alpha, H0, 3, alpha0=alpha0)
    want = ref.dense_loss(R, W, H, lam, alpha, alpha0, 0.0)
    assert abs(losses[-1] - want) <= 1e-6 * abs(want), (losses, want)
    assert losses[1] <= losses[0] * (1 + 1e-6) and losses[2] <= losses[1] * (1 + 1e-6)


@pytest.mark.parametrize("k,d", [(24, None), (64, None), (160, 64)])
def test_determinism_across_handles_and_memspaces(mfx, k, d):
    import torch  # noqa: F401  (device-resident inputs)
    R = _random_matrix(5, rows=2500, cols=400, density=0.03)
    R.csr_val[:5] = 0.0  # explicit zeros in both orientations
    from mfx import dataset as ds
    r = np.repeat(np.arange(R.rows), np.diff(R.csr_row_ptr.astype(np.int64)))
    R = ds.from_coo(R.rows, R.cols, r, R.csr_col_idx, R.csr_val)
    H0 = (np.random.default_rng(k).standard_normal((R.cols, k)) * 0.1).astype(np.float32)
    kw = dict(alpha0=0.3, nu=0.5) if d is None else dict(alpha0=0.3, nu=0.5, block=d)
    a = _train(mfx, R, k, 0.1, 2.0, H0, 2, **kw)
    b = _train(mfx, R, k, 0.1, 2.0, H0, 2, **kw)
    c = _train(mfx, R, k, 0.1, 2.0, H0, 2, device_arrays=_device_arrays(R), **kw)
    for other in (b, c):
        assert same(a[0], other[0]) and same(a[1], other[1])
        assert a[2] == other[2]
    plain = _train(mfx, R, k, 0.1, 2.0, H0, 2, **({} if d is None else {"block": d}))
    assert not same(a[0], plain[0])  # another objective: other factors


# ------------------------------------------------------------------------------------------------ 6. end to end
def test_planted_clusters_recommend_end_to_end(mfx):
    """The data and the bar of tests/test_gpu_ials.py::test_planted_clusters_recommend_end_to_end (20 clusters of 30 items,
    2 000 users with 25 training items of their own cluster and 2 random ones, one in-cluster item held out; k = 32,
    lambda = 0.1, alpha = 40, 10 iterations; HR@10 >= 0.9) at alpha0 = 0.3, nu = 0.5, exact and by block sweeps."""
    from mfx import dataset as ds
    rng = np.random.default_rng(11)
    nc, per, users = 20, 30, 2000
    items = nc * per
    tr_r, tr_c, te_r, te_c = [], [], [], []
    for u in range(users):
        cl = u % nc
        own = cl * per + rng.permutation(per)[:26]
        others = np.setdiff1d(np.arange(items), cl * per + np.arange(per))
        extra = rng.choice(others, 2, replace=False)
        tr = np.concatenate([own[:25], extra])
        tr_r += [u] * tr.size
        tr_c += list(tr)
        te_r.append(u)
        te_c.append(own[25])
    R = ds.from_coo(users, items, np.array(tr_r), np.array(tr_c), np.ones(len(tr_r), np.float32),
                    np.array(te_r), np.array(te_c), np.ones(len(te_r), np.float32))
    k = 32
    H0 = (rng.standard_normal((items, k)) * 0.1).astype(np.float32)
    for kw in ({}, {"block": 16}):
        s = mfx.ImplicitAlsSolver(R, _params(mfx, k, 0.1), 40.0, alpha0=0.3, nu=0.5, **kw)
        s.set_factors(H0)
        s.iterate(10)
        W, H = s.get_factors()
        s.close()
        top, _ = mfx.recommend(W, H, 1, 10, exclude=R)
        m = mfx.topn_metrics(top, mfx.test_data_of(R))
        print(f"ialsr-measured planted-clusters k={k} {kw} alpha0=0.3 nu=0.5 hr@10={m['hr']:.4f}")
        assert m["users"] == users
        assert m["hr"] >= 0.9, (kw, m)


# ------------------------------------------------------------------------------------------------ 7. refusals
@pytest.mark.parametrize("block", [None, 16])
@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf")])
def test_bad_strengths_rejected_at_create(mfx, bad, block):
    R = _random_matrix(7, rows=50, cols=40, density=0.2)
    from mfx import dataset as ds
    r = np.repeat(np.arange(R.rows), np.diff(R.csr_row_ptr.astype(np.int64)))
    v = R.csr_val.copy()
    v[len(v) // 2] = bad
    Rb = ds.from_coo(R.rows, R.cols, r, R.csr_col_idx, v)
    kw = dict(alpha0=0.3, nu=0.5) if block is None else dict(alpha0=0.3, nu=0.5, block=block)
    with pytest.raises(mfx.MfxError, match="implicit ALS"):
        mfx.ImplicitAlsSolver(Rb, _params(mfx, 8, 0.1), 1.0, **kw)
    with pytest.raises(mfx.MfxError, match="implicit ALS"):  # alpha * r overflowing fp32
        mfx.ImplicitAlsSolver(ds.from_coo(R.rows, R.cols, r, R.csr_col_idx, R.csr_val * np.float32(1e37)), _params(mfx, 8, 0.1), 100.0, **kw)
    H0 = (np.random.default_rng(1).standard_normal((R.cols, 8)) * 0.1).astype(np.float32)
    a = _train(mfx, R, 8, 0.1, 1.0, H0, 1, **kw)  # the library is usable afterwards
    assert np.isfinite(a[0]).all() and np.isfinite(a[2][0])


def test_operators_reject_bad_strengths_and_stay_usable(mfx):
    ptr, idx, val, X = data(16)
    good = mfx.ials_half(ptr, idx, val, X, 16, 0.1, 1.0, alpha0=0.3, nu=0.5)
    goodb = mfx.ials_block_half(ptr, idx, val, X, 16, 0.1, 1.0, 4, alpha0=0.3, nu=0.5)
    for bad in (-1.0, float("nan"), float("inf")):
        v = val.copy()
        v[100] = bad
        with pytest.raises(mfx.MfxError, match="mfx_ials_half_reg"):
            mfx.ials_half(ptr, idx, v, X, 16, 0.1, 1.0, alpha0=0.3, nu=0.5)
        with pytest.raises(mfx.MfxError, match="mfx_ials_block_half_reg"):
            mfx.ials_block_half(ptr, idx, v, X, 16, 0.1, 1.0, 4, alpha0=0.3, nu=0.5)
    i = idx.copy()
    i[100] = NROWS_X
    with pytest.raises(mfx.MfxError):
        mfx.ials_half(ptr, i, val, X, 16, 0.1, 1.0, alpha0=0.3, nu=0.5)
    assert same(mfx.ials_half(ptr, idx, val, X, 16, 0.1, 1.0, alpha0=0.3, nu=0.5), good)
    assert same(mfx.ials_block_half(ptr, idx, val, X, 16, 0.1, 1.0, 4, alpha0=0.3, nu=0.5), goodb)


def test_bad_memory_space_is_refused_and_the_library_stays_usable(mfx):
    import ctypes as C
    from mfx.api import _csx
    R = _random_matrix(8, rows=50, cols=40, density=0.2)
    cp = _params(mfx, 8, 0.1).to_c()
    csx = _csx(R)
    for fn, extra in ((mfx.lib().mfx_ials_create_reg, ()), (mfx.lib().mfx_ials_block_create_reg, (4,))):
        h = C.c_void_p()
        rc = fn(C.byref(h), C.byref(csx), C.byref(cp), 1.0, 0.3, 0.5, *extra, 7)
        assert rc == -1 and not h.value and b"memory space" in mfx.lib().mfx_last_error(), (rc, mfx.lib().mfx_last_error())
    H0 = (np.random.default_rng(1).standard_normal((R.cols, 8)) * 0.1).astype(np.float32)
    assert np.isfinite(_train(mfx, R, 8, 0.1, 1.0, H0, 1, alpha0=0.3, nu=0.5)[0]).all()
