"""GPU tests of implicit ALS by block subspace sweeps (mfx_ials_block_create / mfx_ials_block_half) against the fp64
reference of tests/ialsb_ref.py.

Tolerances are those of tests/test_gpu_ials.py for the same quantities: relative error of a segment's row at most
1e-3 where the condition number of its dense system is at most 1e3 (here the gate is asserted to skip NO segment),
backward error of a single-block sweep from zero against the dense system at most 3e-5, factors of one iteration
within 1e-3 of the largest reference entry, loss to 1e-6.

Measured maxima of the relative error per (k, d) over all segments, alphas and both starts (MI355X, printed by the
tests as `ialsb-measured` lines; profiles/r10_ialsb_accuracy.txt):
    k =  160, d =  64: 3.343e-06  (largest condition number 18.7)
    k =  256, d =  64: 2.943e-06  (largest condition number 29.1)
    k =  256, d = 128: 4.461e-06  (largest condition number 29.1)
    k =  192, d =  32: 2.663e-06  (largest condition number 20.2)
    k =  130, d = 128: 2.867e-05  (largest condition number 13.9)
    k = 1024, d = 128: 2.426e-06  (largest condition number 144.1)
    k =  512, d =  96: 2.918e-06  (largest condition number 60.3)
    k =  100, d = 128: 1.965e-05  (largest condition number 11.4)
    k =   64, d =  16: 4.545e-06  (largest condition number 6.5)
    k =   37, d =   5: 3.989e-06  (largest condition number 4.3)
    k =  256, d =  64: 5.857e-06  (largest condition number 3.2)  [20 000-entry segment, ten chunks]
    single-block k=16 worst_backward_error=4.264e-07
    single-block k=64 worst_backward_error=4.067e-07
    single-block k=100 worst_backward_error=5.119e-07
    single-block k=128 worst_backward_error=4.263e-07
    four-sweeps k=256 d=64 max_rel=3.708e-07
    iteration k=160 d=64 W=1.438e-06 H=1.632e-06
    planted-clusters k=160 d=64 hr@10=1.0000
"""
import numpy as np
import pytest

import ials_ref
import ialsb_ref
from test_gpu_ials import SIZES, _device_arrays, _params, _random_matrix, _segments

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1
    return m


def _cond(A):
    """2-norm condition number of a symmetric positive definite matrix (= np.linalg.cond(A), from the eigenvalues)."""
    ev = np.linalg.eigvalsh(A)
    return float(ev[-1] / ev[0]) if ev[0] > 0 else float("inf")


def _rel_errors(Y, Yr, sizes):
    out = []
    for s, n in enumerate(sizes):
        if n == 0:
            assert not np.any(Y[s]), s  # exactly zero
            assert not np.any(Yr[s]), s
            continue
        out.append(float(np.linalg.norm(Y[s] - Yr[s]) / max(np.linalg.norm(Yr[s]), 1e-30)))
    return out


def _check_operator(mfx, k, d, nrows_x, sizes, seed, alphas):
    ptr, idx, val = _segments(seed, nrows_x, sizes)
    X = (np.random.default_rng(k).standard_normal((nrows_x, k)) / np.sqrt(k)).astype(np.float32)
    lam = 0.1
    Y0 = (0.1 * np.random.default_rng(1000 + k).standard_normal((len(sizes), k))).astype(np.float32)
    worst, worst_cond = 0.0, 0.0
    for alpha in alphas:
        for s, n in enumerate(sizes):
            if n:
                A, _ = ials_ref.dense_system(ptr, idx, val, s, X, lam, alpha)
                c = _cond(A)
                worst_cond = max(worst_cond, c)
                assert c <= 1e3, (k, d, alpha, s, n, c)  # the gate of test_gpu_ials.py: it may skip no segment
        for Y_in in (Y0, None):
            Y = mfx.ials_block_half(ptr, idx, val, X, k, lam, alpha, d, Y_in=Y_in)
            Yr = ialsb_ref.block_sweep(ptr, idx, val, X, Y0 if Y_in is not None else np.zeros_like(Y0), lam, alpha, d)
            rel = _rel_errors(Y, Yr, sizes)
            print(f"ialsb-measured operator k={k} d={d} alpha={alpha} start={'Y0' if Y_in is not None else 'zero'} "
                  f"max_rel={max(rel):.3e}")
            worst = max(worst, max(rel))
            assert max(rel) <= 1e-3, (k, d, alpha, Y_in is None, rel)
    print(f"ialsb-measured operator k={k} d={d} worst_rel={worst:.3e} worst_cond={worst_cond:.1f}")


@pytest.mark.parametrize("k,d", [(160, 64), (256, 64), (256, 128), (192, 32), (130, 128), (1024, 128), (512, 96), (100, 128),
                                 (64, 16), (37, 5)])
def test_block_half_against_fp64_block_sweep(mfx, k, d):
    _check_operator(mfx, k, d, 6000, SIZES, 100 + k, (0.0, 1.0, 40.0))


def test_block_half_on_a_segment_of_ten_chunks(mfx):
    _check_operator(mfx, 256, 64, 30000, [20000, 0, 5], 100 + 256, (0.0, 1.0, 40.0))


@pytest.mark.parametrize("k", [16, 64, 100, 128])
def test_single_block_from_zero_solves_the_dense_system(mfx, k):
    nrows_x = 6000
    ptr, idx, val = _segments(100 + k, nrows_x, SIZES)
    X = (np.random.default_rng(k).standard_normal((nrows_x, k)) / np.sqrt(k)).astype(np.float32)
    worst = 0.0
    for alpha in (0.0, 1.0, 40.0):
        Y = mfx.ials_block_half(ptr, idx, val, X, k, 0.1, alpha, 128)
        for s, n in enumerate(SIZES):
            if n == 0:
                assert not np.any(Y[s]), (k, alpha, s)
                continue
            A, b = ials_ref.dense_system(ptr, idx, val, s, X, 0.1, alpha)
            be = ials_ref.backward_error(A, Y[s], b)
            worst = max(worst, be)
            assert be <= 3e-5, (k, alpha, s, n, be)
    print(f"ialsb-measured single-block k={k} worst_backward_error={worst:.3e}")


def test_four_chained_sweeps(mfx):
    k, d, alpha, lam, nrows_x = 256, 64, 40.0, 0.1, 6000
    ptr, idx, val = _segments(100 + k, nrows_x, SIZES)
    X = (np.random.default_rng(k).standard_normal((nrows_x, k)) / np.sqrt(k)).astype(np.float32)
    Y = (0.1 * np.random.default_rng(1000 + k).standard_normal((len(SIZES), k))).astype(np.float32)
    Yr = Y.astype(np.float64)
    for _ in range(4):
        Y = mfx.ials_block_half(ptr, idx, val, X, k, lam, alpha, d, Y_in=Y)
        Yr = ialsb_ref.block_sweep(ptr, idx, val, X, Yr, lam, alpha, d)
    rel = _rel_errors(Y, Yr, SIZES)
    print(f"ialsb-measured four-sweeps k={k} d={d} max_rel={max(rel):.3e}")
    assert max(rel) <= 1e-3, rel


def _solver(mfx, R, k, lam, alpha, d, H0, W0, n, device_arrays=None):
    s = mfx.ImplicitAlsSolver(R if device_arrays is None else None, _params(mfx, k, lam), alpha, device_arrays=device_arrays, block=d)
    s.set_factors(H0, W0)
    rep = s.iterate(n)
    W, H = s.get_factors()
    kt = s.kernel_times()
    s.close()
    return W, H, rep, kt


def test_one_iteration_matches_fp64_reference_and_warm_start(mfx):
    R = _random_matrix(1)
    k, d, lam, alpha = 160, 64, 0.1, 5.0
    H0 = (np.random.default_rng(2).standard_normal((R.cols, k)) * 0.1).astype(np.float32)
    W, H, rep, kt = _solver(mfx, R, k, lam, alpha, d, H0, None, 1)
    assert rep[0].update_time > 0 and rep[0].rmse == 0
    Wr, Hr = ialsb_ref.iteration(R, H0.astype(np.float64), np.zeros((R.rows, k)), lam, alpha, d)
    print(f"ialsb-measured iteration k={k} d={d} W={np.max(np.abs(W - Wr)) / np.max(np.abs(Wr)):.3e} "
          f"H={np.max(np.abs(H - Hr)) / np.max(np.abs(Hr)):.3e}")
    assert np.max(np.abs(W - Wr)) <= 1e-3 * np.max(np.abs(Wr))
    assert np.max(np.abs(H - Hr)) <= 1e-3 * np.max(np.abs(Hr))
    assert not np.any(W[7]) and not np.any(H[11])
    assert set(kt) == {"ialsb_half_rows(W over H)", "ialsb_half_cols(H over W)", "ialsb_base_gram(H)", "ialsb_base_gram(W)"}
    # warm start: W0 is read
    W0 = (np.random.default_rng(3).standard_normal((R.rows, k)) * 0.1).astype(np.float32)
    W2, H2, _, _ = _solver(mfx, R, k, lam, alpha, d, H0, W0, 1)
    Wr2, Hr2 = ialsb_ref.iteration(R, H0.astype(np.float64), W0.astype(np.float64), lam, alpha, d)
    assert np.max(np.abs(W2 - Wr2)) <= 1e-3 * np.max(np.abs(Wr2))
    assert np.max(np.abs(H2 - Hr2)) <= 1e-3 * np.max(np.abs(Hr2))
    assert not np.any(W2[7]) and not np.any(H2[11])
    assert np.max(np.abs(W2 - W)) > 1e-3 * np.max(np.abs(Wr))  # ... and changes the result


def test_loss_matches_dense_loss_and_decreases(mfx):
    R = _random_matrix(3)
    k, d, lam, alpha = 160, 64, 0.05, 10.0
    H0 = (np.random.default_rng(4).standard_normal((R.cols, k)) * 0.1).astype(np.float32)
    s = mfx.ImplicitAlsSolver(R, _params(mfx, k, lam), alpha, block=d)
    s.set_factors(H0)
    prev = None
    for it in range(8):
        s.iterate(1)
        got = s.loss()
        W, H = s.get_factors()
        want = ials_ref.dense_loss(R, W, H, lam, alpha)
        assert abs(got - want) <= 1e-6 * abs(want), (it, got, want)
        if prev is not None:
            assert got <= prev * (1 + 1e-6), (it, prev, got)
        prev = got
    s.close()


def test_loss_at_rank_1024(mfx):
    R = _random_matrix(9, rows=60, cols=50, density=0.1)
    k, lam, alpha = 1024, 0.05, 10.0
    H0 = (np.random.default_rng(4).standard_normal((R.cols, k)) * 0.03).astype(np.float32)
    s = mfx.ImplicitAlsSolver(R, _params(mfx, k, lam), alpha, block=0)
    s.set_factors(H0)
    s.iterate(1)
    got = s.loss()
    W, H = s.get_factors()
    s.close()
    want = ials_ref.dense_loss(R, W, H, lam, alpha)
    assert abs(got - want) <= 1e-6 * abs(want), (got, want)


def test_determinism_across_handles_and_memspaces(mfx):
    import torch  # noqa: F401  (device-resident inputs)
    R = _random_matrix(5, rows=2500, cols=400, density=0.03)
    k = 256
    H0 = (np.random.default_rng(k).standard_normal((R.cols, k)) * 0.1).astype(np.float32)
    for d in (64, 128):
        a = _solver(mfx, R, k, 0.1, 2.0, d, H0, None, 3)
        b = _solver(mfx, R, k, 0.1, 2.0, d, H0, None, 3)
        c = _solver(mfx, R, k, 0.1, 2.0, d, H0, None, 3, device_arrays=_device_arrays(R))
        for x, y, z in zip(a[:2], b[:2], c[:2]):
            assert np.all(np.isfinite(x))
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
            assert np.array_equal(x.view(np.uint32), z.view(np.uint32))


def test_planted_clusters_recommend_end_to_end(mfx):
    """The data of test_gpu_ials.py's test of the same name: 20 clusters of 30 items, 2 000 users with 25 training items
    of their own cluster plus 2 random ones, one more in-cluster item held out.  k = 160 in blocks of 64, 10 iterations
    from W = 0: the top-10 lists must find the held-out item for at least 90 % of the users."""
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
    k = 160
    H0 = (rng.standard_normal((items, k)) * 0.1).astype(np.float32)
    W, H, _, _ = _solver(mfx, R, k, 0.1, 40.0, 64, H0, None, 10)
    top, _ = mfx.recommend(W, H, 1, 10, exclude=R)
    m = mfx.topn_metrics(top, mfx.test_data_of(R))
    print(f"ialsb-measured planted-clusters k={k} d=64 hr@10={m['hr']:.4f}")
    assert m["users"] == users
    assert m["hr"] >= 0.9, m
