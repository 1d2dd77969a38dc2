"""GPU tests of explicit ALS by block subspace sweeps (mfx_als_block_create / mfx_als_block_half) against the fp64
reference of tests/alsb_ref.py.

Data of the operator tests: the shapes of tests/test_gpu_ials.py (segments of 0, 1, 2 and 3 chunks of 2048 entries over
6000 rows of X ~ N(0, 1/k), values 0..5 with explicit zeros, lambda = 0.1).  Tolerances are the project's for this kernel
family: relative error of a segment's row at most 1e-3 where the condition number of its dense system is at most 1e3 (the
gate is asserted to skip NO segment: the worst is 40.3 at reg 0, k = 256, and 12.8 at reg 1, k = 100), backward error of a
single-block sweep against the dense system at most 3e-5, factors of one iteration within 1e-3 of the largest reference
entry, the trainer at k <= 128 with one block within the bounds of test_als_medium_vs_oracle.

The RMSE trace of the trainer above rank 128 (test_trainer_above_rank_128) is asserted at RMSE_TRACE_TOL = four times the
maximum measured on the MI355X; that maximum and every other measured figure is printed as an `alsb-measured` line and
kept in profiles/r12_alsb_accuracy.txt.

Measured maxima of the relative error per (k, d) over all segments, both reg values and both starts (MI355X):
    k =  160, d =  64: 1.011e-06  (largest condition number 30.7)
    k =  256, d =  64: 9.108e-07  (largest condition number 40.3)
    k =  256, d = 128: 1.265e-06  (largest condition number 40.3)
    k =  192, d =  32: 1.363e-06  (largest condition number 36.4)
    k =  130, d = 128: 1.576e-06  (largest condition number 20.5)
    k = 1024, d = 128: 2.267e-06  (largest condition number 23.6)
    k =  512, d =  96: 1.609e-06  (largest condition number 30.8)
    k =  100, d = 128: 1.345e-06  (largest condition number 19.2)
    k =   64, d =  16: 1.007e-06  (largest condition number 25.4)
    k =   37, d =   5: 1.066e-06  (largest condition number 28.5)
    k =  256, d =  64: 1.953e-06  (largest condition number 12.6)  [20 000-entry segment, ten chunks]
    single-block k = 16 / 64 / 100 / 128: worst backward error 4.0e-07 / 3.9e-07 / 5.3e-07 / 4.5e-07
    40 sweeps from zero at k = 256, d = 64: worst distance to the dense solve 7.060e-05 (reg 0), 1.956e-06 (reg 1)
    one-block trainer against the pinned oracle: RMSE gap 3.1e-07 (k = 40), 3.1e-05 (k = 128); H 1.2e-04, 3.7e-03
    RMSE trace k = 160, d = 64: max gap 2.729e-06 (reg 0), 2.324e-08 (reg 1)
"""
import numpy as np
import pytest

import alsb_ref
from test_gpu_als import relerr
from test_gpu_ials import SIZES, _device_arrays, _params, _segments

pytestmark = pytest.mark.gpu

LAM = 0.1
CASES = [(160, 64), (256, 64), (256, 128), (192, 32), (130, 128), (1024, 128), (512, 96), (100, 128), (64, 16), (37, 5)]
# |rmse(GPU) - rmse(fp64 reference)| over three iterations at k = 160, d = 64 on the 300 x 200 matrix: four times the
# measured maximum (see the docstring of test_trainer_above_rank_128)
RMSE_TRACE_TOL = 4 * 2.729e-6


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1
    return m


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def _cond(A):
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


def _operator_data(k, nrows_x=6000, sizes=SIZES):
    ptr, idx, val = _segments(100 + k, nrows_x, sizes)
    X = (np.random.default_rng(k).standard_normal((nrows_x, k)) / np.sqrt(k)).astype(np.float32)
    return ptr, idx, val, X


def _check_operator(mfx, k, d, nrows_x, sizes):
    ptr, idx, val, X = _operator_data(k, nrows_x, sizes)
    assert (val == 0).any() and val.max() == 5
    Y0 = (0.1 * np.random.default_rng(1000 + k).standard_normal((len(sizes), k))).astype(np.float32)
    worst, worst_cond = 0.0, 0.0
    for reg in (0, 1):
        for s, n in enumerate(sizes):
            if n:
                c = _cond(alsb_ref.dense_system(ptr, idx, val, s, X, LAM, reg)[0])
                worst_cond = max(worst_cond, c)
                assert c <= 1e3, (k, d, reg, s, n, c)  # the project's gate: it may skip no segment
        for Y_in in (Y0, None):
            Y = mfx.als_block_half(ptr, idx, val, X, k, LAM, d, Y_in=Y_in, count_reg=bool(reg))
            Yr = alsb_ref.block_sweep(ptr, idx, val, X, Y0 if Y_in is not None else np.zeros_like(Y0), LAM, min(d, k), reg)
            rel = _rel_errors(Y, Yr, sizes)
            print(f"alsb-measured operator k={k} d={d} reg={reg} start={'Y0' if Y_in is not None else 'zero'} max_rel={max(rel):.3e}")
            worst = max(worst, max(rel))
            assert max(rel) <= 1e-3, (k, d, reg, Y_in is None, rel)
    print(f"alsb-measured operator k={k} d={d} worst_rel={worst:.3e} worst_cond={worst_cond:.1f}")


# ------------------------------------------------------------------------------------------------ 1. operator
@pytest.mark.parametrize("k,d", CASES)
def test_block_half_against_fp64_block_sweep(mfx, k, d):
    _check_operator(mfx, k, d, 6000, SIZES)


def test_block_half_on_a_segment_of_ten_chunks(mfx):
    _check_operator(mfx, 256, 64, 30000, [20000, 0, 5])


# ------------------------------------------------------------------------------------------------ 2. single block
@pytest.mark.parametrize("k", [16, 64, 100, 128])
def test_single_block_solves_the_dense_system_from_any_start(mfx, k):
    ptr, idx, val, X = _operator_data(k)
    Y0 = (0.1 * np.random.default_rng(1000 + k).standard_normal((len(SIZES), k))).astype(np.float32)
    for reg in (0, 1):
        for Y_in in (None, Y0):
            Y = mfx.als_block_half(ptr, idx, val, X, k, LAM, 128, Y_in=Y_in, count_reg=bool(reg))
            worst = 0.0
            for s, n in enumerate(SIZES):
                if n == 0:
                    assert not np.any(Y[s]), (k, reg, s)
                    continue
                A, b = alsb_ref.dense_system(ptr, idx, val, s, X, LAM, reg)
                be = alsb_ref.backward_error(A, Y[s], b)
                worst = max(worst, be)
                assert be <= 3e-5, (k, reg, Y_in is None, s, n, be)
            print(f"alsb-measured single-block k={k} reg={reg} start={'zero' if Y_in is None else 'Y0'} worst_backward_error={worst:.3e}")


# ------------------------------------------------------------------------------------------------ 3. chained sweeps
@pytest.mark.parametrize("reg", [0, 1])
def test_four_chained_sweeps(mfx, reg):
    k, d = 256, 64
    ptr, idx, val, X = _operator_data(k)
    Y = (0.1 * np.random.default_rng(1000 + k).standard_normal((len(SIZES), k))).astype(np.float32)
    Yr = Y.astype(np.float64)
    for _ in range(4):
        Y = mfx.als_block_half(ptr, idx, val, X, k, LAM, d, Y_in=Y, count_reg=bool(reg))
        Yr = alsb_ref.block_sweep(ptr, idx, val, X, Yr, LAM, d, reg)
    rel = _rel_errors(Y, Yr, SIZES)
    print(f"alsb-measured four-sweeps k={k} d={d} reg={reg} max_rel={max(rel):.3e}")
    assert max(rel) <= 1e-3, rel


# ------------------------------------------------------------------------------------------------ 4. convergence
@pytest.mark.parametrize("reg", [0, 1])
def test_sweeps_converge_to_the_als_solution(mfx, reg):
    """40 chained sweeps from zero end within 1e-3 of the dense solve on every non-empty segment (the fp64 reference gets
    there after at most 28 sweeps at reg 0 and 22 at reg 1)."""
    k, d = 256, 64
    ptr, idx, val, X = _operator_data(k)
    Y = None
    for _ in range(40):
        Y = mfx.als_block_half(ptr, idx, val, X, k, LAM, d, Y_in=Y, count_reg=bool(reg))
    worst = 0.0
    for s, n in enumerate(SIZES):
        if n == 0:
            assert not np.any(Y[s])
            continue
        A, b = alsb_ref.dense_system(ptr, idx, val, s, X, LAM, reg)
        want = np.linalg.solve(A, b)
        dist = float(np.linalg.norm(Y[s] - want) / np.linalg.norm(want))
        worst = max(worst, dist)
        assert dist <= 1e-3, (reg, s, n, dist)
    print(f"alsb-measured convergence k={k} d={d} reg={reg} sweeps=40 worst_distance={worst:.3e}")


# ------------------------------------------------------------------------------------------------ 5. pinned oracle
@pytest.mark.parametrize("k", [40, 128])
def test_trainer_with_one_block_against_the_pinned_oracle(mfx, orc, k):
    """The matrix, iterations and tolerances of test_als_medium_vs_oracle (tests/test_gpu_als.py)."""
    d = mfx.dataset.synth_ratings(3000, 400, 150_000, seed=31 + k, skew=1.1, test_frac=0.01, empty_row_frac=0.02)
    H0 = mfx.initial_col(d.cols, k)
    Wr, Hr, rmse_ref, _ = orc.als(d, H0, k, 0.05, 2, orc.max_threads())
    p = _params(mfx, k, 0.05)
    s = mfx.AlsSolver(d, mfx.test_data_of(d), p, block=128)
    s.set_factors(H0.copy())
    rep = s.iterate(2)
    W, H = s.get_factors()
    s.close()
    rmse = np.array([r.rmse for r in rep])
    print(f"alsb-measured oracle k={k} rmse_gap={np.max(np.abs(rmse - rmse_ref)):.3e} W={relerr(W, Wr):.3e} H={relerr(H, Hr):.3e}")
    assert np.all(np.abs(rmse - rmse_ref) < 1e-4), (rmse, rmse_ref)
    assert relerr(W, Wr) < 5e-3 and relerr(H, Hr) < 5e-3


# ------------------------------------------------------------------------------------------------ 6. above rank 128
def _matrix_with_test(seed, rows=300, cols=200, density=0.06, held_out=500):
    from mfx import dataset as ds
    rng = np.random.default_rng(seed)
    mask = rng.random((rows, cols)) < density
    mask[7, :] = False  # an empty user
    mask[:, 11] = False  # an empty item
    r, c = np.nonzero(mask)
    v = rng.integers(0, 6, r.size).astype(np.float32)
    free = np.flatnonzero(~mask.ravel())
    t = rng.choice(free, held_out, replace=False)
    return ds.from_coo(rows, cols, r, c, v, t // cols, t % cols, rng.integers(0, 6, held_out).astype(np.float32))


def _solver(mfx, R, k, d, H0, W0, reg=0, device_arrays=None, lam=LAM):
    s = mfx.AlsSolver(R if device_arrays is None else None, mfx.test_data_of(R) if device_arrays is None else None,
                      _params(mfx, k, lam), device_arrays=device_arrays, block=d, count_reg=bool(reg))
    s.set_factors(H0, W0)
    return s


@pytest.mark.parametrize("reg", [0, 1])
def test_trainer_above_rank_128(mfx, reg):
    """One iteration against the fp64 reference from a cold and a warm start, then the reported RMSE of three iterations
    against the reference's trace.  Measured on the MI355X (profiles/r12_alsb_accuracy.txt): the largest
    |rmse - rmse_ref| over the three iterations is 2.729e-06 at reg 0 (RMSE 2.88, 2.31, 2.21: most rows hold fewer entries
    than k, so the rounding noise of these underdetermined systems moves with the summation order) and 2.324e-08 at
    reg 1; asserted at RMSE_TRACE_TOL = four times the larger."""
    R = _matrix_with_test(1)
    T = mfx.test_data_of(R)
    assert T.nnz == 500
    k, d = 160, 64
    H0 = (np.random.default_rng(2).standard_normal((R.cols, k)) * 0.1).astype(np.float32)
    s = _solver(mfx, R, k, d, H0, None, reg)
    rep = s.iterate(1)
    W, H = s.get_factors()
    kt = s.kernel_times()
    assert rep[0].update_time > 0
    Wr, Hr = alsb_ref.iteration(R, H0.astype(np.float64), np.zeros((R.rows, k)), LAM, d, reg)
    print(f"alsb-measured iteration k={k} d={d} reg={reg} W={np.max(np.abs(W - Wr)) / np.max(np.abs(Wr)):.3e} "
          f"H={np.max(np.abs(H - Hr)) / np.max(np.abs(Hr)):.3e}")
    assert np.max(np.abs(W - Wr)) <= 1e-3 * np.max(np.abs(Wr))
    assert np.max(np.abs(H - Hr)) <= 1e-3 * np.max(np.abs(Hr))
    assert not np.any(W[7]) and not np.any(H[11])
    assert set(kt) == {"alsb_half_rows(W over H)", "alsb_half_cols(H over W)"}
    # the RMSE trace: three iterations in all
    got, want, gaps = [rep[0].rmse], [alsb_ref.test_rmse(T, Wr, Hr)], []
    assert abs(got[0] - mfx.test_rmse(T, W, H, R.rows, R.cols, k, True)) <= 1e-9
    for _ in range(2):
        got.append(s.iterate(1)[0].rmse)
        Wg, Hg = s.get_factors()
        assert abs(got[-1] - mfx.test_rmse(T, Wg, Hg, R.rows, R.cols, k, True)) <= 1e-9
        Wr, Hr = alsb_ref.iteration(R, Hr, Wr, LAM, d, reg)
        want.append(alsb_ref.test_rmse(T, Wr, Hr))
    s.close()
    gaps = np.abs(np.array(got) - np.array(want))
    print(f"alsb-measured rmse-trace k={k} d={d} reg={reg} gpu={got} fp64={want} max_gap={gaps.max():.3e}")
    assert gaps.max() <= RMSE_TRACE_TOL, (got, want)
    # warm start: W0 is read
    W0 = (np.random.default_rng(3).standard_normal((R.rows, k)) * 0.1).astype(np.float32)
    s = _solver(mfx, R, k, d, H0, W0, reg)
    s.iterate(1)
    W2, H2 = s.get_factors()
    s.close()
    Wr2, Hr2 = alsb_ref.iteration(R, H0.astype(np.float64), W0.astype(np.float64), LAM, d, reg)
    assert np.max(np.abs(W2 - Wr2)) <= 1e-3 * np.max(np.abs(Wr2))
    assert np.max(np.abs(H2 - Hr2)) <= 1e-3 * np.max(np.abs(Hr2))
    assert not np.any(W2[7]) and not np.any(H2[11])
    assert np.max(np.abs(W2 - W)) > 1e-3 * np.max(np.abs(W))  # ... and changes the result


# ------------------------------------------------------------------------------------------------ 7. objective
@pytest.mark.parametrize("reg", [0, 1])
def test_training_objective_never_increases(mfx, reg):
    R = _matrix_with_test(3)
    k, d, lam = 160, 64, 0.05
    H0 = (np.random.default_rng(4).standard_normal((R.cols, k)) * 0.1).astype(np.float32)
    s = _solver(mfx, R, k, d, H0, None, reg, lam=lam)
    prev, trace = alsb_ref.objective(R, np.zeros((R.rows, k)), H0, lam, reg), []
    for it in range(8):
        s.iterate(1, with_rmse=False)
        W, H = s.get_factors()
        cur = alsb_ref.objective(R, W, H, lam, reg)
        trace.append(cur)
        assert cur <= prev * (1 + 1e-6), (reg, it, prev, cur)
        prev = cur
    s.close()
    print(f"alsb-measured objective k={k} d={d} reg={reg} trace={['%.6e' % t for t in trace]}")


# ------------------------------------------------------------------------------------------------ 8. rank 1024
def test_one_iteration_at_rank_1024(mfx):
    R = _matrix_with_test(9, rows=60, cols=50, density=0.1, held_out=50)
    k, d = 1024, 128
    H0 = (np.random.default_rng(4).standard_normal((R.cols, k)) * 0.03).astype(np.float32)
    s = _solver(mfx, R, k, d, H0, None)
    s.iterate(1)
    W, H = s.get_factors()
    s.close()
    Wr, Hr = alsb_ref.iteration(R, H0.astype(np.float64), np.zeros((R.rows, k)), LAM, d, 0)
    print(f"alsb-measured iteration k={k} d={d} reg=0 W={np.max(np.abs(W - Wr)) / np.max(np.abs(Wr)):.3e} "
          f"H={np.max(np.abs(H - Hr)) / np.max(np.abs(Hr)):.3e}")
    assert np.max(np.abs(W - Wr)) <= 1e-3 * np.max(np.abs(Wr))
    assert np.max(np.abs(H - Hr)) <= 1e-3 * np.max(np.abs(Hr))
    assert not np.any(W[7]) and not np.any(H[11])


# ------------------------------------------------------------------------------------------------ 9. determinism
def test_determinism_across_handles_and_memspaces(mfx):
    import torch  # noqa: F401  (device-resident inputs)
    from test_gpu_ials import _random_matrix
    R = _random_matrix(5, rows=1500, cols=400, density=0.03)
    k = 256
    H0 = (np.random.default_rng(k).standard_normal((R.cols, k)) * 0.1).astype(np.float32)

    def run(d, device_arrays=None):
        s = _solver(mfx, R, k, d, H0, None, device_arrays=device_arrays)
        s.iterate(2, with_rmse=False)
        out = s.get_factors()
        s.close()
        return out

    for d in (64, 128):
        a, b, c = run(d), run(d), run(d, _device_arrays(R))
        for x, y, z in zip(a, b, c):
            assert np.all(np.isfinite(x))
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
            assert np.array_equal(x.view(np.uint32), z.view(np.uint32))


# ------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_values_must_be_finite_and_negative_values_count(mfx, bad):
    ptr, idx, val, X = _operator_data(37, 500, [3, 0, 10, 25])
    v = val.copy()
    v[17] = bad
    with pytest.raises(mfx.MfxError, match="finite"):
        mfx.als_block_half(ptr, idx, v, X, 37, LAM, 5)
    v[17] = -3.0  # an entry like any other
    Y = mfx.als_block_half(ptr, idx, v, X, 37, LAM, 5)
    Yr = alsb_ref.block_sweep(ptr, idx, v, X, np.zeros((4, 37)), LAM, 5, 0)
    assert max(_rel_errors(Y, Yr, [3, 0, 10, 25])) <= 1e-3
