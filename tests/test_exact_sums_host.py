"""Host checks of tests/exact_sums.py, the order-independent inputs of test_gpu_ccd_exact.py and test_gpu_als_exact_sums.py:
the bounds hold for every shape and value set the GPU modules use (the full-size pattern excepted: it exists on the device
only and is checked there), the CPU oracle equals the integer formula bit for bit at any thread count, a sequential fp32 sum
in random order gives the same bits, value sets that break a bound are refused, and the negative control's arithmetic is right.
"""
import numpy as np
import pytest

import exact_sums as ex
from exact_sums import bits


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def pattern():
    from mfx import dataset
    return ex.ml1m_pattern(dataset)


def _bit_equal(a, b):
    return np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------ preconditions of everything the GPU modules use
def test_preconditions_hold_for_the_ccd_module(pattern):
    for k, live in ex.CCD_RANKS:
        for cfg in ("A", "B"):
            choice, (data, W0, lam) = ex.ccd_case(pattern, cfg, k, live)
            b = ex.preconditions(data, W0, live, lam, cfg)
            assert all(v["g"] <= ex.SIGNIFICAND and v["h"] <= ex.SIGNIFICAND for v in b.values()), (cfg, k, live, b)
    from mfx import dataset
    for name, d in ex.small_patterns(dataset).items():
        for cfg in ("A", "B"):
            ex.ccd_case(d, cfg, 3, 1)


def test_largest_sum_of_the_ml1m_pattern_leaves_headroom(pattern):
    """the issue's figure: the longest column has 5913 entries, the longest row 3593, and the widest value sets fit"""
    lens_c = np.diff(pattern.csc_col_ptr.astype(np.int64)); lens_r = np.diff(pattern.csr_row_ptr.astype(np.int64))
    assert lens_c.max() == 5913 and lens_r.max() == 3593
    choice, (data, W0, lam) = ex.ccd_case(pattern, "A", 7, 1)
    assert choice == ex.A_LADDER[0]
    need = max(max(v["g"], v["h"]) for v in ex.preconditions(data, W0, 1, lam, "A").values())
    assert np.log2(need) < 24


@pytest.mark.parametrize("long_segment", [0, 250_000])
def test_preconditions_hold_for_the_segment_lists(long_segment):
    ptr, idx, nvec, lens = ex.segment_pattern(long_segment)
    assert lens.max() == max(20011, long_segment) and (lens == 0).sum() > 5 and (lens == 1).sum() >= 700
    val, vec, lam = ex.sweep_inputs(ptr, idx, nvec)
    ex.check_sweep(ptr, val, vec, lam)
    assert set(np.unique(val)) <= set(range(1, 6)) and ex.granularity(vec) >= 1 / 8 and np.abs(vec).max() <= 1


def test_preconditions_hold_for_the_als_module():
    for k in ex.GRAMIAN_KS:
        X = ex.dyadic_table(300, k, k)
        assert ex.check_gramian(max(ex.GRAMIAN_COUNTS), X) <= ex.SIGNIFICAND
    for k, nrows in ex.DIAGONAL_CASES:
        X, x = ex.one_hot_table(nrows, k, k)
        ptr, idx, val = ex.diagonal_segments(nrows, ex.DIAGONAL_SIZES, 100 + k)
        assert np.count_nonzero(X) == nrows and set(np.unique(np.abs(x))) == {0.5, 1.0}
        for alpha in (None,) + ex.IALS_ALPHAS:
            if alpha is None and k > 128:
                continue
            assert ex.check_sensitivity(ptr, idx, val, x, k, ex.ALS_LAMBDA, alpha) >= ex.ULP_SENSITIVITY
            A, b, y = ex.diagonal_solution(ptr, idx, val, x, k, ex.ALS_LAMBDA, alpha)
            # A and b are exact: integers in units of 1/16 (lambda = 1/4, weights of 1/2) well inside 24 bits
            assert np.all(A * 16 == np.rint(A * 16)) and np.all(b * 16 == np.rint(b * 16)) and A.max() * 16 < ex.SIGNIFICAND


# ------------------------------------------------------------------ oracle == integer formula, any thread count, any order
def test_oracle_sweep_equals_integer_formula_on_the_segment_lists(orc):
    for long_segment in (0, 250_000):
        ptr, idx, nvec, lens = ex.segment_pattern(long_segment)
        val, vec, lam = ex.sweep_inputs(ptr, idx, nvec)
        want = ex.int_sweep(ptr, idx, val, vec, lam)
        for threads in (1, 4, orc.max_threads()):
            assert _bit_equal(orc.rank_one_sweep(ptr, idx, val, vec, lam, threads), want), (long_segment, threads)
        assert np.all(want[lens == 0] == 0)


@pytest.mark.parametrize("cfg", ["A", "B"])
@pytest.mark.parametrize("k,live", [(7, 0), (7, 1), (7, 6), (1, 0)])
def test_oracle_ccd_equals_integer_formula(orc, pattern, cfg, k, live):
    _, (data, W0, lam) = ex.ccd_case(pattern, cfg, k, live)
    v, u, csc, csr = ex.int_ccd_rank(data, W0, live, lam, with_u=(cfg == "B"))
    outs = [orc.ccdr1(data, W0, k, lam, 1, 1, t) for t in (1, 4, orc.max_threads())]
    for W, H, _, _, c, r in outs:
        assert _bit_equal(H[live], v)
        dead = np.arange(k) != live
        assert np.all(H[dead] == 0) and np.all(W[dead] == 0)
        if cfg == "B":
            assert _bit_equal(W[live], u) and _bit_equal(c, csc) and _bit_equal(r, csr)
            assert _bit_equal(v, data_c(data) * np.float32(0.5))  # v_j = c_j / 2 exactly
        for a, b in zip((W, H, c, r), outs[0][:2] + outs[0][4:]):
            assert _bit_equal(a, b)  # the oracle's own thread counts agree on every output, config A's u-pass included


def data_c(data):
    c = np.zeros(data.cols, np.float32)
    c[ex.col_of_csc(data)] = data.csc_val
    return c


def test_random_summation_orders_give_the_same_bits(pattern):
    rng = np.random.default_rng(17)
    ptr, idx, nvec, lens = ex.segment_pattern(0)
    val, vec, lam = ex.sweep_inputs(ptr, idx, nvec)
    want = ex.int_sweep(ptr, idx, val, vec, lam)
    for _ in range(3):
        assert _bit_equal(ex.permuted_fp32_sweep(ptr, idx, val, vec, lam, rng), want)
    for cfg in ("A", "B"):
        _, (data, W0, lam) = ex.ccd_case(pattern, cfg, 7, 1)
        v, u, _, _ = ex.int_ccd_rank(data, W0, 1, lam, with_u=(cfg == "B"))
        assert _bit_equal(ex.permuted_fp32_sweep(data.csc_col_ptr, data.csc_row_idx, data.csc_val, W0[1], lam, rng), v)
        if cfg == "B":
            assert _bit_equal(ex.permuted_fp32_sweep(data.csr_row_ptr, data.csr_col_idx, data.csr_val, v, lam, rng), u)


def test_order_matters_on_ordinary_inputs(pattern):
    """... and the claim is not vacuous: on non-dyadic values of the same pattern two orders differ in some segment"""
    rng = np.random.default_rng(18)
    u = rng.uniform(0.001, 0.101, pattern.rows).astype(np.float32)
    a = ex.permuted_fp32_sweep(pattern.csc_col_ptr, pattern.csc_row_idx, pattern.csc_val, u, 0.05, rng)
    b = ex.permuted_fp32_sweep(pattern.csc_col_ptr, pattern.csc_row_idx, pattern.csc_val, u, 0.05, rng)
    assert not _bit_equal(a, b)


# ------------------------------------------------------------------ the generators refuse what breaks a bound
def test_generators_reject_value_sets_that_break_a_bound(pattern):
    with pytest.raises(ex.BoundExceeded):
        ex.config_a(pattern, 3, 1, r_max=4000)            # 5913 entries x 4000 x 8 eighths > 2^24
    with pytest.raises(ex.BoundExceeded):
        ex.config_a(pattern, 3, 1, lam=0.05)              # lambda is not dyadic
    with pytest.raises(ex.BoundExceeded):
        ex.config_b(pattern, 3, 1, c_quarters=256)        # rows of 3593 entries: sum c^2 / 4 in units of 1/64 > 2^24
    ptr, idx, nvec, _ = ex.segment_pattern(250_000)
    with pytest.raises(ex.BoundExceeded):                 # the widest set does not fit a 250 000-entry segment: h needs 24.5 bits
        ex.sweep_inputs(ptr, idx, nvec, ladder=ex.A_LADDER[:1])
    data, W0, lam = ex.config_a(pattern, 3, 1)
    W0[0, 5] = 0.5
    with pytest.raises(ex.BoundExceeded):
        ex.preconditions(data, W0, 1, lam, "A")           # a dead rank that is not zero
    with pytest.raises(ex.BoundExceeded):
        ex.preconditions(data, ex.live_rank(3, pattern.rows, 1, np.float32(1)), 1, 1.0, "B")  # ratings not constant per column
    with pytest.raises(ex.BoundExceeded):
        ex.granularity([0.1])
    with pytest.raises(ex.BoundExceeded):
        ex.check_gramian(1 << 19, ex.dyadic_table(8, 4, 0))


# ------------------------------------------------------------------ the negative control
@pytest.mark.parametrize("cfg", ["A", "B"])
def test_negative_control_arithmetic(orc, pattern, cfg):
    """One rating of the longest column changed by 1: the integer formula moves exactly that column of v (and, config B,
    rows of that column and no others in u)."""
    _, (data, W0, lam) = ex.ccd_case(pattern, cfg, 7, 1)
    changed, j, rows = ex.one_rating_changed(data, W0[1])
    assert np.count_nonzero(changed.csc_val != data.csc_val) == 1 and np.count_nonzero(changed.csr_val != data.csr_val) == 1
    assert np.array_equal(changed.csr_val[ex.csc_of_csr(data)], changed.csc_val)
    v, u, _, _ = ex.int_ccd_rank(data, W0, 1, lam, with_u=(cfg == "B"))
    v2 = ex.int_sweep(changed.csc_col_ptr, changed.csc_row_idx, changed.csc_val, W0[1], lam)
    assert list(np.nonzero(bits(v) != bits(v2))[0]) == [j]
    n = int(np.diff(data.csc_col_ptr.astype(np.int64)).max())
    print(f"negative-control config={cfg} column={j} entries={n} relerr_seen_by_the_2e-5_check={ex.relerr(v2, v):.3e}")
    # the move is u_i / den on a column of n entries: far below the kernels' own rounding on ordinary data of that length
    assert abs(float(v2[j]) - float(v[j])) * n < 4.0
    if cfg == "B":
        # the changed reference's u-pass sees its own v and ratings: rows of column j move (those whose sums are short
        # enough to feel 1 / (2 n)), no other row does
        Wc, Hc, *_ = orc.ccdr1(changed, W0, 7, lam, 1, 1, 1)
        assert _bit_equal(Hc[1], v2)
        moved = np.nonzero(bits(u) != bits(Wc[1]))[0]
        assert moved.size > 0 and np.all(np.isin(moved, rows))
