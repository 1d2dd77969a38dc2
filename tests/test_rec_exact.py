"""CPU tests of the exact top-N reference (tests/rec_exact.py): fmaf32 against libm fmaf bit for bit, the FMA chain
against a scalar libm loop, and expected_topn on hand-worked cases."""
import ctypes
import ctypes.util

import numpy as np
import pytest

from rec_exact import PAD, chain_scores, eligible_mask, expected_topn, fmaf32

F32 = np.float32
INF = np.inf


@pytest.fixture(scope="module")
def libm_fmaf():
    name = ctypes.util.find_library("m")
    assert name, "libm not found"
    f = ctypes.CDLL(name).fmaf
    f.restype = ctypes.c_float
    f.argtypes = [ctypes.c_float] * 3
    return lambda a, b, c: np.array([f(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], F32)


def same_bits(x, y):
    """Bitwise equal, except that any NaN equals any NaN (payloads are not part of the contract)."""
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    return (x.view(np.uint32) == y.view(np.uint32)) | (np.isnan(x) & np.isnan(y))


def check_against_libm(libm_fmaf, a, b, c):
    a, b, c = (np.ascontiguousarray(v, F32) for v in (a, b, c))
    got, want = fmaf32(a, b, c), libm_fmaf(a, b, c)
    bad = ~same_bits(got, want)
    assert not bad.any(), [(a[i], b[i], c[i], got[i], want[i]) for i in np.nonzero(bad)[0][:5]]


def wide(rng, n, lo, hi):
    with np.errstate(over="ignore"):
        return (rng.standard_normal(n) * 2.0 ** rng.integers(lo, hi, n)).astype(F32)


def test_fmaf32_random_wide_exponents(libm_fmaf):
    rng = np.random.default_rng(1)
    n = 60000
    a, b, c = wide(rng, n, -150, 128), wide(rng, n, -150, 128), wide(rng, n, -150, 128)
    # half the addends of the product's own size, so that the sum cancels and rounds in every way
    with np.errstate(over="ignore"):
        c[::2] = (a[::2].astype(np.float64) * b[::2] * rng.uniform(-2, 2, n // 2)).astype(F32)
    check_against_libm(libm_fmaf, a, b, c)


def midpoint_cases():
    """c on the fp32 grid, p = a*b = +-(1 - 2^-46) 2^E with 2^(E+1) the ulp of c: c + p lies just inside an fp32
    midpoint, so fp64 rounds the sum onto the midpoint and a second rounding to fp32 would go the wrong way half of
    the time.  Normal, subnormal and overflow-threshold grids, both signs, both mantissa parities."""
    a, b, c = [], [], []
    fmax = np.finfo(F32).max
    grid = [F32(2.0 ** 24), F32(2.0 ** 24 + 2), F32(1.5), F32(1.75), F32(3.0 * 2.0 ** -100), F32(2.0 ** -126),
            F32(5 * 2.0 ** -149), F32(1234567 * 2.0 ** -149), F32(2.0 ** -149), fmax, np.nextafter(fmax, F32(0)),
            F32(0.0)]
    for g in grid:
        for sc in (1, -1):
            cv = F32(sc * g)
            ulp = 2.0 ** 104 if g == fmax else np.float64(np.spacing(np.abs(cv)))  # spacing above |c|
            E = int(np.log2(ulp)) - 1
            ia = E // 2
            for sp in (1, -1):
                a.append(F32((1 + 2.0 ** -23) * 2.0 ** ia))
                b.append(F32(sp * (1 - 2.0 ** -23) * 2.0 ** (E - ia)))
                c.append(cv)
    return np.array(a, F32), np.array(b, F32), np.array(c, F32)


def test_fmaf32_constructed_midpoints(libm_fmaf):
    a, b, c = midpoint_cases()
    check_against_libm(libm_fmaf, a, b, c)
    # the cases are real: rounding p + c in fp64 and then to fp32 gets some of them wrong
    with np.errstate(over="ignore"):
        naive = (a.astype(np.float64) * b + c).astype(F32)
    assert (~same_bits(naive, libm_fmaf(a, b, c))).sum() >= 4


def test_fmaf32_subnormal_range(libm_fmaf):
    rng = np.random.default_rng(2)
    n = 40000
    ea = rng.integers(-149, -40, n)
    a = (rng.standard_normal(n) * 2.0 ** ea).astype(F32)                      # subnormal and tiny normal factors
    b = (rng.standard_normal(n) * 2.0 ** (-140 - ea + rng.integers(-20, 12, n))).astype(F32)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-160, -120, n)).astype(F32)
    c[::3] = 0.0
    c[1::3] = -0.0
    check_against_libm(libm_fmaf, a, b, c)
    got = fmaf32(a, b, c)
    assert (np.abs(got[got != 0]) < np.finfo(F32).tiny).sum() > n // 10     # many results are subnormal
    assert (np.signbit(got) & (got == 0)).any() and (~np.signbit(got) & (got == 0)).any()  # -0 and +0 both occur


def test_fmaf32_overflow_inf_nan(libm_fmaf):
    rng = np.random.default_rng(3)
    n = 20000
    a = (rng.uniform(0.5, 2, n) * 2.0 ** rng.integers(60, 66, n) * rng.choice([-1, 1], n)).astype(F32)
    b = (rng.uniform(0.5, 2, n) * 2.0 ** rng.integers(60, 66, n) * rng.choice([-1, 1], n)).astype(F32)
    with np.errstate(over="ignore"):
        c = (-(a.astype(np.float64) * b) * rng.uniform(0, 2, n)).astype(F32)
    c[::5] = np.where(rng.random(len(c[::5])) < 0.5, INF, -INF)
    fmax = np.finfo(F32).max
    special = np.array([
        (F32(1e20), F32(1e20), F32(0)), (F32(1e20), F32(-1e20), F32(0)), (F32(1e20), F32(1e20), F32(-INF)),
        (F32(INF), F32(1), F32(-INF)), (F32(INF), F32(0), F32(1)), (F32(np.nan), F32(1), F32(1)),
        (F32(1), F32(1), F32(np.nan)), (fmax, F32(1), fmax), (fmax, F32(-1), -fmax), (F32(-INF), F32(-1), F32(INF)),
        (fmax, F32(1 + 2.0 ** -23), F32(0)), (F32(2.0 ** 64), F32(2.0 ** 64), -fmax),
    ], F32)
    a, b, c = (np.concatenate([x, special[:, i]]) for i, x in enumerate((a, b, c)))
    check_against_libm(libm_fmaf, a, b, c)
    got = fmaf32(a, b, c)
    assert np.isinf(got).sum() > 100 and np.isnan(got).sum() >= 4


@pytest.mark.parametrize("k", [1, 2, 3])
def test_chain_scores_is_the_scalar_fmaf_loop(libm_fmaf, k):
    rng = np.random.default_rng(10 + k)
    rows, cols = 7, 41
    W = wide(rng, rows * k, -70, 60).reshape(rows, k)
    H = wide(rng, cols * k, -70, 60).reshape(cols, k)
    H[3] = 0.0
    W[2] = (rng.standard_normal(k) * 2.0 ** -140).astype(F32)                  # scores that underflow to +-0
    users = np.array([0, 2, 5, 2, 6])
    S = chain_scores(W, H, users, chunk_elems=64)                               # several chunks
    for s, u in enumerate(users):
        acc = np.zeros(cols, F32)
        for t in range(k):
            acc = libm_fmaf(np.full(cols, W[u, t], F32), H[:, t], acc)
        assert same_bits(S[s], acc).all(), (u, S[s], acc)


# ------------------------------------------------------------------------------------------------ expected_topn
def topn(S, n_top, elig=True):
    S = np.array(S, F32)
    return expected_topn(S, np.broadcast_to(np.asarray(elig, bool), S.shape), n_top)


def test_expected_topn_ties_across_nth():
    items, scores = topn([[1.0, 3.0, 2.0, 3.0, 2.0, 2.0, 0.5]], 4)
    assert items.tolist() == [[1, 3, 2, 4]]
    assert scores.tolist() == [[3.0, 3.0, 2.0, 2.0]]
    items, _ = topn([[-0.0, 0.0, -0.0, 1.0]], 3)                               # -0 == +0: item order decides
    assert items.tolist() == [[3, 0, 1]]


def test_expected_topn_inf_nan():
    S = [[-INF, np.nan, INF, 0.0, -INF, np.nan, 5.0]]
    items, scores = topn(S, 7)
    assert items.tolist() == [[2, 6, 3, 0, 4, PAD, PAD]]
    assert scores.tolist()[0][:5] == [INF, 5.0, 0.0, -INF, -INF] and np.isneginf(scores[0, 5:]).all()
    items, _ = topn(S, 4)
    assert items.tolist() == [[2, 6, 3, 0]]


def test_expected_topn_exclusion_and_padding():
    from mfx import dataset as ds
    rows, cols = 4, 6
    # user 0: every item; user 1: nothing; user 2: duplicates (2, 2, 5, 5, 5); user 3: one item
    r = [0] * cols + [2] * 5 + [3]
    c = list(range(cols)) + [2, 2, 5, 5, 5] + [1]
    d = ds.from_coo(rows, cols, np.array(r, np.uint32), np.array(c, np.uint32), np.ones(len(r), F32))
    S = np.array([[6, 5, 4, 3, 2, 1]] * rows, F32)
    el = eligible_mask(d, np.arange(rows), cols)
    assert el.sum(axis=1).tolist() == [0, 6, 4, 5]
    items, scores = expected_topn(S, el, 8)                                     # n_top > cols
    assert (items[0] == PAD).all() and np.isneginf(scores[0]).all()
    assert items[1].tolist() == [0, 1, 2, 3, 4, 5, PAD, PAD]
    assert items[2].tolist() == [0, 1, 3, 4] + [PAD] * 4
    assert items[3].tolist() == [0, 2, 3, 4, 5] + [PAD] * 3
    assert scores[3].tolist()[:5] == [6, 4, 3, 2, 1] and np.isneginf(scores[3, 5:]).all()
    items, _ = expected_topn(S[[2, 2]], el[[2, 2]], 2)
    assert items.tolist() == [[0, 1], [0, 1]]
