"""Every ALS solve kernel at every rank and block width from 1 to 128, against the fp64 references of tests/solve_sweep.py.

csrc/als_solver.hip is compiled once per kernel family; five of them are swept here (k_als_*, k_alsn_*, k_ials_*, k_ialsb_*,
k_alsb_*; test_gpu_ials_reg.py holds k_ialsr_* / k_ialsrb_* to k_ials_* / k_ialsb_* bit for bit).  In each family launch_half
picks one of eight kernel classes from the rank k (in a block step: the block width d) and the mean entries per work item,
and every class solves an unsplit segment in the gram kernel itself and a split one in its reducer:

    class         chosen when                            gram kernel           Cholesky / solves
    N1            k <= 32                                gram<1>               registers
    G16 short     32 < k < 64, k % 4 == 0, mean < 1024   gram16<4,2,false>     registers
    G16 long      32 < k < 64, k % 4 == 0, mean >= 1024  gram16<2,2,false>     registers
    G16 short-64  k = 64, mean < 1024                    gram16<4,2,true>      permuted image
    G16 long-64   k = 64, mean >= 1024                   gram16<2,2,true>      permuted image
    N2            32 < k < 64, k % 4 != 0                gram<2>               registers
    N3            64 < k <= 96                           gram<3>               chol_blocked<3>, 32-column solves
    N4            96 < k <= 128                          gram<4>               chol_blocked<4>, 32-column solves

Coverage of the solve (a launch whose result is compared with a reference that is not the kernel itself), read from the rank
and size lists of every ALS test; u = an unsplit segment, s = a split one (reducer), - = never.  BEFORE this module:

    class         k_als             k_alsn     k_ials     k_ialsb    k_alsb
    N1            u s               u s        u s        u s        u s        k = 1 .. 32; d = 2, 5, 16, 32
    G16 short     u s               u s        u s        -          -          k = 36, 40, 60 (k_alsn: 36); no such d
    G16 long      -                 -          -          -          -
    G16 short-64  u s               u s        u s        u s        u s        k = 64; d = 64
    G16 long-64   u s               -          u s        u s        u s        exact-sum tables / full size; d = 64, ten chunks
    N2            u (k = 36 only)   -          -          -          -          the 2^24-row gather table, three segments
    N3            - (k = 68 *)      -          u s        u s        u s        k = 68; d = 96
    N4            u s               u s        u s        u s        u s        k = 100, 128; d = 100, 128
    (*) als_half at k = 68 runs in test_fold_in_equals_the_single_operators, which compares it with fold-in bit for bit: the
    kernel against itself.  No rank or width above 32 that is not a multiple of 4 was solved anywhere but in that one N2
    launch; reduce<2> was never launched; as written (variant 0): k = 3, 8, 40, 64, 72, 100, 128 and the exact-sum ranks.
    The ranks seen by a half-sweep, fold-in or block step were 1, 3, 5, 8, 10, 16, 32, 36, 40, 60, 64, 68, 72, 100, 128, the
    block widths 5, 16, 32, 64, 96, 128 and the ragged last widths 2, 32, 100.

AFTER (this module; set S has mean 622 and splits in two and three, set L has mean 1 638 and splits in two and four):

    class         every family                                                   ranks / widths
    N1            u s                                                            1 .. 32, on S and on L
    G16 short     u s                                                            36, 40 .. 60 on S
    G16 long      u s                                                            36, 40 .. 60 on L
    G16 short-64  u s                                                            64 on S
    G16 long-64   u s                                                            64 on L
    N2            u s                                                            33 .. 63 except multiples of 4, on S and on L
    N3            u s                                                            65 .. 96, on S and on L
    N4            u s                                                            97 .. 128, on S and on L
    as written (variant 0): every rank 1 .. 128 on S, bit for bit against the oracle.

Bounds: the project's own (tests/test_gpu_ials.py, tests/test_gpu_alsb.py): backward error <= 3e-5 and relative error <= 1e-3
on EVERY non-empty segment; tests/test_solve_sweep_host.py shows that every condition number is within the gate of 1e3 (so
none is left out), that an honest fp32 solve stays under both, and that a lost entry or two exchanged coordinates do not.

Measured maxima over all ranks, both sets and all segments on the MI355X (`sweep-measured` / `sweep-detail` lines), at
(rank, set, segment), next to the fp32 control of the host test (numpy Cholesky in fp32 on the fp32 Gramian):
    family                         backward error            relative error             fp32 control
    k_als                          2.17e-06 (1, L, 1)        4.35e-06 (2, S, 10)        5.2e-07 / 1.4e-06
    as written (printed only)      2.11e-06 (2, S, 10)       4.34e-06 (2, S, 10)        (bit-equal to the oracle at every rank)
    k_alsn                         2.27e-06 (2, S, 10)       4.62e-06 (2, S, 10)        2.2e-06 / 4.3e-06
    k_ials alpha 0                 2.53e-06 (1, L, 0)        5.06e-06 (1, L, 0)         8.3e-07 / 1.7e-06
    k_ials alpha 1                 3.02e-06 (1, L, 0)        6.04e-06 (1, L, 0)         9.7e-07 / 2.0e-06
    k_ials alpha 40                4.99e-06 (2, S, 10)       1.02e-05 (2, S, 10)        4.1e-06 / 8.1e-06
    k_alsb one block               2.27e-06 (2, S, 10)       -                          as k_als / k_alsn
    k_alsb two blocks              -                         1.78e-04 (51, S, 1)
    k_ialsb one block              4.99e-06 (2, S, 10)       -                          as k_ials
    k_ialsb two blocks             -                         1.05e-04 (111, S, 1)
    All the maxima sit at ranks 1 and 2 (sums of up to 6145 squares of one sign in sequential fp32); from rank 17 on the
    backward error of every solve and every one-block step is below 1e-6.  No family is more than ten times its
    control (the largest ratio is 4.2, k_als).  The two-block maxima are one-entry segments, whose swept row is small next
    to its start Y0.

What the sweep found: a one-block step from Y0 missed the backward-error bound in k_ialsb at alpha = 1 with 5.7e-05 at
(1, L, 0) and 1.1e-04 at (2, S, 13), and was at 7e-06 .. 1e-05 at every other width against 7e-07 from zero.  A step forms
the residual of its start in fp32, so its error is relative to |Y0| (0.09 there, next to answers of 0.0016 and 0.0005), and
with one block the answer does not depend on the start at all.  A one-block sweep now starts from zero (ials_block.hip,
one_block_start); the test asserts that such a step returns the bits of the step from zero.
"""
import numpy as np
import pytest

import alsb_ref
import ialsb_ref
import solve_sweep as sw

pytestmark = pytest.mark.gpu

LAM = sw.LAM
FOLD_EQUAL_RANKS = [33, 37, 63, 65, 95, 96]  # N2 and N3 ranks the equality test of test_gpu_foldin.py lacks


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1
    return m


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _solved(w, Y, k, name, family, what, backward=True, rel=True, part=None):
    errors = sw.segment_errors(Y, k, name, family)
    w.add(k, name, errors, part)
    w.misses += sw.check_bounds(errors, what + (k, name), backward=backward, rel=rel)


# ------------------------------------------------------------------------------------------------ the families
def _als(mfx, orc, ranks, w):
    """k_als_*: als_half variant 1 against the dense solve"""
    for k in ranks:
        for name in sw.SETS:
            ptr, idx, val, X = sw.data(k, name)
            _solved(w, mfx.als_half(ptr, idx, val, X, k, LAM, variant=1), k, name, ("explicit", 0), ("als_half",))


def _as_written(mfx, orc, ranks, w):
    """als_half variant 0 against the oracle, bit for bit (its distance to the dense solve is printed only)"""
    for k in ranks:
        ptr, idx, val, X = sw.data(k, "S")
        Y = mfx.als_half(ptr, idx, val, X, k, LAM, variant=0)
        ref = orc.als_half(ptr, idx, val, X, k, LAM, orc.max_threads())
        bad = np.nonzero((bits(Y) != bits(ref)).any(axis=1))[0]
        assert bad.size == 0, ("as written", k, bad.tolist())
        w.add(k, "S", sw.segment_errors(Y, k, "S", ("explicit", 0)))


def _alsn(mfx, orc, ranks, w):
    """k_alsn_*: fold-in with MFX_FOLD_CCD against the dense solve with fp32(lambda) * fp32(n) on the diagonal"""
    for k in ranks:
        X = sw.table(k)
        with mfx.Recommender(np.zeros((1, k), np.float32), X, 1) as r:
            r.fold_in_setup(mfx.MFX_FOLD_CCD, LAM)
            for name in sw.SETS:
                ptr, idx, val, _ = sw.data(k, name)
                _solved(w, r.fold_in((ptr, idx, val))[2], k, name, ("explicit", 1), ("fold_in MFX_FOLD_CCD",))


def _ials(mfx, orc, ranks, w):
    """k_ials_*: ials_half at alpha 0, 1 and 40 against the dense system over all rows of X"""
    for k in ranks:
        for name in sw.SETS:
            ptr, idx, val, X = sw.data(k, name)
            for fam in sw.IMPLICIT:
                _solved(w, mfx.ials_half(ptr, idx, val, X, k, LAM, fam[1]), k, name, fam, ("ials_half", fam[1]), part="alpha %g" % fam[1])


def _block(step, reference, families, what):
    """One block at k = d (from zero and from Y0: backward error against the dense system), two blocks at k = d + 3 (from
    Y0: relative error against the fp64 block sweep; the second block is 3 wide)."""
    def run(mfx, orc, ranks, w):
        for d in ranks:
            for name in sw.SETS:
                ptr, idx, val, X = sw.data(d, name)
                Y0 = sw.start(d, name)
                for fam in families:
                    for Y_in in (None, Y0):
                        Y = step(mfx, ptr, idx, val, X, d, d, fam[1], Y_in)
                        if Y_in is None:
                            cold = Y
                        else:  # one block: the start is not read (include/mfx.h)
                            assert np.array_equal(bits(Y), bits(cold)), (what, "one block: the start shows", fam[1], d, name)
                        _solved(w, Y, d, name, fam, (what, "one block", fam[1], "zero" if Y_in is None else "Y0"), rel=False,
                                part="one block from " + ("zero" if Y_in is None else "Y0"))
                k = d + 3
                ptr, idx, val, X = sw.data(k, name)
                Y0 = sw.start(k, name)
                for fam in families:
                    Y = step(mfx, ptr, idx, val, X, k, d, fam[1], Y0)
                    errors = sw.sweep_errors(Y, reference(ptr, idx, val, X, Y0, d, fam[1]), name)
                    w.add(d, name, errors, "two blocks from Y0")
                    w.misses += sw.check_bounds(errors, (what, "two blocks", fam[1], d, name), backward=False)
    run.__doc__ = what
    return run


_alsb = _block(lambda mfx, ptr, idx, val, X, k, d, reg, Y_in: mfx.als_block_half(ptr, idx, val, X, k, LAM, d, Y_in=Y_in, count_reg=bool(reg)),
               lambda ptr, idx, val, X, Y0, d, reg: alsb_ref.block_sweep(ptr, idx, val, X, Y0, LAM, d, reg),
               sw.EXPLICIT, "als_block_half")
_ialsb = _block(lambda mfx, ptr, idx, val, X, k, d, alpha, Y_in: mfx.ials_block_half(ptr, idx, val, X, k, LAM, alpha, d, Y_in=Y_in),
                lambda ptr, idx, val, X, Y0, d, alpha: ialsb_ref.block_sweep(ptr, idx, val, X, Y0, LAM, alpha, d),
                sw.IMPLICIT[1:], "ials_block_half")

FAMILIES = {"k_als": _als, "as_written": _as_written, "k_alsn": _alsn, "k_ials": _ials, "k_alsb": _alsb, "k_ialsb": _ialsb}


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("ranks", sw.RANGES, ids=lambda r: "%d-%d" % r)
def test_solve_sweep(mfx, orc, ranks, family):
    w = sw.Worst()
    try:
        FAMILIES[family](mfx, orc, range(ranks[0], ranks[1] + 1), w)
    finally:
        print(w.line(family, *ranks))
    assert not w.misses, "\n".join(map(str, w.misses))


@pytest.mark.parametrize("k", FOLD_EQUAL_RANKS)
def test_fold_in_als_equals_als_half(mfx, k):
    X = sw.table(k)
    with mfx.Recommender(np.zeros((1, k), np.float32), X, 1) as r:
        r.fold_in_setup(mfx.MFX_FOLD_ALS, LAM)
        for name in sw.SETS:
            ptr, idx, val, _ = sw.data(k, name)
            got, want = r.fold_in((ptr, idx, val))[2], mfx.als_half(ptr, idx, val, X, k, LAM, variant=1)
            bad = np.nonzero((bits(got) != bits(want)).any(axis=1))[0]
            assert bad.size == 0, (k, name, bad.tolist())
