"""Host checks of the per-rank solve sweep (tests/solve_sweep.py), for every rank 1..131, both size sets and every family
parameter: what tests/test_gpu_solve_sweep.py asserts on the GPU is (1) aimed at every kernel class, (2) asserted on every
segment, (3) reachable by an honest fp32 solver and (4) out of reach for a solver that loses one entry or exchanges two
coordinates.

Measured here (maxima / minima over ranks 1..131, both sets and all segments; printed as `sweep-host` lines), for
explicit lambda / explicit lambda n / implicit alpha 0 / 1 / 40:
    largest condition number                                49.4 / 17.8 / 1.7 / 2.0 / 12.0         (gate: 1e3)
    fp32 control, backward error                            5.2e-07 / 2.2e-06 / 8.3e-07 / 9.7e-07 / 4.1e-06  (bound: 3e-5)
    fp32 control, relative error                            1.4e-06 / 4.3e-06 / 1.7e-06 / 2.0e-06 / 8.1e-06  (bound: 1e-3)
    drop_one, smallest backward error                       1.96e-04 / 2.98e-04 / 1.80e-03 / 1.29e-03 / 3.26e-04  (required: >= 4 x 3e-5)
    swap_last_two, smallest backward error                  5.7e-05 / 5.7e-05 / 6.6e-04 / 8.9e-04 / 2.8e-04  (required: > 3e-5)
drop_one keeps the segment's true count on the diagonal at lambda n, as a kernel that loses an entry from its sums would.
"""
import numpy as np
import pytest

import alsb_ref
import ials_ref
import ialsb_ref
import solve_sweep as sw

FAMILIES = sw.EXPLICIT + sw.IMPLICIT
HOST_RANGES = sw.RANGES + [(129, 131)]  # 129..131: the ranks of the two-block steps d + 3
DROP_FACTOR = 4


def _id(v):
    return "%s-%g" % v if isinstance(v[0], str) else "%d-%d" % v


# ------------------------------------------------------------------------------------------------ 0. the helper itself
def test_size_sets_and_dispatch_constants():
    assert sw.dispatch_constants() == (2048, 1024)
    assert (len(sw.S), sum(sw.S), sw.work_items(sw.S), sum(sw.S) // sw.work_items(sw.S)) == (14, 10579, 17, 622)
    assert (len(sw.L), sum(sw.L), sw.work_items(sw.L), sum(sw.L) // sw.work_items(sw.L)) == (5, 16385, 10, 1638)
    assert sorted(-(-n // 2048) for n in sw.S if sw.is_split(n)) == [2, 3]
    assert sorted(-(-n // 2048) for n in sw.L if sw.is_split(n)) == [2, 2, 4]


def test_segments_are_distinct_sorted_rows_with_explicit_zeros():
    for name, sizes in sw.SETS.items():
        ptr, idx, val, X = sw.data(37, name)
        assert X.shape == (sw.NROWS, 37) and X.dtype == np.float32 and list(np.diff(ptr.astype(np.int64))) == sizes
        for s in range(len(sizes)):
            seg = idx[int(ptr[s]):int(ptr[s + 1])].astype(np.int64)
            assert np.all(np.diff(seg) > 0) and (seg.size == 0 or seg[-1] < sw.NROWS)
        assert set(np.unique(val)) == {0.0, 1.0, 2.0, 3.0, 4.0, 5.0}


@pytest.mark.parametrize("k", [1, 37, 64, 131])
def test_implicit_systems_are_the_dense_systems(k):
    """solve_sweep forms A with X^T X built once per k: the same system as ials_ref.dense_system over all rows of X."""
    for name in sw.SETS:
        ptr, idx, val, X = sw.data(k, name)
        for fam in sw.IMPLICIT:
            for s, ref in enumerate(sw.systems(k, name, fam)):
                if ref is None or s % 3:
                    continue
                A, b = ials_ref.dense_system(ptr, idx, val, s, X, sw.LAM, fam[1])
                assert np.linalg.norm(ref[0] - A) <= 1e-12 * np.linalg.norm(A) and np.linalg.norm(ref[1] - b) <= 1e-12 * max(np.linalg.norm(b), 1.0)


# ------------------------------------------------------------------------------------------------ 1. every class is reached
def test_every_class_is_reached_split_and_unsplit():
    seen = {}
    for k in range(1, 129):
        for name, sizes in sw.SETS.items():
            seen.setdefault(sw.launch_class(k, sizes), set()).add(name)
            assert any(sw.is_split(n) for n in sizes) and any(0 < n and not sw.is_split(n) for n in sizes)
    assert set(seen) == set(sw.CLASSES), seen
    for c in ("N1", "N2", "N3", "N4"):
        assert seen[c] == {"S", "L"}, (c, seen[c])
    assert seen["G16 short"] == seen["G16 short-64"] == {"S"} and seen["G16 long"] == seen["G16 long-64"] == {"L"}
    # the classes by rank, as the table of the dispatcher states them
    assert {k for k in range(1, 129) if sw.launch_class(k, sw.S) == "N2"} == {k for k in range(33, 64) if k % 4}
    assert {k for k in range(1, 129) if sw.launch_class(k, sw.L) == "G16 long"} == set(range(36, 64, 4))
    assert [sw.launch_class(k, sw.S) for k in (32, 33, 64, 65, 96, 97, 128)] == ["N1", "N2", "G16 short-64", "N3", "N3", "N4", "N4"]
    # the second block of a two-block step d + 3 is 3 wide: N1
    assert sw.launch_class(3, sw.S) == sw.launch_class(3, sw.L) == "N1"


# ------------------------------------------------------------------------------------------------ 2 - 4. gate and controls
@pytest.mark.parametrize("ranks", HOST_RANGES, ids=_id)
@pytest.mark.parametrize("family", FAMILIES, ids=_id)
def test_gate_and_controls(family, ranks):
    worst_cond, ctl, drop_min, swap_min, swapped = 0.0, sw.Worst(), (np.inf, None), (np.inf, None), 0
    for k in range(ranks[0], ranks[1] + 1):
        for name, sizes in sw.SETS.items():
            refs = sw.systems(k, name, family)
            # 2. the project's gate holds for ALL segments: the cap on skipped segments is zero
            for s, ref in enumerate(refs):
                assert (ref is None) == (sizes[s] == 0)
                if ref is not None:
                    assert ref[3] <= sw.MAX_COND, (family, k, name, s, ref[3])
                    worst_cond = max(worst_cond, ref[3])
            # 3. the bounds are reachable in fp32
            errors = sw.segment_errors(sw.fp32_solve(k, name, family), k, name, family)
            assert not sw.check_bounds(errors, ("fp32 control", family, k, name))
            ctl.add(k, name, errors)
            # 4. the bounds cannot hide a lost entry or two exchanged coordinates
            for s, ref in enumerate(refs):
                if ref is None:
                    continue
                A, b, y, _ = ref
                lost = sw.drop_one(k, name, family, s)
                assert (lost is None) == (sizes[s] < 2 or sw.rhs_is_zero(k, name, s)), (family, k, name, s)
                if lost is not None:
                    be = ials_ref.backward_error(A, lost, b)
                    assert be >= DROP_FACTOR * sw.MAX_BACKWARD, (family, k, name, s, sizes[s], be)
                    drop_min = min(drop_min, (be, (k, name, s)))
                if k >= 2 and abs(y[-1] - y[-2]) > 1e-3 * np.linalg.norm(y):
                    be = ials_ref.backward_error(A, sw.swap_last_two(y), b)
                    assert be > sw.MAX_BACKWARD, (family, k, name, s, sizes[s], be)
                    swap_min, swapped = min(swap_min, (be, (k, name, s))), swapped + 1
    print(f"sweep-host {_id(family)} ranks {ranks[0]}..{ranks[1]} worst_cond={worst_cond:.1f} "
          f"fp32_control max_backward={ctl.backward[0]:.3e} {ctl.backward[1]} max_rel={ctl.rel[0]:.3e} {ctl.rel[1]} "
          f"drop_one min_backward={drop_min[0]:.3e} {drop_min[1]} swap_last_two min_backward={swap_min[0]:.3e} {swap_min[1]} "
          f"({swapped} segments)")
    assert swapped > 0


# ------------------------------------------------------------------------------------------------ 5. block-sweep references
@pytest.mark.parametrize("ranks", sw.RANGES, ids=_id)
def test_two_block_references(ranks):
    """The fp64 references of the two-block steps (k = d + 3 in blocks of d, from Y0): every row is finite and away from
    zero, so that a relative error against it is defined, and a sweep never increases the segment's objective."""
    for d in range(ranks[0], ranks[1] + 1):
        k = d + 3
        for name, sizes in sw.SETS.items():
            ptr, idx, val, X = sw.data(k, name)
            Y0 = sw.start(k, name)
            sweeps = [(("explicit", reg), alsb_ref.block_sweep(ptr, idx, val, X, Y0, sw.LAM, d, reg)) for reg in (0, 1)]
            sweeps += [(("implicit", a), ialsb_ref.block_sweep(ptr, idx, val, X, Y0, sw.LAM, a, d)) for a in (1.0, 40.0)]
            for fam, Yr in sweeps:
                assert np.all(np.isfinite(Yr)), (fam, d, name)
                for s, ref in enumerate(sw.systems(k, name, fam)):
                    if ref is None:
                        assert not np.any(Yr[s])
                        continue
                    A, b, y, _ = ref
                    f = lambda v: float(v @ A @ v - 2.0 * (b @ v))  # the segment's objective up to a constant
                    y0 = Y0[s].astype(np.float64)
                    assert np.linalg.norm(Yr[s]) >= 1e-3 * np.linalg.norm(y0), (fam, d, name, s)
                    assert f(y) - 1e-9 * abs(f(y)) <= f(Yr[s]) <= f(y0) + 1e-9 * abs(f(y0)), (fam, d, name, s)
