"""Every CCD++ schedule the solver can choose (the table of schedules), one case per row: WHICH kernels an
outer iteration launches and how often, as a closed form in k, T and the number of outer iterations, and that the same work is
enqueued with and without profiling (for the graph-capturable schedules: eagerly and under hipGraph capture / replay).

Each case runs k = 3 (one rank pair plus a single rank where ranks are paired) with T = 1 and T = 2, profiled, as iterate(1),
a read of the residual (which applies the pending subtraction: flush_pending), iterate(2) and a second read; the launch
counts of kernel_times() must equal the case's closed form.  A second solver without profiling and with graph = 0 runs the same
three iterations in one call and must end with the same bits in W, H, both residual copies and the RMSE trace.

The closed forms are read off the launch sequences of the host code and say nothing about the arithmetic; the bits of every
schedule against the oracle are test_gpu_ccd_exact.py's and test_gpu_ccd_reforder.py's business.

The matrix is 600 x 400, so no segment can reach 4096 entries; the reference-order owner case that sets MFX_REF_LONG sets it to
64 instead, which puts the longest segments of both sides on the split kernel and its second stream just the same."""
import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

K = 3
CALLS = (1, 2)       # outer iterations per iterate() call of the profiled solver; the residual is read after each call
N = sum(CALLS)
FLUSHES = len(CALLS)  # reads of the residual that find a subtraction pending (fused schedules: after every call)
REF_LONG = 64

KNOBS = ("MFX_FUSE_FINALIZE", "MFX_SCATTER_WGS", "MFX_SLICE_KB", "MFX_EQUAL_PANELS", "MFX_OVERLAP_GROUPS", "MFX_COMM_RESERVE_CUS",
         "MFX_OWNER_PASSES", "MFX_REF_FUSED", "MFX_DEFER_RESID", "MFX_FLAT_PERSIST", "MFX_FLAT_WGS", "MFX_SCATTER_PANEL_MULT",
         "MFX_REF_QUAD_TAB", "MFX_REF_QUAD_TAB_BYTES", "MFX_REF_QUAD_WGS", "MFX_REF_LONG", "MFX_REF_SWEEP_DPP", "MFX_OWNER_LONG")


def _packs(T):
    """operand packs: re-primed after every rank when T > 1, and by every flush"""
    return 2 * K * N * (T > 1) + 2 * FLUSHES


def flat(T):
    """launch_flat + finalize per half-step; T - 1 read-only sweep pairs, each sweep with its finalize"""
    return {"ccd_fused_csc_pass": K * N, "ccd_fused_csr_pass": K * N, "ccd_finalize": 2 * K * N * T,
            "ccd_flat_sweep": 2 * K * N * (T - 1), "ccd_pack": _packs(T), "ccd_flat_resid": 2 * FLUSHES}


def flat_fused_plain(T):
    """in-pass finalize on the plain layout: no finalize launch at all, the read-only sweeps included"""
    return {"ccd_fused_csc_pass": K * N, "ccd_fused_csr_pass": K * N, "ccd_flat_sweep": 2 * K * N * (T - 1),
            "ccd_pack": _packs(T), "ccd_flat_resid": 2 * FLUSHES}


def flat_fused_panels(T):
    """in-pass finalize on LDS panels: the first half-steps only; the read-only sweeps keep the separate finalize"""
    return dict(flat_fused_plain(T), ccd_finalize=2 * K * N * (T - 1))


def flat_pairs(T):
    """T = 1: ranks (0, 1) as a pair -- two read-only passes booked as sweeps, two catch-up passes booked as the fused passes, a
    finalize behind each -- and rank 2 as a single flat rank.  T > 1 is not paired: the flat schedule."""
    if T > 1:
        return flat(T)
    pairs = K // 2
    return {"ccd_flat_sweep": 2 * pairs * N, "ccd_fused_csc_pass": (K - pairs) * N, "ccd_fused_csr_pass": (K - pairs) * N,
            "ccd_finalize": 2 * K * N, "ccd_pack": _packs(T), "ccd_flat_resid": 2 * FLUSHES}


def owner(T):
    """one launch per half-step and per read-only sweep: the owners finalize in the pass"""
    return {"ccd_fused_csc_pass": K * N, "ccd_fused_csr_pass": K * N, "ccd_flat_sweep": 2 * K * N * (T - 1),
            "ccd_pack": _packs(T), "ccd_flat_resid": 2 * FLUSHES}


def scatter(T):
    """scatter pass + one finalize from its slabs, per half-step and per read-only sweep"""
    return {"ccd_scatter_v_pass": K * N, "ccd_scatter_u_pass": K * N, "ccd_finalize": 2 * K * N * T,
            "ccd_scatter_sweep": 2 * K * N * (T - 1), "ccd_pack": _packs(T), "ccd_scatter_resid": 2 * FLUSHES}


def scatter_groups(T, G=2):
    """sharded, the column pass by G panel groups: G column launches per rank; every column-side finalize (first half-step
    and read-only sweeps) is combine -> all-reduce -> finalize per group, the row side one finalize; the RMSE is all-reduced"""
    return {"ccd_scatter_v_pass": G * K * N, "ccd_scatter_u_pass": K * N, "ccd_scatter_combine": G * K * N * T,
            "rccl_allreduce": G * K * N * T + N, "ccd_finalize": (G + 1) * K * N * T, "ccd_scatter_sweep": 2 * K * N * (T - 1),
            "ccd_pack": _packs(T), "ccd_scatter_resid": 2 * FLUSHES}


def as_written(T, wave):
    """the reference's sequence: add-back (not in the first outer iteration), T x (sweep + finalize, sweep + finalize), subtraction;
    nothing stays pending, so the reads of the residual launch nothing"""
    sweep, resid = ("ccd_wave_sweep", "ccd_wave_resid") if wave else ("ccd_flat_sweep", "ccd_flat_resid")
    return {sweep: 2 * K * N * T, "ccd_finalize": 2 * K * N * T, resid: 2 * K * (N - 1) + 2 * K * N}


def ref_as_written(T):
    """reference-order sweeps (sums and division in one kernel); the subtraction of a rank stays pending and is merged with the
    next rank's add-back into one pass per copy (two packs feed it), applied alone where there is no add-back (first outer
    iteration) or by a read of the residual; after such a read the next rank's add-back runs alone.  The flush primes no packs."""
    merged = K * (N - 1) - (FLUSHES - 1)  # ranks of iterations 2 .. N that find a subtraction pending
    return {"ccd_ref_order_sweep": 2 * K * N * T, "ccd_pack": 2 * merged,
            "ccd_flat_resid": 2 * (K - 1) + 2 * K * (N - 1) + 2 * FLUSHES}


def ref_owner(T):
    """two owner launches per rank, two per read-only sweep pair; in the first outer iteration every rank re-packs the column
    operands with a zero add-back term (one pack)"""
    return {"ccd_ref_order_sweep": 2 * K * N * T, "ccd_pack": K + _packs(T), "ccd_flat_resid": 2 * FLUSHES}


OFF = {"MFX_OWNER_PASSES": "0", "MFX_DEFER_RESID": "0"}
# id, (schedule, kernel_variant, panel_rows), environment, sharded, closed form of the launch counts
CASES = [
    ("flat_plain", (1, 1, 0), OFF, False, flat),
    ("flat_panels", (1, 1, 64), OFF, False, flat),
    ("flat_fused_plain", (1, 1, 0), dict(OFF, MFX_FUSE_FINALIZE="1"), False, flat_fused_plain),
    ("flat_fused_panels", (1, 1, 64), dict(OFF, MFX_FUSE_FINALIZE="1"), False, flat_fused_panels),
    ("flat_pairs", (1, 1, 64), {"MFX_OWNER_PASSES": "0"}, False, flat_pairs),
    ("owner", (1, 1, 0), {}, False, owner),
    ("scatter", (1, 2, 0), {}, False, scatter),
    ("scatter_groups", (1, 2, 64), {"MFX_OVERLAP_GROUPS": "2"}, True, scatter_groups),
    ("as_written_wave", (0, 0, 0), {}, False, lambda T: as_written(T, True)),
    ("as_written_flat", (0, 1, 0), {}, False, lambda T: as_written(T, False)),
    ("ref_as_written", (0, -1, 0), {"MFX_REF_FUSED": "0"}, False, ref_as_written),
    ("ref_owner", (0, -1, 0), {}, False, ref_owner),
    ("ref_owner_split", (0, -1, 0), {"MFX_REF_LONG": str(REF_LONG)}, False, ref_owner),
]


def make_data(mfx, rows=600, cols=400, nnz=20_000):
    return mfx.dataset.synth_ratings(rows, cols, nnz, seed=47, skew=0.9, test_frac=0.01, empty_row_frac=0.01, empty_col_frac=0.02)


def set_env(setenv, delenv, env):
    for name in KNOBS:
        delenv(name)
    for name, value in env.items():
        setenv(name, value)


_group = [5200]


def solve(mfx, d, case, k, T, profile, calls):
    """One solver of `case`: iterate(n) for n in calls, the residual read after each.  Returns the final W, H, both residual
    copies, the RMSE of every outer iteration, and the launch counts (empty without profiling)."""
    _, (schedule, variant, panel_rows), _, sharded, _ = case
    p = mfx.parameter()
    p.k, p.lambda_, p.maxiter, p.maxinneriter = k, 0.05, sum(calls), T
    p.schedule, p.kernel_variant, p.panel_rows, p.graph, p.profile = schedule, variant, panel_rows, 0, profile
    comm = cnt = None
    if sharded:
        _group[0] += 1
        comm = mfx.Comm(None, 0, 1, 0, local_group=_group[0])
        cnt = np.ascontiguousarray(np.diff(d.csc_col_ptr.astype(np.int64)).astype(np.uint32))
    s = mfx.CcdSolver(d, mfx.test_data_of(d), p, comm=comm, global_col_nnz=cnt, global_test_nnz=d.nnz_test)
    try:
        s.set_factors(mfx.initial_col(k, d.rows))
        rmse = []
        for n in calls:
            rmse += [r.rmse for r in s.iterate(n)]
            csc, csr = s.get_residual(d.nnz)
        W, H = s.get_factors()
        launches = {name: int(c) for name, (_, c) in s.kernel_times().items()}
    finally:
        s.close()
        if comm:
            comm.close()
    return (W, H, csc, csr, np.array(rmse)), launches


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1, "no HIP device: these tests must run on the GPU box"
    return m


@pytest.fixture(scope="module")
def data(mfx):
    d = make_data(mfx)
    lens_c, lens_r = np.diff(d.csc_col_ptr.astype(np.int64)), np.diff(d.csr_row_ptr.astype(np.int64))
    assert (lens_c == 0).any() and (lens_r == 0).any()
    assert lens_c.max() >= REF_LONG and lens_r.max() >= REF_LONG and d.nnz_test > 0
    return d


@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_schedule_launches_and_replay(mfx, data, monkeypatch, case, T):
    set_env(monkeypatch.setenv, lambda n: monkeypatch.delenv(n, raising=False), case[2])
    profiled, launches = solve(mfx, data, case, K, T, 1, CALLS)
    launches.pop("host_enqueue_outer_iteration", None)
    want = {name: c for name, c in dict(case[4](T), test_rmse=N).items() if c}
    print(case[0], T, launches)
    assert launches == want
    plain, _ = solve(mfx, data, case, K, T, 0, (N,))
    for a, b in zip(profiled, plain):
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b))
