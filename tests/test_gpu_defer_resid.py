"""Deferred residual writes (CcdSolver::rank_pair, the default on LDS panels at T = 1): ranks t, t + 1 of an outer
iteration stream each residual copy once read-only and once with a store, instead of storing twice.  Rank t + 1's pass
redoes rank t's update in registers, so every factor, every stored residual and the test RMSE must be BIT-identical to
today's schedule (MFX_DEFER_RESID=0), whatever k, the number of outer iterations, graph replay or profiling -- and the
configurations it does not cover (T > 1, eps) must still run today's launches."""
import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1, "no HIP device: these tests must run on the GPU box"
    return m


@pytest.fixture(scope="module")
def data(mfx):
    # ML-1M sized, with empty rows / columns; forced panels give both copies several LDS panels
    return mfx.dataset.synth_ratings(6040, 3706, 1_000_000, seed=11, skew=0.9, test_frac=0.01,
                                     empty_row_frac=0.01, empty_col_frac=0.02)


@pytest.fixture(autouse=True)
def _no_owner_passes(monkeypatch):
    monkeypatch.setenv("MFX_OWNER_PASSES", "0")  # (small matrices take the segment-owner passes otherwise)
    monkeypatch.delenv("MFX_FUSE_FINALIZE", raising=False)


def _params(mfx, k, T, panel_rows, graph=0, profile=0, eps=0.0):
    p = mfx.parameter()
    p.k, p.lambda_, p.maxiter, p.maxinneriter = k, 0.05, 3, T
    p.schedule, p.kernel_variant, p.panel_rows, p.graph, p.profile = 1, 1, panel_rows, graph, profile
    if eps > 0:
        p.libpmf_flags, p.eps = 1, eps
    return p


def _run(mfx, d, monkeypatch, defer, p, calls):
    """iterate(n) for n in calls; after each call: W, H, both residual orders, the test RMSEs; plus the launch counts"""
    monkeypatch.setenv("MFX_DEFER_RESID", "1" if defer else "0")
    s = mfx.CcdSolver(d, mfx.test_data_of(d), p)
    try:
        lay = s.layout_info()
        s.set_factors(mfx.initial_col(p.k, d.rows))
        snaps = []
        for n in calls:
            rep = s.iterate(n)
            W, H = s.get_factors()
            csc, csr = s.get_residual(d.nnz)
            snaps.append((W, H, csc, csr, np.array([r.rmse for r in rep])))
        launches = {name: int(c) for name, (_, c) in s.kernel_times().items()}
    finally:
        s.close()
    return lay, snaps, launches


def _same(a, b):
    assert len(a) == len(b)
    for sa, sb in zip(a, b):
        for x, y in zip(sa, sb):
            assert x.shape == y.shape
            assert np.array_equal(bits(x), bits(y))


@pytest.mark.parametrize("panel_rows", [512, 1500])
@pytest.mark.parametrize("graph", [0, -1])
@pytest.mark.parametrize("k", [1, 4, 7])
def test_deferred_writes_are_bit_identical(mfx, data, monkeypatch, panel_rows, graph, k):
    """k even / odd / 1; 1 then 2 more outer iterations with the residual read in between (flush_pending), and 3 in one
    call (the capture and replays of the hipGraph with graph = 0)"""
    for calls in ((1, 2), (3,)):
        lay, on, _ = _run(mfx, data, monkeypatch, True, _params(mfx, k, 1, panel_rows, graph), calls)
        assert lay["csc"]["kind"] == "lds" and lay["csr"]["kind"] == "lds"
        assert lay["csc"]["panels"] > 2 and lay["csr"]["panels"] > 2
        _, off, _ = _run(mfx, data, monkeypatch, False, _params(mfx, k, 1, panel_rows, graph), calls)
        _same(on, off)


@pytest.mark.parametrize("k", [2, 5])
def test_deferred_writes_under_profiling(mfx, data, monkeypatch, k):
    """profiled launches: the pair's read-only passes are booked as ccd_flat_sweep, its catch-up passes as the fused ones"""
    _, on, lon = _run(mfx, data, monkeypatch, True, _params(mfx, k, 1, 700, profile=1), (2,))
    _, off, loff = _run(mfx, data, monkeypatch, False, _params(mfx, k, 1, 700, profile=1), (2,))
    _same(on, off)
    pairs = k // 2
    assert lon.get("ccd_flat_sweep", 0) == 2 * 2 * pairs
    assert lon["ccd_fused_csc_pass"] == lon["ccd_fused_csr_pass"] == 2 * (k - pairs)
    assert lon["ccd_finalize"] == loff["ccd_finalize"] == 2 * 2 * k
    assert "ccd_flat_sweep" not in loff and loff["ccd_fused_csc_pass"] == 2 * k


@pytest.mark.parametrize("T,eps", [(2, 0.0), (1, 1e-3)])
def test_uncovered_configurations_keep_todays_launches(mfx, data, monkeypatch, T, eps):
    """T > 1 and the eps rule are not paired: the same launches, and the same bits, with the knob on or off"""
    _, on, lon = _run(mfx, data, monkeypatch, True, _params(mfx, 4, T, 700, profile=1, eps=eps), (2,))
    _, off, loff = _run(mfx, data, monkeypatch, False, _params(mfx, 4, T, 700, profile=1, eps=eps), (2,))
    _same(on, off)
    lon.pop("host_enqueue_outer_iteration", None)
    loff.pop("host_enqueue_outer_iteration", None)
    assert lon == loff
