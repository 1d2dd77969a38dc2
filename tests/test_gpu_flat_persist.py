"""Persistent panel passes (k_flat's PERSIST form, the default for the catch-up passes of CcdSolver::rank_pair): a resident
workgroup walks a contiguous range of chunks and stages a panel's LDS slice once per panel it meets instead of once per
chunk.  Every span is still summed by one wave in the same order, so every factor, every stored residual and the test RMSE
must be BIT-identical to the one-chunk launches (MFX_FLAT_PERSIST=0), whatever the workgroup count (MFX_FLAT_WGS), k, the
workgroup size, graph replay or profiling -- and the configurations without paired ranks (T > 1, eps) must run the same
launches with the knob on or off."""
import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

# 1 .. 64: fewer workgroups than chunks, so ranges of several chunks that cross panel boundaries; the last one is more than
# there are chunks (the launcher falls back to one chunk per workgroup)
WGS = [1, 2, 3, 7, 64, 1_000_000]


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1, "no HIP device: these tests must run on the GPU box"
    return m


@pytest.fixture(scope="module")
def data(mfx):
    # the data set of test_gpu_defer_resid.py: ML-1M sized, with empty rows / columns
    return mfx.dataset.synth_ratings(6040, 3706, 1_000_000, seed=11, skew=0.9, test_frac=0.01,
                                     empty_row_frac=0.01, empty_col_frac=0.02)


@pytest.fixture(scope="module")
def reference():
    return {}  # one-chunk results by configuration: computed once, compared with every workgroup count


@pytest.fixture(autouse=True)
def _no_owner_passes(monkeypatch):
    monkeypatch.setenv("MFX_OWNER_PASSES", "0")  # (small matrices take the segment-owner passes otherwise)
    monkeypatch.delenv("MFX_FUSE_FINALIZE", raising=False)
    monkeypatch.delenv("MFX_DEFER_RESID", raising=False)


def _params(mfx, k, T, panel_rows, graph=0, profile=0, eps=0.0, wg_waves=0, tiles=0):
    p = mfx.parameter()
    p.k, p.lambda_, p.maxiter, p.maxinneriter = k, 0.05, 3, T
    p.schedule, p.kernel_variant, p.panel_rows, p.graph, p.profile = 1, 1, panel_rows, graph, profile
    p.wg_waves, p.tiles_per_span = wg_waves, tiles
    if eps > 0:
        p.libpmf_flags, p.eps = 1, eps
    return p


def _run(mfx, d, monkeypatch, wgs, p, calls):
    """wgs: None = MFX_FLAT_PERSIST=0, 0 = the default grid, n = MFX_FLAT_WGS=n.  iterate(n) for n in calls; after each call:
    W, H, both residual orders, the test RMSEs; plus the launch counts"""
    monkeypatch.delenv("MFX_FLAT_WGS", raising=False)
    monkeypatch.delenv("MFX_FLAT_PERSIST", raising=False)
    if wgs is None:
        monkeypatch.setenv("MFX_FLAT_PERSIST", "0")
    elif wgs:
        monkeypatch.setenv("MFX_FLAT_WGS", str(wgs))
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


def _reference(mfx, d, monkeypatch, reference, key, make_params, calls):
    if key not in reference:
        reference[key] = _run(mfx, d, monkeypatch, None, make_params(), calls)
    return reference[key]


@pytest.mark.parametrize("wgs", WGS)
@pytest.mark.parametrize("panel_rows", [512, 1500])
@pytest.mark.parametrize("graph", [0, -1])
@pytest.mark.parametrize("k", [1, 4, 7])
def test_persistent_passes_are_bit_identical(mfx, data, monkeypatch, reference, k, graph, panel_rows, wgs):
    """k even / odd / 1 (no pair at all); 1 then 2 more outer iterations with the residual read in between, and 3 in one call
    (capture and replays of the hipGraph with graph = 0); 1024-thread workgroups (wg_waves = 16), what the benchmark runs"""
    for calls in ((1, 2), (3,)):
        make = lambda: _params(mfx, k, 1, panel_rows, graph, wg_waves=16)
        lay, off, _ = _reference(mfx, data, monkeypatch, reference, (k, graph, panel_rows, calls), make, calls)
        assert lay["csc"]["kind"] == "lds" and lay["csr"]["kind"] == "lds"
        assert lay["csc"]["panels"] > 2 and lay["csr"]["panels"] > 2  # so that a range of chunks crosses panel boundaries
        _, on, _ = _run(mfx, data, monkeypatch, wgs, make(), calls)
        _same(on, off)


@pytest.mark.parametrize("wgs", [0, 3, 64])
@pytest.mark.parametrize("wg_waves", [4, 8])
def test_smaller_workgroups(mfx, data, monkeypatch, reference, wg_waves, wgs):
    """256- and 512-thread workgroups (several window entries per thread), the default grid among the workgroup counts"""
    make = lambda: _params(mfx, 5, 1, 700, wg_waves=wg_waves)
    _, off, _ = _reference(mfx, data, monkeypatch, reference, ("waves", wg_waves), make, (1, 2))
    _, on, _ = _run(mfx, data, monkeypatch, wgs, make(), (1, 2))
    _same(on, off)


@pytest.mark.parametrize("wgs", [2, 5, 64])
@pytest.mark.parametrize("wg_waves", [16, 4])
def test_window_overflow_instantiation(mfx, data, monkeypatch, reference, wg_waves, wgs):
    """The PSCHK instantiation: some chunk touches more ranks than the 1024-entry operand window holds.  Established on the
    host by counting: a copy stores one rank per non-empty (segment, panel) pair, every panel is padded to whole chunks, so
    there are at most nnz / chunk + panels + 1 chunks, and with more than 1024 pairs per chunk on average some chunk starts more
    than 1024 ranks.  64-entry panels cut the rows and columns of this data set into runs of 3.6 entries."""
    pr, tiles = 64, 64 // wg_waves  # chunks of 16384 entries
    make = lambda: _params(mfx, 4, 1, pr, wg_waves=wg_waves, tiles=tiles)
    lay, off, _ = _reference(mfx, data, monkeypatch, reference, ("pschk", wg_waves), make, (1, 2))
    d = data
    rows = np.repeat(np.arange(d.rows, dtype=np.int64), np.diff(d.csr_row_ptr))
    cols = np.asarray(d.csr_col_idx, dtype=np.int64)
    for name, seg, idx in (("csr", rows, cols), ("csc", cols, rows)):
        assert lay[name]["kind"] == "lds" and lay[name]["panel_rows"] == pr and lay[name]["tiles_per_span"] == tiles
        pairs = np.unique(seg * (1 << 20) + idx // pr).size
        chunk = wg_waves * tiles * 256
        most_chunks = d.nnz // chunk + lay[name]["panels"] + 1
        assert pairs > 1024 * most_chunks, (name, pairs, most_chunks)
    _, on, _ = _run(mfx, data, monkeypatch, wgs, make(), (1, 2))
    _same(on, off)


@pytest.mark.parametrize("k", [2, 5])
def test_persistent_passes_under_profiling(mfx, data, monkeypatch, k):
    """profiled (eager, timed) launches: the same bits, and the same booking as the one-chunk launches"""
    _, off, loff = _run(mfx, data, monkeypatch, None, _params(mfx, k, 1, 700, profile=1), (2,))
    for wgs in (3, 64):
        _, on, lon = _run(mfx, data, monkeypatch, wgs, _params(mfx, k, 1, 700, profile=1), (2,))
        _same(on, off)
        lon.pop("host_enqueue_outer_iteration", None)
        loff.pop("host_enqueue_outer_iteration", None)
        assert lon == loff
        pairs = k // 2
        assert lon.get("ccd_flat_sweep", 0) == 2 * 2 * pairs
        assert lon["ccd_fused_csc_pass"] == lon["ccd_fused_csr_pass"] == 2 * (k - pairs)


@pytest.mark.parametrize("T,eps", [(2, 0.0), (1, 1e-3)])
def test_uncovered_configurations_keep_todays_launches(mfx, data, monkeypatch, T, eps):
    """T > 1 and the eps rule run no paired ranks, hence no persistent pass: the same launches, and the same bits, with the
    knob on (and the workgroup count pinned) or off"""
    _, off, loff = _run(mfx, data, monkeypatch, None, _params(mfx, 4, T, 700, profile=1, eps=eps), (2,))
    _, on, lon = _run(mfx, data, monkeypatch, 3, _params(mfx, 4, T, 700, profile=1, eps=eps), (2,))
    _same(on, off)
    lon.pop("host_enqueue_outer_iteration", None)
    loff.pop("host_enqueue_outer_iteration", None)
    assert lon == loff
