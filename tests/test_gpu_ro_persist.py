"""Persistent read-only passes (k_flat<FM_FCSC_RO> / <FM_FCSR_RO> in the PERSIST form, the default in CcdSolver::rank_pair
next to the persistent catch-up passes): a resident workgroup walks a contiguous range of chunks with ONE operand window,
sends the first tile of its span in the next chunk during the span's last tile, and stages the LDS slice again only where
the panel changes.  A span is still summed by one wave in the same order, so W, H, both residual copies and the test RMSEs
must be BIT-identical to the one-chunk launches (MFX_FLAT_PERSIST=0): with the read-only passes alone persistent (mask
0x30), the catch-up passes alone (0xC0) or both (the default), whatever the workgroup count, k, the workgroup size, the
panel size, graph replay or profiling."""
import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

# fewer workgroups than chunks (ranges of several chunks that cross panel boundaries), and more than there are chunks
# (the launcher falls back to one chunk per workgroup)
WGS = [1, 2, 3, 7, 64, 1_000_000]
MASKS = [0x30, 0xC0, None]  # read-only passes alone, catch-up passes alone, the default (all four)


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1, "no HIP device: these tests must run on the GPU box"
    return m


@pytest.fixture(scope="module")
def data(mfx):
    # the data set of test_gpu_defer_resid.py / test_gpu_flat_persist.py: ML-1M sized, with empty rows / columns
    return mfx.dataset.synth_ratings(6040, 3706, 1_000_000, seed=11, skew=0.9, test_frac=0.01,
                                     empty_row_frac=0.01, empty_col_frac=0.02)


@pytest.fixture(scope="module")
def reference():
    return {}  # one-chunk results by configuration: computed once, compared with every mask and workgroup count


@pytest.fixture(autouse=True)
def _no_owner_passes(monkeypatch):
    monkeypatch.setenv("MFX_OWNER_PASSES", "0")  # (small matrices take the segment-owner passes otherwise)
    monkeypatch.delenv("MFX_FUSE_FINALIZE", raising=False)
    monkeypatch.delenv("MFX_DEFER_RESID", raising=False)


def _params(mfx, k, panel_rows, graph=0, profile=0, wg_waves=16, tiles=0):
    p = mfx.parameter()
    p.k, p.lambda_, p.maxiter, p.maxinneriter = k, 0.05, 3, 1
    p.schedule, p.kernel_variant, p.panel_rows, p.graph, p.profile = 1, 1, panel_rows, graph, profile
    p.wg_waves, p.tiles_per_span = wg_waves, tiles
    return p


def _run(mfx, d, monkeypatch, mask, wgs, p, calls):
    """mask: 0 = MFX_FLAT_PERSIST=0, None = the default mask, else MFX_FLAT_PERSIST=mask; wgs: 0 = the default grid, n =
    MFX_FLAT_WGS=n.  iterate(n) for n in calls; after each call: W, H, both residual copies, the test RMSEs; plus the launch counts"""
    monkeypatch.delenv("MFX_FLAT_WGS", raising=False)
    monkeypatch.delenv("MFX_FLAT_PERSIST", raising=False)
    if mask is not None:
        monkeypatch.setenv("MFX_FLAT_PERSIST", hex(mask))
    if wgs:
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
        reference[key] = _run(mfx, d, monkeypatch, 0, 0, make_params(), calls)
    return reference[key]


@pytest.mark.parametrize("wgs", WGS)
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("k,panel_rows", [(2, 512), (5, 1500), (5, 512), (2, 1500)])
def test_masks_and_workgroup_counts(mfx, data, monkeypatch, reference, k, panel_rows, mask, wgs):
    """k even / odd (the last rank alone); more than two panels per copy, so that chunk ranges cross panel boundaries; 1 then 2
    more outer iterations with the residual read in between (capture and replay of the hipGraph); 1024-thread workgroups"""
    make = lambda: _params(mfx, k, panel_rows)
    lay, off, _ = _reference(mfx, data, monkeypatch, reference, (k, panel_rows, 0, (1, 2)), make, (1, 2))
    assert lay["csc"]["kind"] == "lds" and lay["csr"]["kind"] == "lds"
    assert lay["csc"]["panels"] > 2 and lay["csr"]["panels"] > 2
    _, on, _ = _run(mfx, data, monkeypatch, mask, wgs, make(), (1, 2))
    _same(on, off)


@pytest.mark.parametrize("calls", [(1, 2), (3,)])
@pytest.mark.parametrize("graph", [0, -1])
@pytest.mark.parametrize("k", [2, 5])
def test_graph_replay_and_eager_launches(mfx, data, monkeypatch, reference, k, graph, calls):
    """graph = 0: captured once, replayed (3 in one call: capture and two replays); graph = -1: eager launches"""
    make = lambda: _params(mfx, k, 512, graph)
    _, off, _ = _reference(mfx, data, monkeypatch, reference, (k, 512, graph, calls), make, calls)
    for mask in (0x30, None):
        _, on, _ = _run(mfx, data, monkeypatch, mask, 3, make(), calls)
        _same(on, off)


@pytest.mark.parametrize("wgs", [0, 3, 64])
@pytest.mark.parametrize("wg_waves", [4, 8, 16])
def test_workgroup_sizes(mfx, data, monkeypatch, reference, wg_waves, wgs):
    """256-, 512- and 1024-thread workgroups (several window entries per thread), the default grid among the counts"""
    make = lambda: _params(mfx, 5, 700, wg_waves=wg_waves)
    _, off, _ = _reference(mfx, data, monkeypatch, reference, ("waves", wg_waves), make, (1, 2))
    for mask in (0x30, None):
        _, on, _ = _run(mfx, data, monkeypatch, mask, wgs, make(), (1, 2))
        _same(on, off)


@pytest.mark.parametrize("wgs", [2, 5, 64])
@pytest.mark.parametrize("wg_waves", [16, 4])
def test_window_overflow_instantiation(mfx, data, monkeypatch, reference, wg_waves, wgs):
    """The PSCHK instantiation: some chunk touches more ranks than the 1024-entry operand window holds.  Established on the
    host by counting, as in test_gpu_flat_persist.py: a copy stores one rank per non-empty (segment, panel) pair, every panel
    is padded to whole chunks, so there are at most nnz / chunk + panels + 1 chunks, and with more than 1024 pairs per chunk
    on average some chunk starts more than 1024 ranks.  64-entry panels cut the rows and columns into runs of 3.6 entries."""
    pr, tiles = 64, 64 // wg_waves  # chunks of 16384 entries
    make = lambda: _params(mfx, 4, pr, wg_waves=wg_waves, tiles=tiles)
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
    for mask in (0x30, None):
        _, on, _ = _run(mfx, data, monkeypatch, mask, wgs, make(), (1, 2))
        _same(on, off)


@pytest.mark.parametrize("k", [2, 5])
def test_under_profiling(mfx, data, monkeypatch, k):
    """profiled (eager, timed) launches: the same bits, and the same booking as the one-chunk launches"""
    _, off, loff = _run(mfx, data, monkeypatch, 0, 0, _params(mfx, k, 700, profile=1), (2,))
    loff.pop("host_enqueue_outer_iteration", None)
    for mask, wgs in ((0x30, 3), (None, 64)):
        _, on, lon = _run(mfx, data, monkeypatch, mask, wgs, _params(mfx, k, 700, profile=1), (2,))
        _same(on, off)
        lon.pop("host_enqueue_outer_iteration", None)
        assert lon == loff
        pairs = k // 2
        assert lon.get("ccd_flat_sweep", 0) == 2 * 2 * pairs
        assert lon["ccd_fused_csc_pass"] == lon["ccd_fused_csr_pass"] == 2 * (k - pairs)
