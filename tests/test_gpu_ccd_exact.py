"""CCD++ product paths against the pinned oracle BIT FOR BIT, on inputs whose sums do not depend on the order of addition
(tests/exact_sums.py; the construction, its bounds and oracle == integer formula are checked on the host by
test_exact_sums_host.py).

Every other comparison of a summing pass with the oracle goes through a tolerance relative to the largest entry of the whole
vector (2e-5 per sweep, 2e-3 per solve), which cannot see one lost, doubled or misattributed entry of a long segment.  Here
every term and every partial sum is exact in fp32, so trees, DPP scans, carries across spans, chunks, LDS panels, persistent
workgroup ranges, scatter slabs and shards, and the 2^-36 fixed point must all give the oracle's bits; den = lambda n + h and
g / den are one correctly rounded operation each in k_finalize, as in the oracle.

W0 is zero outside one live rank, whose position picks the pass under test (first rank of a pair: the read-only passes;
second: the persistent catch-up passes; last rank of an odd k: an ordinary fused pass); maxiter = 1, T = 1.  The live rank is
compared as uint32; dead ranks with == 0 (a tree may give -0 where the reference loop gives +0).  Config A makes the v-pass
exact (H[live]); config B the v-pass, the u-pass and the residual update (W[live], H[live], both residual copies).

The negative controls change one rating of the longest column on the REFERENCE side only and require the bit comparison to
flag exactly that column; they print the relerr that the 2e-5 check would have seen (`negative-control` lines).
"""
import numpy as np
import pytest

import exact_sums as ex
from exact_sums import bits

pytestmark = pytest.mark.gpu

KNOBS = ("MFX_OWNER_PASSES", "MFX_FLAT_WGS", "MFX_FLAT_PERSIST", "MFX_DEFER_RESID", "MFX_FUSE_FINALIZE", "MFX_SCATTER_WGS",
         "MFX_OVERLAP_GROUPS", "MFX_COMM_RESERVE_CUS")


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1, "no HIP device: these tests must run on the GPU box"
    return m


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def pattern(mfx):
    return ex.ml1m_pattern(mfx.dataset)


@pytest.fixture(scope="module")
def cases():
    return {}  # (pattern name, config, k, live) -> inputs and the oracle's outputs, computed once per module


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)


def _case(cases, orc, name, d, cfg, k, live):
    """Inputs of config `cfg` on pattern `d` and what the oracle makes of them -- which must be the integer formula."""
    key = (name, cfg, k, live)
    if key not in cases:
        choice, (data, W0, lam) = ex.ccd_case(d, cfg, k, live)
        Wr, Hr, _, _, csc, csr = orc.ccdr1(data, W0, k, lam, 1, 1, orc.max_threads())
        v, u, icsc, icsr = ex.int_ccd_rank(data, W0, live, lam, with_u=(cfg == "B"))
        assert np.array_equal(bits(Hr[live]), bits(v))
        if cfg == "B":
            assert np.array_equal(bits(Wr[live]), bits(u))
            assert np.array_equal(bits(csc), bits(icsc)) and np.array_equal(bits(csr), bits(icsr))
        cases[key] = dict(data=data, W0=W0, lam=lam, W=Wr, H=Hr, csc=csc, csr=csr, cfg=cfg, k=k, live=live, choice=choice)
    return cases[key]


def _solve(mfx, c, **params):
    p = mfx.parameter()
    p.k, p.lambda_, p.maxiter, p.maxinneriter = c["k"], c["lam"], 1, 1
    for a, b in params.items():
        setattr(p, a, b)
    d = c["data"]
    s = mfx.CcdSolver(d, mfx.test_data_of(d), p)
    try:
        lay = s.layout_info()
        s.set_factors(c["W0"].copy())
        s.iterate(1)
        W, H = s.get_factors()
        csc, csr = s.get_residual(d.nnz)
        launches = {n: int(cnt) for n, (_, cnt) in s.kernel_times().items()}
    finally:
        s.close()
    return dict(W=W, H=H, csc=csc, csr=csr, lay=lay, launches=launches)


def _assert_exact(got, c, what="", inexact_side=True):
    live, k, cfg = c["live"], c["k"], c["cfg"]
    dead = np.arange(k) != live
    assert np.all(got["H"][dead] == 0) and np.all(got["W"][dead] == 0), what
    bad = np.nonzero(bits(got["H"][live]) != bits(c["H"][live]))[0]
    assert np.array_equal(bits(got["H"][live]), bits(c["H"][live])), (what, "H[live] differs in columns", bad[:20], bad.size)
    if cfg == "B":
        bad = np.nonzero(bits(got["W"][live]) != bits(c["W"][live]))[0]
        assert np.array_equal(bits(got["W"][live]), bits(c["W"][live])), (what, "W[live] differs in rows", bad[:20], bad.size)
        assert np.array_equal(bits(got["csc"]), bits(c["csc"])), (what, "csc residual")
        assert np.array_equal(bits(got["csr"]), bits(c["csr"])), (what, "csr residual")
    elif inexact_side:
        # config A's u-pass sums non-dyadic terms: the order matters again, the sweep tests' tolerance applies
        assert ex.relerr(got["W"][live], c["W"][live]) < 2e-5, what


def _negative_control(orc, c, got, what):
    """One rating of the longest column changed by 1 on the reference side only: the bit comparison flags exactly that
    column (config B: and rows of that column, no others), where the relerr of the sweep tests stays silent."""
    live, lam = c["live"], c["lam"]
    changed, j, rows = ex.one_rating_changed(c["data"], c["W0"][live])
    v2 = orc.rank_one_sweep(changed.csc_col_ptr, changed.csc_row_idx, changed.csc_val, c["W0"][live], lam, orc.max_threads())
    flagged = np.nonzero(bits(got["H"][live]) != bits(v2))[0]
    assert list(flagged) == [j], (what, flagged[:10], j)
    n = int(changed.csc_col_ptr[j + 1]) - int(changed.csc_col_ptr[j])
    line = f"negative-control {what} config={c['cfg']} column={j} entries={n} relerr_of_H={ex.relerr(got['H'][live], v2):.3e}"
    if c["cfg"] == "B":
        u2 = orc.rank_one_sweep(changed.csr_row_ptr, changed.csr_col_idx, changed.csr_val, v2, lam, orc.max_threads())
        moved = np.nonzero(bits(got["W"][live]) != bits(u2))[0]
        assert moved.size > 0 and np.all(np.isin(moved, rows)), (what, moved[:10])
        line += f" rows_flagged={moved.size}/{rows.size} relerr_of_W={ex.relerr(got['W'][live], u2):.3e}"
    print(line + "  (the sweep tests allow 2e-5)")


# ------------------------------------------------------------------ single operators
SWEEP_VARIANTS = [0, 1, 2, 16, 100, 333, 1000, -16, -333, -1]


def _check_sweep(mfx, orc, ptr, idx, nvec, what, seed):
    val, vec, lam = ex.sweep_inputs(ptr, idx, nvec, seed=seed)
    want = ex.int_sweep(ptr, idx, val, vec, lam)
    assert np.array_equal(bits(orc.rank_one_sweep(ptr, idx, val, vec, lam, orc.max_threads())), bits(want)), what
    lens = np.diff(ptr.astype(np.int64))
    # the negative control's reference: one value of the longest segment, met by vec != 0, changed by 1
    s = int(np.argmax(lens))
    q = (int(ptr[s]) + int(ptr[s + 1])) // 2
    while vec[idx[q]] == 0:
        q += 1
    val2 = val.copy()
    val2[q] += 1
    want2 = ex.int_sweep(ptr, idx, val2, vec, lam)
    assert list(np.nonzero(bits(want) != bits(want2))[0]) == [s]
    for variant in SWEEP_VARIANTS:
        out = mfx.rank_one_sweep(ptr, idx, val, vec, lam, variant)
        bad = np.nonzero(bits(out) != bits(want))[0]
        assert np.all(out[lens == 0] == 0), (what, variant)
        assert np.array_equal(bits(out[lens > 0]), bits(want[lens > 0])), (what, variant, "segments", bad[:20], "lengths", lens[bad[:20]])
        assert list(np.nonzero(bits(out) != bits(want2))[0]) == [s], (what, variant)
    print(f"negative-control sweep {what} segment={s} entries={int(lens[s])} relerr={ex.relerr(want, want2):.3e}  (the sweep tests allow 2e-5)")


@pytest.mark.parametrize("side", ["csc", "csr"])
def test_rank_one_sweep_ml1m_pattern_bit_exact(mfx, orc, pattern, side):
    d = pattern
    if side == "csc":
        _check_sweep(mfx, orc, d.csc_col_ptr, d.csc_row_idx, d.rows, "ml1m-columns", 1)
    else:
        _check_sweep(mfx, orc, d.csr_row_ptr, d.csr_col_idx, d.cols, "ml1m-rows", 2)


@pytest.mark.parametrize("long_segment", [0, 250_000])
def test_rank_one_sweep_long_and_degenerate_segments_bit_exact(mfx, orc, long_segment):
    """the segment lengths of test_flat_kernel_long_and_degenerate_segments; with one segment of 250 000 entries the single
    operators carry a Netflix-length column across their spans, chunks and panels"""
    ptr, idx, nvec, lens = ex.segment_pattern(long_segment)
    _check_sweep(mfx, orc, ptr, idx, nvec, f"segment-list+{long_segment}", 3)


# ------------------------------------------------------------------ resident solver, ML-1M-shaped pattern
def _kinds(*want):
    def check(r, c):
        got = (r["lay"]["csc"]["kind"], r["lay"]["csr"]["kind"])
        assert all(g in w.split("|") for g, w in zip(got, want)), (got, want)
    return check


def _lds(panel_rows, tiles=None):
    def check(r, c):
        for side in ("csc", "csr"):
            lay = r["lay"][side]
            assert lay["kind"] == "lds" and lay["panel_rows"] == panel_rows and lay["panels"] > 2, lay
            assert tiles is None or lay["tiles_per_span"] == tiles, lay
    return check


def _owner_launches(r, c):
    k, n = c["k"], r["launches"]
    assert n.get("ccd_finalize", 0) == 0 and n["ccd_fused_csc_pass"] == k and n["ccd_fused_csr_pass"] == k, n


def _paired_launches(r, c):
    """the pair's read-only passes are booked as ccd_flat_sweep, its catch-up passes as the fused ones"""
    k, n = c["k"], r["launches"]
    pairs = k // 2
    assert n.get("ccd_flat_sweep", 0) == 2 * pairs and n["ccd_fused_csc_pass"] == n["ccd_fused_csr_pass"] == k - pairs, n
    assert n["ccd_finalize"] == 2 * k, n


def _unpaired_launches(r, c):
    k, n = c["k"], r["launches"]
    assert "ccd_flat_sweep" not in n and n["ccd_fused_csc_pass"] == n["ccd_fused_csr_pass"] == k and n["ccd_finalize"] == 2 * k, n


def _no_finalize_kernel(r, c):
    assert r["launches"].get("ccd_finalize", 0) == 0 and r["launches"]["ccd_fused_csc_pass"] == c["k"], r["launches"]


def _window_overflow(wg_waves, tiles):
    """test_window_overflow_instantiation's counting argument: more than 1024 (segment, panel) pairs per chunk on average"""
    def check(r, c):
        _lds(64, tiles)(r, c)
        d = c["data"]
        rows, cols = ex.row_of_csr(d), d.csr_col_idx.astype(np.int64)
        for name, seg, idx in (("csr", rows, cols), ("csc", cols, rows)):
            pairs = np.unique(seg * (1 << 20) + idx // 64).size
            most_chunks = d.nnz // (wg_waves * tiles * 256) + r["lay"][name]["panels"] + 1
            assert pairs > 1024 * most_chunks, (name, pairs, most_chunks)
    return check


FLAT = {"MFX_OWNER_PASSES": "0"}
# name -> (environment, parameters, check that the intended path ran)
CONFIGS = {
    "default_owner_passes": ({}, dict(profile=1), _owner_launches),
    "default_graph_replay": ({}, dict(), _kinds("plain", "plain")),
    "default_eager": ({}, dict(graph=-1), _kinds("plain", "plain")),
    "flat_panel_rows_0": (FLAT, dict(panel_rows=0), _kinds("plain", "plain")),
    "flat_panel_rows_64": (FLAT, dict(panel_rows=64), _lds(64)),
    "flat_panel_rows_512": (FLAT, dict(panel_rows=512), _lds(512)),
    "flat_panel_rows_1500": (FLAT, dict(panel_rows=1500), _lds(1500)),
    "flat_panel_rows_-1": (FLAT, dict(panel_rows=-1), _kinds("plain", "plain")),
    "flat_panel_rows_-700": (FLAT, dict(panel_rows=-700), _kinds("cache", "cache")),
    "wg_waves_4": (FLAT, dict(panel_rows=700, wg_waves=4, tiles_per_span=4), _lds(700, 4)),
    "wg_waves_8": (FLAT, dict(panel_rows=700, wg_waves=8, tiles_per_span=2), _lds(700, 2)),
    "wg_waves_16": (FLAT, dict(panel_rows=700, wg_waves=16, tiles_per_span=8), _lds(700, 8)),
    "window_overflow_16": (FLAT, dict(panel_rows=64, wg_waves=16, tiles_per_span=4), _window_overflow(16, 4)),
    "window_overflow_4": (FLAT, dict(panel_rows=64, wg_waves=4, tiles_per_span=16), _window_overflow(4, 16)),
    "flat_wgs_1": ({**FLAT, "MFX_FLAT_WGS": "1"}, dict(panel_rows=512, wg_waves=16), _lds(512)),
    "flat_wgs_3": ({**FLAT, "MFX_FLAT_WGS": "3"}, dict(panel_rows=512, wg_waves=16), _lds(512)),
    "flat_wgs_64": ({**FLAT, "MFX_FLAT_WGS": "64"}, dict(panel_rows=1500, wg_waves=16), _lds(1500)),
    "flat_wgs_3_overflow": ({**FLAT, "MFX_FLAT_WGS": "3"}, dict(panel_rows=64, wg_waves=16, tiles_per_span=4), _window_overflow(16, 4)),
    "flat_persist_0": ({**FLAT, "MFX_FLAT_PERSIST": "0"}, dict(panel_rows=512, wg_waves=16), _lds(512)),
    "paired_profiled": (FLAT, dict(panel_rows=700, profile=1), _paired_launches),
    "paired_profiled_wgs_3": ({**FLAT, "MFX_FLAT_WGS": "3"}, dict(panel_rows=700, profile=1), _paired_launches),
    "defer_resid_0": ({**FLAT, "MFX_DEFER_RESID": "0"}, dict(panel_rows=512), _lds(512)),
    "defer_resid_0_profiled": ({**FLAT, "MFX_DEFER_RESID": "0"}, dict(panel_rows=700, profile=1), _unpaired_launches),
    "graph_0": (FLAT, dict(panel_rows=512, graph=0), _lds(512)),
    "graph_-1": (FLAT, dict(panel_rows=512, graph=-1), _lds(512)),
    "layout_build_1": (FLAT, dict(panel_rows=512, layout_build=1), _lds(512)),
    "layout_build_2": (FLAT, dict(panel_rows=512, layout_build=2), _lds(512)),
    "schedule_0_variant_0": ({}, dict(schedule=0, kernel_variant=0), None),
    "schedule_0_variant_1": ({}, dict(schedule=0, kernel_variant=1), None),
    "schedule_0_variant_1_panels": (FLAT, dict(schedule=0, kernel_variant=1, panel_rows=700), _lds(700)),
    "scatter_variant_2": ({}, dict(kernel_variant=2), _kinds("scatter", "scatter")),
    "scatter_variant_2_panels": ({}, dict(kernel_variant=2, panel_rows=150, tiles_per_span=2), _kinds("scatter", "scatter")),
    "scatter_variant_3": ({}, dict(kernel_variant=3), _kinds("scatter32", "scatter32")),
    "fuse_finalize_1_panels": ({**FLAT, "MFX_FUSE_FINALIZE": "1"}, dict(panel_rows=300, tiles_per_span=4), _lds(300, 4)),
    "fuse_finalize_1_plain": ({**FLAT, "MFX_FUSE_FINALIZE": "1"}, dict(panel_rows=0, profile=1), _no_finalize_kernel),
    "fuse_finalize_2_panels": ({**FLAT, "MFX_FUSE_FINALIZE": "2"}, dict(panel_rows=64), _lds(64)),
}


@pytest.mark.parametrize("cfg", ["A", "B"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_resident_solver_bit_exact(mfx, orc, pattern, cases, monkeypatch, name, cfg):
    """k = 7 with the live rank first of a pair / second of a pair / the odd last rank, and k = 1"""
    env, params, check = CONFIGS[name]
    for a, b in env.items():
        monkeypatch.setenv(a, b)
    for k, live in ex.CCD_RANKS:
        c = _case(cases, orc, "ml1m", pattern, cfg, k, live)
        got = _solve(mfx, c, **params)
        if check is not None:
            check(got, c)
        _assert_exact(got, c, (name, cfg, k, live))


@pytest.mark.parametrize("cfg", ["A", "B"])
@pytest.mark.parametrize("name", ["default_owner_passes", "flat_panel_rows_512", "scatter_variant_2"])
def test_resident_solver_negative_control(mfx, orc, pattern, cases, monkeypatch, name, cfg):
    env, params, _ = CONFIGS[name]
    for a, b in env.items():
        monkeypatch.setenv(a, b)
    c = _case(cases, orc, "ml1m", pattern, cfg, 7, 1)
    got = _solve(mfx, c, **params)
    _assert_exact(got, c, name)
    _negative_control(orc, c, got, name)


# ------------------------------------------------------------------ hyper-sparse, scatter ranges, shards
def test_hyper_sparse_layouts_bit_exact(mfx, orc, cases):
    """the shape of test_hyper_sparse_shard_layouts: scatter on both sides by default, cache + plain from the host builder,
    cache panels forced, the as-written schedule over the scatter layout"""
    d = ex.small_patterns(mfx.dataset, "hyper_sparse")["hyper_sparse"]
    for cfg, live in (("A", 0), ("B", 1), ("B", 0)):
        c = _case(cases, orc, "hyper_sparse", d, cfg, 2, live)
        for params, check in ((dict(), _kinds("scatter", "scatter")), (dict(layout_build=1), _kinds("cache", "plain")),
                              (dict(schedule=0, kernel_variant=2), _kinds("scatter", "scatter")),
                              (dict(panel_rows=-262144), _kinds("cache", "cache|plain"))):
            got = _solve(mfx, c, **params)
            check(got, c)
            _assert_exact(got, c, ("hyper_sparse", cfg, live, params))
    _negative_control(orc, c, got, "hyper_sparse")


@pytest.mark.parametrize("wgs", ["1", "2", "3", "7", "64", "100000"])
def test_scatter_persistent_workgroup_ranges_bit_exact(mfx, orc, cases, monkeypatch, wgs):
    """the shape and layout of test_scatter_persistent_workgroup_ranges: ranges that split panels at odd places"""
    monkeypatch.setenv("MFX_SCATTER_WGS", wgs)
    d = ex.small_patterns(mfx.dataset, "scatter_ranges")["scatter_ranges"]
    for cfg in ("A", "B"):
        for live in (0, 1, 2):
            c = _case(cases, orc, "scatter_ranges", d, cfg, 3, live)
            got = _solve(mfx, c, kernel_variant=2, panel_rows=200, tiles_per_span=2)
            _kinds("scatter", "scatter")(got, c)
            _assert_exact(got, c, ("scatter_ranges", wgs, cfg, live))


@pytest.mark.parametrize("nshards,schedule,variant", [(2, 1, 1), (3, 1, 2), (4, 0, 1), (2, 0, 0), (4, 1, 2)])
def test_sharded_loopback_bit_exact(mfx, orc, pattern, cases, nshards, schedule, variant):
    """The loopback shards of test_sharded_solve_multi_rank_loopback (threads of this process): local (g, h) partials, the
    all-reduce, division by lambda * GLOBAL count.  Partial sums of exact sums are exact, so every rank's H replica and its
    rows of W equal the UNSHARDED oracle bit for bit."""
    import threading
    d = pattern
    bounds = mfx.partition_rows(d, nshards)
    for cfg, k, live in (("A", 3, 0), ("B", 3, 1), ("B", 3, 2)):
        c = _case(cases, orc, "ml1m", d, cfg, k, live)
        data = c["data"]
        gcnt = np.ascontiguousarray(np.diff(data.csc_col_ptr.astype(np.int64)).astype(np.uint32))
        out, errs = [None] * nshards, []
        group = 3000 + ((nshards * 2 + schedule) * 3 + variant) * 4 + live + (cfg == "B")

        def run(r):
            try:
                lo, hi = int(bounds[r]), int(bounds[r + 1])
                shard = mfx.extract_shard(data, lo, hi)
                comm = mfx.Comm(None, r, nshards, 0, local_group=group)
                p = mfx.parameter()
                p.k, p.lambda_, p.maxiter, p.maxinneriter, p.schedule, p.kernel_variant = k, c["lam"], 1, 1, schedule, variant
                s = mfx.CcdSolver(shard, mfx.test_data_of(shard), p, comm=comm, global_col_nnz=gcnt, global_test_nnz=data.nnz_test)
                s.set_factors(np.ascontiguousarray(c["W0"][:, lo:hi]))
                s.iterate(1)
                out[r] = s.get_factors()
                s.close(); comm.close()
            except Exception as e:  # surface failures instead of dead-locking the other ranks' rendezvous
                errs.append(e)
                raise

        th = [threading.Thread(target=run, args=(r,)) for r in range(nshards)]
        [x.start() for x in th]
        [x.join(timeout=120) for x in th]
        assert not errs and all(o is not None for o in out), errs
        dead = np.arange(k) != live
        for r, (Wl, Hl) in enumerate(out):
            lo, hi = int(bounds[r]), int(bounds[r + 1])
            assert np.array_equal(bits(Hl[live]), bits(c["H"][live])), (cfg, live, "rank", r)
            assert np.all(Hl[dead] == 0) and np.all(Wl[dead] == 0)
            if cfg == "B":
                assert np.array_equal(bits(Wl[live]), bits(c["W"][live][lo:hi])), (cfg, live, "rank", r)


# ------------------------------------------------------------------ full size, once
ROWS, COLS, NNZ = 480189, 17770, 99072112


def test_fullsize_paired_persistent_schedule_bit_exact(mfx, orc):
    """Netflix shape (480 189 x 17 770, 99 M ratings), k = 2, the benchmarked paired and persistent schedule: live = 0 with
    config A (the read-only passes) and live = 1 with config B (the catch-up passes, both residual copies).  Two solvers.  The
    value sets are the widest of the ladders that the device pattern's longest column and row allow (checked here: the pattern
    exists on the device only), the values are built on the device, the oracle runs on the host copy."""
    import torch
    from mfx import synth_torch
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    d = synth_torch.synth_ratings_device(ROWS, COLS, NNZ, seed=2024, device="cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    col_len = int((d["csc_col_ptr"][1:] - d["csc_col_ptr"][:-1]).max())
    row_len = int((d["csr_row_ptr"][1:] - d["csr_row_ptr"][:-1]).max())
    print(f"fullsize longest column {col_len} longest row {row_len}")
    k = 2

    def fits(maxlen, vmax, rmax, gv, gr, lam):
        return ex.units(maxlen, vmax, rmax, gv, gr, lam)

    for cfg, live in (("A", 0), ("B", 1)):
        if cfg == "A":
            choice = next(c for c in ex.A_LADDER if max(fits(col_len, c["u_eighths"] / 8, c["r_max"], 1 / 8, 1.0, c["lam"])) <= ex.SIGNIFICAND)
            lam = choice["lam"]
            csr_val = torch.randint(1, choice["r_max"] + 1, (NNZ,), generator=g, device=dev).float()
            e = choice["u_eighths"]
            u = (torch.randint(-e, e + 1, (ROWS,), generator=g, device=dev).float() / 8).cpu().numpy()
        else:
            choice = next(c for c in ex.B_LADDER
                          if max(fits(col_len, 1.0, c["c_quarters"] / 4, 1.0, 1 / 4, 1.0)
                                 + fits(row_len, c["c_quarters"] / 8, c["c_quarters"] / 4, 1 / 8, 1 / 4, 1.0)) <= ex.SIGNIFICAND)
            lam = 1.0
            q = choice["c_quarters"]
            cj = torch.randint(1, q + 1, (COLS,), generator=g, device=dev).float() / 4
            cj = cj * (torch.randint(0, 2, (COLS,), generator=g, device=dev).float() * 2 - 1)
            csr_val = cj[d["csr_col_idx"].long()].contiguous()
            u = np.ones(ROWS, np.float32)
        print(f"fullsize config {cfg} value set {choice}")
        dd = dict(d)
        dd["csr_val"] = csr_val
        dd["csc_val"] = csr_val[d["csc_of_csr"]].contiguous()
        torch.cuda.synchronize()
        host = synth_torch.to_rating_data(dd)
        W0 = ex.live_rank(k, ROWS, live, u)
        print("fullsize bounds", ex.preconditions(host, W0, live, lam, cfg))  # raises if a partial sum could be inexact

        p = mfx.parameter()
        p.k, p.lambda_, p.maxiter, p.maxinneriter = k, lam, 1, 1
        s = mfx.CcdSolver(None, None, p, device_arrays=dd)
        try:
            lay = s.layout_info()
            s.set_factors(W0.copy())
            s.iterate(1)
            W, H = s.get_factors()
            csc, csr = s.get_residual(NNZ)
        finally:
            s.close()
        assert lay["csc"]["kind"] == "lds" and lay["csr"]["kind"] == "lds" and lay["csc"]["panels"] > 2, lay
        Wr, Hr, _, _, csc_ref, csr_ref = orc.ccdr1(host, W0, k, lam, 1, 1, orc.max_threads())
        assert np.array_equal(bits(Hr[live]), bits(ex.int_sweep(host.csc_col_ptr, host.csc_row_idx, host.csc_val, u, lam)))
        if cfg == "B":
            assert np.array_equal(bits(Wr[live]), bits(ex.int_sweep(host.csr_row_ptr, host.csr_col_idx, host.csr_val, Hr[live], lam)))
        c = dict(data=host, W0=W0, lam=lam, W=Wr, H=Hr, csc=csc_ref, csr=csr_ref, cfg=cfg, k=k, live=live)
        got = dict(W=W, H=H, csc=csc, csr=csr)
        _assert_exact(got, c, ("fullsize", cfg, live), inexact_side=False)
        _negative_control(orc, c, got, "fullsize")
        del dd, host, csr_val, got, c, csc, csr, csc_ref, csr_ref


# ------------------------------------------------------------------ general inputs: a per-element bound instead of a share of the maximum
def _sum64(ptr, terms):
    """per-segment fp64 sums (pairwise inside a segment), 0 for empty segments"""
    p = ptr.astype(np.int64)
    n = np.diff(p)
    out = np.zeros(n.size)
    if terms.size:
        out[n > 0] = np.add.reduceat(terms, p[:-1][n > 0])
    return out


def _check_per_element(out, ptr, idx, val, vec, lam, what):
    """|out - out64| <= n 2^-24 (sum |vec r| / den + |out64|) + 4 ulp(out64) for every non-empty segment of n <= 1024 entries:
    the first-order bound of n fp32 additions in ANY order on numerator and denominator, one rounding per product, and the
    division.  Longer segments, where this bound says nothing, are what the exact inputs above are for."""
    n = np.diff(ptr.astype(np.int64))
    x = vec.astype(np.float64)[idx.astype(np.int64)]
    r = val.astype(np.float64)
    den = np.float64(np.float32(lam)) * n + _sum64(ptr, x * x)
    short = (n > 0) & (n <= 1024)
    out64 = np.zeros(n.size)
    out64[n > 0] = _sum64(ptr, x * r)[n > 0] / den[n > 0]
    bound = n * 2.0 ** -24 * (_sum64(ptr, np.abs(x * r)) / np.where(n > 0, den, 1.0) + np.abs(out64)) \
        + 4 * np.spacing(np.abs(out64).astype(np.float32)).astype(np.float64)
    err = np.abs(out.astype(np.float64) - out64)
    ratio = float(np.max(err[short] / bound[short]))
    print(f"per-element {what}: {int(short.sum())} of {int((n > 0).sum())} non-empty segments checked, worst error / bound = {ratio:.3f}")
    assert short.sum() > 0
    worst = int(np.argmax(np.where(short, err / np.where(bound > 0, bound, 1.0), 0)))
    assert np.all(err[short] <= bound[short]), (what, "segment", worst, "entries", int(n[worst]), err[worst], bound[worst])


@pytest.mark.parametrize("variant", [0, 1, 2, 1000])
def test_single_ops_medium_per_element_bound(mfx, orc, variant):
    """test_single_ops_medium's inputs (non-dyadic, random): every non-empty segment of up to 1024 entries against its own
    fp64 value, not against the largest entry of the vector"""
    d = mfx.dataset.synth_ratings(6040, 3706, 1_000_000, seed=7, skew=0.9, test_frac=0.01, empty_row_frac=0.01, empty_col_frac=0.02)
    u = np.random.default_rng(3).uniform(0.001, 0.101, d.rows).astype(np.float32)
    v = mfx.rank_one_sweep(d.csc_col_ptr, d.csc_row_idx, d.csc_val, u, 0.05, variant)
    _check_per_element(v, d.csc_col_ptr, d.csc_row_idx, d.csc_val, u, 0.05, f"variant {variant} columns")
    v_ref = orc.rank_one_sweep(d.csc_col_ptr, d.csc_row_idx, d.csc_val, u, 0.05, 4)
    u2 = mfx.rank_one_sweep(d.csr_row_ptr, d.csr_col_idx, d.csr_val, v_ref, 0.05, variant)
    _check_per_element(u2, d.csr_row_ptr, d.csr_col_idx, d.csr_val, v_ref, 0.05, f"variant {variant} rows")
