"""Explanations above rank 128 (mfx_rec_explain_cg, Recommender.explain_cg) against the fp64 reference of
tests/explain_cg_ref.py, the dense systems of tests/foldin_cg_ref.py and the exact lists of tests/explain_exact.py.

Data: foldin_cg_ref.inputs (6000 columns, rows of 0 .. 5000 entries with 15 % explicit zeros, lambda = 0.1, alpha in {0, 1, 40};
the explicit models on the values minus 2), targets explain_cg_ref.targets (T = 5: the row's first item, three random items,
one padding) and explain_cg_ref.zero_target (a zeroed row of H as a target).  tests/test_explain_cg_host.py asserts every
numerical condition below for the fp64 reference on exactly these inputs.

Bounds: those of tests/test_gpu_foldin_cg.py: normwise backward error against the DENSE system at most 3e-5, relative error at
most 1e-3 with the condition gate of 1e3 asserted to skip nothing, step counts within one of the fp64 reference's.  The split:
<b, z> - <h_t, w> = <r_w, z> - <r_z, w> for symmetric A, and a residual is at most its backward error times
(|A| |x| + |rhs|), so |<b, Z> - <h_t, W>| <= 3e-5 [(|A| |w| + |b|) |z| + (|A| |z| + |h_t|) |w|].

Every test prints its worst measured values as `explcg-measured` lines.  Measured on the MI355X
(profiles/r20_explain_cg_accuracy.txt), worst over the cases: relative error 2.757e-05 (implicit k = 1024, alpha = 40, condition
144.1), backward error 3.444e-06, most steps 38 (ALS k = 256), split gap 1.260e-06 of its bracket, the step counts at
tol = 1e-4, k = 160 equal to the fp64 reference's for every pair, Z at k = 64 within 1.177e-05 of mfx_rec_explain's."""
import numpy as np
import pytest

import explain_cg_ref as xr
import explain_exact as ex
import foldin_cg_ref as ref
from test_gpu_foldin import F32, MFX_ERR_INVALID, handle, host, same, select

pytestmark = pytest.mark.gpu

LAM = ref.LAM
PAD = xr.PAD
SETUP = {ref.ALS: "als", ref.CCD: "ccd", ref.IMPLICIT: "implicit"}
TEN_CHUNKS = (30000, (20000, 0, 5))  # a row of ten chunks, an empty row, a short one (tests/test_gpu_foldin_cg.py)
CASES = [(ref.IMPLICIT, k, a) for k in ref.KS for a in ref.ALPHAS] + [(m, k, 0.0) for m in (ref.ALS, ref.CCD) for k in (160, 256)]
PAIR_KEYS = ("Z", "target_steps", "totals", "items", "contrib")
ROW_KEYS = ("W", "row_steps")


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1, m.lib().mfx_last_error()
    return m


def rec(mfx, H, layout=1):
    """A recommender over H and a one-row dummy W."""
    return handle(mfx, np.zeros((1, H.shape[1]), F32), H, layout)


def data(model, k, cols=ref.COLS, sizes=tuple(ref.SIZES)):
    ptr, idx, val, H, _ = ref.inputs(k, cols, sizes)
    return ptr, idx, (val if model == ref.IMPLICIT else ref.explicit_values(val)), H


def call(r, rows, tg, n_expl=3, **kw):
    return r.explain_cg(rows, tg, n_expl=n_expl, return_W=True, return_Z=True, return_steps=True, **kw)


_converged = {}


def converged(mfx, model, k, alpha):
    """steps = 64, tol = 1e-5 on the standard rows and targets, once per case: (explain_cg's dict, fold_in's tuple, errors)."""
    key = (model, k, alpha)
    if key not in _converged:
        ptr, idx, val, H = data(model, k)
        tg = xr.targets(k)
        with rec(mfx, H, ref.KS.index(k) % 2) as r:
            r.fold_in_cg_setup(model, LAM, alpha, steps=64, tol=1e-5)
            out = call(r, (ptr, idx, val), tg)
            fold = r.fold_in((ptr, idx, val), return_sweeps=True)
        _converged[key] = (out, fold, xr.errors(model, k, alpha, tg, out["Z"], out["W"], H))
    return _converged[key]


# ------------------------------------------------------------------------------------------------ 1. converged targets
@pytest.mark.parametrize("model,k,alpha", CASES)
def test_converged_targets(mfx, model, k, alpha):
    out, _, (rel, be, gap, cn) = converged(mfx, model, k, alpha)
    tg = xr.targets(k)
    Z, steps = out["Z"], out["target_steps"]
    assert np.isfinite(Z).all() and steps.dtype == np.int32 and steps.shape == tg.shape
    live = xr.live_pairs(model, k, alpha, tg)
    print(f"explcg-measured converged model={model} k={k} alpha={alpha} worst_rel={rel:.3e} worst_backward={be:.3e} "
          f"most_steps={int(steps.max())} worst_cond={cn:.1f}")
    assert cn <= 1e3, (model, k, alpha, cn)  # the gate may skip no pair
    assert rel <= 1e-3 and be <= 3e-5, (model, k, alpha, rel, be)
    assert (steps[live] >= 1).all() and (steps[live] < 64).all(), (model, k, alpha, steps.tolist())
    # padding targets and rows without counting entries: exactly zero, 0 steps; totals -inf for the padding
    assert not steps[~live].any() and same(Z[~live], np.zeros_like(Z[~live])), (model, k, alpha)
    assert np.isneginf(out["totals"][tg == PAD]).all() and np.isfinite(out["totals"][tg != PAD]).all()
    if alpha == 40.0 or model != ref.IMPLICIT:  # a zero row of H as a target: exactly zero, 0 steps, the slot's other targets solved
        ptr, idx, val, _ = data(model, k)
        Hz, tz = xr.zero_target(k)
        q = xr.ZERO_AT[0]
        with rec(mfx, Hz) as r:
            r.fold_in_cg_setup(model, LAM, alpha, steps=64, tol=1e-5)
            oz = call(r, select(ptr, idx, val, [q]), tz[[q]])
        assert oz["target_steps"][0, xr.ZERO_AT[1]] == 0 and same(oz["Z"][0, xr.ZERO_AT[1]], np.zeros(k, F32))
        assert oz["totals"][0, xr.ZERO_AT[1]] == 0 and (oz["target_steps"][0, [0, 1, 3]] >= 1).all() and np.isfinite(oz["Z"]).all()


# ------------------------------------------------------------------------------------------------ 2. the row of fold-in
@pytest.mark.parametrize("model,k,alpha", CASES)
def test_same_row_as_fold_in(mfx, model, k, alpha):
    out, fold, _ = converged(mfx, model, k, alpha)
    _, _, Wf, cnt = fold
    assert same(out["W"], Wf) and out["row_steps"].dtype == np.int32 and np.array_equal(out["row_steps"], cnt)
    tg, H = xr.targets(k), ref.inputs(k)[3]
    for q in range(tg.shape[0]):
        want = np.where(tg[q] == PAD, F32(-np.inf), ex.chain(Wf[q], H[np.where(tg[q] == PAD, 0, tg[q])])).astype(F32)
        assert same(out["totals"][q], want), (model, k, alpha, q)


# ------------------------------------------------------------------------------------------------ 3. the lists from Z_out
def check_lists(mfx, model, k, alpha, cols=ref.COLS, sizes=tuple(ref.SIZES), layout=1):
    ptr, idx, val, H = data(model, k, cols, sizes)
    tg = xr.targets(k, cols, sizes)
    with rec(mfx, H, layout) as r:
        r.fold_in_cg_setup(model, LAM, alpha, steps=64, tol=1e-5)
        outs = {n: call(r, (ptr, idx, val), tg, n) for n in (64, 3, 0)}
    first = outs[64]
    items, contrib = ex.expected(SETUP[model], ptr, idx, val, tg, first["Z"], H, 64, alpha)
    for n, out in outs.items():
        assert all(same(out[key], first[key]) for key in ("Z", "W", "totals", "row_steps", "target_steps")), n
        assert out["items"].shape == out["contrib"].shape == tg.shape + (n,)
        bad = np.nonzero((out["items"] != items[..., :n]).any(axis=2) |
                         (out["contrib"].view(np.uint32) != contrib[..., :n].view(np.uint32)).any(axis=2))
        assert bad[0].size == 0, (model, k, n, list(zip(*bad))[:5])
    live = xr.live_pairs(model, k, alpha, tg, cols, sizes)
    print(f"explcg-measured lists model={model} k={k} cols={cols} pairs={int(live.sum())} "
          f"listed={int((first['items'] != PAD).sum())} bitwise=equal")
    assert (first["items"][~live] == PAD).all() and np.isneginf(first["contrib"][~live]).all()
    assert (first["items"][live][:, 0] != PAD).all()


@pytest.mark.parametrize("model", [ref.ALS, ref.CCD, ref.IMPLICIT])
def test_lists_are_bit_for_bit_those_of_the_reference(mfx, model):
    check_lists(mfx, model, 130, 40.0 if model == ref.IMPLICIT else 0.0)


def test_lists_of_a_row_of_ten_chunks(mfx):
    check_lists(mfx, ref.IMPLICIT, 256, 40.0, *TEN_CHUNKS, layout=0)


# ------------------------------------------------------------------------------------------------ 4. the split
@pytest.mark.parametrize("model,k,alpha", CASES)
def test_contributions_sum_to_the_total(mfx, model, k, alpha):
    out, _, (_, _, gap, _) = converged(mfx, model, k, alpha)
    assert np.isfinite(out["Z"]).all() and np.isfinite(out["W"]).all()
    print(f"explcg-measured split model={model} k={k} alpha={alpha} worst_gap_over_bracket={gap:.3e}")
    assert gap <= 3e-5, (model, k, alpha, gap)


# ------------------------------------------------------------------------------------------------ 5. independence
@pytest.mark.parametrize("k", [130, 256])
def test_a_pair_does_not_depend_on_its_batch(mfx, k):
    import torch
    alpha, model = 40.0, ref.IMPLICIT
    ptr, idx, val, H = data(model, k)
    tg = xr.targets(k)
    U = tg.shape[0]
    rng = np.random.default_rng(5)
    perm = np.concatenate([rng.permutation(U), [2, 5, 5, 0, 9]])
    t32 = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
    # the five targets of a row at other positions, among other neighbours, in slots of 1, 3 and 64 targets
    wide = rng.integers(0, ref.COLS, (U, 64)).astype(np.uint32)
    wide[:, 7] = PAD
    at64 = [63, 17, 40, 5, 0]
    wide[:, at64] = tg
    others = [(tg[:, [1]], [0], [1]), (tg[:, [3, 0, 1]], [0, 1, 2], [3, 0, 1]), (wide, at64, [0, 1, 2, 3, 4])]
    with rec(mfx, H, 1) as r, rec(mfx, H, 0) as r2:
        for tol, steps in ((1e-4, 64), (0.0, 6)):
            for h in (r, r2):
                h.fold_in_cg_setup(model, LAM, alpha, steps=steps, tol=tol)
            full = call(r, (ptr, idx, val), tg)
            live = xr.live_pairs(model, k, alpha, tg)
            if tol == 0.0:
                assert (full["target_steps"][live] == steps).all() and not full["target_steps"][~live].any()
            keys = PAIR_KEYS + ROW_KEYS
            lay = call(r2, (ptr, idx, val), tg)                                    # two handles, two layouts
            assert all(same(lay[key], full[key]) for key in keys), tol
            sh = call(r, select(ptr, idx, val, perm), tg[perm])                    # permuted, with duplicates
            assert all(same(sh[key], full[key][perm]) for key in keys), tol
            for q in (1, 2, 5, 7, 9):                                              # the row alone
                one = call(r, select(ptr, idx, val, [q]), tg[[q]])
                assert all(same(one[key][0], full[key][q]) for key in keys), (tol, q)
            for other, pos, cols in others:                                        # other slot widths, positions, neighbours
                o = call(r, (ptr, idx, val), other)
                assert all(same(o[key][:, pos], full[key][:, cols]) for key in PAIR_KEYS), (tol, other.shape)
                assert all(same(o[key], full[key]) for key in ROW_KEYS), (tol, other.shape)
            dev = call(r, (t32(ptr), t32(idx), t32(val)), t32(tg))                 # device tensors in
            torch.cuda.synchronize()
            assert dev["target_steps"].dtype == torch.int32 and dev["row_steps"].dtype == torch.int32
            assert all(same(host(dev[key]).view(np.uint32), full[key].view(np.uint32)) for key in keys), tol
            cut = call(r, (ptr, idx, val), tg, max_ws_bytes=4 * k * (5 * xr.T + 4) * 3)  # three rows per piece
            assert all(same(cut[key], full[key]) for key in keys), tol
            print(f"explcg-measured independence k={k} tol={tol} steps={sorted(set(full['target_steps'][live].tolist()))} bitwise=equal")


@pytest.mark.parametrize("k,T", [(64, 17), (256, 9)])
def test_a_pair_of_a_split_row_does_not_depend_on_its_gather_group(mfx, k, T):
    """A row of ten chunks (ten partial slots, summed per target) with a slot of T targets that spans two gather groups, the
    second holding one target (k = 64: 16 + 1; k = 256: 8 + 1): every pair bit for bit the pair in a slot of its own."""
    alpha, model, steps = 40.0, ref.IMPLICIT, 4
    cols, sizes = TEN_CHUNKS
    ptr, idx, val, H = data(model, k, cols, sizes)
    rng = np.random.default_rng(11 + k)
    tg = rng.integers(0, cols, (len(sizes), T)).astype(np.uint32)
    tg[:, 0] = idx[0]   # an item of the long row
    tg[:, 3] = PAD
    with rec(mfx, H) as r:
        r.fold_in_cg_setup(model, LAM, alpha, steps=steps, tol=0.0)
        full = call(r, (ptr, idx, val), tg)
        live = xr.live_pairs(model, k, alpha, tg, cols, sizes)
        assert live[0].sum() == T - 1 and (full["target_steps"][live] == steps).all() and not full["target_steps"][~live].any()
        assert np.isfinite(full["Z"]).all() and full["Z"][live].any(axis=1).all()
        for t in range(T):
            one = call(r, (ptr, idx, val), tg[:, [t]])
            assert all(same(one[key][:, 0], full[key][:, t]) for key in ("Z", "target_steps")), (k, T, t)
            assert all(same(one[key], full[key]) for key in ROW_KEYS), (k, T, t)
    print(f"explcg-measured gather-groups k={k} T={T} chunks=10 pairs={int(live.sum())} bitwise=equal")


# ------------------------------------------------------------------------------------------------ 6. stop rule, counts
def test_pairs_stop_on_their_own(mfx):
    k, alpha, tol, model = 160, 40.0, 1e-4, ref.IMPLICIT
    ptr, idx, val, H = data(model, k)
    tg = xr.targets(k)
    live = xr.live_pairs(model, k, alpha, tg)
    _, want = xr.solve(model, ptr, idx, val, H, LAM, alpha, tg, 64, tol)
    with rec(mfx, H) as r:
        r.fold_in_cg_setup(model, LAM, alpha, steps=64, tol=tol)
        got = call(r, (ptr, idx, val), tg)
        cnt = got["target_steps"]
        print(f"explcg-measured stop-rule k={k} alpha={alpha} tol={tol} counts={cnt.tolist()} fp64={want.tolist()}")
        assert np.abs(cnt.astype(np.int64) - want).max() <= 1, (cnt.tolist(), want.tolist())
        assert cnt[live].min() >= 1 and cnt[live].max() < 64 and len(set(cnt[live].tolist())) >= 2, cnt.tolist()
        assert not cnt[~live].any()
        for c in sorted(set(cnt[live].tolist())):  # a stopped pair is the pair after exactly that many steps
            r.fold_in_cg_setup(model, LAM, alpha, steps=c, tol=0.0)
            fixed = call(r, (ptr, idx, val), tg)
            at = live & (cnt == c)
            assert (fixed["target_steps"][at] == c).all()
            assert all(same(fixed[key][at], got[key][at]) for key in ("Z", "items", "contrib")), c


# ------------------------------------------------------------------------------------------------ 7. below rank 128
def test_agrees_with_the_closed_form_explanation_at_rank_64(mfx):
    k, alpha = 64, 40.0
    tg = xr.targets(k)
    with rec(mfx, ref.inputs(k)[3]) as r:
        for model in (mfx.MFX_FOLD_ALS, mfx.MFX_FOLD_CCD, mfx.MFX_FOLD_IMPLICIT):
            ptr, idx, val, _ = data(model, k)
            r.fold_in_setup(model, LAM, alpha)
            want = r.explain((ptr, idx, val), tg, n_expl=3, return_W=True, return_Z=True)
            r.fold_in_cg_setup(model, LAM, alpha)
            got = call(r, (ptr, idx, val), tg)
            live = xr.live_pairs(model, k, alpha if model == mfx.MFX_FOLD_IMPLICIT else 0.0, tg)
            rows = np.nonzero(live.any(axis=1))[0]
            dist = lambda a, b: float(np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b))
            rz = max(dist(got["Z"][q, t], want["Z"][q, t]) for q, t in zip(*np.nonzero(live)))
            rw = max(dist(got["W"][q], want["W"][q]) for q in rows)
            print(f"explcg-measured closed-form k={k} model={model} worst_rel_Z={rz:.3e} worst_rel_W={rw:.3e} pairs={int(live.sum())}")
            assert len(rows) >= 7 and live.sum() >= 28 and rz <= 1e-3 and rw <= 1e-3, (model, rz, rw)


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_leave_the_handle_usable(mfx):
    from mfx.api import _vp
    from test_gpu_foldin import factors, segments
    cols, k, nt = 500, 64, 4
    ptr, idx, val = segments(7, cols, [3, 0, 10, 25])
    U = len(ptr) - 1
    _, H = factors(7, cols, k)
    tg = np.random.default_rng(8).integers(0, cols, (U, nt)).astype(np.uint32)
    tg[1, 2] = PAD
    lib = mfx.lib()

    def raw(r, nt=nt, n_expl=5, tg=tg, space=0, null_targets=False, nusers=U):
        it, co = np.empty((U, max(nt, 1), max(n_expl, 1)), np.uint32), np.empty((U, max(nt, 1), max(n_expl, 1)), F32)
        rc = lib.mfx_rec_explain_cg(r.handle, nusers, idx.size, _vp(ptr), _vp(idx), _vp(val), nt, None if null_targets else _vp(tg), n_expl,
                                    _vp(it), _vp(co), None, None, None, None, None, space)
        return rc, lib.mfx_last_error().decode()

    def refused(r, word, **kw):
        rc, msg = raw(r, **kw)
        return rc == MFX_ERR_INVALID and word in msg

    ALPHA = 2.0
    with mfx.Recommender(np.zeros((3, k), F32), H, 1) as r:
        assert refused(r, "mfx_rec_fold_in_cg_setup")                              # before any setup
        cg = lambda: r.fold_in_cg_setup(mfx.MFX_FOLD_IMPLICIT, LAM, ALPHA, steps=20, tol=1e-4)
        cg()
        good = call(r, (ptr, idx, val), tg, 5)
        again = lambda: all(same(a, b) for a, b in zip(call(r, (ptr, idx, val), tg, 5).values(), good.values()))
        assert again() and (good["target_steps"][[0, 2, 3]][tg[[0, 2, 3]] != PAD] >= 1).all() and not good["target_steps"][1].any()
        wrong = [lambda: r.fold_in_setup(mfx.MFX_FOLD_IMPLICIT, LAM, ALPHA),
                 lambda: r.fold_in_setup(mfx.MFX_FOLD_ALS, LAM),
                 lambda: r.fold_in_setup(mfx.MFX_FOLD_IMPLICIT, LAM, ALPHA, alpha0=0.5, nu=0.5),
                 lambda: r.fold_in_block_setup(LAM, ALPHA, block=16, sweeps=2),
                 lambda: r.fold_in_block_setup_reg(LAM, ALPHA, 0.5, 0.5, block=16, sweeps=2),
                 lambda: r.fold_in_block_setup_als(LAM, block=16, sweeps=2)]
        for i, other in enumerate(wrong):
            other()
            assert refused(r, "mfx_rec_fold_in_cg_setup"), i
            r.fold_in((ptr, idx, val), 3)                                          # the handle still folds in under that setup
            cg()
            assert again(), i
        for kw, word in ((dict(nt=0), "n_targets"), (dict(nt=65), "n_targets"), (dict(n_expl=-1), "n_expl"), (dict(n_expl=65), "n_expl"),
                         (dict(null_targets=True), "targets"), (dict(space=7), "memory space")):
            assert refused(r, word, **kw), kw
            assert again(), kw
        for badid in (cols, cols + 1, 0xFFFFFFFE):
            t2 = tg.copy()
            t2[2, 3] = badid
            assert refused(r, "mfx_rec_explain_cg: target 3 of slot 2", tg=t2), badid
            assert again(), badid
        v = val.copy()
        v[17] = -1.0                                                               # the rows are checked as fold-in checks them
        it, co = np.empty((U, nt, 5), np.uint32), np.empty((U, nt, 5), F32)
        assert lib.mfx_rec_explain_cg(r.handle, U, idx.size, _vp(ptr), _vp(idx), _vp(v), nt, _vp(tg), 5, _vp(it), _vp(co), None, None, None,
                                      None, None, 0) == MFX_ERR_INVALID and "mfx_rec_explain_cg" in lib.mfx_last_error().decode()
        assert again()
        with pytest.raises(mfx.MfxError, match="mfx_rec_fold_in_cg_setup"):        # mfx_rec_explain keeps refusing
            r.explain((ptr, idx, val), tg, n_expl=3)
        assert again()
        assert lib.mfx_rec_explain_cg(r.handle, 0, 0, None, None, None, nt, None, 5, None, None, None, None, None, None, None, 0) == 0
        assert raw(r)[0] == 0
        t = r.explain_times()
        assert set(t) == {"build", "solve", "contrib"} and all(x > 0 for x in t.values())
