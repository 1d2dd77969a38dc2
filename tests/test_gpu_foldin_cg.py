"""Fold-in by preconditioned conjugate gradients (mfx_rec_fold_in_cg_setup, Recommender.fold_in_cg_setup) against the fp64
reference of tests/foldin_cg_ref.py and the dense systems of tests/ials_ref.py / tests/alsb_ref.py.

Data: those of tests/test_gpu_ialsb.py (foldin_cg_ref.inputs): 6000 columns, the segment sizes of the operator tests (0, 1, 2
and 3 chunks of 2048 entries, empty rows, 15 % explicit zeros), H ~ N(0, 1/k), lambda = 0.1, alpha in {0, 1, 40}, the warm
start 0.1 N(0, 1); the explicit models run on the values minus 2 (zeros and negatives included).  tests/test_foldin_cg_host.py
asserts every numerical condition below for the fp64 reference on exactly these inputs.

Bounds: the project's own (tests/test_gpu_ials.py): normwise backward error against the DENSE system at most 3e-5, relative
error at most 1e-3 with the condition gate of 1e3 asserted to skip no row; 1e-3 for "the same method in fp64"
(tests/test_gpu_ialsb.py).  Step counts against the reference's within one step: fp32 against fp64 sits at the threshold.
A row whose entries are all explicit zeros has no right-hand side under the implicit model: zero, 0 steps.

Measured on the MI355X (printed by the tests as `foldcg-measured` lines; profiles/r19_foldin_cg_accuracy.txt), worst over
alpha and both starts: relative error / backward error / most steps (largest condition number)
    implicit k =   37: 1.507e-05 / 7.090e-06 / 11  (4.3)
    implicit k =   64: 1.566e-05 / 7.220e-06 / 14  (6.5)
    implicit k =  130: 2.045e-05 / 8.812e-06 / 19  (13.9)
    implicit k =  160: 1.780e-05 / 7.208e-06 / 22  (18.7)
    implicit k =  256: 2.382e-05 / 7.351e-06 / 24  (29.1)
    implicit k = 1024: 2.794e-05 / 5.568e-06 / 31  (144.1)
    implicit k =  256: 3.578e-05 / 1.616e-05 /  6  (3.2)   [20 000-entry row, ten chunks]
    ALS      k =  160: 1.426e-05 / 3.224e-06 / 30  (30.7)
    ALS      k =  256: 2.328e-05 / 3.272e-06 / 33  (40.3)
    CCD      k =  160: 8.344e-06 / 3.688e-06 /  6  (11.6)
    CCD      k =  256: 7.713e-06 / 3.438e-06 /  6  (11.9)
    rows of 1 / 3 / 17 entries after 2 / 4 / 18 steps from zero: at most 2.477e-06 from the dense solve (all k, alpha)
    iterate after 1 / 2 / 3 warm steps against fp64: at most 2.121e-05 (k = 130, alpha = 0: the start row's residual in fp32)
    stop rule k=160 alpha=40 tol=1e-4: counts [0, 1, 2, 0, 8, 17, 8, 8, 8, 5, 1], the fp64 reference's exactly
    closed form k=64: ALS 8.925e-06, CCD 3.808e-06, IMPLICIT 7.274e-06
"""
import numpy as np
import pytest

import foldin_cg_ref as ref
from test_gpu_foldin import F32, MFX_ERR_INVALID, handle, host, same, select

pytestmark = pytest.mark.gpu

LAM = ref.LAM
TEN_CHUNKS = (30000, (20000, 0, 5))  # a row of ten chunks, an empty row, a short one (tests/test_gpu_ialsb.py)


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1, m.lib().mfx_last_error()
    return m


def rec(mfx, H, layout=1):
    """A recommender over H and a one-row dummy W."""
    return handle(mfx, np.zeros((1, H.shape[1]), F32), H, layout)


def bad_rows(a, b):
    return np.nonzero((a.view(np.uint32) != b.view(np.uint32)).any(axis=1))[0].tolist()


def check_converged(mfx, model, k, alpha, cols=ref.COLS, sizes=tuple(ref.SIZES), layout=1):
    """steps = 64, tol = 1e-5 from zero and from the warm start: the bounds of the module docstring; returns the counts."""
    ptr, idx, val, H, W0 = ref.inputs(k, cols, sizes)
    if model != ref.IMPLICIT:
        val = ref.explicit_values(val)
    live = ref.counting(model, k, alpha, cols, sizes)
    out = []
    with rec(mfx, H, layout) as r:
        r.fold_in_cg_setup(model, LAM, alpha, steps=64, tol=1e-5)
        for start in (None, W0):
            _, _, Y, cnt = r.fold_in((ptr, idx, val), W_init=start, return_sweeps=True)
            assert np.isfinite(Y).all()
            rel, be, cn = ref.errors(model, k, alpha, Y, cols, sizes)
            print(f"foldcg-measured converged model={model} k={k} cols={cols} alpha={alpha} start={'W0' if start is not None else 'zero'} "
                  f"worst_rel={rel:.3e} worst_backward={be:.3e} most_steps={int(cnt.max())} worst_cond={cn:.1f}")
            assert cn <= 1e3, (model, k, alpha, cn)  # the gate may skip no row
            assert rel <= 1e-3 and be <= 3e-5, (model, k, alpha, start is not None, rel, be)
            assert cnt.dtype == np.int32
            for u in range(len(sizes)):
                if u in live:
                    assert 1 <= cnt[u] < 64, (model, k, alpha, u, cnt.tolist())
                else:  # exactly zero and 0 steps, whatever W_init held
                    assert cnt[u] == 0 and same(Y[u], np.zeros(k, F32)), (model, k, alpha, u)
            out.append(cnt)
    return out


# ------------------------------------------------------------------------------------------------ 1. converged solve
@pytest.mark.parametrize("alpha", ref.ALPHAS)
@pytest.mark.parametrize("k", ref.KS)
def test_converged_solve(mfx, k, alpha):
    check_converged(mfx, ref.IMPLICIT, k, alpha, layout=ref.KS.index(k) % 2)


# ------------------------------------------------------------------------------------------------ 2. the preconditioner
@pytest.mark.parametrize("k", ref.KS)
def test_short_rows_end_after_n_plus_one_steps(mfx, k):
    """Without Minv, or with a wrong one, CG is 4.5e-2 (n = 1) and at least 2e-3 (n = 3) off after n + 1 steps."""
    ptr, idx, val, H, _ = ref.inputs(k)
    with rec(mfx, H) as r:
        for alpha in ref.ALPHAS:
            sol = ref.dense_solutions(ref.IMPLICIT, k, alpha)
            for u, n in ((1, 1), (2, 3), (4, 17)):
                r.fold_in_cg_setup(mfx.MFX_FOLD_IMPLICIT, LAM, alpha, steps=n + 1, tol=0.0)
                _, _, Y, cnt = r.fold_in((ptr, idx, val), return_sweeps=True)
                b, y = sol[u][1], sol[u][2]
                if not b.any():  # the row's entries are explicit zeros
                    assert cnt[u] == 0 and not Y[u].any()
                    continue
                rel = float(np.linalg.norm(Y[u] - y) / np.linalg.norm(y))
                print(f"foldcg-measured short-row k={k} alpha={alpha} n={n} steps={int(cnt[u])} rel={rel:.3e}")
                assert 1 <= cnt[u] <= n + 1
                assert rel <= 1e-3, (k, alpha, n, rel)


# ------------------------------------------------------------------------------------------------ 3. the fp64 iterates
@pytest.mark.parametrize("k", ref.KS)
def test_same_iterate_as_the_fp64_method(mfx, k):
    ptr, idx, val, H, W0 = ref.inputs(k)
    pair = ref.base(H, LAM)
    with rec(mfx, H) as r:
        for alpha in ref.ALPHAS:
            live = ref.counting(ref.IMPLICIT, k, alpha)
            for steps in (1, 2, 3):
                want, _ = ref.rows(ref.IMPLICIT, ptr, idx, val, H, LAM, alpha, W0, steps, 0.0, base_pair=pair)
                r.fold_in_cg_setup(mfx.MFX_FOLD_IMPLICIT, LAM, alpha, steps=steps, tol=0.0)
                _, _, Y, cnt = r.fold_in((ptr, idx, val), W_init=W0, return_sweeps=True)
                rel = [float(np.linalg.norm(Y[u] - want[u]) / np.linalg.norm(want[u])) for u in live]
                print(f"foldcg-measured iterate k={k} alpha={alpha} steps={steps} worst_rel={max(rel):.3e}")
                assert max(rel) <= 1e-3, (k, alpha, steps, rel)
                assert cnt.tolist() == [steps if u in live else 0 for u in range(len(ref.SIZES))]


# ------------------------------------------------------------------------------------------------ 4. stop rule, counts
def test_rows_stop_on_their_own(mfx):
    k, alpha, tol = 160, 40.0, 1e-4
    ptr, idx, val, H, _ = ref.inputs(k)
    live = ref.counting(ref.IMPLICIT, k, alpha)
    _, want = ref.rows(ref.IMPLICIT, ptr, idx, val, H, LAM, alpha, None, 64, tol)
    with rec(mfx, H) as r:
        r.fold_in_cg_setup(mfx.MFX_FOLD_IMPLICIT, LAM, alpha, steps=64, tol=tol)
        _, _, got, cnt = r.fold_in((ptr, idx, val), return_sweeps=True)
        print(f"foldcg-measured stop-rule k={k} alpha={alpha} tol={tol} counts={cnt.tolist()} fp64={want.tolist()}")
        assert np.abs(cnt.astype(np.int64) - want).max() <= 1, (cnt.tolist(), want.tolist())
        assert cnt[live].max() < 64 and len(set(cnt[live].tolist())) >= 2, cnt.tolist()
        # a stopped row is the row after exactly that many steps, in the batch and alone
        for c in sorted(set(cnt[live].tolist())):
            r.fold_in_cg_setup(mfx.MFX_FOLD_IMPLICIT, LAM, alpha, steps=c, tol=0.0)
            rows_c = np.nonzero(cnt == c)[0]
            fixed = r.fold_in((ptr, idx, val))[2]
            assert same(fixed[rows_c], got[rows_c]), (c, rows_c.tolist())
            u = int(rows_c[0])
            _, _, alone, ac = r.fold_in(select(ptr, idx, val, [u]), return_sweeps=True)
            assert same(alone[0], got[u]) and ac[0] == c, (c, u)
        # the converged rows as the start: the test on the start row stops every row at once.  (The rows of a tol = 1e-5 run: a
        # row that stopped at 1e-4 by the recurrence's residual may sit on either side of 1e-4 by the residual formed anew.)
        r.fold_in_cg_setup(mfx.MFX_FOLD_IMPLICIT, LAM, alpha, steps=64, tol=1e-5)
        conv = r.fold_in((ptr, idx, val))[2]
        r.fold_in_cg_setup(mfx.MFX_FOLD_IMPLICIT, LAM, alpha, steps=64, tol=tol)
        _, _, again, zero = r.fold_in((ptr, idx, val), W_init=conv, return_sweeps=True)
        assert not zero.any(), zero.tolist()
        assert same(again[live], conv[live]) and not again[[u for u in range(len(ref.SIZES)) if u not in live]].any()


# ------------------------------------------------------------------------------------------------ 5. batch independence
@pytest.mark.parametrize("k", [130, 256])
def test_a_row_does_not_depend_on_its_batch(mfx, k):
    import torch
    alpha = 40.0
    ptr, idx, val, H, W0 = ref.inputs(k)
    t = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
    rng = np.random.default_rng(5)
    sel = np.concatenate([rng.permutation(len(ref.SIZES)), [2, 5, 5, 0, 9]])
    with rec(mfx, H, 1) as r, rec(mfx, H, 0) as r2:
        for tol, start in ((1e-4, None), (1e-4, W0), (0.0, W0)):
            for h in (r, r2):
                h.fold_in_cg_setup(mfx.MFX_FOLD_IMPLICIT, LAM, alpha, steps=6 if tol == 0.0 else 64, tol=tol)
            bi, bs, got, cnt = r.fold_in((ptr, idx, val), 10, W_init=start, return_sweeps=True)
            oi, os_, other, oc = r2.fold_in((ptr, idx, val), 10, W_init=start, return_sweeps=True)
            assert bad_rows(other, got) == [] and np.array_equal(oc, cnt) and same(oi, bi) and same(os_, bs)  # two handles, two layouts
            gi, gs, gw, gc = r.fold_in(select(ptr, idx, val, sel), 10, W_init=None if start is None else start[sel], return_sweeps=True)
            assert bad_rows(gw, got[sel]) == [] and np.array_equal(gc, cnt[sel]) and same(gi, bi[sel]) and same(gs, bs[sel])
            for u in (1, 2, 5, 7, 9):
                ai, as_, aw, ac = r.fold_in(select(ptr, idx, val, [u]), 10, W_init=None if start is None else start[[u]], return_sweeps=True)
                assert same(aw[0], got[u]) and ac[0] == cnt[u] and same(ai[0], bi[u]) and same(as_[0], bs[u]), (tol, u)
            dev = r.fold_in((t(ptr), t(idx), t(val)), 10, W_init=None if start is None else t(start), return_sweeps=True)
            torch.cuda.synchronize()
            assert same(host(dev[0]), bi) and same(host(dev[1]), bs) and same(host(dev[2]), got)
            assert dev[3].dtype == torch.int32 and np.array_equal(host(dev[3]).view(np.int32), cnt)


# ------------------------------------------------------------------------------------------------ 6. a ten-chunk row
@pytest.mark.parametrize("alpha", ref.ALPHAS)
def test_a_row_of_ten_chunks(mfx, alpha):
    check_converged(mfx, ref.IMPLICIT, 256, alpha, *TEN_CHUNKS)


# ------------------------------------------------------------------------------------------------ 7. explicit models
@pytest.mark.parametrize("k", [160, 256])
@pytest.mark.parametrize("model", [ref.ALS, ref.CCD])
def test_explicit_models(mfx, model, k):
    cold, _ = check_converged(mfx, model, k, 0.0)
    for u, n in enumerate(ref.SIZES):  # rank n plus a multiple of the identity: n + 1 steps at the most
        if 0 < n < k:
            assert cold[u] <= n + 1, (model, k, u, n, cold.tolist())


# ------------------------------------------------------------------------------------------------ 8. below rank 128
def test_agrees_with_the_closed_form_solve_at_rank_64(mfx):
    k, alpha = 64, 40.0
    ptr, idx, val, H, _ = ref.inputs(k)
    with rec(mfx, H) as r:
        for model in (mfx.MFX_FOLD_ALS, mfx.MFX_FOLD_CCD, mfx.MFX_FOLD_IMPLICIT):
            v = val if model == mfx.MFX_FOLD_IMPLICIT else ref.explicit_values(val)
            r.fold_in_setup(model, LAM, alpha)
            want = r.fold_in((ptr, idx, v))[2]
            r.fold_in_cg_setup(model, LAM, alpha)
            got = r.fold_in((ptr, idx, v))[2]
            rel = [float(np.linalg.norm(got[u] - want[u]) / np.linalg.norm(want[u])) for u in range(len(ref.SIZES)) if want[u].any()]
            print(f"foldcg-measured closed-form k={k} model={model} worst_rel={max(rel):.3e}")
            assert len(rel) >= 7 and max(rel) <= 1e-3, (model, rel)
            assert not got[[u for u in range(len(ref.SIZES)) if not want[u].any()]].any()


# ------------------------------------------------------------------------------------------------ 9. end to end
@pytest.mark.parametrize("layout", [0, 1])
def test_lists_equal_query_on_the_solved_rows(mfx, layout):
    from test_gpu_foldin import factors, segments
    cols, k, n_top = 3001, 160, 10
    rng = np.random.default_rng(70 + layout)
    sizes = list(rng.integers(0, 400, 40))
    sizes[::11] = [0] * len(sizes[::11])
    sizes += [cols - 5, cols, 2500]  # fewer than n_top eligible items: padded lists
    ptr, idx, val = segments(80 + layout, cols, sizes)
    W, H = factors(80 + layout, cols, k)
    H[2000:2100] = H[10:110]  # ties across tiles: ordered by item
    keep = rng.random(cols) < 0.7
    n = len(sizes)
    ex = mfx.dataset.from_coo(n, cols, np.repeat(np.arange(n), np.diff(ptr.astype(np.int64))), idx, val)
    assert np.array_equal(ex.csr_row_ptr, ptr) and np.array_equal(ex.csr_col_idx, idx)
    with handle(mfx, W, H, layout) as r:
        r.set_item_filter(keep)
        r.fold_in_cg_setup(mfx.MFX_FOLD_IMPLICIT, LAM, 2.0)
        items, scores, Wq = r.fold_in((ptr, idx, val), n_top)
        assert same(Wq, r.fold_in((ptr, idx, val))[2])
        t = r.fold_in_times()
        assert set(t) == {"build", "solve", "score"} and t["solve"] > 0
    with mfx.Recommender(Wq, H, 1, exclude=ex) as r2:
        r2.set_item_filter(keep)
        qi, qs = r2.query(n_top)
    assert same(items, qi) and same(scores, qs), layout
    real = items != 0xFFFFFFFF
    assert keep[items[real]].all()
    assert (items[-2] == 0xFFFFFFFF).all() and (items[-3, 5:] == 0xFFFFFFFF).all()


# ------------------------------------------------------------------------------------------------ 10. refusals
def test_refusals_leave_the_handle_usable(mfx):
    from mfx.api import _vp
    from test_gpu_foldin import factors, segments
    cols, k = 500, 64
    ptr, idx, val = segments(7, cols, [3, 0, 10, 25])
    W, H = factors(7, cols, k)
    nan = float("nan")
    lib = mfx.lib()
    IMP, EXACT = mfx.MFX_FOLD_IMPLICIT, mfx.MFX_FOLD_ALS_EXACT

    def warm(r):
        n = len(ptr) - 1
        Wo, items, done = np.empty((n, k), F32), np.empty((n, 5), np.uint32), np.empty(n, np.int32)
        rc = lib.mfx_rec_fold_in_warm(r.handle, n, idx.size, _vp(ptr), _vp(idx), _vp(val), None, _vp(Wo), _vp(done), 5, _vp(items), None, 0)
        return rc, lib.mfx_last_error().decode()

    with mfx.Recommender(W, H, 1) as r:
        r.fold_in_cg_setup(IMP, LAM, 2.0, steps=20, tol=1e-4)
        good = r.fold_in((ptr, idx, val), 5, return_sweeps=True)
        again = lambda: all(same(a, b) for a, b in zip(r.fold_in((ptr, idx, val), 5, return_sweeps=True), good))
        assert good[3].tolist()[1] == 0 and all(c >= 1 for i, c in enumerate(good[3].tolist()) if i != 1)
        for bad, word in (((IMP, LAM, 2.0, 0, 0.0), "steps"), ((IMP, LAM, 2.0, 1025, 0.0), "steps"), ((IMP, LAM, 2.0, 20, -1.0), "tol"),
                          ((IMP, LAM, 2.0, 20, nan), "tol"), ((IMP, 0.0, 2.0, 20, 0.0), "lambda"), ((EXACT, LAM, 2.0, 20, 0.0), "model"),
                          ((7, LAM, 2.0, 20, 0.0), "model"), ((IMP, LAM, -1.0, 20, 0.0), "alpha")):
            assert lib.mfx_rec_fold_in_cg_setup(r.handle, *bad) == MFX_ERR_INVALID, bad
            assert word in lib.mfx_last_error().decode(), (bad, lib.mfx_last_error())
            assert again(), bad
        # mfx_rec_explain: closed-form setups only
        with pytest.raises(mfx.MfxError, match="mfx_rec_fold_in_cg_setup"):
            r.explain((ptr, idx, val), good[0], n_expl=3)
        assert again()
        # the warm call: valid now, refused after a closed-form setup, valid again after this one
        assert warm(r)[0] == 0
        r.fold_in_setup(IMP, LAM, 2.0)
        direct = r.fold_in((ptr, idx, val))[2]
        rc, msg = warm(r)
        assert rc == MFX_ERR_INVALID and "mfx_rec_fold_in_cg_setup" in msg
        assert same(r.fold_in((ptr, idx, val))[2], direct)
        r.fold_in_cg_setup(IMP, LAM, 2.0, steps=20, tol=1e-4)
        assert again()
        assert np.linalg.norm(good[2] - direct) <= 1e-3 * np.linalg.norm(direct)
