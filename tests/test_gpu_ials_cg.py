"""GPU tests of implicit ALS by preconditioned conjugate gradients (mfx_ials_cg_create / mfx_ials_cg_half / mfx_ials_cg_stats)
against the fp64 references of tests/foldin_cg_ref.py, tests/ials_cg_ref.py and the dense systems of tests/ials_ref.py.

Data of the operator tests: foldin_cg_ref.inputs (6000 columns, rows of 0 / 1 / 3 / 17 / 250 / 2048 / 2049 / 2100 / 5000 entries,
so rows split over 2 and 3 chunks, 15 % explicit zeros, H ~ N(0, 1/k), lambda = 0.1, alpha in {0, 1, 40}).

Bounds: the project's own for these data (tests/test_gpu_foldin_cg.py): relative error at most 1e-3 and normwise backward
error against the DENSE system at most 3e-5 after steps = 64, tol = 1e-5; factors of one iteration within 1e-3 of the largest
entry of ials_ref.iteration; loss to 1e-6; HR@10 >= 0.9 on the planted clusters.  The preconditioner is made in fp32 on the
device, so a row may take one step more than the fp64 reference, not more.

Measured on the MI355X (printed as `ialscg-measured` lines; profiles/r22_ials_cg_accuracy.txt):
    operator, k = 37 ... 1024, worst over alpha and both starts: relative error 2.8e-05, backward error 8.8e-06, at most 31
    steps (k = 1024, alpha = 40); step counts equal to the fp64 reference's in 30 of 36 cases, 2 - 3 rows one step more in
    the other 6 (alpha = 0 from the warm start, every k)
    rows of 1 / 3 / 17 entries after 2 / 4 / 18 steps from zero: at most 2.4e-06 from the dense solve
    one iteration at k = 160, tol = 1e-5, against ials_ref.iteration: W 1.6e-05, H 7.5e-05 (the fp64 reference of the method:
    1.5e-05 / 6.9e-05), at most 12 / 13 steps; planted clusters HR@10 = 0.9990
    loss at k = 1024: the library's formula on the fp32 scores to 1e-6; 1.2e-6 from dense_loss on the fp64 product (see the test)
"""
import functools

import numpy as np
import pytest

import foldin_cg_ref as ref
import ials_cg_ref
import ials_ref
from test_gpu_foldin import select
from test_gpu_ials import _device_arrays, _params, _random_matrix

pytestmark = pytest.mark.gpu

LAM = ref.LAM
MFX_ERR_INVALID = -1  # include/mfx.h


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1, m.lib().mfx_last_error()
    return m


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@functools.lru_cache(maxsize=None)
def base_pair(k):
    return ref.base(ref.inputs(k)[3], LAM)


# ------------------------------------------------------------------------------------------------ 1. the operator
@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("k", ref.KS)
def test_half_converges_within_the_bounds(mfx, k, warm):
    ptr, idx, val, H, W0 = ref.inputs(k)
    start = W0 if warm else None
    for alpha in ref.ALPHAS:
        live = ref.counting(ref.IMPLICIT, k, alpha)
        Y, cnt = mfx.ials_cg_half(ptr, idx, val, H, k, LAM, alpha, 64, 1e-5, Y_in=start, return_steps=True)
        assert np.isfinite(Y).all() and cnt.dtype == np.int32
        rel, be, cn = ref.errors(ref.IMPLICIT, k, alpha, Y)
        _, want = ref.rows(ref.IMPLICIT, ptr, idx, val, H, LAM, alpha, start, 64, 1e-5, base_pair=base_pair(k))
        differ = int(np.count_nonzero(cnt != want))
        print(f"ialscg-measured operator k={k} alpha={alpha} start={'W0' if warm else 'zero'} worst_rel={rel:.3e} "
              f"worst_backward={be:.3e} most_steps={int(cnt.max())} rows_with_other_count_than_fp64={differ} "
              f"counts={cnt.tolist()} fp64={want.tolist()}")
        assert rel <= 1e-3 and be <= 3e-5, (k, alpha, warm, rel, be)
        assert np.all(cnt <= want + 1), (k, alpha, warm, cnt.tolist(), want.tolist())
        for u in range(len(ref.SIZES)):
            if u in live:
                assert 1 <= cnt[u] < 64, (k, alpha, u, cnt.tolist())
            else:  # exactly zero and 0 steps, whatever the start held
                assert cnt[u] == 0 and not Y[u].any(), (k, alpha, u)


@pytest.mark.parametrize("k", ref.KS)
def test_short_rows_end_after_n_plus_one_steps(mfx, k):
    """The check of the preconditioner: without Minv, or with a wrong one, CG is 4.5e-2 (n = 1) and at least
    2e-3 (n = 3) off after n + 1 steps."""
    ptr, idx, val, H, _ = ref.inputs(k)
    for alpha in ref.ALPHAS:
        sol = ref.dense_solutions(ref.IMPLICIT, k, alpha)
        for u, n in ((1, 1), (2, 3), (4, 17)):
            Y, cnt = mfx.ials_cg_half(ptr, idx, val, H, k, LAM, alpha, n + 1, 0.0, return_steps=True)
            b, y = sol[u][1], sol[u][2]
            if not b.any():  # the row's entries are explicit zeros
                assert cnt[u] == 0 and not Y[u].any()
                continue
            rel = float(np.linalg.norm(Y[u] - y) / np.linalg.norm(y))
            print(f"ialscg-measured short-row k={k} alpha={alpha} n={n} steps={int(cnt[u])} rel={rel:.3e}")
            assert 1 <= cnt[u] <= n + 1
            assert rel <= 1e-3, (k, alpha, n, rel)


# ------------------------------------------------------------------------------------------------ 2. bits
@pytest.mark.parametrize("k", [130, 256])
def test_a_row_does_not_depend_on_the_call_or_its_batch(mfx, k):
    alpha = 40.0
    ptr, idx, val, H, W0 = ref.inputs(k)
    sel = np.concatenate([np.random.default_rng(5).permutation(len(ref.SIZES))[:8], [2, 5]])  # a permuted subset, two rows twice
    for tol, steps, start in ((1e-4, 64, None), (1e-4, 64, W0), (0.0, 6, W0)):
        Y, cnt = mfx.ials_cg_half(ptr, idx, val, H, k, LAM, alpha, steps, tol, Y_in=start, return_steps=True)
        Y2, cnt2 = mfx.ials_cg_half(ptr, idx, val, H, k, LAM, alpha, steps, tol, Y_in=start, return_steps=True)
        assert same(Y, Y2) and np.array_equal(cnt, cnt2)
        sp, si, sv = select(ptr, idx, val, sel)
        Ys, cs = mfx.ials_cg_half(sp, si, sv, H, k, LAM, alpha, steps, tol, Y_in=None if start is None else np.ascontiguousarray(start[sel]),
                                  return_steps=True)
        assert same(Ys, Y[sel]) and np.array_equal(cs, cnt[sel]), (tol, steps)


def _solver(mfx, R, k, lam, alpha, cg, H0, W0, n, device_arrays=None):
    s = mfx.ImplicitAlsSolver(R if device_arrays is None else None, _params(mfx, k, lam), alpha, device_arrays=device_arrays, cg=cg)
    s.set_factors(H0, W0)
    rep = s.iterate(n)
    W, H = s.get_factors()
    out = W, H, rep, s.kernel_times(), s.cg_stats()
    s.close()
    return out


def test_two_iterations_equal_four_chained_halves_from_host_and_device_inputs(mfx):
    import torch  # noqa: F401  (device-resident inputs)
    R = _random_matrix(5, rows=2500, cols=400, density=0.03)
    k, lam, alpha, cg = 256, 0.1, 2.0, (64, 1e-4)
    H0 = (np.random.default_rng(k).standard_normal((R.cols, k)) * 0.1).astype(np.float32)
    a = _solver(mfx, R, k, lam, alpha, cg, H0, None, 2)
    b = _solver(mfx, R, k, lam, alpha, cg, H0, None, 2)
    c = _solver(mfx, R, k, lam, alpha, cg, H0, None, 2, device_arrays=_device_arrays(R))
    W, H, cw, ch = None, H0, None, None
    for _ in range(2):
        W, cw = mfx.ials_cg_half(R.csr_row_ptr, R.csr_col_idx, R.csr_val, H, k, lam, alpha, *cg, Y_in=W, return_steps=True)
        H, ch = mfx.ials_cg_half(R.csc_col_ptr, R.csc_row_idx, R.csc_val, W, k, lam, alpha, *cg, Y_in=H, return_steps=True)
    for got in (a, b, c):
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
        assert same(got[0], W) and same(got[1], H)
        for half, cnt in (("rows", cw), ("cols", ch)):  # the stats are those of the last iteration
            st = got[4][half]
            assert st["row_steps"] == int(cnt.sum()) and st["max_steps"] == int(cnt.max()) and st["failed"] == 0, (half, st)
            assert st["unconverged"] == 0 and cnt.max() < cg[0], (half, st)
    print(f"ialscg-measured chain k={k} last iteration: W-half steps mean={cw.mean():.2f} max={int(cw.max())}, "
          f"H-half steps mean={ch.mean():.2f} max={int(ch.max())}")


# ------------------------------------------------------------------------------------------------ 3. the trainer against fp64
def test_one_iteration_matches_the_exact_fp64_iteration(mfx):
    R = _random_matrix(1)
    k, lam, alpha, cg = 160, 0.1, 5.0, (64, 1e-5)
    H0 = (np.random.default_rng(2).standard_normal((R.cols, k)) * 0.1).astype(np.float32)
    W, H, rep, kt, st = _solver(mfx, R, k, lam, alpha, cg, H0, None, 1)
    assert rep[0].update_time > 0 and rep[0].rmse == 0
    Wr, Hr = ials_ref.iteration(R, H0.astype(np.float64), lam, alpha)
    print(f"ialscg-measured iteration k={k} tol={cg[1]:g} W={np.max(np.abs(W - Wr)) / np.max(np.abs(Wr)):.3e} "
          f"H={np.max(np.abs(H - Hr)) / np.max(np.abs(Hr)):.3e} stats={st}")
    assert np.max(np.abs(W - Wr)) <= 1e-3 * np.max(np.abs(Wr))
    assert np.max(np.abs(H - Hr)) <= 1e-3 * np.max(np.abs(Hr))
    assert not np.any(W[7]) and not np.any(H[11])
    assert set(kt) == {"ialscg_half_rows(W over H)", "ialscg_half_cols(H over W)", "ialscg_base_gram(H)", "ialscg_base_gram(W)",
                       "ialscg_inverse(H)", "ialscg_inverse(W)"}
    # cg_stats against the counts of the equivalent operator calls
    W1, cw = mfx.ials_cg_half(R.csr_row_ptr, R.csr_col_idx, R.csr_val, H0, k, lam, alpha, *cg, return_steps=True)
    H1, ch = mfx.ials_cg_half(R.csc_col_ptr, R.csc_row_idx, R.csc_val, W1, k, lam, alpha, *cg, Y_in=H0, return_steps=True)
    assert same(W1, W) and same(H1, H)
    assert cw[7] == 0 and ch[11] == 0
    for half, cnt in (("rows", cw), ("cols", ch)):
        assert st[half] == {"row_steps": int(cnt.sum()), "max_steps": int(cnt.max()), "unconverged": 0, "failed": 0}, (half, st)
    # the reference method in fp64, step counts within one
    _, _, (rw, rh) = ials_cg_ref.iteration(R, H0.astype(np.float64), None, lam, alpha, *cg)
    assert np.all(cw <= rw + 1) and np.all(ch <= rh + 1)
    # W given to set_factors is the warm start of the first half: the rows stop at once on the converged W
    W2, H2, _, _, st2 = _solver(mfx, R, k, lam, alpha, (64, 1e-3), H0, W, 1)
    assert st2["rows"]["row_steps"] < st["rows"]["row_steps"] // 4, (st2, st)


def test_stats_report_rows_that_run_out_of_steps_and_refuse_other_handles(mfx):
    import ctypes as C
    R = _random_matrix(1)
    k, lam, alpha = 160, 0.1, 5.0
    H0 = (np.random.default_rng(2).standard_normal((R.cols, k)) * 0.1).astype(np.float32)
    _, cw = mfx.ials_cg_half(R.csr_row_ptr, R.csr_col_idx, R.csr_val, H0, k, lam, alpha, 64, 1e-5, return_steps=True)
    st = _solver(mfx, R, k, lam, alpha, (3, 1e-5), H0, None, 1)[4]
    assert st["rows"]["unconverged"] == int(np.count_nonzero(cw > 3)) > 0, (st, cw.tolist())
    assert st["rows"]["max_steps"] == 3
    st0 = _solver(mfx, R, k, lam, alpha, (3, 0.0), H0, None, 1)[4]
    assert st0["rows"]["unconverged"] == 0 and st0["cols"]["unconverged"] == 0  # tol = 0: nothing to meet
    s = mfx.ImplicitAlsSolver(R, _params(mfx, k, lam), alpha, block=64)
    out = (C.c_int64 * 8)()
    assert mfx.lib().mfx_ials_cg_stats(s.handle, out) == MFX_ERR_INVALID
    s.close()


# ------------------------------------------------------------------------------------------------ 4. the loss
def test_loss_matches_dense_loss_and_never_increases_with_two_steps(mfx):
    R = _random_matrix(3)
    k, lam, alpha = 160, 0.05, 10.0
    H0 = (np.random.default_rng(4).standard_normal((R.cols, k)) * 0.1).astype(np.float32)
    s = mfx.ImplicitAlsSolver(R, _params(mfx, k, lam), alpha, cg=(2, 0.0))
    s.set_factors(H0)
    prev = None
    for it in range(8):
        s.iterate(1)
        got = s.loss()
        W, H = s.get_factors()
        want = ials_ref.dense_loss(R, W, H, lam, alpha)
        assert abs(got - want) <= 1e-6 * abs(want), (it, got, want)
        if prev is not None:
            assert got <= prev * (1 + 1e-6), (it, prev, got)
        prev = got
    s.close()


def test_one_iteration_and_the_loss_at_rank_1024(mfx):
    R = _random_matrix(9, rows=60, cols=50, density=0.1)
    k, lam, alpha = 1024, 0.05, 10.0
    H0 = (np.random.default_rng(4).standard_normal((R.cols, k)) * 0.03).astype(np.float32)
    s = mfx.ImplicitAlsSolver(R, _params(mfx, k, lam), alpha, cg=(64, 1e-5))
    s.set_factors(H0)
    s.iterate(1)
    got = s.loss()
    W, H = s.get_factors()
    st = s.cg_stats()
    s.close()
    assert np.isfinite(W).all() and np.isfinite(H).all()
    assert st["rows"]["failed"] == 0 and st["cols"]["failed"] == 0 and st["rows"]["unconverged"] == 0 and st["cols"]["unconverged"] == 0, st
    # The 1e-6 comparison with ials_ref.dense_loss is test_loss_matches_dense_loss_and_never_increases_with_two_steps (k = 160).
    # Here one iteration fits the 60 x 50 matrix almost exactly (s ~ 1 on the stored pairs) and the loss is what is left of two
    # sums of about 300 that cancel: sum over the stored pairs of -s^2 on the fp32 scores (include/mfx.h, mfx_ials_loss: s_ui
    # the fp32 fused multiply-add chain in ascending t) and <W^T W, H^T H>_F in fp64.  A chain of 1024 terms is 5e-7 from the
    # fp64 product, which moves the loss by sum 2 s (s32 - s64) over 600 pairs: measured 1.7e-5 of 14.0008 = 1.2e-6, a property
    # of the loss's definition at these factors, not of the trainer.  So the library's own formula (ials_ref.shortcut_loss)
    # is evaluated on the scores as it defines them, the same chain with its products exact in fp64; the distance to
    # dense_loss is printed.
    S = np.zeros((R.rows, R.cols), np.float32)
    for t in range(k):
        S = (W[:, t, None].astype(np.float64) * H[None, :, t].astype(np.float64) + S.astype(np.float64)).astype(np.float32)
    want = ials_ref.shortcut_loss(R, W, H, lam, alpha, scores=S)
    dense = ials_ref.dense_loss(R, W, H, lam, alpha)
    print(f"ialscg-measured loss k={k}: library {got!r}, the library's formula on the fp32 scores {want!r}, dense_loss on the fp64 "
          f"product {dense!r} (library off by {abs(got - dense) / dense:.3e}); stats={st}")
    assert abs(got - want) <= 1e-6 * abs(want), (got, want)
    assert abs(got - dense) <= 1e-5 * abs(dense), (got, dense)


# ------------------------------------------------------------------------------------------------ 5. end to end
def test_planted_clusters_recommend_end_to_end(mfx):
    """The data of test_gpu_ialsb.py's test of the same name: 20 clusters of 30 items, 2 000 users with 25 training items
    of their own cluster plus 2 random ones, one more in-cluster item held out.  k = 160, alpha = 40, at most 64 steps to
    tol = 1e-4, 10 iterations from a cold W: the top-10 lists must find the held-out item for at least 90 % of the users."""
    from mfx import dataset as ds
    rng = np.random.default_rng(11)
    nc, per, users = 20, 30, 2000
    items = nc * per
    tr_r, tr_c, te_r, te_c = [], [], [], []
    for u in range(users):
        cl = u % nc
        own = cl * per + rng.permutation(per)[:26]
        others = np.setdiff1d(np.arange(items), cl * per + np.arange(per))
        extra = rng.choice(others, 2, replace=False)
        tr = np.concatenate([own[:25], extra])
        tr_r += [u] * tr.size
        tr_c += list(tr)
        te_r.append(u)
        te_c.append(own[25])
    R = ds.from_coo(users, items, np.array(tr_r), np.array(tr_c), np.ones(len(tr_r), np.float32),
                    np.array(te_r), np.array(te_c), np.ones(len(te_r), np.float32))
    k = 160
    H0 = (rng.standard_normal((items, k)) * 0.1).astype(np.float32)
    W, H, _, _, st = _solver(mfx, R, k, 0.1, 40.0, (64, 1e-4), H0, None, 10)
    top, _ = mfx.recommend(W, H, 1, 10, exclude=R)
    m = mfx.topn_metrics(top, mfx.test_data_of(R))
    print(f"ialscg-measured planted-clusters k={k} hr@10={m['hr']:.4f} last iteration {st}")
    assert m["users"] == users
    assert m["hr"] >= 0.9, m
