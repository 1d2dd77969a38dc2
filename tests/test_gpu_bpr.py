"""GPU tests of BPR training (mfx_bpr_*) against the exact reference of tests/bpr_exact.py: every comparison of factors is
bit for bit and every count exact, because the contract of include/mfx.h fixes each fp32 operation and the sums of a step are
integer sums."""
import ctypes as C

import numpy as np
import pytest

import bpr_exact as bx

pytestmark = pytest.mark.gpu

MFX_ERR_INVALID = -1  # include/mfx.h
F = np.float32
ROWS, COLS = 37, 29
KEYS = ("slots", "skipped", "bad", "correct")


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1
    return m


@pytest.fixture(scope="module")
def R():
    return bx.small_matrix()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def counts(rep):
    return [rep[key] for key in KEYS]


def _check_apply(mfx, W, H, u, i, j, lr, lam, skipped=None):
    """bpr_apply against the reference: W, H and the four counts; returns the reference's result."""
    Wr, Hr, st = bx.step(W, H, u, i, j, skipped, lr, lam)
    Wg, Hg, rep = mfx.bpr_apply(W, H, u, i, j, lr, lam, skipped=skipped)
    assert counts(rep) == st, (counts(rep), st)
    assert same_bits(Wg, Wr), int((bits(Wg) != bits(Wr)).sum())
    assert same_bits(Hg, Hr), int((bits(Hg) != bits(Hr)).sum())
    return Wr, Hr, st


def _params(mfx, k, lam):
    p = mfx.parameter()
    p.k, p.lambda_ = k, lam
    return p


# ------------------------------------------------------------------------------------------------ the operator
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("k", [1, 3, 4, 63, 64, 65, 128, 129, 200, 1024])
def test_apply_bit_for_bit(mfx, k, n):
    rng = np.random.default_rng(1000 * k + n)
    W, H = bx.initial_factors(ROWS, COLS, k, k + n)
    W *= F(4.0)  # scores of a few units: the sigmoid away from 1/2
    lr, lam = 0.05, 0.01

    # a random batch over a part of the rows (the others must keep their bits), caller skip flags on a fifth of the slots,
    # and item 5 as the positive of some slots and the sampled item of others; i == j happens by chance and is allowed
    u = rng.integers(0, ROWS - 7, n)
    i = rng.integers(0, COLS - 5, n)
    j = rng.integers(0, COLS - 5, n)
    i[::3] = 5
    j[1::3] = 5
    skipped = rng.random(n) < 0.2
    Wr, Hr, st = _check_apply(mfx, W, H, u, i, j, lr, lam, skipped)
    assert st[1] == int(skipped.sum()) and st[2] == 0
    assert same_bits(Wr[ROWS - 7:], W[ROWS - 7:]) and same_bits(Hr[COLS - 5:], H[COLS - 5:])
    if not skipped.all():
        assert not same_bits(Wr, W) and not same_bits(Hr, H)

    # every slot the same user, no flags, lambda = 0
    _check_apply(mfx, W, H, np.full(n, 3), i, rng.integers(0, COLS, n), lr, 0.0)

    # lr = 0: every bit stays
    Wz, Hz, _ = _check_apply(mfx, W, H, u, i, j, 0.0, lam, skipped)
    assert same_bits(Wz, W) and same_bits(Hz, H)

    # a slot whose term reaches 64 and a slot with a NaN factor are counted bad, the others are applied
    if n >= 3:
        Wb, Hb = W.copy(), H.copy()
        Wb[ROWS - 1] = 0.0
        Wb[ROWS - 1, 0] = 200.0
        Hb[COLS - 1, 0] = Hb[COLS - 2, 0]     # d_0 = 0: x = 0, g = 1/2 and the term g * 200 = 100
        Hb[COLS - 3, k - 1] = np.nan
        ub, ib, jb = u.copy(), i.copy(), j.copy()
        ub[0], ib[0], jb[0] = ROWS - 1, COLS - 1, COLS - 2
        ub[n - 1], ib[n - 1], jb[n - 1] = 1, 2, COLS - 3
        Wr, Hr, st = _check_apply(mfx, Wb, Hb, ub, ib, jb, lr, lam)
        assert st[2] == 2 and st[1] == 0
        assert same_bits(Wr[ROWS - 1], Wb[ROWS - 1]) and same_bits(Hr[COLS - 3:], Hb[COLS - 3:])
        assert not same_bits(Wr, Wb)


def test_apply_saturated_scores(mfx):
    """Scores far out on both sides: g is 1 or the smallest value, never NaN, and the bits still agree."""
    k, n = 4, 64
    rng = np.random.default_rng(5)
    W, H = bx.initial_factors(ROWS, COLS, k, 9)
    W *= F(60.0)
    H *= F(60.0)
    u, i, j = rng.integers(0, ROWS, n), rng.integers(0, COLS, n), rng.integers(0, COLS, n)
    x, _ = bx.slot_scores(W, H, u, i, j)
    assert x.min() < -90 and x.max() > 90
    _check_apply(mfx, W, H, u, i, j, 0.05, 0.01)


def test_apply_order_of_the_slots_plays_no_part(mfx):
    k, n = 65, 1000
    rng = np.random.default_rng(77)
    W, H = bx.initial_factors(ROWS, COLS, k, 77)
    u, i, j = rng.integers(0, ROWS, n), rng.integers(0, COLS, n), rng.integers(0, COLS, n)
    s = rng.random(n) < 0.1
    a = mfx.bpr_apply(W, H, u, i, j, 0.05, 0.01, skipped=s)
    for seed in (1, 2):
        o = np.random.default_rng(seed).permutation(n)
        b = mfx.bpr_apply(W, H, u[o], i[o], j[o], 0.05, 0.01, skipped=s[o])
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and counts(a[2]) == counts(b[2])


def test_apply_refuses_ids_out_of_range(mfx):
    W, H = bx.initial_factors(ROWS, COLS, 8, 0)
    z = np.zeros(70, np.uint32)
    for which, bad in ((0, ROWS), (1, COLS), (2, COLS)):
        ids = [z.copy(), z.copy(), z.copy()]
        ids[which][66] = bad
        ids[which][69] = bad + 5
        with pytest.raises(mfx.MfxError, match="slot 66"):
            mfx.bpr_apply(W, H, *ids, 0.05, 0.01)
    Wg, Hg, rep = mfx.bpr_apply(W, H, z[:0], z[:0], z[:0], 0.05, 0.01)
    assert same_bits(Wg, W) and same_bits(Hg, H) and counts(rep) == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ the solver
@pytest.mark.parametrize("batch", [1, 64, 100, 1 << 20])
@pytest.mark.parametrize("k", [8, 65])
def test_solver_step_is_the_operator_on_the_sampled_triples(mfx, R, k, batch):
    """Three epochs, one steps(1) at a time, beside bpr_apply on bpr_triples of the same slots: the counts of every step, and
    the factors at every step (batch = 1: at every 50th step and at the end of every epoch)."""
    lr, lam, seed = 0.05, 0.01, 21
    nnz = R.nnz
    assert nnz % 64 and nnz % 100 and nnz < (1 << 20)
    W, H = bx.initial_factors(R.rows, R.cols, k, 4)
    s = mfx.BprSolver(R, _params(mfx, k, lam), lr, batch, seed=seed)
    s.set_factors(W, H)
    assert s.position() == 0
    pos = 0
    for epoch in range(3):
        plan = bx.epoch_steps(nnz, batch, pos)
        assert sum(c for _, c in plan) == nnz and plan[-1][1] == (nnz % batch or batch)
        for n_step, (first, cnt) in enumerate(plan):
            assert first == pos
            u, i, j, sk = mfx.bpr_triples(R, seed, first, cnt)
            W, H, want = mfx.bpr_apply(W, H, u, i, j, lr, lam, skipped=sk)
            got = s.steps(1)
            assert counts(got) == counts(want) and got["slots"] == cnt
            pos += cnt
            assert s.position() == pos
            if batch > 1 or n_step % 50 == 0 or n_step == len(plan) - 1:
                Ws, Hs = s.get_factors()
                assert same_bits(Ws, W) and same_bits(Hs, H), (epoch, n_step)
    assert pos == 3 * nnz
    s.close()


def test_iterate_finishes_a_started_epoch_and_matches_the_reference(mfx, R):
    k, batch, lr, lam, seed = 8, 100, 0.05, 0.01, 33
    W0, H0 = bx.initial_factors(R.rows, R.cols, k, 6)
    s = mfx.BprSolver(R, _params(mfx, k, lam), lr, batch, seed=seed)
    s.set_factors(W0, H0)
    part = s.steps(2)
    assert part["slots"] == 200 and s.position() == 200
    reps = s.iterate(2)
    assert [r["slots"] for r in reps] == [R.nnz - 200, R.nnz] and s.position() == 2 * R.nnz
    assert s.iterate(0) == [] and s.steps(0)["slots"] == 0 and s.position() == 2 * R.nnz
    Wr, Hr, st, pos = bx.train(R, W0, H0, lr, lam, batch, seed, 2)
    assert pos == 2 * R.nnz
    assert st[0].tolist() == [part[key] + reps[0][key] for key in KEYS] and st[1].tolist() == counts(reps[1])
    for r in reps:
        assert r["auc"] == r["correct"] / (r["slots"] - r["skipped"] - r["bad"]) and r["seconds"] > 0
    Ws, Hs = s.get_factors()
    assert same_bits(Ws, Wr) and same_bits(Hs, Hr)
    s.close()


def _device_arrays(R):
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a)).to(dev)
    return {"rows": R.rows, "cols": R.cols, "csr_row_ptr": t(R.csr_row_ptr), "csr_col_idx": t(R.csr_col_idx),
            "csr_val": t(R.csr_val), "csc_col_ptr": t(R.csc_col_ptr), "csc_row_idx": t(R.csc_row_idx), "csc_val": t(R.csc_val)}


def test_same_bits_twice_other_seed_differs_memory_spaces_agree(mfx, R):
    import torch  # noqa: F401  (device-resident inputs)
    k, batch = 12, 64

    def run(seed, device_arrays=None, init_seed=8):
        s = mfx.BprSolver(R if device_arrays is None else None, _params(mfx, k, 0.01), 0.05, batch, seed=seed,
                          device_arrays=device_arrays, init_seed=init_seed)
        reps = s.iterate(2)
        W, H = s.get_factors()
        s.close()
        return W, H, [counts(r) for r in reps]

    a, b, c = run(5), run(5), run(5, device_arrays=_device_arrays(R))
    for other in (b, c):
        assert same_bits(a[0], other[0]) and same_bits(a[1], other[1]) and a[2] == other[2]
    d = run(6)
    assert not same_bits(a[0], d[0]) and not same_bits(a[1], d[1])
    # the default factors are those of numpy.random.default_rng(init_seed)
    W0, H0 = bx.initial_factors(R.rows, R.cols, k, 8)
    Wr, Hr, st, _ = bx.train(R, W0, H0, 0.05, 0.01, batch, 5, 2)
    assert same_bits(a[0], Wr) and same_bits(a[1], Hr) and a[2] == st.tolist()


def test_create_refuses_broken_rows_and_ranges(mfx, R):
    from mfx import api
    row = int(np.argmax(np.diff(R.csr_row_ptr.astype(np.int64)) >= 3))
    lo = int(R.csr_row_ptr[row])
    for what in ("unsorted", "duplicate", "too large"):
        B = R.copy()
        if what == "unsorted":
            B.csr_col_idx[lo], B.csr_col_idx[lo + 1] = R.csr_col_idx[lo + 1], R.csr_col_idx[lo]
        elif what == "duplicate":
            B.csr_col_idx[lo + 1] = R.csr_col_idx[lo]
        else:
            B.csr_col_idx[int(R.csr_row_ptr[row + 1]) - 1] = R.cols
        with pytest.raises(mfx.MfxError, match=f"row {row} "):
            mfx.BprSolver(B, _params(mfx, 8, 0.01), 0.05, 64)
    for kw in (dict(k=0), dict(k=1025), dict(batch=0), dict(batch=(1 << 20) + 1), dict(lr=-1.0), dict(lr=float("nan")),
               dict(lam=-0.5), dict(lam=float("inf"))):
        a = {"k": 8, "lam": 0.01, "lr": 0.05, "batch": 64, **kw}
        with pytest.raises(mfx.MfxError, match="mfx_bpr_create"):
            mfx.BprSolver(R, _params(mfx, a["k"], a["lam"]), a["lr"], a["batch"])
    # stepping before the factors are set is refused and leaves the handle usable
    h = C.c_void_p()
    csx, cp = api._csx(R), _params(mfx, 8, 0.01).to_c()
    lib = mfx.lib()
    assert lib.mfx_bpr_create(C.byref(h), C.byref(csx), C.byref(cp), 0.05, 64, 3, 0) == 0
    stats = (C.c_int64 * 4)()
    assert lib.mfx_bpr_steps(h, 1, stats, None) == MFX_ERR_INVALID
    assert lib.mfx_bpr_epochs(h, 1, stats, None) == MFX_ERR_INVALID
    W, H = bx.initial_factors(R.rows, R.cols, 8, 1)
    assert lib.mfx_bpr_get_factors(h, api._vp(W), api._vp(H), 0) == MFX_ERR_INVALID
    assert lib.mfx_bpr_steps(h, -1, stats, None) == MFX_ERR_INVALID
    assert lib.mfx_bpr_set_factors(h, api._vp(W), None, 0) == MFX_ERR_INVALID
    assert lib.mfx_bpr_set_factors(h, api._vp(W), api._vp(H), 0) == 0
    assert lib.mfx_bpr_steps(h, 1, stats, None) == 0 and stats[0] == 64
    u, i, j, sk = mfx.bpr_triples(R, 3, 0, 64)
    Wr, Hr, st = bx.step(W, H, u, i, j, sk, 0.05, 0.01)
    assert list(stats) == st
    assert lib.mfx_bpr_get_factors(h, api._vp(W), api._vp(H), 0) == 0
    assert same_bits(W, Wr) and same_bits(H, Hr)
    assert lib.mfx_bpr_destroy(h) == 0


# ------------------------------------------------------------------------------------------------ end to end
def test_planted_clusters_recommend_end_to_end(mfx):
    """The planted clusters of test_gpu_ials.py (bpr_exact.planted_clusters): k = 32, batch 1 024, lr 0.05, lambda 0.01, 10
    epochs.  The top-10 lists (training items excluded) must find the held-out item for at least 90 % of the users, and the
    last epoch must rank more of its sampled pairs correctly than the first."""
    P = bx.planted_clusters()
    s = mfx.BprSolver(P, _params(mfx, 32, 0.01), 0.05, 1024, seed=7, init_seed=5)
    reps = s.iterate(10)
    W, H = s.get_factors()
    s.close()
    assert all(r["slots"] == P.nnz and r["bad"] == 0 for r in reps)
    print("auc per epoch:", [round(r["auc"], 4) for r in reps])
    assert reps[-1]["auc"] > reps[0]["auc"]
    top, _ = mfx.recommend(W, H, 1, 10, exclude=P)
    m = mfx.topn_metrics(top, mfx.test_data_of(P))
    print("metrics:", m)
    assert m["users"] == P.rows
    assert m["hr"] >= 0.9, m
