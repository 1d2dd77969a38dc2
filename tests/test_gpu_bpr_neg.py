"""GPU tests of negative sampling by trials (mfx_bpr_create_neg, mfx_bpr_apply_neg) against the exact reference of
tests/bpr_neg_exact.py: factors bit for bit, counts, chosen items and chosen trials exact, in both modes (hardest of M and
WARP), at the sizes where a lane group, a round of trials and a wave turn over."""
import ctypes as C
import os

import numpy as np
import pytest

import bpr_exact as bx
import bpr_neg_exact as nx

pytestmark = pytest.mark.gpu

MFX_ERR_INVALID = -1  # include/mfx.h
F = np.float32
ROWS, COLS = 37, 29
KEYS = ("slots", "skipped", "bad", "correct")
MODES = {"bpr": nx.HARDEST, "warp": nx.WARP}


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


def table(m):
    """A rank-weight table of the tests' own: 2.5 / t, the last entry 0 when there is more than one."""
    rw = (F(2.5) / np.arange(1, m + 1, dtype=F)).astype(F)
    if m > 1:
        rw[-1] = 0.0
    return rw


def factors(k, seed):
    """Factors whose scores have a standard deviation of about 2, whatever k: margins on both sides of 1."""
    W, H = bx.initial_factors(ROWS, COLS, k, seed)
    s = F(10.0 * np.sqrt(2.0 / np.sqrt(k)))
    return W * s, H * s


def _check(mfx, W, H, u, i, items, member, lr, lam, rw=None, losses=("bpr", "warp")):
    """bpr_apply_neg against the reference in the given modes: W, H, the four counts, t, and j where a trial was chosen.
    Returns {loss: the reference's result}."""
    items = np.asarray(items)
    rw = table(items.shape[1]) if rw is None else rw
    sc = nx.trial_scores(np.asarray(W, F), np.asarray(H, F), np.asarray(u, np.int64), np.asarray(i, np.int64), items.astype(np.int64))
    out = {}
    for loss in losses:
        Wr, Hr, st, jr, tr = nx.step_neg(W, H, u, i, items, member, MODES[loss], rw, lr, lam, scores=sc)
        Wg, Hg, rep, jg, tg = mfx.bpr_apply_neg(W, H, u, i, items, lr, lam, loss=loss, member=member, rank_weight=rw)
        assert np.array_equal(tg, tr), (loss, np.nonzero(tg != tr)[0][:5], tg[tg != tr][:5], tr[tg != tr][:5])
        assert np.array_equal(jg[tr > 0], jr[tr > 0]), loss
        assert counts(rep) == st, (loss, counts(rep), st)
        assert same_bits(Wg, Wr), (loss, int((bits(Wg) != bits(Wr)).sum()))
        assert same_bits(Hg, Hr), (loss, int((bits(Hg) != bits(Hr)).sum()))
        out[loss] = (Wr, Hr, st, jr, tr)
    return out


def _random_case(k, n, m, seed):
    rng = np.random.default_rng(seed)
    W, H = factors(k, seed)
    u = rng.integers(0, ROWS - 7, n)          # the last rows and items must keep their bits
    i = rng.integers(0, COLS - 5, n)
    items = rng.integers(0, COLS - 5, (n, m))
    i[::3] = 5
    items[1::3, 0] = 5                        # item 5 as the positive of some slots and as a trial of others
    member = rng.random((n, m)) < 0.2
    member[2::7] = True                       # slots with no eligible trial
    return W, H, u, i, items, member


# ------------------------------------------------------------------------------------------------ the operator
@pytest.mark.parametrize("k", [1, 3, 4, 63, 64, 65, 128, 129, 200, 1024])
def test_apply_neg_bit_for_bit_over_k(mfx, k):
    n, m = 65, 9
    W, H, u, i, items, member = _random_case(k, n, m, 100 + k)
    ref = _check(mfx, W, H, u, i, items, member, 0.05, 0.01)
    for loss, (Wr, Hr, st, jr, tr) in ref.items():
        assert same_bits(Wr[ROWS - 7:], W[ROWS - 7:]) and same_bits(Hr[COLS - 5:], H[COLS - 5:])
        assert not same_bits(Wr, W) and not same_bits(Hr, H)
        assert np.all(tr[2::7] == 0) and st[2] == 0
    assert len(set(ref["warp"][4].tolist())) >= 3 and len(set(ref["bpr"][4].tolist())) >= 4


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("m", [1, 2, 7, 8, 9, 16, 63, 64, 65, 200, 1024])
def test_apply_neg_bit_for_bit_over_trials_and_slots(mfx, m, n):
    for k in (4, 65):
        W, H, u, i, items, member = _random_case(k, n, m, 7000 + 10 * m + n + k)
        member |= np.random.default_rng(m + n).random((n, m)) < 0.5  # later trials get their turn
        if k == 65:
            H = H * F(0.5)  # fewer violators: WARP walks further down the trials
        _check(mfx, W, H, u, i, items, member, 0.05, 0.01)


def test_no_bit_depends_on_the_lanes_per_slot(mfx):
    k, n, m = 12, 300, 37
    W, H, u, i, items, member = _random_case(k, n, m, 41)
    rw = table(m)
    try:
        for loss in MODES:
            base = mfx.bpr_apply_neg(W, H, u, i, items, 0.05, 0.01, loss=loss, member=member, rank_weight=rw)
            for width in (1, 2, 4, 16, 64):
                os.environ["MFX_BPR_TRIAL_GROUP"] = str(width)
                got = mfx.bpr_apply_neg(W, H, u, i, items, 0.05, 0.01, loss=loss, member=member, rank_weight=rw)
                assert same_bits(got[0], base[0]) and same_bits(got[1], base[1]) and counts(got[2]) == counts(base[2])
                assert np.array_equal(got[3], base[3]) and np.array_equal(got[4], base[4]), (loss, width)
                os.environ.pop("MFX_BPR_TRIAL_GROUP")
    finally:
        os.environ.pop("MFX_BPR_TRIAL_GROUP", None)
    _check(mfx, W, H, u, i, items, member, 0.05, 0.01, rw)


def test_crafted_trials_both_modes(mfx):
    k, n, m = 6, 40, 9
    W, H, u, i, items, member = _random_case(k, n, m, 3)
    member[:] = False

    # a repeated item among the trials: equal scores, the smaller t wins
    rep = items.copy()
    rep[:, :] = rep[:, :1]
    ref = _check(mfx, W, H, u, i, rep, None, 0.05, 0.01)
    assert np.all(ref["bpr"][4] == 1) and set(ref["warp"][4].tolist()) <= {0, 1}
    mem = member.copy()
    mem[:, :4] = True
    ref = _check(mfx, W, H, u, i, rep, mem, 0.05, 0.01)
    assert np.all(ref["bpr"][4] == 5) and set(ref["warp"][4].tolist()) <= {0, 5}

    # every trial a member: skipped, t = 0, nothing moves
    ref = _check(mfx, W, H, u, i, items, np.ones((n, m), bool), 0.05, 0.01)
    for loss in MODES:
        Wr, Hr, st, jr, tr = ref[loss]
        assert st == [n, n, 0, 0] and np.all(tr == 0) and same_bits(Wr, W) and same_bits(Hr, H)

    # the positive item itself as the only trial outside the row: d = 0, the row of H is this slot's twice, updated once
    own = np.repeat(i[:, None], m, axis=1)
    ref = _check(mfx, W, H, u[:1], i[:1], own[:1], None, 0.05, 0.01)
    lr, lam = F(0.05), F(0.01)
    for loss in MODES:
        Wr, Hr, st, jr, tr = ref[loss]
        assert st[:3] == [1, 0, 0] and tr[0] == 1 and jr[0] == i[0]
        assert same_bits(Wr[u[0]], W[u[0]] + lr * (F(0) - (lam * F(1)) * W[u[0]]))  # the terms g * d are zero
        assert same_bits(Hr[i[0]], H[i[0]] + lr * (F(0) - (lam * F(2)) * H[i[0]]))  # g * w and its negative cancel
    _check(mfx, W, H, u, i, own, None, 0.05, 0.01)

    # one user in every slot; an item that is the positive of some slots and a trial of the others
    _check(mfx, W, H, np.full(n, 3), i, items, None, 0.05, 0.01)
    shared_i, shared_items = i.copy(), items.copy()
    shared_i[::2] = 7
    shared_items[1::2] = 7
    _check(mfx, W, H, u, shared_i, shared_items, None, 0.05, 0.01)

    # lambda = 0; lr = 0: every bit stays
    _check(mfx, W, H, u, i, items, None, 0.05, 0.0)
    ref = _check(mfx, W, H, u, i, items, None, 0.0, 0.01)
    for loss in MODES:
        assert same_bits(ref[loss][0], W) and same_bits(ref[loss][1], H)


@pytest.mark.parametrize("what", [np.nan, np.inf, -np.inf])
def test_nan_and_infinities_in_the_factors(mfx, what):
    """A value that is no number in W[u], in H[i] and in a trial's row, one slot each among ordinary ones: the counts, the
    chosen trials and every bit agree, and the rows of the bad slots keep their bits."""
    k, n, m = 5, 30, 4
    W, H, u, i, items, member = _random_case(k, n, m, 17)
    member[:] = False
    u[:] = np.arange(n) % (ROWS - 7)
    i[:] = np.arange(n) % 11
    items[:] = 11 + (np.arange(n * m).reshape(n, m) % 9)
    W[ROWS - 1, 2] = what          # slot 0: its user
    H[COLS - 1, 1] = what          # slot 1: its positive item
    H[COLS - 2, k - 1] = what      # slot 2: its second trial (and slot 3: all four)
    u[0], i[1] = ROWS - 1, COLS - 1
    items[2, 1] = COLS - 2
    items[3, :] = COLS - 2
    W[u[2], k - 1] = W[u[3], k - 1] = 1.0  # the sign of that trial's score is the sign of `what`
    ref = _check(mfx, W, H, u, i, items, member, 0.05, 0.01)
    for loss in MODES:
        Wr, Hr, st, jr, tr = ref[loss]
        assert st[2] >= 2, (loss, st)                       # slots 0 and 1 are bad in both modes
        assert same_bits(Wr[ROWS - 1], W[ROWS - 1]) and same_bits(Hr[COLS - 2:], H[COLS - 2:])
        assert not same_bits(Wr, W)
    assert ref["warp"][4][0] == 0 and ref["warp"][4][1] == 0  # s_i is not finite: no trial is chosen
    # slot 3, whose trials all score `what`: hardest must take one (bad: x is no number); WARP passes over -Inf (skipped)
    assert ref["bpr"][4][3] == 1 and ref["bpr"][2][2] >= 3
    assert ref["warp"][4][3] == (0 if what == -np.inf else 1) and (ref["warp"][2][2] >= 3 or what == -np.inf)
    if what != np.inf:
        assert ref["bpr"][4][2] != 2                          # a NaN or -Inf score does not win against numbers


def test_crafted_trials_warp_only(mfx):
    k = 4
    W = np.zeros((ROWS, k), F)
    H = np.zeros((COLS, k), F)
    # user 0: s_i = 1 for item 0 (a margin of exactly 1 against the zero row of item 9: no violation) and s_i = 1 - 2^-24
    # for item 1 (the next fp32 below 1: a violation); every product and sum is exact
    W[0, :2] = [1.0, 2.0 ** -24]
    H[0, :2] = [1.0, 0.0]
    H[1, :2] = [1.0, -1.0]
    # user 1: s_i = 5 for item 2; items 3 (score 1, margin 4) and 4 (score 4.5, margin 0.5)
    W[1, 0] = 1.0
    H[2, 0], H[3, 0], H[4, 0] = 5.0, 1.0, 4.5
    m = 5
    u = np.array([0, 0, 1, 1, 1])
    i = np.array([0, 1, 2, 2, 2])
    items = np.array([[9] * m, [9] * m, [3, 3, 3, 3, 4], [3] * m, [4, 3, 3, 3, 3]])
    member = np.zeros(items.shape, bool)
    member[4, 0] = True  # the violator is in the row: passed over, and no other violates
    rw = np.array([1.0, 0.5, 0.25, 0.125, 3.0], F)
    ref = _check(mfx, W, H, u, i, items, member, 0.05, 0.01, rw, losses=("warp",))["warp"]
    assert ref[4].tolist() == [0, 1, m, 0, 0] and ref[2] == [5, 3, 0, 2]
    assert ref[3][1] == 9 and ref[3][2] == 4
    assert not same_bits(ref[1][4], H[4]) and same_bits(ref[1][3], H[3])

    # a weight of 0 still counts the slot: regularisation alone moves its rows
    ref = _check(mfx, W, H, u, i, items, member, 0.05, 0.01, np.zeros(m, F), losses=("warp",))["warp"]
    assert ref[2] == [5, 3, 0, 2]
    lr, lam = F(0.05), F(0.01)
    assert same_bits(ref[1][4], H[4] + lr * (F(0) - (lam * F(1)) * H[4]))
    assert same_bits(ref[0][1], W[1] + lr * (F(0) - (lam * F(1)) * W[1]))

    # a table entry of 100 makes the term g * W[u][0] = 100 >= 64: bad, nothing moves
    big = rw.copy()
    big[m - 1] = 100.0
    ref = _check(mfx, W, H, u, i, items, member, 0.05, 0.01, big, losses=("warp",))["warp"]
    assert ref[2] == [5, 3, 1, 1] and ref[4].tolist() == [0, 1, m, 0, 0]
    assert same_bits(ref[1][4], H[4]) and same_bits(ref[0][1], W[1])


def test_crafted_trials_hardest_only(mfx):
    k = 1  # (a second term +0 * +0 would turn the -0 into +0)
    W = np.zeros((ROWS, k), F)
    H = np.zeros((COLS, k), F)
    tiny = F(2.0 ** -100)
    W[0, 0] = tiny
    H[1, 0], H[2, 0] = -tiny, tiny     # the products underflow: scores -0 and +0, a tie
    H[3, 0] = np.nan                   # for user 1 a NaN score, which must lose to the -Inf of item 4
    H[4, 0] = -np.inf
    W[1, 0] = 1.0
    H[5, 0] = 0.5
    u = np.array([0, 0, 1, 1])
    i = np.array([5, 5, 5, 5])
    items = np.array([[1, 2, 1], [2, 1, 2], [3, 4, 3], [3, 3, 3]])
    sc = nx.trial_scores(W, H, u, i, items)[1]
    assert bits(sc[0]).tolist() == [0x80000000, 0, 0x80000000] and bits(sc[1]).tolist() == [0, 0x80000000, 0]
    ref = _check(mfx, W, H, u, i, items, None, 0.05, 0.01, losses=("bpr",))["bpr"]
    assert ref[4].tolist() == [1, 1, 2, 1] and ref[3][:3].tolist() == [1, 2, 4]
    assert ref[2] == [4, 0, 2, ref[2][3]]  # (the chosen -Inf and NaN rows make x no number: bad)


def test_order_of_the_slots_plays_no_part(mfx):
    k, n, m = 65, 1000, 9
    W, H, u, i, items, member = _random_case(k, n, m, 77)
    rw = table(m)
    for loss in MODES:
        a = mfx.bpr_apply_neg(W, H, u, i, items, 0.05, 0.01, loss=loss, member=member, rank_weight=rw)
        for seed in (1, 2):
            o = np.random.default_rng(seed).permutation(n)
            b = mfx.bpr_apply_neg(W, H, u[o], i[o], items[o], 0.05, 0.01, loss=loss, member=member[o], rank_weight=rw)
            assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and counts(a[2]) == counts(b[2])
            assert np.array_equal(a[3][o], b[3]) and np.array_equal(a[4][o], b[4])


def test_apply_neg_refuses_ids_out_of_range(mfx):
    W, H = bx.initial_factors(ROWS, COLS, 8, 0)
    z, it = np.zeros(70, np.uint32), np.zeros((70, 3), np.uint32)
    for which, bad in ((0, ROWS), (1, COLS), (2, COLS)):
        args = [z.copy(), z.copy(), it.copy()]
        if which == 2:
            args[2][66, 2] = bad
            args[2][69, 0] = bad + 5
        else:
            args[which][66] = bad
            args[which][69] = bad + 5
        for loss in MODES:
            with pytest.raises(mfx.MfxError, match="slot 66"):
                mfx.bpr_apply_neg(W, H, *args, 0.05, 0.01, loss=loss)
    Wg, Hg, rep, j, t = mfx.bpr_apply_neg(W, H, z[:0], z[:0], it[:0], 0.05, 0.01)
    assert same_bits(Wg, W) and same_bits(Hg, H) and counts(rep) == [0, 0, 0, 0] and j.size == t.size == 0


# ------------------------------------------------------------------------------------------------ the solver
def _params(mfx, k, lam):
    p = mfx.parameter()
    p.k, p.lambda_ = k, lam
    return p


@pytest.mark.parametrize("loss", ["bpr", "warp"])
@pytest.mark.parametrize("m", [1, 9, 65])
@pytest.mark.parametrize("batch", [1, 64, 100, 1 << 20])
@pytest.mark.parametrize("k", [8, 65])
def test_solver_step_is_the_operator_on_the_sampled_trials(mfx, R, k, batch, m, loss):
    """Three epochs, one steps(1) at a time, beside bpr_apply_neg on bpr_trials of the same slots: the counts of every step,
    the factors at every step (batch = 1: at every 50th step and at the end of every epoch), and trial_stats at the end."""
    lr, lam, seed = 0.05, 0.01, 21
    nnz = R.nnz
    W, H = bx.initial_factors(R.rows, R.cols, k, 4)
    W, H = W * F(8.0), H * F(8.0)
    rw = table(m)
    s = mfx.BprSolver(R, _params(mfx, k, lam), lr, batch, seed=seed, negatives=m, loss=loss, rank_weight=rw)
    s.set_factors(W, H)
    pos, none, tsum = 0, 0, 0
    for epoch in range(3):
        plan = bx.epoch_steps(nnz, batch, pos)
        for n_step, (first, cnt) in enumerate(plan):
            u, i, items, member = mfx.bpr_trials(R, seed, first, cnt, m)
            W, H, want, j, t = mfx.bpr_apply_neg(W, H, u, i, items, lr, lam, loss=loss, member=member, rank_weight=rw)
            none += int((t == 0).sum())
            tsum += int(t.sum())
            got = s.steps(1)
            assert counts(got) == counts(want) and got["slots"] == cnt
            pos += cnt
            assert s.position() == pos
            if batch > 1 or n_step % 50 == 0 or n_step == len(plan) - 1:
                Ws, Hs = s.get_factors()
                assert same_bits(Ws, W) and same_bits(Hs, H), (epoch, n_step)
    assert pos == 3 * nnz
    assert s.trial_stats() == {"none_chosen": none, "chosen_trial_sum": tsum}
    s.close()


def test_one_negative_is_the_existing_solver(mfx, R):
    from mfx import api
    k, batch, lr, lam, seed = 8, 100, 0.05, 0.01, 33
    W0, H0 = bx.initial_factors(R.rows, R.cols, k, 6)

    def run(make):
        s = make()
        s.set_factors(W0, H0)
        reps = s.iterate(2)
        out = s.get_factors(), [counts(r) for r in reps], s.trial_stats()
        s.close()
        return out

    old = run(lambda: mfx.BprSolver(R, _params(mfx, k, lam), lr, batch, seed=seed))
    new = run(lambda: mfx.BprSolver(R, _params(mfx, k, lam), lr, batch, seed=seed, negatives=1, loss="bpr"))
    # hardest of one through mfx_bpr_create_neg: the trials kernel runs and must change nothing
    hard = run(lambda: mfx.BprSolver(R, _params(mfx, k, lam), lr, batch, seed=seed, negatives=1, loss="bpr", rank_weight=[0.0]))
    Wr, Hr, st, _ = bx.train(R, W0, H0, lr, lam, batch, seed, 2)
    skipped = int(st[:, 1].sum())
    for got in (old, new, hard):
        assert same_bits(got[0][0], Wr) and same_bits(got[0][1], Hr) and got[1] == st.tolist()
        assert got[2] == {"none_chosen": skipped, "chosen_trial_sum": 2 * R.nnz - skipped}
    h = C.c_void_p()
    csx, cp = api._csx(R), _params(mfx, k, lam).to_c()
    lib = mfx.lib()
    assert lib.mfx_bpr_create_neg(C.byref(h), C.byref(csx), C.byref(cp), lr, batch, seed, 0, 1, None, 0) == 0  # the uniform mode
    stats = (C.c_int64 * 8)()
    assert lib.mfx_bpr_set_factors(h, api._vp(W0), api._vp(H0), 0) == 0
    assert lib.mfx_bpr_epochs(h, 2, stats, None) == 0 and list(stats) == st.ravel().tolist()
    Wu, Hu = np.empty_like(W0), np.empty_like(H0)
    assert lib.mfx_bpr_get_factors(h, api._vp(Wu), api._vp(Hu), 0) == 0 and same_bits(Wu, Wr) and same_bits(Hu, Hr)
    assert lib.mfx_bpr_destroy(h) == 0


def _device_arrays(R):
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a)).to(dev)
    return {"rows": R.rows, "cols": R.cols, "csr_row_ptr": t(R.csr_row_ptr), "csr_col_idx": t(R.csr_col_idx),
            "csr_val": t(R.csr_val), "csc_col_ptr": t(R.csc_col_ptr), "csc_row_idx": t(R.csc_row_idx), "csc_val": t(R.csc_val)}


@pytest.mark.parametrize("loss", ["bpr", "warp"])
def test_same_bits_twice_other_seed_differs_spaces_agree_iterate_matches_the_reference(mfx, R, loss):
    k, batch, m, lr, lam = 12, 64, 6, 0.05, 0.01
    rw = table(m)

    def run(seed, device_arrays=None):
        s = mfx.BprSolver(R if device_arrays is None else None, _params(mfx, k, lam), lr, batch, seed=seed,
                          device_arrays=device_arrays, init_seed=8, negatives=m, loss=loss, rank_weight=rw)
        part = s.steps(2)
        assert part["slots"] == 2 * batch and s.position() == 2 * batch
        reps = s.iterate(2)  # the first finishes the started epoch
        assert [r["slots"] for r in reps] == [R.nnz - 2 * batch, R.nnz]
        W, H = s.get_factors()
        ts = s.trial_stats()
        s.close()
        return W, H, [counts(part)] + [counts(r) for r in reps], ts

    a, b, c = run(5), run(5), run(5, device_arrays=_device_arrays(R))
    for other in (b, c):
        assert same_bits(a[0], other[0]) and same_bits(a[1], other[1]) and a[2] == other[2] and a[3] == other[3]
    d = run(6)
    assert not same_bits(a[0], d[0]) and not same_bits(a[1], d[1])
    W0, H0 = bx.initial_factors(R.rows, R.cols, k, 8)
    Wr, Hr, st, pos, ts = nx.train_neg(R, W0, H0, lr, lam, batch, 5, 2, m, MODES[loss], rank_weight=rw)
    assert pos == 2 * R.nnz
    assert same_bits(a[0], Wr) and same_bits(a[1], Hr)
    assert st[0].tolist() == (np.array(a[2][0]) + np.array(a[2][1])).tolist() and st[1].tolist() == a[2][2]
    assert a[3] == {"none_chosen": int(ts[0]), "chosen_trial_sum": int(ts[1])}


def test_the_default_rank_weights_are_the_table_of_the_library(mfx, R):
    k, batch, m = 8, 100, 5
    out = []
    for rw in (None, mfx.bpr_rank_weights(R.cols, m)):
        s = mfx.BprSolver(R, _params(mfx, k, 0.01), 0.05, batch, seed=2, init_seed=3, negatives=m, loss="warp", rank_weight=rw)
        reps = s.iterate(1)
        out.append((s.get_factors(), counts(reps[0])))
        s.close()
    assert same_bits(out[0][0][0], out[1][0][0]) and same_bits(out[0][0][1], out[1][0][1]) and out[0][1] == out[1][1]
    W, H = factors(k, 1)
    u, i, items, member = mfx.bpr_trials(bx.small_matrix(rows=ROWS, cols=COLS, nnz=300), 4, 0, 64, m)
    a = mfx.bpr_apply_neg(W, H, u, i, items, 0.05, 0.01, loss="warp", member=member)
    b = mfx.bpr_apply_neg(W, H, u, i, items, 0.05, 0.01, loss="warp", member=member, rank_weight=mfx.bpr_rank_weights(COLS, m))
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and not same_bits(a[0], W)


def test_create_neg_refuses_broken_rows_and_bad_modes(mfx, R):
    row = int(np.argmax(np.diff(R.csr_row_ptr.astype(np.int64)) >= 3))
    lo = int(R.csr_row_ptr[row])
    B = R.copy()
    B.csr_col_idx[lo], B.csr_col_idx[lo + 1] = R.csr_col_idx[lo + 1], R.csr_col_idx[lo]
    with pytest.raises(mfx.MfxError, match=f"row {row} "):
        mfx.BprSolver(B, _params(mfx, 8, 0.01), 0.05, 64, negatives=4)
    for kw in (dict(negatives=0), dict(negatives=1025), dict(negatives=3, loss="warp", rank_weight=[1.0, -1.0, 0.0]),
               dict(negatives=2, loss="warp", rank_weight=[1.0, float("nan")])):
        with pytest.raises(mfx.MfxError, match="mfx_bpr_create_neg"):
            mfx.BprSolver(R, _params(mfx, 8, 0.01), 0.05, 64, **kw)


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("loss,m,lr,epochs", [("warp", 16, 0.01, 10), ("bpr", 8, 0.05, 5)])
def test_planted_clusters_recommend_end_to_end(mfx, loss, m, lr, epochs):
    """The planted clusters (bpr_exact.planted_clusters) at k = 32, batch 1 024, lambda 0.01 with the default rank weights:
    the settings at which the exact reference reaches 0.9665 (WARP) and 1.0 (hardest of 8) in tests/test_bpr_neg_host.py.  The
    top-10 lists (training items excluded) must find the held-out item for at least 90 % of the users."""
    P = bx.planted_clusters()
    s = mfx.BprSolver(P, _params(mfx, 32, 0.01), lr, 1024, seed=7, init_seed=5, negatives=m, loss=loss)
    reps, ts = [], []
    for _ in range(epochs):
        reps += s.iterate(1)
        ts.append(s.trial_stats())
    W, H = s.get_factors()
    s.close()
    assert all(r["slots"] == P.nnz and r["bad"] == 0 for r in reps)
    print("auc per epoch:", [round(r["auc"], 4) for r in reps])
    print("trial stats after each epoch:", ts)
    top, _ = mfx.recommend(W, H, 1, 10, exclude=P)
    mt = mfx.topn_metrics(top, mfx.test_data_of(P))
    print("metrics:", mt)
    assert mt["users"] == P.rows
    assert mt["hr"] >= 0.9, mt
