"""Catalogue ranks of (user, item) pairs and full-rank evaluation (mfx_rec_rank, mfx_rec_evaluate; Recommender.rank_of,
Recommender.evaluate) checked bit for bit against the exact reference of tests/rank_exact.py: ranks, score bits and
eligible counts of every pair of a catalogue, against the reference and against the handle's own query, under
exclusion rows, item filters, ties, item slices, batch order and memory space; the metrics against topn_metrics on
query lists and a numpy fp64 MRR / AUC."""
import ctypes as C

import numpy as np
import pytest

from rank_exact import expected_ranks, mrr_auc
from rec_exact import PAD, chain_scores, eligible_mask, expected_topn

pytestmark = pytest.mark.gpu

F32 = np.float32
MFX_ERR_INVALID = -1  # include/mfx.h
ROWS, COLS = 130, 997  # one full workgroup and a two-slot one; 31 full tiles and one of 5 items


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1, m.lib().mfx_last_error()
    return m


def host(a):
    """numpy view of a result (torch int32 tensors become their uint32 bits)."""
    if not isinstance(a, np.ndarray):
        a = a.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def all_pairs(rows, cols):
    return np.divmod(np.arange(rows * cols), cols)


def assert_exact(got, want, what):
    names = ("ranks", "score bits", "n_eligible")
    for g, w, name in zip(got, want, names):
        g, w = host(g), np.asarray(w)
        if name == "score bits":
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        bad = np.nonzero(g != w)[0]
        if bad.size:
            p = bad[:6]
            pytest.fail(f"{what}: {bad.size} of {g.size} {name} differ; pairs {p.tolist()}: {g[p].tolist()} vs {w[p].tolist()}")


def regime_factors(regime, rows, cols, k, seed):
    rng = np.random.default_rng(seed)
    W = rng.standard_normal((rows, k))
    H = rng.standard_normal((cols, k))
    if regime == "scaled":            # per-t scales 2^-20 .. 2^20: the rounding of each step depends on the order
        W *= 2.0 ** rng.integers(-20, 21, k)
        H *= 2.0 ** rng.integers(-20, 21, k)
    elif regime == "subnormal":       # products around 2^-136: subnormal W and H entries, subnormal sums, +-0
        ew = rng.integers(-134, -2, k)
        W *= 2.0 ** ew
        H *= 2.0 ** (-136 - ew + rng.integers(-16, 8, (cols, k)))
        W[::7] *= 2.0 ** -40          # every product underflows: the score is a signed zero
    elif regime == "huge":            # products near and beyond FLT_MAX: +-inf scores, inf - inf = NaN
        for t in {0, k // 2, k - 1}:
            W[:, t] *= 1e19 * 2.0 ** rng.integers(0, 4, rows)
            H[:, t] *= np.where(rng.random(cols) < 0.4, 1e20, 1.0)
    return W.astype(F32), H.astype(F32)


def exclusion(mfx, rng, rows, cols, n_top, S=None):
    """RatingData of mixed exclusion rows, six kinds cycling within every wave of 32 users: empty; about half the
    items; the user's own top 2 n_top items by S [rows][cols] (without S: a random half instead); every item but
    n_top / 2; every item; a random quarter of the items with duplicate indices."""
    r, c = [], []
    top = None
    if S is not None:
        top = expected_topn(S[2::6], True, 2 * n_top)[0]
    for u in range(rows):
        kind = u % 6
        if kind == 0:
            ids = np.zeros(0, np.int64)
        elif kind == 1 or (kind == 2 and top is None):
            ids = np.nonzero(rng.random(cols) < 0.5)[0]
        elif kind == 2:
            ids = top[u // 6]
            ids = np.sort(ids[ids != PAD].astype(np.int64))
        elif kind == 3:
            ids = np.setdiff1d(np.arange(cols), rng.choice(cols, n_top // 2, replace=False))
        elif kind == 4:
            ids = np.arange(cols)
        else:
            ids = rng.choice(cols, cols // 4, replace=False)
            ids = np.sort(np.repeat(ids, rng.integers(1, 4, ids.size)))
        r.append(np.full(ids.size, u, np.int64))
        c.append(ids)
    r, c = np.concatenate(r), np.concatenate(c)
    return mfx.dataset.from_coo(rows, cols, r.astype(np.uint32), c.astype(np.uint32), np.ones(r.size, F32))


def positions_of_query(items):
    """pos [U, cols-or-more]: the position of every returned item in its user's list, PAD for the absent ones."""
    U = items.shape[0]
    pos = np.full((U, COLS), PAD, np.uint32)
    for u in range(U):
        real = items[u] != PAD
        pos[u, items[u, real]] = np.nonzero(real)[0]
    return pos


# ------------------------------------------------------------------------------------------------ a. score and rank bits
@pytest.mark.parametrize("k", [1, 2, 3, 17, 64, 65, 129, 257, 1024])
@pytest.mark.parametrize("regime", ["normal", "scaled", "subnormal", "huge"])
def test_rank_score_and_count_bits_of_every_pair(mfx, regime, k):
    W, H = regime_factors(regime, ROWS, COLS, k, seed=1000 * k + len(regime))
    if regime == "huge":
        # An fma adds the exact product, so a chain of finite factors overflows to +-inf and stays there: it never meets
        # inf - inf.  NaN keys need infinite entries: 0 * inf, and (+inf) + (-inf) where an item has both signs.
        H[5::97, 0], H[11::97, k - 1] = np.inf, -np.inf
        W[3::13, 0], W[4::13, k - 1] = 0.0, 0.0
        if k > 1:
            H[17::97, 0], H[17::97, k - 1] = np.inf, np.inf
    uu, ii = all_pairs(ROWS, COLS)
    S = chain_scores(W, H, np.arange(ROWS))
    want = expected_ranks(S, True, uu, ii)
    if regime == "huge":   # the NaN, +inf and -inf branches are taken
        t = want[1]
        assert (np.isnan(t) & (want[0] == PAD)).any() and np.isposinf(t).any() and np.isneginf(t).any()
        assert (want[0][np.isinf(t)] != PAD).all()
    for layout in (1, 0):
        Wl, Hl = (W, H) if layout == 1 else (np.ascontiguousarray(W.T), np.ascontiguousarray(H.T))
        with mfx.Recommender(Wl, Hl, layout) as r:
            got = r.rank_of(uu, ii)
            assert_exact(got, want, f"{regime} k={k} layout={layout}")
            if layout == 1:  # the handle's own complete lists (cols < 1024): every position, every absent item
                pos = positions_of_query(r.query(1024)[0])
                assert np.array_equal(got[0].reshape(ROWS, COLS), pos), f"{regime} k={k}: rank_of != position in query"


# ------------------------------------------------------------------------------------------------ b. exclusion
@pytest.fixture(scope="module")
def base_case():
    k = 17
    W, H = regime_factors("normal", ROWS, COLS, k, seed=4242)
    return W, H, chain_scores(W, H, np.arange(ROWS))


def test_exclusion_rows_of_every_kind(mfx, base_case):
    W, H, S = base_case
    ex = exclusion(mfx, np.random.default_rng(20), ROWS, COLS, 20, S)
    uu, ii = all_pairs(ROWS, COLS)
    el = eligible_mask(ex, np.arange(ROWS), COLS)
    want = expected_ranks(S, el, uu, ii)
    with mfx.Recommender(W, H, 1, exclude=ex) as r:
        got = r.rank_of(uu, ii)
        assert_exact(got, want, "exclusion")
        pos = positions_of_query(r.query(1024)[0])
    assert np.array_equal(got[0].reshape(ROWS, COLS), pos)
    n_el = got[2].reshape(ROWS, COLS)
    assert np.all(n_el[4::6] == 0) and np.all(got[0].reshape(ROWS, COLS)[4::6] == PAD)      # all excluded
    assert np.all(n_el[3::6] == 10) and np.all(n_el[0::6] == COLS)
    excl = ~el.reshape(-1)
    assert excl.any() and np.all(got[0][excl] == PAD)                                      # an excluded target: PAD ...
    assert np.array_equal(got[1][excl].view(np.uint32), S.reshape(-1)[excl].view(np.uint32))  # ... and still its score


# ------------------------------------------------------------------------------------------------ c. item filter
@pytest.mark.parametrize("with_ex", [False, True])
def test_item_filter(mfx, base_case, with_ex):
    W, H, S = base_case
    rng = np.random.default_rng(31 + with_ex)
    ex = exclusion(mfx, rng, ROWS, COLS, 20, S) if with_ex else None
    uu, ii = all_pairs(ROWS, COLS)
    el = eligible_mask(ex, np.arange(ROWS), COLS)
    plain = expected_ranks(S, el, uu, ii)
    with mfx.Recommender(W, H, 1, exclude=ex) as r:
        assert_exact(r.rank_of(uu, ii), plain, "before any filter")
        for name, keep in (("half", rng.random(COLS) < 0.5), ("all kept", np.ones(COLS, bool)), ("all dropped", np.zeros(COLS, bool))):
            r.set_item_filter(keep)
            want = expected_ranks(S, el & keep[None, :], uu, ii)
            got = r.rank_of(uu, ii)
            assert_exact(got, want, f"filter {name}, exclusion {with_ex}")
            if name == "all dropped":
                assert np.all(got[0] == PAD) and np.all(got[2] == 0)
            if name == "half":
                assert np.array_equal(got[0].reshape(ROWS, COLS), positions_of_query(r.query(1024)[0]))
        r.set_item_filter(None)
        assert_exact(r.rank_of(uu, ii), plain, "filter removed")


# ------------------------------------------------------------------------------------------------ d. ties
def test_ties_are_decided_by_item_id(mfx):
    k = 6
    rng = np.random.default_rng(99)
    # factors from a few values: thousands of equal scores.  Users 100.. have entries of 2^-100 against items of
    # 2^-60: every product underflows to a signed zero; users 120.. are all zero
    W = (rng.integers(-2, 3, (ROWS, k)) * 2.0 ** 60).astype(F32)
    H = (rng.integers(-2, 3, (5, k))[rng.integers(0, 5, COLS)] * 2.0 ** -60).astype(F32)
    W[100:120] = (rng.choice([-1.0, 1.0], (20, k)) * 2.0 ** -100).astype(F32)
    W[120:] = 0
    S = chain_scores(W, H, np.arange(ROWS))
    assert np.all(S[100:] == 0) and np.signbit(S[100:120]).any() and not np.signbit(S[100:120]).all()
    assert max(len(np.unique(S[u])) for u in range(100)) <= 60
    uu, ii = all_pairs(ROWS, COLS)
    ex = exclusion(mfx, rng, ROWS, COLS, 20, S)
    for e in (ex, None):
        want = expected_ranks(S, eligible_mask(e, np.arange(ROWS), COLS), uu, ii)
        with mfx.Recommender(W, H, 1, exclude=e) as r:
            assert_exact(r.rank_of(uu, ii), want, f"ties, exclusion {e is not None}")
    assert np.array_equal(want[0].reshape(ROWS, COLS)[120], np.arange(COLS))  # all-zero user, no exclusion row: item order


# ------------------------------------------------------------------------------------------------ e. independence
def test_batch_order_slices_and_memory_space_do_not_matter(mfx):
    import torch
    rows, cols, k = 150, 6007, 8
    rng = np.random.default_rng(6007)
    W = rng.standard_normal((rows, k)).astype(F32)
    H = rng.standard_normal((cols, k)).astype(F32)
    H[3000:3100] = H[10:110]          # ties across slices
    S = chain_scores(W, H, np.arange(rows))
    ex = exclusion(mfx, rng, rows, cols, 20, S)
    # user 0: 997 targets; users 1 .. 20: 5; users 21 .. 100: 1; the rest none
    uu = np.concatenate([np.zeros(997, np.int64), np.repeat(np.arange(1, 21), 5), np.arange(21, 101)])
    ii = np.concatenate([rng.choice(cols, 997, replace=False), rng.integers(0, cols, 100), rng.integers(0, cols, 80)])
    ii[-1] = cols - 1
    want = expected_ranks(S, eligible_mask(ex, np.arange(rows), cols), uu, ii)
    perm = rng.permutation(np.concatenate([np.arange(uu.size), rng.integers(0, uu.size, 300)]))  # shuffled, with repeats
    with mfx.Recommender(W, H, 1, exclude=ex) as r:
        base = r.rank_of(uu, ii, item_slices=1)
        assert_exact(base, want, "slices=1")
        for sl in (0, 3, 7):
            assert_exact(r.rank_of(uu, ii, item_slices=sl), base, f"slices={sl}")
            assert_exact(r.rank_of(uu[perm], ii[perm], item_slices=sl), [b[perm] for b in base], f"permuted, slices={sl}")
        one = r.rank_of(uu[:1], ii[:1])
        assert_exact(one, [b[:1] for b in base], "a batch of one pair")
        tu = torch.from_numpy(uu[perm].astype(np.uint32).view(np.int32)).cuda()
        ti = torch.from_numpy(ii[perm].astype(np.uint32).view(np.int32)).cuda()
        dev = r.rank_of(tu, ti)
        torch.cuda.synchronize()
        assert all(t.is_cuda for t in dev) and dev[0].dtype == torch.int32 and dev[2].dtype == torch.int32
        assert_exact(dev, [b[perm] for b in base], "device tensors")
        assert_exact(r.rank_of(uu, ii, on_device=True), base, "on_device")
    with mfx.Recommender(np.ascontiguousarray(W.T), np.ascontiguousarray(H.T), 0, exclude=ex) as r:
        assert_exact(r.rank_of(uu[perm], ii[perm]), [b[perm] for b in base], "layout 0")
    with mfx.Recommender(torch.from_numpy(W).cuda(), torch.from_numpy(H).cuda(), 1, exclude=ex) as r:
        assert_exact(r.rank_of(uu, ii), base, "device factors")


# ------------------------------------------------------------------------------------------------ f. evaluate
@pytest.fixture(scope="module")
def eval_case(mfx):
    """Planted clusters: user u and item i of the same cluster score high.  Implicit training entries are the exclusion;
    the held-out set has repeats and values on both sides of min_rating = 1."""
    rows, cols, k, ncl = 300, 1500, 16, 12
    rng = np.random.default_rng(300)
    cu, ci = rng.integers(0, ncl, rows), rng.integers(0, ncl, cols)
    C0 = rng.standard_normal((ncl, k))
    W = (C0[cu] + 0.4 * rng.standard_normal((rows, k))).astype(F32)
    H = (C0[ci] + 0.4 * rng.standard_normal((cols, k))).astype(F32)
    tr_r, tr_c, te_r, te_c, te_v = [], [], [], [], []
    for u in range(rows):
        own = np.nonzero(ci == cu[u])[0]
        seen = rng.choice(own, min(len(own), 12), replace=False)
        n_tr = len(seen) - 4
        tr = np.concatenate([seen[:n_tr], rng.choice(cols, 10)])
        te = np.concatenate([seen[n_tr:], rng.choice(cols, 2)])
        if u == 7:      # no eligible target: every target is also a training entry
            tr = np.concatenate([tr, te])
        if u == 8:      # no negatives: everything but the targets is excluded
            tr = np.setdiff1d(np.arange(cols), te)
        if u % 50 == 9:  # no test entry at all
            te = te[:0]
        tr_r.append(np.full(tr.size, u)); tr_c.append(tr)
        te = np.concatenate([te, te[:2]])                              # repeated test entries
        v = rng.choice([0.5, 1.0, 2.0], te.size).astype(F32)
        if u % 50 == 10:
            v[:] = 0.5                                                  # nothing reaches min_rating
        if u in (7, 8):
            v[:] = 2.0
        te_r.append(np.full(te.size, u)); te_c.append(te); te_v.append(v)
    cat = lambda x, dt: np.concatenate(x).astype(dt)
    tr_r, tr_c = cat(tr_r, np.uint32), cat(tr_c, np.uint32)
    ex = mfx.dataset.from_coo(rows, cols, tr_r, tr_c, np.ones(tr_r.size, F32))
    T = mfx.TestData(rows, cols, cat(te_r, np.uint32), cat(te_c, np.uint32), cat(te_v, F32))
    S = chain_scores(W, H, np.arange(rows))
    return W, H, ex, T, S


def test_evaluate_against_query_lists_and_the_numpy_reference(mfx, eval_case):
    W, H, ex, T, S = eval_case
    rows, cols = S.shape
    min_rating = 1.0
    m = T.test_val >= min_rating
    pairs = np.unique(np.stack([T.test_row[m], T.test_col[m]], 1).astype(np.int64), axis=0)
    assert pairs.shape[0] < m.sum() < T.nnz                            # repeats and entries below min_rating are there
    el = eligible_mask(ex, np.arange(rows), cols)
    ranks, _, n_el = expected_ranks(S, el, pairs[:, 0], pairs[:, 1])
    want_mrr, want_auc, want_users, want_auc_users = mrr_auc(pairs[:, 0], ranks, n_el)
    assert np.all(ranks[pairs[:, 0] == 7] == PAD) and np.all(n_el[pairs[:, 0] == 8] == (pairs[:, 0] == 8).sum())
    assert want_auc_users == want_users - 2 and 250 < want_users < rows
    cutoffs = (1, 10, 100, 5000)
    with mfx.Recommender(W, H, 1, exclude=ex) as r:
        ev = r.evaluate(T, cutoffs=cutoffs, min_rating=min_rating)
        assert ev["cutoffs"] == list(cutoffs)
        for c, n in enumerate(cutoffs[:3]):
            ref = mfx.topn_metrics(r.query(n)[0], T, min_rating=min_rating)
            for name in ("hr", "precision", "recall", "ndcg"):
                print(n, name, ev[name][c], ref[name])
                assert abs(ev[name][c] - ref[name]) <= 1e-12, (n, name, ev[name][c], ref[name])
            assert ev["users"] == ref["users"] == want_users
        got_r, _, got_n = r.rank_of(pairs[:, 0], pairs[:, 1])
        assert np.array_equal(got_r, ranks) and np.array_equal(got_n, n_el)
        none = r.evaluate(T, cutoffs=(), min_rating=min_rating)
    print("mrr", ev["mrr"], want_mrr, "auc", ev["auc"], want_auc)
    assert abs(ev["mrr"] - want_mrr) <= 1e-12 and abs(ev["auc"] - want_auc) <= 1e-12
    assert ev["auc_users"] == want_auc_users and ev["users"] == want_users
    # N = 5000 > 1024 (and > cols): every eligible target is a hit, so recall is the eligible share of R_u
    users = np.unique(pairs[:, 0])
    share = np.array([np.mean(ranks[pairs[:, 0] == u] != PAD) for u in users])
    assert (share == 1).sum() > 200 and (share < 1).any()
    assert abs(ev["recall"][3] - share.mean()) <= 1e-12 and abs(ev["hr"][3] - np.mean(share > 0)) <= 1e-12
    with mfx.Recommender(W, H, 1) as r:                                 # no exclusion: every target eligible, recall exactly 1
        assert r.evaluate(T, cutoffs=(5000,), min_rating=min_rating)["recall"] == [1.0]
    assert none["hr"] == [] and none["users"] == want_users and abs(none["mrr"] - want_mrr) <= 1e-12


# ------------------------------------------------------------------------------------------------ g. refusals
def test_refusals_leave_the_handle_usable(mfx, base_case):
    W, H, S = base_case
    lib = mfx.lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    uu, ii = all_pairs(ROWS, COLS)
    want = expected_ranks(S, True, uu, ii)
    u = np.array([0, 5, ROWS - 1], np.uint32)
    i = np.array([0, 5, COLS - 1], np.uint32)
    ranks, scores, nel = np.zeros(3, np.uint32), np.zeros(3, F32), np.zeros(3, np.uint32)
    bad_u, bad_i = u.copy(), i.copy()
    bad_u[1], bad_i[2] = ROWS, COLS

    def rank(h, n=3, pu=u, pi=i, pr=ranks, space=0, slices=0):
        return lib.mfx_rec_rank(h, n, vp(pu), vp(pi), vp(pr) if pr is not None else None, vp(scores), vp(nel), space, slices)

    with mfx.Recommender(W, H, 1) as r:
        for word, rc in (("user id", lambda: rank(r.handle, pu=bad_u)), ("item id", lambda: rank(r.handle, pi=bad_i)),
                         ("ranks is NULL", lambda: rank(r.handle, pr=None)), ("item_slices", lambda: rank(r.handle, slices=-1)),
                         ("memory space", lambda: rank(r.handle, space=7))):
            code = rc()
            msg = lib.mfx_last_error().decode()
            assert code == MFX_ERR_INVALID and word in msg, (word, code, msg)
            assert_exact(r.rank_of(uu, ii), want, f"after the refusal of {word}")
        assert lib.mfx_rec_rank(r.handle, 0, None, None, None, None, None, 0, 0) == 0
        assert rank(r.handle) == 0
        sel = u.astype(np.int64) * COLS + i
        assert np.array_equal(ranks, want[0][sel]) and np.array_equal(nel, want[2][sel])
        assert np.array_equal(scores.view(np.uint32), want[1][sel].view(np.uint32))
