"""Diversity re-ranking (mfx_rec_diversify; Recommender.diversify, Recommender.query_diverse) checked bit for bit: items,
score bits, value bits (compared as uint32) and eligible counts against the exact reference of tests/diversify_exact.py
and against the handle's own query_candidates, under every rank path, both layouts, both metrics, both forms of the
selection kernel, exclusion rows, item filters, ties, special values, list lengths up to the limit, batch order and
memory space."""
import ctypes as C

import numpy as np
import pytest

from cand_exact import exclusion, random_lists, regime_factors
from diversify_exact import LazyGram, expected_diversify, item_gram
from rec_exact import PAD, chain_scores, eligible_mask, expected_topn
from sim_exact import COSINE, DOT, collinear_ramp

pytestmark = pytest.mark.gpu

F32 = np.float32
MFX_ERR_INVALID = -1  # include/mfx.h
ROWS, COLS = 70, 300
LIMIT = 2048          # candidates of one list
LDS_BUDGET = 65280    # bytes of LDS that form 1 may take (rec_diversify.hip)


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1, m.lib().mfx_last_error()
    return m


def kt_of(k):
    """The padded rank of the handle's rows (Recommender::create)."""
    steps = (k + 1) // 2
    kc = 1
    while kc < steps and kc < 64:
        kc *= 2
    return -(-steps // kc) * 2 * kc


def form1_fits(longest, k):
    """16 bytes per candidate of the longest list rounded up to 64, and its rows kt + 4 floats apart."""
    kt = kt_of(k)
    ks = kt + 4 if kt % 4 == 0 else kt
    return max(64, -(-longest // 64) * 64) * 16 + longest * ks * 4 <= LDS_BUDGET


def host(a):
    if not isinstance(a, np.ndarray):
        a = a.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def assert_exact(got, want, what, names=("items", "score bits", "value bits", "n_eligible")):
    assert len(got) == len(want) == len(names), (what, len(got), len(want))
    for g, w, name in zip(got, want, names):
        g, w = host(g), np.asarray(w)
        if name.endswith("bits"):
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        bad = np.argwhere(g != w)
        if bad.size:
            p = tuple(bad[:6].T)
            pytest.fail(f"{what}: {len(bad)} of {g.size} {name} differ; at {bad[:6].tolist()}: {g[p].tolist()} vs {w[p].tolist()}")


def check_forms(mfx, r, k, want, n_top, lists, what, **kw):
    """The call under form 0, 1 and 2 against `want`; form 1 is refused exactly where the rows do not fit."""
    ptr = np.asarray(host(lists[0]), np.int64)
    longest = int(np.diff(ptr).max()) if ptr.size > 1 else 0
    for form in (0, 1, 2):
        call = lambda: r.diversify(n_top, lists, canonical=True, return_values=True, return_counts=True, form=form, **kw)
        if form == 1 and not form1_fits(longest, k):
            with pytest.raises(mfx.MfxError, match="form 1"):
                call()
            continue
        assert_exact(call(), want, f"{what}, form {form}")


class Model:
    """Factors with their exact scores, item chains and the library's own inverse norms."""
    def __init__(self, mfx, W, H, lazy=False):
        self.W, self.H, self.k = W, H, H.shape[1]
        self.S = chain_scores(W, H, np.arange(W.shape[0]))
        self.G = LazyGram(H) if lazy else item_gram(H)
        with mfx.Recommender(W, H, 1) as r:
            r.similar_setup()
            self.c = r.item_norms()[1]      # (the rounding of 1 / sqrt is pinned by tests/test_gpu_similar.py)

    def want(self, ptr, idx, eligible, n_top, tradeoff, metric, users=None, S=None):
        S = self.S if S is None else S
        return expected_diversify(S if users is None else S[users], ptr, idx, eligible, self.G, n_top, tradeoff, metric, self.c)


@pytest.fixture(scope="module")
def base(mfx):
    W, H = regime_factors("normal", ROWS, COLS, 17, seed=1717)
    return Model(mfx, W, H)


def lengths_for(rng, n_top, nslots, longest):
    pool = np.minimum(np.array([0, 1, n_top - 1, n_top, n_top + 1, 63, 64, 65, 100, 129, 255, 257, COLS]), longest)
    return pool[np.arange(nslots) % pool.size][rng.permutation(nslots)]


# ------------------------------------------------------------------------------------------------ a. every rank path
@pytest.mark.parametrize("k", [1, 3, 37, 64, 65, 128, 200])
def test_every_rank_path_both_layouts_both_forms(mfx, k):
    W, H = regime_factors("normal", ROWS, COLS, k, seed=900 + k)
    m = Model(mfx, W, H)
    rng = np.random.default_rng(k)
    fit = max(L for L in range(1, COLS + 1) if form1_fits(L, k))     # the longest list form 1 takes at this k
    assert (fit < COLS) == (k >= 37)                                 # (from there on the long batch has form 1 refused)
    short = random_lists(rng, lengths_for(rng, 10, ROWS, fit), COLS)
    long_ = random_lists(rng, lengths_for(rng, 10, ROWS, COLS), COLS)
    for layout in (1, 0):
        Wl, Hl = (W, H) if layout == 1 else (np.ascontiguousarray(W.T), np.ascontiguousarray(H.T))
        with mfx.Recommender(Wl, Hl, layout) as r:
            for lists, metric, t in ((short, COSINE, 0.3), (long_, COSINE, 0.7), (short, DOT, 0.7), (long_, DOT, 0.3)):
                if layout == 0 and metric == DOT:
                    continue
                want = m.want(*lists, True, 10, t, metric)
                check_forms(mfx, r, k, want, 10, lists, f"k {k}, layout {layout}, metric {metric}, tradeoff {t}", tradeoff=t, metric=metric)


def test_rank_1024(mfx):
    rows, cols, k = 20, 96, 1024
    W, H = regime_factors("normal", rows, cols, k, seed=1024)
    m = Model(mfx, W, H)
    rng = np.random.default_rng(1024)
    assert form1_fits(15, k) and not form1_fits(16, k)
    with mfx.Recommender(W, H, 1) as r:
        for longest in (15, cols):
            lens = rng.integers(0, longest + 1, rows)
            lens[3] = longest
            lists = random_lists(rng, lens, cols)
            check_forms(mfx, r, k, m.want(*lists, True, 10, 0.5, COSINE), 10, lists, f"k 1024, lists up to {longest}", tradeoff=0.5)


# ------------------------------------------------------------------------------------------------ b. tradeoff, metric, n_top
@pytest.mark.parametrize("metric", [DOT, COSINE])
def test_tradeoffs_and_list_widths(mfx, base, metric):
    rng = np.random.default_rng(5 + metric)
    nslots = 16
    lists = random_lists(rng, lengths_for(rng, 10, nslots, 200), COLS)
    users = rng.permutation(ROWS)[:nslots]
    with mfx.Recommender(base.W, base.H, 1) as r:
        for t in (0.0, 0.3, 0.7, 1.0):
            for n_top in (1, 10, 128):
                want = base.want(*lists, True, n_top, t, metric, users)
                check_forms(mfx, r, base.k, want, n_top, lists, f"metric {metric}, tradeoff {t}, n_top {n_top}", users=users, tradeoff=t,
                            metric=metric)
        times = r.diversify_times()
        assert set(times) == {"check", "relevance", "select"} and all(v > 0 for v in times.values())


# ------------------------------------------------------------------------------------------------ c. list shapes
def test_empty_single_and_padded_lists(mfx, base):
    rng = np.random.default_rng(77)
    ex = exclusion(mfx, rng, ROWS, COLS, 10, base.S)       # every sixth user: all items excluded, or all but five
    el = eligible_mask(ex, np.arange(ROWS), COLS)
    lens = np.array([0, 1, 2, 9, 10, 11, 30] * 10)
    lists = random_lists(rng, lens, COLS)
    with mfx.Recommender(base.W, base.H, 1, exclude=ex) as r:
        want = base.want(*lists, el, 10, 0.5, COSINE)
        assert (want[3] == 0).sum() > 10 and ((want[3] > 0) & (want[3] < 10)).sum() > 10 and (want[0] == PAD).any()
        check_forms(mfx, r, base.k, want, 10, lists, "short lists under exclusion", tradeoff=0.5)
        none = (np.zeros(ROWS + 1, np.uint32), np.zeros(0, np.uint32))
        check_forms(mfx, r, base.k, base.want(*none, el, 3, 0.5, COSINE), 3, none, "every list empty")
        got = r.diversify(4, lists, canonical=True)        # scores only; values and counts left out
        assert len(got) == 2
        assert_exact(got, base.want(*lists, el, 4, 0.5, COSINE)[:2], "items and scores only", names=("items", "score bits"))


def test_lists_at_the_limit_and_past_it(mfx):
    rows, cols, k = 6, 2100, 8
    rng = np.random.default_rng(2048)
    W = rng.standard_normal((rows, k)).astype(F32)
    H = rng.standard_normal((cols, k)).astype(F32)
    H[1000:1040] = H[10:50]                                # ties far apart in the list
    m = Model(mfx, W, H, lazy=True)
    lens = np.array([LIMIT, 3, LIMIT - 1, 0, LIMIT, 700])
    lists = random_lists(rng, lens, cols)
    keep = rng.random(cols) < 0.6
    with mfx.Recommender(W, H, 1) as r:
        assert not form1_fits(LIMIT, k)
        check_forms(mfx, r, k, m.want(*lists, True, 10, 0.4, COSINE), 10, lists, "2048 candidates", tradeoff=0.4)
        r.set_item_filter(keep)
        check_forms(mfx, r, k, m.want(*lists, keep[None, :], 128, 0.6, DOT), 128, lists, "2048 candidates, filter", tradeoff=0.6, metric=DOT)
        r.set_item_filter(None)
        lens[4] = LIMIT + 1
        too_long = random_lists(rng, lens, cols)
        with pytest.raises(mfx.MfxError, match=r"slot 4 holds more than 2048"):
            r.diversify(10, too_long, canonical=True)
        lens[1] = LIMIT + 5
        with pytest.raises(mfx.MfxError, match=r"slot 1 holds more than 2048"):       # the first offending slot
            r.diversify(10, random_lists(rng, lens, cols), canonical=True, form=2)
        check_forms(mfx, r, k, m.want(*lists, True, 1, 0.4, COSINE), 1, lists, "after the refusals", tradeoff=0.4)


# ------------------------------------------------------------------------------------------------ d. ties and special values
def test_duplicated_rows_and_a_zero_row(mfx):
    rng = np.random.default_rng(31)
    k = 12
    W = rng.standard_normal((ROWS, k)).astype(F32)
    H = rng.standard_normal((8, k)).astype(F32)[rng.integers(0, 8, COLS)]   # eight distinct rows: equal rel, similarity 1
    H[::23] = 0                                                              # n2 = 0: c = 0, every cosine with them is 0
    m = Model(mfx, W, H)
    assert (m.c == 0).sum() == len(H[::23])
    lists = random_lists(rng, lengths_for(rng, 10, ROWS, 120), COLS)
    with mfx.Recommender(W, H, 1) as r:
        for metric in (COSINE, DOT):
            for t in (0.0, 0.5, 1.0):
                check_forms(mfx, r, k, m.want(*lists, True, 20, t, metric), 20, lists, f"duplicated rows, metric {metric}, tradeoff {t}",
                            tradeoff=t, metric=metric)


def test_collinear_ramp(mfx):
    k = 9
    H = collinear_ramp(COLS, k, seed=3)
    W = np.random.default_rng(3).standard_normal((ROWS, k)).astype(F32)
    m = Model(mfx, W, H)
    rng = np.random.default_rng(4)
    lists = random_lists(rng, lengths_for(rng, 10, ROWS, 150), COLS)
    with mfx.Recommender(W, H, 1) as r:
        for t in (0.0, 0.3):
            check_forms(mfx, r, k, m.want(*lists, True, 10, t, COSINE), 10, lists, f"collinear ramp, tradeoff {t}", tradeoff=t)


def test_infinite_and_nan_scores_and_nan_values(mfx):
    rng = np.random.default_rng(8)
    k = 5
    W = rng.standard_normal((ROWS, k)).astype(F32)
    H = rng.standard_normal((COLS, k)).astype(F32)
    H[rng.random((COLS, k)) < 0.2] = 0                      # 0 * inf = NaN scores
    W[::3, 2] = np.inf                                      # +-inf scores by the sign of H[i][2]
    W[1::9, 0], W[1::9, 4] = np.inf, -np.inf                # inf - inf
    m = Model(mfx, W, H)
    assert np.isnan(m.S).any() and np.isposinf(m.S).any() and np.isneginf(m.S).any()
    lists = random_lists(rng, lengths_for(rng, 10, ROWS, 150), COLS)
    with mfx.Recommender(W, H, 1) as r:
        for t in (0.0, 0.5, 1.0):
            want = m.want(*lists, True, 20, t, COSINE)
            if t == 0.0:                                    # 0 * inf: NaN values are ranked last and returned as computed
                assert (np.isnan(want[2]) & (want[0] != PAD)).any()
            check_forms(mfx, r, k, want, 20, lists, f"special values, tradeoff {t}", tradeoff=t)
    Hi = H.copy()
    Hi[7::31, 1] = np.inf                                   # infinite and NaN similarities, c = 0 at those items
    m = Model(mfx, W[2::3].copy(), Hi)
    lists = random_lists(rng, lengths_for(rng, 10, m.W.shape[0], 150), COLS)
    with mfx.Recommender(m.W, Hi, 1) as r:
        for metric in (DOT, COSINE):
            check_forms(mfx, r, k, m.want(*lists, True, 20, 0.5, metric), 20, lists, f"infinite rows of H, metric {metric}", tradeoff=0.5,
                        metric=metric)


# ------------------------------------------------------------------------------------------------ e. exclusion, filter, tradeoff 1
def test_exclusion_flag_filter_and_tradeoff_one(mfx, base):
    rng = np.random.default_rng(12)
    ex = exclusion(mfx, rng, ROWS, COLS, 10, base.S)
    el = eligible_mask(ex, np.arange(ROWS), COLS)
    keep = rng.random(COLS) < 0.5
    lists = random_lists(rng, lengths_for(rng, 10, ROWS, 200), COLS)
    with mfx.Recommender(base.W, base.H, 1, exclude=ex) as r:
        for filt in (None, keep):
            r.set_item_filter(filt)
            f = keep[None, :] if filt is not None else True
            check_forms(mfx, r, base.k, base.want(*lists, el & f, 10, 0.5, COSINE), 10, lists, f"exclusion, filter {filt is not None}")
            check_forms(mfx, r, base.k, base.want(*lists, f, 10, 0.5, COSINE), 10, lists, f"MFX_DIV_NO_EXCLUDE, filter {filt is not None}",
                        apply_exclude=False)
            for apply in (True, False):                    # tradeoff 1 is query_candidates
                ci, cs, cn = r.query_candidates(10, lists, apply_exclude=apply, canonical=True, return_counts=True)
                for metric in (DOT, COSINE):
                    got = r.diversify(10, lists, tradeoff=1.0, metric=metric, apply_exclude=apply, canonical=True, return_values=True,
                                      return_counts=True)
                    assert_exact(got, (ci, cs, cs, cn), f"tradeoff 1 against query_candidates, exclusion {apply}, metric {metric}")


# ------------------------------------------------------------------------------------------------ f. query vectors
def test_query_vectors_in_place_of_users(mfx, base):
    import torch
    rng = np.random.default_rng(13)
    ex = exclusion(mfx, rng, ROWS, COLS, 10, base.S)
    lists = random_lists(rng, lengths_for(rng, 10, ROWS, 200), COLS)
    with mfx.Recommender(base.W, base.H, 1, exclude=ex) as r:
        by_id = r.diversify(10, lists, apply_exclude=False, canonical=True, return_values=True, return_counts=True)
        assert_exact(by_id, base.want(*lists, True, 10, 0.5, COSINE), "ids, MFX_DIV_NO_EXCLUDE")
        for form in (0, 1, 2):
            got = r.diversify(10, lists, vectors=base.W, apply_exclude=False, canonical=True, return_values=True, return_counts=True, form=form)
            assert_exact(got, by_id, f"the rows of W as vectors, form {form}")
        dev = r.diversify(10, lists, vectors=torch.from_numpy(base.W).cuda(), apply_exclude=False, canonical=True, return_values=True,
                          return_counts=True)
        assert all(t.is_cuda for t in dev)
        assert_exact(dev, by_id, "vectors on the device")
        # the rows a fold-in solved
        fp, fi = random_lists(rng, rng.integers(1, 30, 25), COLS)
        r.fold_in_setup(mfx.MFX_FOLD_ALS, 0.1)
        Wf = r.fold_in((fp, fi, rng.uniform(1, 5, fi.size).astype(F32)))[2]
        Sf = chain_scores(Wf, base.H, np.arange(25))
        sub = random_lists(rng, lengths_for(rng, 10, 25, 200), COLS)
        want = base.want(*sub, True, 10, 0.3, COSINE, S=Sf)
        check_forms(mfx, r, base.k, want, 10, sub, "fold-in rows", vectors=Wf, apply_exclude=False, tradeoff=0.3)


# ------------------------------------------------------------------------------------------------ g. independence
def test_batch_order_and_memory_space_do_not_matter(mfx, base):
    import torch
    rng = np.random.default_rng(8)
    ex = exclusion(mfx, rng, ROWS, COLS, 10, base.S)
    ptr, idx = random_lists(rng, lengths_for(rng, 10, ROWS, 200), COLS)
    sel = np.concatenate([rng.permutation(ROWS), rng.integers(0, ROWS, 30)])      # slots permuted, with duplicates
    kw = dict(canonical=True, return_values=True, return_counts=True, tradeoff=0.4)

    def take(sel):
        lens = (ptr[1:] - ptr[:-1])[sel]
        p = np.zeros(sel.size + 1, np.int64)
        np.cumsum(lens, out=p[1:])
        i = np.concatenate([idx[ptr[q]:ptr[q + 1]] for q in sel]) if sel.size else idx[:0]
        return p.astype(np.uint32), i.astype(np.uint32)

    with mfx.Recommender(base.W, base.H, 1, exclude=ex) as r:
        full = r.diversify(10, (ptr, idx), **kw)
        assert_exact(full, base.want(ptr, idx, eligible_mask(ex, np.arange(ROWS), COLS), 10, 0.4, COSINE), "users = None")
        assert_exact(r.diversify(10, take(sel), users=sel, **kw), [b[sel] for b in full], "permuted, with duplicates")
        for q in (0, 33, ROWS - 1):                        # alone: the batch's longest list, and with it the workgroup, changes
            for form in (1, 2):
                assert_exact(r.diversify(10, take(np.array([q])), users=[q], form=form, **kw), [b[q:q + 1] for b in full], f"slot {q} alone")
        tp, ti = (torch.from_numpy(a.view(np.int32)).cuda() for a in take(sel))
        tu = torch.from_numpy(sel.astype(np.uint32).view(np.int32)).cuda()
        dev = r.diversify(10, (tp, ti), users=tu, **kw)
        torch.cuda.synchronize()
        assert all(t.is_cuda for t in dev) and dev[0].dtype == torch.int32 and dev[2].dtype == torch.float32 and dev[3].dtype == torch.int32
        assert_exact(dev, [b[sel] for b in full], "device tensors")
        assert_exact(r.diversify(10, (ptr, idx), on_device=True, **kw), full, "on_device")
        empty = r.diversify(10, (np.zeros(1, np.uint32), idx[:0]), users=[], **kw)
        assert [a.shape for a in empty] == [(0, 10), (0, 10), (0, 10), (0,)]
    with mfx.Recommender(torch.from_numpy(base.W).cuda(), torch.from_numpy(base.H).cuda(), 1, exclude=ex) as r:
        assert_exact(r.diversify(10, (ptr, idx), **kw), full, "device factors")


def test_query_diverse_is_the_reference_on_the_exact_pool(mfx, base):
    rng = np.random.default_rng(14)
    ex = exclusion(mfx, rng, ROWS, COLS, 10, base.S)
    users = rng.permutation(ROWS)[:40]
    el = eligible_mask(ex, users, COLS)
    with mfx.Recommender(base.W, base.H, 1, exclude=ex) as r:
        for pool, n_top, t in ((50, 10, 0.5), (10, 10, 0.2), (257, 128, 0.7)):
            top = expected_topn(base.S[users], el, pool)[0]
            rows = [np.sort(row[row != PAD]) for row in top]
            ptr = np.zeros(len(rows) + 1, np.int64)
            np.cumsum([len(x) for x in rows], out=ptr[1:])
            want = base.want(ptr, np.concatenate(rows), el, n_top, t, COSINE, users)[:2]
            assert_exact(r.query_diverse(n_top, pool, users=users, tradeoff=t), want, f"pool {pool}", names=("items", "score bits"))
            dev = r.query_diverse(n_top, pool, users=users, tradeoff=t, on_device=True)
            assert dev[0].is_cuda
            assert_exact(dev, want, f"pool {pool}, on_device", names=("items", "score bits"))
        all_users = r.query_diverse(5, 20)
        assert all_users[0].shape == (ROWS, 5)
        assert_exact([a[users] for a in all_users], r.query_diverse(5, 20, users=users), "users = None", names=("items", "score bits"))


# ------------------------------------------------------------------------------------------------ h. refusals
def test_refusals_leave_the_handle_usable(mfx, base):
    lib = mfx.lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    n_top = 5
    good_ptr = np.array([0, 3, 3, 7], np.uint32)
    good_idx = np.array([1, 5, 9, 0, 2, 4, COLS - 1], np.uint32)
    users = np.array([4, 0, ROWS - 1], np.uint32)
    V = base.W[users].copy()
    want = base.want(good_ptr, good_idx, True, n_top, 0.5, COSINE, users)
    items, scores, values = np.zeros((3, n_top), np.uint32), np.zeros((3, n_top), F32), np.zeros((3, n_top), F32)
    nel = np.zeros(3, np.uint32)

    def call(h, ptr=good_ptr, idx=good_idx, u=users, wq=None, flags=0, metric=COSINE, t=0.5, n=n_top, out=items, space=0, form=0):
        return lib.mfx_rec_diversify(h, 3, vp(u), vp(wq), vp(ptr), vp(idx), flags, metric, t, n, vp(out), vp(scores), vp(values), vp(nel),
                                     space, form)

    def edit(a, pos, val):
        b = a.copy()
        b[pos] = val
        return b

    cases = [
        ("strictly ascending", "slot 2", lambda h: call(h, idx=edit(good_idx, 5, 1))),
        ("strictly ascending", "slot 0", lambda h: call(h, idx=edit(good_idx, 1, 1))),
        ("out of range", "slot 2", lambda h: call(h, idx=edit(good_idx, 6, COLS))),
        ("non-decreasing", "slot 1", lambda h: call(h, ptr=np.array([0, 3, 2, 7], np.uint32))),
        ("non-decreasing", "slot 0", lambda h: call(h, ptr=np.array([1, 3, 3, 7], np.uint32))),
        ("n_top", "", lambda h: call(h, n=0)),
        ("n_top", "", lambda h: call(h, n=129)),
        ("flag", "", lambda h: call(h, flags=2)),
        ("flag", "", lambda h: call(h, flags=-1)),
        ("metric", "", lambda h: call(h, metric=2)),
        ("metric", "", lambda h: call(h, metric=-1)),
        ("tradeoff", "", lambda h: call(h, t=-0.25)),
        ("tradeoff", "", lambda h: call(h, t=1.5)),
        ("tradeoff", "", lambda h: call(h, t=float("nan"))),
        ("tradeoff", "", lambda h: call(h, t=float("inf"))),
        ("form", "", lambda h: call(h, form=3)),
        ("form", "", lambda h: call(h, form=-1)),
        ("users must be NULL", "", lambda h: call(h, wq=V, flags=1)),
        ("MFX_DIV_NO_EXCLUDE", "", lambda h: call(h, wq=V, u=None)),
        ("user id", "", lambda h: call(h, u=edit(users, 1, ROWS))),
        ("cand_ptr is NULL", "", lambda h: call(h, ptr=None)),
        ("items is NULL", "", lambda h: call(h, out=None)),
        ("cand_idx is NULL", "", lambda h: call(h, idx=None)),
        ("memory space", "", lambda h: call(h, space=7)),
    ]
    with mfx.Recommender(base.W, base.H, 1) as r:
        for word, slot, f in cases:
            code = f(r.handle)
            msg = lib.mfx_last_error().decode()
            assert code == MFX_ERR_INVALID and word in msg and slot in msg, (word, slot, code, msg)
            assert call(r.handle) == 0, (word, lib.mfx_last_error().decode())
            assert_exact((items, scores, values, nel), want, f"after the refusal of {word}")
        # users = NULL with more slots than rows
        assert lib.mfx_rec_diversify(r.handle, ROWS + 1, None, None, vp(good_ptr), vp(good_idx), 0, COSINE, 0.5, n_top, vp(items), None, None,
                                     None, 0, 0) == MFX_ERR_INVALID
        # nothing to do; empty lists need no ids; scores, values and counts may be left out
        assert lib.mfx_rec_diversify(r.handle, 0, None, None, None, None, 0, COSINE, 0.5, n_top, None, None, None, None, 0, 0) == 0
        assert call(r.handle, ptr=np.zeros(4, np.uint32), idx=None) == 0 and np.all(items == PAD) and np.all(nel == 0)
        assert lib.mfx_rec_diversify(r.handle, 3, vp(users), None, vp(good_ptr), vp(good_idx), 0, COSINE, 0.5, n_top, vp(items), None, None,
                                     None, 0, 0) == 0
        assert np.array_equal(items, want[0])
        # query vectors through the C ABI
        assert call(r.handle, wq=V, u=None, flags=1) == 0
        assert_exact((items, scores, values, nel), want, "Wq")


# ------------------------------------------------------------------------------------------------ i. the other paths
def test_other_queries_are_unchanged_by_a_diversify(mfx, base):
    rng = np.random.default_rng(15)
    ex = exclusion(mfx, rng, ROWS, COLS, 10, base.S)
    lists = random_lists(rng, lengths_for(rng, 10, ROWS, 200), COLS)
    keep = rng.random(COLS) < 0.7

    def others(r):
        return r.similar_items(10) + r.similar_items(7, metric=DOT) + r.query(10) + r.query_candidates(10, lists, canonical=True, return_counts=True)

    with mfx.Recommender(base.W, base.H, 1, exclude=ex) as r:   # the diversify is the first call: it runs the setup itself
        d0 = r.diversify(10, lists, canonical=True, return_values=True, return_counts=True)
        after = others(r)
    with mfx.Recommender(base.W, base.H, 1, exclude=ex) as r:
        before = others(r)
        d1 = r.diversify(10, lists, canonical=True, return_values=True, return_counts=True)
        again = others(r)
        r.set_item_filter(keep)
        r.diversify(10, lists, canonical=True)
        r.set_item_filter(None)
        last = others(r)
    for a, b, c, d in zip(before, after, again, last):
        assert np.array_equal(host(a).view(np.uint32), host(b).view(np.uint32))
        assert np.array_equal(host(a).view(np.uint32), host(c).view(np.uint32))
        assert np.array_equal(host(a).view(np.uint32), host(d).view(np.uint32))
    assert_exact(d0, d1, "diversify first or later")
