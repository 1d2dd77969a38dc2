"""IVF retrieval (mfx_rec_ivf_setup / _lists / _probe, mfx_rec_query_ivf; Recommender.ivf_*, query_ivf) checked bit for bit:
items and score bits (compared as uint32) against the exact reference of tests/ivf_exact.py (rec_exact.py's top-N over the
centroid scores, cand_exact.py's re-ranking over the union of the probed lists) and against the handle's own query and
query_candidates, under exclusion rows, item filters, ties across lists, empty and one-tile lists, several work items per
list, batch order and memory space."""
import ctypes as C
import functools

import numpy as np
import pytest

from cand_exact import exclusion, regime_factors
from ivf_exact import expected_probe, expected_query, lists_of, union_lists
from rec_exact import PAD, chain_scores, eligible_mask

pytestmark = pytest.mark.gpu

F32 = np.float32
MFX_ERR_INVALID = -1  # include/mfx.h
ROWS, COLS, NLIST = 160, 1000, 9
SIZES = [0, 1, 31, 32, 33, 0, 64, 65]     # the first eight lists: empty, below / at / above one tile and two tiles; the rest: list 8


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1, m.lib().mfx_last_error()
    return m


def host(a):
    if not isinstance(a, np.ndarray):
        a = a.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def assert_exact(got, want, what):
    for g, w, name in zip(got, want, ("ids", "score bits")):
        g, w = host(g), np.asarray(host(w))
        if name == "score bits":
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        bad = np.argwhere(g != w)
        if bad.size:
            p = tuple(bad[:6].T)
            pytest.fail(f"{what}: {len(bad)} of {g.size} {name} differ; at {bad[:6].tolist()}: {g[p].tolist()} vs {w[p].tolist()}")


def forced_assign(rng, cols=COLS):
    """An assignment with the list sizes SIZES + [rest], the items of every list scattered over the catalogue."""
    a = np.full(cols, len(SIZES), np.uint32)
    perm = rng.permutation(cols)
    at = 0
    for l, n in enumerate(SIZES):
        a[perm[at:at + n]] = l
        at += n
    return a


@functools.lru_cache(maxsize=None)
def case(k, regime):
    """W, H, centroids, assignment, lists, and the exact scores of every user against H: computed once per (k, regime)."""
    W, H = regime_factors(regime, ROWS, COLS, k, seed=1000 + k)
    _, Cn = regime_factors(regime, ROWS, NLIST, k, seed=2000 + k)
    assign = forced_assign(np.random.default_rng(k))
    list_ptr, list_idx = lists_of(assign, NLIST)
    return W, H, Cn, assign, list_ptr, list_idx, chain_scores(W, H, np.arange(ROWS))


# ------------------------------------------------------------------------------------------------ 1. the lists
@pytest.mark.parametrize("layout", [1, 0])
def test_lists_are_the_assignment_in_ascending_order(mfx, layout):
    import torch
    W, H, Cn, assign, list_ptr, list_idx, _ = case(37, "normal")
    assert np.diff(list_ptr.astype(np.int64)).tolist() == SIZES + [COLS - sum(SIZES)]
    Wl, Hl = (W, H) if layout == 1 else (np.ascontiguousarray(W.T), np.ascontiguousarray(H.T))
    with mfx.Recommender(Wl, Hl, layout) as r:
        for dev in (False, True):
            if dev:
                r.ivf_setup(torch.from_numpy(assign.view(np.int32)).cuda(), torch.from_numpy(Cn).cuda())
            else:
                r.ivf_setup(assign, Cn)
            ptr, idx = r.ivf_lists()
            assert ptr.dtype == np.uint32 and idx.dtype == np.uint32
            assert np.array_equal(ptr, list_ptr) and np.array_equal(idx, list_idx)
            assert np.array_equal(np.sort(idx), np.arange(COLS))          # every item once
            for l in range(NLIST):
                assert np.array_equal(idx[ptr[l]:ptr[l + 1]], np.nonzero(assign == l)[0])


# ------------------------------------------------------------------------------------------------ 2. the probe
@pytest.mark.parametrize("regime", ["normal", "scaled", "huge"])
@pytest.mark.parametrize("k", [1, 37, 64, 130])
def test_probe_against_the_exact_reference(mfx, k, regime):
    W, H, Cn, assign, *_ = case(k, regime)
    users = np.arange(ROWS)
    SC = chain_scores(W, Cn, users)
    if regime == "huge":
        assert np.isnan(SC).any() and np.isinf(SC).any()
    with mfx.Recommender(W, H, 1) as r:
        r.ivf_setup(assign, Cn)
        for nprobe in (1, 3, NLIST):
            want = expected_probe(W, Cn, users, nprobe)
            if regime == "huge" and nprobe == NLIST:
                assert (want[0] == PAD).any()                             # NaN lists are never probed: padding
            assert_exact(r.ivf_probe(nprobe), want, f"probe k {k} {regime} nprobe {nprobe}")
            assert_exact(r.ivf_probe(nprobe, users[::-1].copy()), tuple(w[::-1] for w in want), f"probe reversed k {k} {regime} nprobe {nprobe}")
    # the probe is query on a handle whose items are the centroids
    with mfx.Recommender(W, Cn, 1) as rc:
        assert_exact(rc.query(3), expected_probe(W, Cn, users, 3), f"centroid handle k {k} {regime}")


# ------------------------------------------------------------------------------------------------ 3. the query
def batches(rng, probes_all):
    """Slot -> user for batch sizes 1, 127, 129, 300: arbitrary order with duplicates; in the batch of 300, 200 slots are
    users that probe the most probed list, so that list has several work items."""
    counts = np.bincount(probes_all[probes_all != PAD], minlength=NLIST)
    counts[np.array(SIZES + [1]) == 0] = 0                 # (an empty list has no work item)
    popular = counts.argmax()
    fans = np.nonzero((probes_all == popular).any(1))[0]
    out = [rng.integers(0, ROWS, n) for n in (1, 127, 129)]
    big = np.concatenate([rng.choice(fans, 200), rng.integers(0, ROWS, 100)])
    out.append(big[rng.permutation(300)])
    return out, popular


@pytest.mark.parametrize("regime", ["normal", "scaled", "huge"])
@pytest.mark.parametrize("k", [1, 37, 64, 130])
def test_query_against_the_exact_reference(mfx, k, regime):
    W, H, Cn, assign, list_ptr, list_idx, S = case(k, regime)
    rng = np.random.default_rng(50 + k)
    ex = exclusion(mfx, rng, ROWS, COLS, 10, S)
    el = eligible_mask(ex, np.arange(ROWS), COLS)
    short = False
    with mfx.Recommender(W, H, 1, exclude=ex) as r:
        r.ivf_setup(assign, Cn)
        for nprobe in (1, 3, NLIST):
            probes_all, _ = expected_probe(W, Cn, np.arange(ROWS), nprobe)
            bs, popular = batches(rng, probes_all)
            assert (probes_all[bs[-1]] == popular).sum() > 128            # several work items for one list
            for users in bs:
                for n_top in (1, 10, 100):
                    want = expected_query(S[users], probes_all[users], list_ptr, list_idx, el[users], n_top)
                    short |= n_top == 100 and bool((want[2] < 100).any())
                    assert_exact(r.query_ivf(n_top, nprobe, users), want[:2], f"k {k} {regime} nprobe {nprobe} n_top {n_top} batch {len(users)}")
    assert short                                                          # some unions hold fewer than 100 eligible items


# ------------------------------------------------------------------------------------------------ 4. nprobe = nlist is query
@pytest.mark.parametrize("nlist", [1, 8])
def test_probing_every_list_equals_query(mfx, nlist):
    rows, cols, k = 140, 1500, 24
    W, H = regime_factors("normal", rows, cols, k, seed=77)
    rng = np.random.default_rng(nlist)
    assign = rng.integers(0, nlist, cols).astype(np.uint32)
    Cn = rng.standard_normal((nlist, k)).astype(F32)
    keep = rng.random(cols) < 0.5
    S = chain_scores(W, H, np.arange(rows))
    ex = exclusion(mfx, rng, rows, cols, 10, S)
    for when in ("none", "before", "after"):
        with mfx.Recommender(W, H, 1, exclude=ex) as r:
            if when == "before":
                r.set_item_filter(keep)
            r.ivf_setup(assign, Cn)
            if when == "after":
                r.set_item_filter(keep)
            for n_top in (1, 10, 1024):
                assert_exact(r.query_ivf(n_top, nlist), r.query(n_top), f"nlist {nlist} filter {when} n_top {n_top}")
            if when == "after":                                           # and taken off again
                r.set_item_filter(None)
                assert_exact(r.query_ivf(10, nlist), r.query(10), f"nlist {nlist} filter removed")


def test_user_chunked_launches_equal_query(mfx):
    """nprobe * L * 8 bytes of candidate lists per slot: at nprobe = 8, n_top = 1024 (L = 2048) the 1 GiB workspace cap
    holds 8192 slots, so 8300 users take two launches, the second of 108 slots."""
    rows, cols, k, nlist = 8300, 200, 3, 8
    rng = np.random.default_rng(44)
    W = rng.standard_normal((rows, k)).astype(F32)
    H = rng.standard_normal((cols, k)).astype(F32)
    assign = rng.integers(0, nlist, cols).astype(np.uint32)
    Cn = rng.standard_normal((nlist, k)).astype(F32)
    users = rng.permutation(rows)
    with mfx.Recommender(W, H, 1) as r:
        r.ivf_setup(assign, Cn)
        assert_exact(r.query_ivf(1024, nlist, users), r.query(1024, users), "two launches")
        probes, _ = r.ivf_probe(2, users)
        ptr, idx = union_lists(probes, *r.ivf_lists())
        assert_exact(r.query_ivf(1024, 2, users), r.query_candidates(1024, (ptr, idx), users=users, canonical=True)[:2], "one launch, nprobe 2")


# ------------------------------------------------------------------------------------------------ 5. ties across lists
def test_ties_are_ordered_by_item_id_across_lists(mfx):
    rows, cols, k, nlist = 70, 400, 5, 4
    rng = np.random.default_rng(9)
    W = rng.integers(-2, 3, (rows, k)).astype(F32)
    W[::5] = 0.0                                           # every score of these users is +-0
    W[1::10] = -0.0
    base = rng.integers(-2, 3, (cols // 4, k)).astype(F32)
    H = np.concatenate([base] * 4)                         # item i, i + 100, i + 200, i + 300 are the same row ...
    assign = ((np.arange(cols) // 100 + np.arange(cols)) % nlist).astype(np.uint32)   # ... in four different lists
    for i in range(100):
        assert len({int(assign[i + 100 * c]) for c in range(4)}) == 4
    Cn = rng.integers(-2, 3, (nlist, k)).astype(F32)
    list_ptr, list_idx = lists_of(assign, nlist)
    S = chain_scores(W, H, np.arange(rows))
    users = rng.permutation(rows)
    with mfx.Recommender(W, H, 1) as r:
        r.ivf_setup(assign, Cn)
        for nprobe in (2, 4):
            probes, _ = expected_probe(W, Cn, users, nprobe)
            for n_top in (7, 64):
                want = expected_query(S[users], probes, list_ptr, list_idx, True, n_top)
                assert_exact(r.query_ivf(n_top, nprobe, users), want[:2], f"ties nprobe {nprobe} n_top {n_top}")
        zi, zs = r.query_ivf(64, 4, np.array([0]))
        assert zi[0].tolist() == list(range(64)) and not zs[0].any()


# ------------------------------------------------------------------------------------------------ 6. GPU against GPU
def test_query_ivf_is_query_candidates_on_the_probed_unions(mfx):
    rows, cols, k, nlist, nprobe, n_top = 2000, 5000, 64, 64, 8, 10
    rng = np.random.default_rng(6)
    W = rng.standard_normal((rows, k)).astype(F32)
    H = rng.standard_normal((cols, k)).astype(F32)
    d = mfx.dataset.synth_ratings(rows, cols, 40_000, seed=3)
    with mfx.Recommender(W, H, 1, exclude=d) as r:
        r.ivf_build(H, nlist, iters=2, seed=1)
        probes, _ = r.ivf_probe(nprobe)
        ptr, idx = union_lists(probes, *r.ivf_lists())
        want = r.query_candidates(n_top, (ptr, idx), canonical=True)
        assert_exact(r.query_ivf(n_top, nprobe), want[:2], "gpu vs gpu")
        t = r.ivf_times()
        assert set(t) == {"probe", "build", "pass", "merge"} and all(v > 0 for v in t.values())


# ------------------------------------------------------------------------------------------------ 7. one long list
def test_one_long_list(mfx):
    rows, cols, k, nlist, n_top = 130, 20100, 8, 3, 10
    rng = np.random.default_rng(7)
    W = rng.standard_normal((rows, k)).astype(F32)
    H = (rng.standard_normal((cols, k)) * np.linspace(0.1, 3.0, cols)[:, None]).astype(F32)   # the threshold keeps rising
    assign = np.ones(cols, np.uint32)
    assign[rng.choice(cols, 100, replace=False)] = np.repeat([0, 2], 50)
    Cn = rng.standard_normal((nlist, k)).astype(F32)
    list_ptr, list_idx = lists_of(assign, nlist)
    assert np.diff(list_ptr.astype(np.int64)).tolist() == [50, 20000, 50]
    users = np.arange(rows)
    S = chain_scores(W, H, users)
    with mfx.Recommender(W, H, 1) as r:
        r.ivf_setup(assign, Cn)
        for nprobe in (1, 2):
            probes, _ = expected_probe(W, Cn, users, nprobe)
            assert (probes == 1).any()
            want = expected_query(S, probes, list_ptr, list_idx, True, n_top)
            assert_exact(r.query_ivf(n_top, nprobe), want[:2], f"long list nprobe {nprobe}")


# ------------------------------------------------------------------------------------------------ 8. independence
def test_a_slot_does_not_depend_on_batch_space_or_an_earlier_index(mfx):
    import torch
    W, H, Cn, assign, list_ptr, list_idx, S = case(37, "normal")
    rng = np.random.default_rng(8)
    users = rng.integers(0, ROWS, 300)
    with mfx.Recommender(W, H, 1) as r:
        r.ivf_setup(assign, Cn)
        bi, bs = r.query_ivf(10, 3, users)
        for s in (0, 150, 299):
            assert_exact(r.query_ivf(10, 3, users[s:s + 1]), (bi[s:s + 1], bs[s:s + 1]), f"alone vs batch, slot {s}")
        di, ds = r.query_ivf(10, 3, torch.from_numpy(users.astype(np.int32)).cuda())
        assert di.is_cuda and ds.is_cuda
        assert_exact((di, ds), (bi, bs), "device vs host")
        pl, ps = r.ivf_probe(3, users)
        assert_exact(r.ivf_probe(3, torch.from_numpy(users.astype(np.int32)).cuda()), (pl, ps), "probe device vs host")
        ai, as_ = r.query_ivf(10, 3, on_device=True)
        assert_exact((host(ai)[users], host(as_)[users]), (bi, bs), "all users on the device vs the batch")
        # a second setup with another assignment replaces the first
        assign2 = np.roll(assign, 17)
        Cn2 = Cn[::-1].copy()
        r.ivf_setup(assign2, Cn2)
        lp2, li2 = lists_of(assign2, NLIST)
        got_ptr, got_idx = r.ivf_lists()
        assert np.array_equal(got_ptr, lp2) and np.array_equal(got_idx, li2)
        probes, _ = expected_probe(W, Cn2, users, 3)
        want = expected_query(S[users], probes, lp2, li2, True, 10)
        assert_exact(r.query_ivf(10, 3, users), want[:2], "after the second setup")


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals_leave_the_handle_usable(mfx):
    W, H, Cn, assign, list_ptr, list_idx, S = case(37, "normal")
    lib = mfx.lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    users = np.array([5, 0, 159], np.uint32)
    items, scores = np.empty((3, 8192), np.uint32), np.empty((3, 8192), F32)
    lp, li = np.empty(NLIST + 1, np.uint32), np.empty(COLS, np.uint32)
    probes, _ = expected_probe(W, Cn, users, 3)
    want = expected_query(S[users], probes, list_ptr, list_idx, True, 10)

    def refused(rc, word):
        assert rc == MFX_ERR_INVALID, (rc, word)
        assert word in lib.mfx_last_error().decode(), (word, lib.mfx_last_error())

    with mfx.Recommender(W, H, 1) as r:
        h = r.handle
        q = lambda nprobe=3, n_top=10, u=users, n=3, space=0, it=items: lib.mfx_rec_query_ivf(h, n, vp(u) if u is not None else None, nprobe, n_top,
                                                                                             vp(it) if it is not None else None, vp(scores), space)
        p = lambda nprobe=3, u=users, n=3, space=0: lib.mfx_rec_ivf_probe(h, n, vp(u), nprobe, vp(items), vp(scores), space)
        # before a successful setup
        refused(q(), "mfx_rec_ivf_setup first")
        refused(p(), "mfx_rec_ivf_setup first")
        refused(lib.mfx_rec_ivf_lists(h, vp(lp), vp(li), 0), "mfx_rec_ivf_setup first")
        bad = assign.copy()
        bad[123] = NLIST
        refused(lib.mfx_rec_ivf_setup(h, NLIST, vp(bad), vp(Cn), 0), "assign entry")
        refused(q(), "mfx_rec_ivf_setup first")                            # a refused setup set nothing up
        for nl in (0, 65537):
            refused(lib.mfx_rec_ivf_setup(h, nl, vp(assign), vp(Cn), 0), "nlist")
        refused(lib.mfx_rec_ivf_setup(h, NLIST, None, vp(Cn), 0), "required")
        refused(lib.mfx_rec_ivf_setup(h, NLIST, vp(assign), vp(Cn), 7), "memory space")
        r.ivf_setup(assign, Cn)

        def still_right():
            assert_exact(r.query_ivf(10, 3, users), want[:2], "after a refusal")

        still_right()
        refused(lib.mfx_rec_ivf_setup(h, NLIST, vp(bad), vp(Cn), 0), "assign entry")   # the index stays as it was
        still_right()
        for f, word in ((lambda: q(nprobe=0), "nprobe"), (lambda: q(nprobe=NLIST + 1), "nprobe"),
                        (lambda: q(n_top=0), "n_top"), (lambda: q(n_top=1025), "n_top"),
                        (lambda: q(nprobe=9, n_top=1000), "nprobe * n_top"),
                        (lambda: q(u=np.array([5, ROWS, 1], np.uint32)), "user id"),
                        (lambda: q(u=None, n=ROWS + 1), "users = NULL"),
                        (lambda: q(space=5), "memory space"), (lambda: q(it=None), "items is NULL"),
                        (lambda: p(nprobe=0), "nprobe"), (lambda: p(nprobe=NLIST + 1), "nprobe"),
                        (lambda: p(u=np.array([ROWS, 0, 1], np.uint32)), "user id"), (lambda: p(space=5), "memory space"),
                        (lambda: lib.mfx_rec_ivf_lists(h, vp(lp), vp(li), 9), "memory space"),
                        (lambda: lib.mfx_rec_ivf_lists(h, None, vp(li), 0), "required")):
            refused(f(), word)
            still_right()
        assert q(n=0) == 0 and p(n=0) == 0
        assert q(nprobe=8, n_top=1024) == 0                               # the largest merge


# ------------------------------------------------------------------------------------------------ 10. build
@pytest.mark.parametrize("layout", [1, 0])
def test_build_on_planted_clusters_finds_the_true_top(mfx, layout):
    import torch
    k, ncl, per, rows = 16, 16, 40, 64
    rng = np.random.default_rng(10)
    centres = 10.0 * np.eye(ncl, k)                        # well separated: orthogonal, far longer than the noise
    # Lloyd iterations keep a planted cluster whole only if no two of the initial rows share one: the rows ivf_kmeans starts
    # from (its documented choice) are given one cluster each, the other items fill the clusters up in random order
    first = np.random.default_rng(0).choice(ncl * per, ncl, replace=False)
    label = np.empty(ncl * per, np.int64)
    label[first] = np.arange(ncl)
    label[np.setdiff1d(np.arange(ncl * per), first)] = rng.permutation(np.repeat(np.arange(ncl), per - 1))
    H = (centres[label] + 0.1 * rng.standard_normal((ncl * per, k))).astype(F32)
    W = (centres[rng.integers(0, ncl, rows)] + 0.1 * rng.standard_normal((rows, k))).astype(F32)
    assign, Cn = mfx.ivf_kmeans(H, ncl, iters=10, seed=0)
    # in fp64 on the CPU: every user's true top 10 lies in the list of its best centroid
    S64 = W.astype(np.float64) @ H.astype(np.float64).T
    best = np.argmax(W.astype(np.float64) @ Cn.astype(np.float64).T, axis=1)
    top = np.argsort(-S64, axis=1, kind="stable")[:, :10]
    assert (assign[top] == best[:, None]).all()
    Wl, Hl = (W, H) if layout == 1 else (np.ascontiguousarray(W.T), np.ascontiguousarray(H.T))
    with mfx.Recommender(Wl, Hl, layout) as r:
        a2, c2 = r.ivf_build(Hl, ncl, iters=10, seed=0)
        assert np.array_equal(a2, assign) and np.array_equal(c2, Cn)
        assert_exact(r.query_ivf(10, 1), r.query(10), f"planted clusters, layout {layout}")
    with mfx.Recommender(torch.from_numpy(W).cuda(), torch.from_numpy(H).cuda(), 1) as r:   # k-means on the device
        a3, c3 = r.ivf_build(torch.from_numpy(H).cuda(), ncl, iters=10, seed=0)
        assert a3.is_cuda and c3.is_cuda and a3.dtype == torch.int32 and c3.dtype == torch.float32
        assert_exact(r.query_ivf(10, 1, on_device=True), r.query(10, on_device=True), "planted clusters, device build")
