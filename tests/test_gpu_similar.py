"""Item-to-item similarity (mfx_rec_similar, Recommender.similar_items) and the item filter (mfx_rec_set_item_filter)
checked bit for bit against the exact reference of tests/sim_exact.py.  Cosine references use the c that item_norms()
returned, so only the ranking and the two multiplies are under test there; c itself is checked against fp64 in (a).

NaN scores compare as NaN: a returned cosine is NaN where an infinite key meets c[q] = 0 (the "huge" regime has
thousands), and the sign and payload of the NaN that inf * 0 produces are the hardware's choice (the reference's x86
multiply gives 0xFFC00000), not part of the contract; every other value compares bitwise."""
import ctypes as C

import numpy as np
import pytest

import sim_exact
from rec_exact import PAD, chain_scores, eligible_mask, expected_topn
from sim_exact import COSINE, DOT, expected_similar
from test_gpu_recommend_exact import exclusion, host, regime_factors

pytestmark = pytest.mark.gpu

F32 = np.float32
MFX_ERR_INVALID = -1  # include/mfx.h


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1, m.lib().mfx_last_error()
    return m


def bits(s):
    """uint32 bits of fp32 scores with every NaN mapped to one pattern."""
    s = np.ascontiguousarray(s, F32)
    return np.where(np.isnan(s), np.uint32(0x7FC00000), s.view(np.uint32))


def assert_exact(got, want, what):
    gi, gs = host(got[0]), host(got[1])
    wi, ws = want[0], want[1]
    assert gi.shape == wi.shape, (what, gi.shape, wi.shape)
    bad = np.nonzero((gi != wi).any(axis=1) | (bits(gs) != bits(ws)).any(axis=1))[0]
    if bad.size:
        s = bad[0]
        p = np.nonzero((gi[s] != wi[s]) | (bits(gs[s]) != bits(ws[s])))[0][:6]
        pytest.fail(f"{what}: {bad.size} rows differ; row {s} at {p.tolist()}: items {gi[s, p].tolist()} vs "
                    f"{wi[s, p].tolist()}, scores {gs[s, p].tolist()} vs {ws[s, p].tolist()}")


def same(a, b):
    a, b = host(a), host(b)
    return a.shape == b.shape and np.array_equal(bits(a) if a.dtype == F32 else a, bits(b) if b.dtype == F32 else b)


def filters(rng, cols, n_top):
    """The four filters: none; a random half; all but n_top // 2 items removed; nothing kept."""
    few = np.zeros(cols, bool)
    few[rng.choice(cols, n_top // 2, replace=False)] = True
    return [("none", None), ("half", rng.random(cols) < 0.5), ("few", few), ("nothing", np.zeros(cols, bool))]


# ------------------------------------------------------------------------------------------------ a. norms
@pytest.mark.parametrize("k", [1, 3, 64, 129, 1024])
def test_norms(mfx, k):
    cols = 700
    rng = np.random.default_rng(k)
    H = rng.standard_normal((cols, k))
    H *= 2.0 ** rng.integers(-30, 31, (cols, 1))
    H[5] = 0.0
    H[6] = -0.0
    H[10:20] *= 2.0 ** -110                      # subnormal entries, n2 underflows to 0 or a subnormal
    H[20:30] = rng.standard_normal((10, k)) * 2.0 ** -74   # n2 around 2^-148: subnormal
    H[30:40] *= 2.0 ** 60                        # n2 overflows
    H[40, 0] = np.inf
    H = H.astype(F32)
    want = sim_exact.item_n2(H)
    assert (want == 0).sum() >= 2 and np.isinf(want).any()
    assert ((want > 0) & (want < 2.0 ** -126)).any()
    for layout in (1, 0):
        Hl = H if layout == 1 else np.ascontiguousarray(H.T)
        W = np.zeros((1, k) if layout == 1 else (k, 1), F32)
        with mfx.Recommender(W, Hl, layout) as r:
            r.similar_setup()
            n2, c = r.item_norms()
            r.similar_setup()                    # idempotent
            n2b, cb = r.item_norms()
        assert np.array_equal(n2.view(np.uint32), want.view(np.uint32)), (k, layout)
        assert same(n2, n2b) and same(c, cb)
        ref = sim_exact.inv_norm64(want)
        dead = ~(np.isfinite(want) & (want > 0))
        assert np.all(c[dead].view(np.uint32) == 0), (k, layout)
        d = sim_exact.ulp_distance(c[~dead], ref[~dead])
        print(f"k={k} layout={layout}: max ulp distance of c {int(d.max())}")
        assert d.max() <= 2, (k, layout, int(d.max()))


# ------------------------------------------------------------------------------------------------ b. score bits
@pytest.mark.parametrize("k", [1, 2, 3, 5, 16, 17, 33, 64, 65, 128, 129, 257, 1024])
@pytest.mark.parametrize("regime", ["normal", "scaled", "subnormal", "huge", "norms"])
def test_score_bits_full_lists(mfx, regime, k):
    cols, nq, n_top = 997, 130, 1024
    rng = np.random.default_rng(k + 7)
    if regime == "norms":                         # row norms over 2^-30 .. 2^30
        H = (rng.standard_normal((cols, k)) * 2.0 ** rng.integers(-30, 31, (cols, 1))).astype(F32)
    else:
        _, H = regime_factors(regime, 1, cols, k, seed=1000 * k + len(regime))
    q = rng.integers(0, cols, nq)
    q[5:9] = q[0]
    S = chain_scores(H, H, q)
    n2 = sim_exact.item_n2(H)
    for layout in (1, 0):
        Hl = H if layout == 1 else np.ascontiguousarray(H.T)
        W = np.zeros((1, k) if layout == 1 else (k, 1), F32)
        with mfx.Recommender(W, Hl, layout) as r:
            dot = r.similar_items(n_top, q, metric=mfx.MFX_SIM_DOT)
            n2g, c = r.item_norms()
            cos = r.similar_items(n_top, q)
        assert np.array_equal(n2g.view(np.uint32), n2.view(np.uint32))
        assert_exact(dot, expected_similar(S, q, n_top, DOT), f"dot {regime} k={k} layout={layout}")
        assert_exact(cos, expected_similar(S, q, n_top, COSINE, c), f"cosine {regime} k={k} layout={layout}")


# ------------------------------------------------------------------------------------------------ c. mid-stream flushes
FLUSH_INPUTS = ["random", "ties", "ramp"]


@pytest.fixture(scope="module", params=FLUSH_INPUTS)
def flush_case(request):
    cols, k, nq = 6007, 8, 224
    rng = np.random.default_rng(FLUSH_INPUTS.index(request.param))
    if request.param == "random":
        H = rng.standard_normal((cols, k)).astype(F32)
    elif request.param == "ties":
        H = rng.standard_normal((5, k))[rng.integers(0, 5, cols)].astype(F32)
    else:
        H = sim_exact.collinear_ramp(cols, k, 2)
    q = rng.integers(0, cols, nq)
    return request.param, H, q, chain_scores(H, H, q)


@pytest.mark.parametrize("n_top", [1, 32, 33, 225, 481, 1024])
def test_mid_stream_flushes(mfx, flush_case, n_top):
    name, H, q, S = flush_case
    cols, k = H.shape
    rng = np.random.default_rng(n_top)
    pairs = 0
    with mfx.Recommender(np.zeros((1, k), F32), H, 1) as r:
        r.similar_setup()
        c = r.item_norms()[1]
        for i, (fname, keep) in enumerate(filters(rng, cols, n_top)):
            r.set_item_filter(keep)
            what = f"{name} n_top={n_top} filter={fname}"
            wi, ws, wk = expected_similar(S, q, n_top, COSINE, c, keep, with_keys=True)
            assert_exact(r.similar_items(n_top, q, item_slices=1), (wi, ws), "cosine " + what)
            pairs += sim_exact.key_order_pairs(wi, ws, wk)
            if fname == "nothing":
                assert (wi == PAD).all()
            if i == n_top % 4:
                assert_exact(r.similar_items(n_top, q, metric=mfx.MFX_SIM_DOT, item_slices=1),
                             expected_similar(S, q, n_top, DOT, None, keep), "dot " + what)
    if name == "ramp" and n_top >= 225:
        assert pairs >= 1                         # lists that ordering by the returned score would get wrong


# ------------------------------------------------------------------------------------------------ d. slices and merge
@pytest.fixture(scope="module")
def slice_case():
    cols, k, nq = 3001, 24, 150
    rng = np.random.default_rng(77)
    H = rng.standard_normal((cols, k)).astype(F32)
    H[2000:2100] = H[10:110]          # ties across slices: the merge must order them by item
    H[500:540] = H[5]
    q = rng.integers(0, cols, nq)
    q[:6] = [5, 510, 10, 2000, 2050, 3000]
    return H, q, chain_scores(H, H, q)


@pytest.mark.parametrize("n_top", [1, 33, 250, 1024])
def test_slices_and_merge(mfx, slice_case, n_top):
    H, q, S = slice_case
    cols, k = H.shape
    nblk = (cols + 31) // 32
    slices = sorted({s for s in (0, 1, 2, 7, nblk, 8192 // n_top) if s * n_top <= 8192})
    assert 8192 // n_top in slices
    keep = np.random.default_rng(n_top).random(cols) < 0.7
    with mfx.Recommender(np.zeros((1, k), F32), H, 1) as r:
        r.similar_setup()
        c = r.item_norms()[1]
        for kp in (None, keep):
            r.set_item_filter(kp)
            want = expected_similar(S, q, n_top, COSINE, c, kp)
            one = r.similar_items(n_top, q, item_slices=1)
            assert_exact(one, want, f"n_top={n_top} slices=1 filter={kp is not None}")
            for sl in slices:
                got = r.similar_items(n_top, q, item_slices=sl)
                assert_exact(got, want, f"n_top={n_top} slices={sl} filter={kp is not None}")
                assert same(got[0], one[0]) and same(got[1], one[1])


# ------------------------------------------------------------------------------------------------ e. partial workgroups
@pytest.mark.parametrize("nq", [1, 31, 32, 33, 127, 128, 129])
def test_partial_workgroups(mfx, nq):
    import torch
    cols, k = 700, 12
    rng = np.random.default_rng(nq)
    H = rng.standard_normal((cols, k)).astype(F32)
    q = rng.integers(0, cols, nq).astype(np.uint32)
    S = chain_scores(H, H, q)
    W = np.zeros((1, k), F32)
    keep = rng.random(cols) < 0.6
    for n_top in (20, 700):
        with mfx.Recommender(W, H, 1) as r:
            r.set_item_filter(keep)
            got = r.similar_items(n_top, q)
            c = r.item_norms()[1]
            want = expected_similar(S, q, n_top, COSINE, c, keep)
            assert_exact(got, want, f"host nq={nq} n_top={n_top}")
            if nq == 129:                         # items=None: the first nq items in order
                r.set_item_filter(None)
                first = np.arange(cols)
                every = r.similar_items(n_top)
                assert_exact((every[0][:40], every[1][:40]),
                             expected_similar(chain_scores(H, H, first[:40]), first[:40], n_top, COSINE, c), "items=None")
        with mfx.Recommender(torch.from_numpy(W).cuda(), torch.from_numpy(H).cuda(), 1) as r:
            r.set_item_filter(torch.from_numpy(keep).cuda())
            got = r.similar_items(n_top, torch.from_numpy(q.view(np.int32)).cuda())
            torch.cuda.synchronize()
            assert got[0].is_cuda and got[1].is_cuda
            assert_exact(got, want, f"device nq={nq} n_top={n_top}")


# ------------------------------------------------------------------------------------------------ f. self
@pytest.mark.parametrize("metric", [DOT, COSINE])
def test_self_and_duplicate_rows(mfx, metric):
    cols, k, n_top = 1500, 10, 40
    rng = np.random.default_rng(3 + metric)
    H = rng.standard_normal((cols, k)).astype(F32)
    H[[40, 900, 1499]] = H[7]                     # duplicates of query 7
    H[100] = 4.0 * H[7]                           # the same direction, longer
    q = np.array([7, 40, 1499, 100, 3, 7])
    S = chain_scores(H, H, q)
    with mfx.Recommender(np.zeros((1, k), F32), H, 1) as r:
        r.similar_setup()
        c = r.item_norms()[1]
        without = r.similar_items(n_top, q, metric=metric, exclude_self=True)
        with_self = r.similar_items(n_top, q, metric=metric, exclude_self=False)
    assert_exact(without, expected_similar(S, q, n_top, metric, c, None, True), f"exclude_self metric={metric}")
    assert_exact(with_self, expected_similar(S, q, n_top, metric, c, None, False), f"with self metric={metric}")
    for s, qq in enumerate(q):
        assert qq not in without[0][s] and qq in with_self[0][s]
    if metric == COSINE:                          # the duplicates of a row tie with it and come in item order
        dup = [i for i in with_self[0][0].tolist() if i in (7, 40, 900, 1499)]
        assert dup == [7, 40, 900, 1499]
        assert [i for i in without[0][0].tolist() if i in (7, 40, 900, 1499)] == [40, 900, 1499]


# ------------------------------------------------------------------------------------------------ g. filter on the existing queries
def test_filter_on_query_with_an_exclude_matrix(mfx):
    rows, cols, k, n_top = 150, 997, 12, 60
    rng = np.random.default_rng(11)
    W = rng.standard_normal((rows, k)).astype(F32)
    H = rng.standard_normal((cols, k)).astype(F32)
    users = np.arange(rows)
    S = chain_scores(W, H, users)
    ex = exclusion(mfx, rng, rows, cols, n_top, S)
    el = eligible_mask(ex, users, cols)
    keep1, keep2 = rng.random(cols) < 0.5, rng.random(cols) < 0.1
    with mfx.Recommender(W, H, 1, exclude=ex) as r:
        base = r.query(n_top)
        assert_exact(base, expected_topn(S, el, n_top), "no filter")
        r.set_item_filter(keep1)
        assert_exact(r.query(n_top), expected_topn(S, el & keep1, n_top), "filter 1")
        assert_exact(r.query(n_top, item_slices=5), expected_topn(S, el & keep1, n_top), "filter 1, 5 slices")
        r.set_item_filter(keep2.astype(np.uint8) * 3)   # replaced; any non-zero byte keeps
        assert_exact(r.query(n_top), expected_topn(S, el & keep2, n_top), "filter 2")
        sub = rng.choice(rows, 40)
        assert_exact(r.query(n_top, users=sub), expected_topn(S[sub], el[sub] & keep2, n_top), "filter 2, user list")
        r.set_item_filter(None)
        again = r.query(n_top)
        assert same(again[0], base[0]) and same(again[1], base[1])
        r.similar_setup()
        r.set_item_filter(keep1)
        assert_exact(r.query(n_top), expected_topn(S, el & keep1, n_top), "filter 1 after similar_setup")
        q = np.arange(0, cols, 9)                 # the exclude matrix plays no part in similar_items
        assert_exact(r.similar_items(n_top, q, metric=mfx.MFX_SIM_DOT),
                     expected_similar(chain_scores(H, H, q), q, n_top, DOT, None, keep1), "similar beside exclude")
        r.set_item_filter(None)
        again = r.query(n_top)
        assert same(again[0], base[0]) and same(again[1], base[1])


@pytest.mark.parametrize("k", [12, 160])
def test_filter_on_fold_in(mfx, k):
    from test_gpu_foldin import factors, segments
    cols, n_top, lam = 3001, 10, 0.1
    rng = np.random.default_rng(k)
    sizes = list(rng.integers(0, 400, 40))
    sizes[::11] = [0] * len(sizes[::11])
    sizes += [cols - 5, cols, 2500]
    ptr, idx, val = segments(60 + k, cols, sizes)
    W, H = factors(60 + k, cols, k)
    n = len(sizes)
    ex = mfx.dataset.from_coo(n, cols, np.repeat(np.arange(n), np.diff(ptr.astype(np.int64))), idx, val)
    el = eligible_mask(ex, np.arange(n), cols)
    keep = rng.random(cols) < 0.5
    with mfx.Recommender(W, H, 1) as r:
        if k <= 128:
            r.fold_in_setup(mfx.MFX_FOLD_ALS, lam)
        else:
            r.fold_in_block_setup(lam, 2.0, block=64, sweeps=2)
        bi, bs, bw = r.fold_in((ptr, idx, val), n_top)
        S = chain_scores(bw, H, np.arange(n))
        assert_exact((bi, bs), expected_topn(S, el, n_top), f"k={k} no filter")
        r.set_item_filter(keep)
        fi, fs, fw = r.fold_in((ptr, idx, val), n_top)
        assert same(fw, bw)                       # the solve still sees all of the user's entries
        assert_exact((fi, fs), expected_topn(S, el & keep, n_top), f"k={k} filter")
        r.set_item_filter(None)
        ai, as_, aw = r.fold_in((ptr, idx, val), n_top)
        assert same(ai, bi) and same(as_, bs) and same(aw, bw)


# ------------------------------------------------------------------------------------------------ h. refusals
def test_refusals_leave_the_handle_usable(mfx):
    cols, k, n_top = 400, 6, 10
    rng = np.random.default_rng(9)
    H = rng.standard_normal((cols, k)).astype(F32)
    W = rng.standard_normal((3, k)).astype(F32)
    lib = mfx.lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    q = np.array([1, 2, 3], np.uint32)
    items = np.zeros((3, 1024), np.uint32)
    scores = np.zeros((3, 1024), F32)
    n2 = np.zeros(cols, F32)
    keep = np.ones(cols, np.uint8)

    def similar(h, nq=3, qi=q, metric=1, n=n_top, space=0, slices=0):
        return lib.mfx_rec_similar(h, nq, vp(qi), metric, 1, n, vp(items), vp(scores), space, slices)

    def refused(rc, word):
        msg = lib.mfx_last_error().decode()
        assert rc == MFX_ERR_INVALID and word in msg, (rc, msg)

    with mfx.Recommender(W, H, 1) as r:
        refused(similar(r.handle), "mfx_rec_similar_setup")
        refused(lib.mfx_rec_item_norms(r.handle, vp(n2), None, 0), "mfx_rec_similar_setup")
        good_q = r.query(n_top)
        r.similar_setup()
        good = r.similar_items(n_top, q)
        refused(similar(r.handle, metric=2), "metric")
        refused(similar(r.handle, metric=-1), "metric")
        refused(similar(r.handle, n=0), "n_top")
        refused(similar(r.handle, n=1025), "n_top")
        refused(similar(r.handle, n=1024, slices=9), "item_slices")
        refused(similar(r.handle, n=n_top, slices=820), "item_slices")
        refused(similar(r.handle, qi=np.array([1, cols, 3], np.uint32)), "query item")
        refused(lib.mfx_rec_similar(r.handle, cols + 1, None, 1, 1, n_top, vp(items), None, 0, 0), "query_items")
        refused(similar(r.handle, space=7), "memory space")
        refused(lib.mfx_rec_item_norms(r.handle, vp(n2), None, 7), "memory space")
        refused(lib.mfx_rec_set_item_filter(r.handle, vp(keep), 7), "memory space")
        refused(similar(None), "null recommender")
        again = r.similar_items(n_top, q)
        assert same(again[0], good[0]) and same(again[1], good[1])
        assert_exact(good, expected_similar(chain_scores(H, H, q), q, n_top, COSINE, r.item_norms()[1]), "after refusals")
        again_q = r.query(n_top)
        assert same(again_q[0], good_q[0]) and same(again_q[1], good_q[1])
