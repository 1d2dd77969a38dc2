"""Top-N recommendations (mfx_rec_*, mfx.Recommender) checked bit for bit against the exact fp32 reference of
tests/rec_exact.py: the returned items equal the reference ranking, and the returned scores equal the fp32 FMA chain
over t ascending, bit for bit.  The shapes drive every MFMA chunking, mid-stream flushes at every candidate list
size, empty and full merge slices, user-chunked launches and partial workgroups."""
import numpy as np
import pytest

from rec_exact import PAD, chain_scores, eligible_mask, expected_topn

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1, m.lib().mfx_last_error()
    return m


def host(a):
    """numpy view of a query result (torch int32 items become their uint32 bits)."""
    if not isinstance(a, np.ndarray):
        a = a.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def assert_exact(got, want, what):
    gi, gs = host(got[0]), host(got[1])
    wi, ws = want
    assert gi.shape == wi.shape, (what, gi.shape, wi.shape)
    bad = np.nonzero((gi != wi).any(axis=1) | (gs.view(np.uint32) != ws.view(np.uint32)).any(axis=1))[0]
    if bad.size:
        s = bad[0]
        p = np.nonzero((gi[s] != wi[s]) | (gs[s].view(np.uint32) != ws[s].view(np.uint32)))[0][:6]
        pytest.fail(f"{what}: {bad.size} rows differ; row {s} at {p.tolist()}: items {gi[s, p].tolist()} vs "
                    f"{wi[s, p].tolist()}, scores {gs[s, p].tolist()} vs {ws[s, p].tolist()}")


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


def expect(S, ex, users, n_top):
    return expected_topn(S, eligible_mask(ex, users, S.shape[1]), n_top)


# ------------------------------------------------------------------------------------------------ a. score bits
KS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 256, 257, 1000, 1024]


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


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("regime", ["normal", "scaled", "subnormal", "huge"])
def test_score_bits_full_lists(mfx, regime, k):
    rows, cols, n_top = 130, 997, 1024
    W, H = regime_factors(regime, rows, cols, k, seed=1000 * k + len(regime))
    users = np.arange(rows)
    want = expect(chain_scores(W, H, users), None, users, n_top)
    if regime == "huge":
        assert np.isneginf(want[1]).any() and np.isposinf(want[1]).any() and (want[0] == PAD).any()
    for layout in (1, 0):
        Wl, Hl = (W, H) if layout == 1 else (np.ascontiguousarray(W.T), np.ascontiguousarray(H.T))
        with mfx.Recommender(Wl, Hl, layout) as r:
            assert_exact(r.query(n_top), want, f"{regime} k={k} layout={layout}")


# ------------------------------------------------------------------------------------------------ b. mid-stream flushes
FLUSH_NTOP = [1, 31, 32, 33, 96, 97, 224, 225, 480, 481, 992, 993, 1024]


@pytest.fixture(scope="module", params=["random", "increasing", "decreasing", "ties"])
def flush_case(request):
    rows, cols, k = 224, 6007, 8
    rng = np.random.default_rng(["random", "increasing", "decreasing", "ties"].index(request.param))
    W = rng.standard_normal((rows, k)).astype(F32)
    if request.param == "random":
        H = rng.standard_normal((cols, k))
    elif request.param in ("increasing", "decreasing"):
        W = rng.uniform(0.5, 1.0, (rows, k)).astype(F32)
        ramp = np.arange(1, cols + 1) if request.param == "increasing" else np.arange(cols, 0, -1)
        H = ramp[:, None] * rng.uniform(0.5, 1.0, k)[None, :]
    else:
        H = rng.standard_normal((5, k))[rng.integers(0, 5, cols)]
    H = H.astype(F32)
    return request.param, W, H, chain_scores(W, H, np.arange(rows))


@pytest.mark.parametrize("n_top", FLUSH_NTOP)
def test_mid_stream_flushes(mfx, flush_case, n_top):
    order, W, H, S = flush_case
    rng = np.random.default_rng(n_top)
    ex = exclusion(mfx, rng, *S.shape, n_top, S)
    users = np.arange(S.shape[0])
    want = expect(S, ex, users, n_top)
    with mfx.Recommender(W, H, 1, exclude=ex) as r:
        assert_exact(r.query(n_top, item_slices=1), want, f"{order} n_top={n_top}")


# ------------------------------------------------------------------------------------------------ c. slices and merge
@pytest.fixture(scope="module")
def slice_case(mfx):
    rows, cols, k = 150, 3001, 24
    rng = np.random.default_rng(77)
    W = rng.standard_normal((rows, k)).astype(F32)
    H = rng.standard_normal((cols, k)).astype(F32)
    H[2000:2100] = H[10:110]          # ties across slices: the merge must order them by item
    H[500:540] = H[5]
    S = chain_scores(W, H, np.arange(rows))
    return W, H, S


@pytest.mark.parametrize("n_top", [1, 33, 250, 1024])
def test_slices_and_merge(mfx, slice_case, n_top):
    W, H, S = slice_case
    rows, cols = S.shape
    nblk = (cols + 31) // 32
    ex = exclusion(mfx, np.random.default_rng(n_top), rows, cols, n_top, S)
    users = np.arange(rows)
    want = expect(S, ex, users, n_top)
    slices = sorted({s for s in (0, 1, 2, 3, 7, nblk, nblk + 5, 8192 // n_top) if s * n_top <= 8192})
    assert 8192 // n_top in slices
    with mfx.Recommender(W, H, 1, exclude=ex) as r:
        one = r.query(n_top, item_slices=1)
        assert_exact(one, want, f"n_top={n_top} slices=1")
        for sl in slices:
            got = r.query(n_top, item_slices=sl)
            assert_exact(got, want, f"n_top={n_top} slices={sl}")
            assert np.array_equal(got[0], one[0]) and np.array_equal(got[1].view(np.uint32), one[1].view(np.uint32))


# ------------------------------------------------------------------------------------------------ d. user chunking
def test_user_chunked_launches(mfx):
    rows, cols, k, n_top, slices = 8500, 1500, 8, 1024, 8
    # Recommender::query: L = pow2 >= n_top + 32 (from 64); users per launch = 1 GiB / (slices * L * 8 bytes), rounded
    # down to a multiple of 128 users
    L = 64
    while L < n_top + 32:
        L *= 2
    cap = max(128, ((1 << 30) // (slices * L * 8)) // 128 * 128)
    assert cap == 8192 and rows > cap
    rng = np.random.default_rng(8500)
    W = rng.standard_normal((rows, k)).astype(F32)
    H = rng.standard_normal((cols, k)).astype(F32)
    ex = exclusion(mfx, rng, rows, cols, n_top)
    users = rng.permutation(rows)
    users[200:400] = users[5000:5200]                 # duplicates, also across the launch boundary
    users[cap - 2:cap + 2] = users[10:14]
    with mfx.Recommender(W, H, 1, exclude=ex) as r:
        parts = [r.query(n_top, users=np.arange(b, min(rows, b + 4000)), item_slices=slices)
                 for b in range(0, rows, 4000)]
        base_i = np.concatenate([p[0] for p in parts])
        base_s = np.concatenate([p[1] for p in parts])
        all_i, all_s = r.query(n_top, item_slices=slices)
        lst_i, lst_s = r.query(n_top, users=users, item_slices=slices)
    assert np.array_equal(all_i, base_i) and np.array_equal(all_s.view(np.uint32), base_s.view(np.uint32))
    assert np.array_equal(lst_i, base_i[users]) and np.array_equal(lst_s.view(np.uint32), base_s[users].view(np.uint32))
    slots = np.unique(np.concatenate([[0, 127, 128, cap - 1, cap, cap + 1, rows - 1], rng.choice(rows, 20)]))
    for name, us, (gi, gs) in (("users=None", slots, (all_i, all_s)), ("users list", users[slots], (lst_i, lst_s))):
        want = expect(chain_scores(W, H, us), ex, us, n_top)
        assert_exact((gi[slots], gs[slots]), want, f"{name}, slots {slots.tolist()}")


# ------------------------------------------------------------------------------------------------ e. partial workgroups
@pytest.mark.parametrize("nusers", [1, 31, 32, 33, 127, 128, 129])
def test_partial_workgroups(mfx, nusers):
    import torch
    rows, cols, k = 300, 700, 12
    rng = np.random.default_rng(nusers)
    W = rng.standard_normal((rows, k)).astype(F32)
    H = rng.standard_normal((cols, k)).astype(F32)
    S = chain_scores(W, H, np.arange(rows))
    users = rng.choice(rows, nusers).astype(np.uint32)
    for n_top in (20, 700):
        ex = exclusion(mfx, rng, *S.shape, n_top, S)
        want = expect(S[users], ex, users, n_top)
        with mfx.Recommender(W, H, 1, exclude=ex) as r:
            assert_exact(r.query(n_top, users=users), want, f"host nusers={nusers} n_top={n_top}")
        with mfx.Recommender(torch.from_numpy(W).cuda(), torch.from_numpy(H).cuda(), 1, exclude=ex) as r:
            got = r.query(n_top, users=torch.from_numpy(users.view(np.int32)).cuda())
            torch.cuda.synchronize()
            assert_exact(got, want, f"device nusers={nusers} n_top={n_top}")
