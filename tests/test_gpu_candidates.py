"""Candidate-list re-ranking and pair scoring (mfx_rec_query_candidates, mfx_rec_score; Recommender.query_candidates,
Recommender.score) checked bit for bit: items, eligible counts and score bits (compared as uint32) against the exact
reference of tests/cand_exact.py and against the handle's own query and rank_of, under exclusion rows, item filters,
ties, list lengths on both sides of every threshold of the kernel, batch order and memory space."""
import ctypes as C

import numpy as np
import pytest

from cand_exact import (canonical_lists, exclusion, expected_candidates, random_lists, regime_factors, whole_catalogue)
from rec_exact import PAD, chain_scores, eligible_mask, expected_topn

pytestmark = pytest.mark.gpu

F32 = np.float32
MFX_ERR_INVALID = -1  # include/mfx.h
ROWS, COLS = 130, 997  # one full workgroup and a two-slot one; 31 full tiles and one of 5 items
CHUNK = 2048           # candidates of one piece of work (rec_candidates.hip): longer lists are merged from partial lists


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1, m.lib().mfx_last_error()
    return m


@pytest.fixture(scope="module", params=["default", "group", "lane"])
def load_form(request):
    """Both forms of the gather of rec_candidates.hip, forced and as the library chooses between them, give the same bits
    (MFX_CAND_LOAD is read at every call)."""
    import os
    old = os.environ.pop("MFX_CAND_LOAD", None)
    if request.param != "default":
        os.environ["MFX_CAND_LOAD"] = request.param
    yield request.param
    os.environ.pop("MFX_CAND_LOAD", None)
    if old is not None:
        os.environ["MFX_CAND_LOAD"] = old


def host(a):
    """numpy view of a result (torch int32 tensors become their uint32 bits)."""
    if not isinstance(a, np.ndarray):
        a = a.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def assert_exact(got, want, what):
    names = ("items", "score bits", "n_eligible")
    for g, w, name in zip(got, want, names):
        g, w = host(g), np.asarray(w)
        if name == "score bits":
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        bad = np.argwhere(g != w)
        if bad.size:
            p = tuple(bad[:6].T)
            pytest.fail(f"{what}: {len(bad)} of {g.size} {name} differ; at {bad[:6].tolist()}: {g[p].tolist()} vs {w[p].tolist()}")


@pytest.fixture(scope="module")
def base_case():
    k = 17
    W, H = regime_factors("normal", ROWS, COLS, k, seed=4242)
    return W, H, chain_scores(W, H, np.arange(ROWS))


def lengths_for(rng, n_top, nslots):
    pool = np.array([0, 1, n_top - 1, n_top, n_top + 1, 63, 64, 65, 255, 256, 257, 997])
    pool = np.minimum(pool, COLS)
    lens = pool[np.arange(nslots) % pool.size]           # every length occurs about ten times, shuffled over the exclusion kinds
    return lens[rng.permutation(nslots)]


# ------------------------------------------------------------------------------------------------ a. the whole catalogue
@pytest.mark.parametrize("layout", [1, 0])
def test_whole_catalogue_lists_equal_the_handles_own_query(mfx, base_case, load_form, layout):
    W, H, S = base_case
    Wl, Hl = (W, H) if layout == 1 else (np.ascontiguousarray(W.T), np.ascontiguousarray(H.T))
    ptr, idx = whole_catalogue(ROWS, COLS)
    rng = np.random.default_rng(7)
    keep = rng.random(COLS) < 0.5
    for ex in (None, exclusion(mfx, rng, ROWS, COLS, 10, S)):
        el = eligible_mask(ex, np.arange(ROWS), COLS)
        with mfx.Recommender(Wl, Hl, layout, exclude=ex) as r:
            for filt in (None, keep):
                r.set_item_filter(filt)
                n_el = (el & (keep[None, :] if filt is not None else True)).sum(1).astype(np.uint32)
                for n_top in (1, 10, 1024):
                    qi, qs = r.query(n_top)
                    got = r.query_candidates(n_top, (ptr, idx), canonical=True, return_counts=True)
                    assert_exact(got, (qi, qs, n_el), f"whole catalogue, layout {layout}, exclusion {ex is not None}, "
                                                      f"filter {filt is not None}, n_top {n_top}")


# ------------------------------------------------------------------------------------------------ b. random lists
@pytest.mark.parametrize("n_top", [1, 10, 100])
def test_random_lists_under_exclusion_flag_and_filter(mfx, base_case, load_form, n_top):
    W, H, S = base_case
    rng = np.random.default_rng(100 + n_top)
    ex = exclusion(mfx, rng, ROWS, COLS, n_top, S)
    el = eligible_mask(ex, np.arange(ROWS), COLS)
    keep = rng.random(COLS) < 0.5
    ptr, idx = random_lists(rng, lengths_for(rng, n_top, ROWS), COLS)
    with mfx.Recommender(W, H, 1, exclude=ex) as r:
        for filt in (None, keep):
            r.set_item_filter(filt)
            f = keep[None, :] if filt is not None else True
            want = expected_candidates(S, ptr, idx, el & f, n_top)
            assert_exact(r.query_candidates(n_top, (ptr, idx), canonical=True, return_counts=True), want,
                         f"n_top {n_top}, filter {filt is not None}")
            want = expected_candidates(S, ptr, idx, f, n_top)
            assert_exact(r.query_candidates(n_top, (ptr, idx), apply_exclude=False, canonical=True, return_counts=True), want,
                         f"MFX_CAND_NO_EXCLUDE, n_top {n_top}, filter {filt is not None}")
        assert want[2][ptr[:-1] == ptr[1:]].tolist() == [0] * int((ptr[:-1] == ptr[1:]).sum())
    with mfx.Recommender(W, H, 1) as r:                    # a handle without exclusion rows
        assert_exact(r.query_candidates(n_top, (ptr, idx), canonical=True, return_counts=True),
                     expected_candidates(S, ptr, idx, True, n_top), f"no exclusion, n_top {n_top}")


def test_one_whole_catalogue_slot_among_short_ones(mfx, base_case, load_form):
    W, H, S = base_case
    rng = np.random.default_rng(33)
    lens = rng.integers(0, 4, ROWS)
    lens[77] = COLS
    ptr, idx = random_lists(rng, lens, COLS)
    users = rng.permutation(ROWS)
    ex = exclusion(mfx, rng, ROWS, COLS, 10, S)
    el = eligible_mask(ex, users, COLS)
    with mfx.Recommender(W, H, 1, exclude=ex) as r:
        for n_top in (10, 1024):
            want = expected_candidates(S[users], ptr, idx, el, n_top)
            assert_exact(r.query_candidates(n_top, (ptr, idx), users=users, canonical=True, return_counts=True), want, f"skew, n_top {n_top}")


# ------------------------------------------------------------------------------------------------ c. lists longer than a chunk
def test_lists_longer_than_a_chunk_are_merged_from_their_pieces(mfx, load_form):
    """Lengths on both sides of the chunk and of its multiples, lists that start, end and lie across chunk boundaries of
    the global candidate position, short lists between them; the whole catalogue against the handle's own query."""
    rows, cols, k = 24, 6007, 8
    rng = np.random.default_rng(6007)
    W = rng.standard_normal((rows, k)).astype(F32)
    H = rng.standard_normal((cols, k)).astype(F32)
    H[3000:3100] = H[10:110]                               # ties across pieces
    S = chain_scores(W, H, np.arange(rows))
    lens = np.array([cols, 0, CHUNK, 3, CHUNK + 1, 2 * CHUNK, 45, 2 * CHUNK + 1, CHUNK - 1, cols, CHUNK - 3, 1, 0, 2 * CHUNK - 5,
                     5, cols, 700, 2049, 1, 4000, 0, 2047, 2048, cols])
    lens[2] = CHUNK - lens[:2].sum() % CHUNK + CHUNK       # slot 2 ends on a boundary and is longer than a chunk
    assert lens.size == rows and (np.cumsum(lens)[2] % CHUNK) == 0
    ptr, idx = random_lists(rng, lens, cols)
    ex = exclusion(mfx, rng, rows, cols, 20, S)
    el = eligible_mask(ex, np.arange(rows), cols)
    keep = rng.random(cols) < 0.5
    with mfx.Recommender(W, H, 1, exclude=ex) as r:
        for n_top in (1, 10, 1000, 1024):
            want = expected_candidates(S, ptr, idx, el, n_top)
            assert_exact(r.query_candidates(n_top, (ptr, idx), canonical=True, return_counts=True), want, f"long lists, n_top {n_top}")
        r.set_item_filter(keep)
        assert_exact(r.query_candidates(10, (ptr, idx), canonical=True, return_counts=True),
                     expected_candidates(S, ptr, idx, el & keep[None, :], 10), "long lists, filter")
        r.set_item_filter(None)
        wp, wi = whole_catalogue(rows, cols)
        for n_top in (10, 1024):
            qi, qs = r.query(n_top)
            got = r.query_candidates(n_top, (wp, wi), canonical=True)
            assert_exact(got, (qi, qs), f"whole catalogue of {cols}, n_top {n_top}")
        times = r.candidates_times()
        assert set(times) == {"check", "score", "select"} and all(t > 0 for t in times.values())


# ------------------------------------------------------------------------------------------------ d. ranks and regimes
@pytest.mark.parametrize("k", [1, 3, 64, 65, 128, 130])
def test_every_rank_path(mfx, load_form, k):
    W, H = regime_factors("normal", ROWS, COLS, k, seed=50 + k)
    S = chain_scores(W, H, np.arange(ROWS))
    rng = np.random.default_rng(k)
    ptr, idx = random_lists(rng, lengths_for(rng, 10, ROWS), COLS)
    want = expected_candidates(S, ptr, idx, True, 10)
    for layout in (1, 0):
        Wl, Hl = (W, H) if layout == 1 else (np.ascontiguousarray(W.T), np.ascontiguousarray(H.T))
        with mfx.Recommender(Wl, Hl, layout) as r:
            assert_exact(r.query_candidates(10, (ptr, idx), canonical=True, return_counts=True), want, f"k {k}, layout {layout}")


def test_rank_1024(mfx, load_form):
    rows, cols, k = 40, 200, 1024
    W, H = regime_factors("normal", rows, cols, k, seed=1024)
    S = chain_scores(W, H, np.arange(rows))
    rng = np.random.default_rng(1024)
    ptr, idx = random_lists(rng, rng.integers(0, cols + 1, rows), cols)
    with mfx.Recommender(W, H, 1) as r:
        assert_exact(r.query_candidates(10, (ptr, idx), canonical=True, return_counts=True), expected_candidates(S, ptr, idx, True, 10), "k 1024")
        uu, ii = np.divmod(np.arange(rows * cols), cols)
        assert np.array_equal(r.score(uu, ii).view(np.uint32), S.reshape(-1).view(np.uint32))


@pytest.fixture(scope="module", params=["normal", "scaled", "subnormal", "huge"])
def regime_case(request):
    k = 33
    W, H = regime_factors(request.param, ROWS, COLS, k, seed=len(request.param))
    return request.param, W, H, chain_scores(W, H, np.arange(ROWS))


def test_factor_regimes(mfx, regime_case, load_form):
    regime, W, H, S = regime_case
    if regime == "huge":    # the NaN, +inf and -inf branches are taken
        assert np.isnan(S).any() and np.isposinf(S).any() and np.isneginf(S).any()
    if regime == "subnormal":
        assert (S == 0).any() and np.signbit(S[S == 0]).any() and (np.abs(S[S != 0]) < 2.0 ** -126).any()
    rng = np.random.default_rng(5)
    ptr, idx = random_lists(rng, lengths_for(rng, 20, ROWS), COLS)
    wp, wi = whole_catalogue(ROWS, COLS)
    with mfx.Recommender(W, H, 1) as r:
        assert_exact(r.query_candidates(20, (ptr, idx), canonical=True, return_counts=True), expected_candidates(S, ptr, idx, True, 20), regime)
        want = expected_topn(S, True, 1024) + ((~np.isnan(S)).sum(1).astype(np.uint32),)
        assert_exact(r.query_candidates(1024, (wp, wi), canonical=True, return_counts=True), want, f"{regime}, whole catalogue")


def test_score_bits_of_every_pair(mfx, regime_case, load_form):
    regime, W, H, S = regime_case
    uu, ii = np.divmod(np.arange(ROWS * COLS), COLS)
    perm = np.random.default_rng(1).permutation(uu.size)
    for layout in (1, 0):
        Wl, Hl = (W, H) if layout == 1 else (np.ascontiguousarray(W.T), np.ascontiguousarray(H.T))
        with mfx.Recommender(Wl, Hl, layout) as r:
            got = r.score(uu, ii)
            assert got.dtype == F32 and np.array_equal(got.view(np.uint32), S.reshape(-1).view(np.uint32)), (regime, layout)
            assert np.array_equal(r.score(uu[perm], ii[perm]).view(np.uint32), got[perm].view(np.uint32))
            if layout == 1:
                assert np.array_equal(r.rank_of(uu, ii)[1].view(np.uint32), got.view(np.uint32)), f"{regime}: score != rank_of scores"
                assert r.score(uu[:0], ii[:0]).shape == (0,)
                dev = r.score(uu[perm[:5000]], ii[perm[:5000]], on_device=True)
                assert dev.is_cuda and np.array_equal(host(dev).view(np.uint32), got[perm[:5000]].view(np.uint32))


# ------------------------------------------------------------------------------------------------ e. ties
def test_ties_are_decided_by_item_id(mfx, load_form):
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
    ptr, idx = random_lists(rng, lengths_for(rng, 50, ROWS), COLS)
    ptr2, idx2 = whole_catalogue(ROWS, COLS)
    ex = exclusion(mfx, rng, ROWS, COLS, 20, S)
    for e in (ex, None):
        el = eligible_mask(e, np.arange(ROWS), COLS)
        with mfx.Recommender(W, H, 1, exclude=e) as r:
            assert_exact(r.query_candidates(50, (ptr, idx), canonical=True, return_counts=True), expected_candidates(S, ptr, idx, el, 50),
                         f"ties, exclusion {e is not None}")
            got = r.query_candidates(1024, (ptr2, idx2), canonical=True, return_counts=True)
            assert_exact(got, expected_candidates(S, ptr2, idx2, el, 1024), f"ties, whole catalogue, exclusion {e is not None}")
    assert np.array_equal(got[0][120, :COLS], np.arange(COLS))  # all-zero user, no exclusion row: item order


# ------------------------------------------------------------------------------------------------ f. independence
def test_batch_order_and_memory_space_do_not_matter(mfx, base_case):
    import torch
    W, H, S = base_case
    rng = np.random.default_rng(8)
    ex = exclusion(mfx, rng, ROWS, COLS, 10, S)
    ptr, idx = random_lists(rng, lengths_for(rng, 10, ROWS), COLS)
    n_top = 10
    want = expected_candidates(S, ptr, idx, eligible_mask(ex, np.arange(ROWS), COLS), n_top)
    sel = np.concatenate([rng.permutation(ROWS), rng.integers(0, ROWS, 70)])      # slots permuted, with duplicates

    def take(sel):
        lens = (ptr[1:] - ptr[:-1])[sel]
        p = np.zeros(sel.size + 1, np.int64)
        np.cumsum(lens, out=p[1:])
        i = np.concatenate([idx[ptr[q]:ptr[q + 1]] for q in sel]) if sel.size else idx[:0]
        return p.astype(np.uint32), i.astype(np.uint32)

    with mfx.Recommender(W, H, 1, exclude=ex) as r:
        base = r.query_candidates(n_top, (ptr, idx), canonical=True, return_counts=True)        # users NULL
        assert_exact(base, want, "users = None")
        assert_exact(r.query_candidates(n_top, (ptr, idx), users=np.arange(ROWS), canonical=True, return_counts=True), want, "users given")
        assert_exact(r.query_candidates(n_top, take(sel), users=sel, canonical=True, return_counts=True), [b[sel] for b in base], "permuted")
        for q in (0, 11, ROWS - 1):
            one = r.query_candidates(n_top, take(np.array([q])), users=[q], canonical=True, return_counts=True)
            assert_exact(one, [b[q:q + 1] for b in base], f"a batch of slot {q} alone")
        items_only = r.query_candidates(n_top, (ptr, idx), canonical=True)
        assert len(items_only) == 2 and np.array_equal(items_only[0], base[0])
        tp, ti = (torch.from_numpy(a.view(np.int32)).cuda() for a in take(sel))
        tu = torch.from_numpy(sel.astype(np.uint32).view(np.int32)).cuda()
        dev = r.query_candidates(n_top, (tp, ti), users=tu, canonical=True, return_counts=True)
        torch.cuda.synchronize()
        assert all(t.is_cuda for t in dev) and dev[0].dtype == torch.int32 and dev[1].dtype == torch.float32 and dev[2].dtype == torch.int32
        assert_exact(dev, [b[sel] for b in base], "device tensors")
        assert_exact(r.query_candidates(n_top, (ptr, idx), canonical=True, on_device=True, return_counts=True), base, "on_device")
        empty = r.query_candidates(n_top, (np.zeros(1, np.uint32), idx[:0]), users=[], canonical=True, return_counts=True)
        assert [a.shape for a in empty] == [(0, n_top), (0, n_top), (0,)]
    with mfx.Recommender(torch.from_numpy(W).cuda(), torch.from_numpy(H).cuda(), 1, exclude=ex) as r:
        assert_exact(r.query_candidates(n_top, (ptr, idx), canonical=True, return_counts=True), base, "device factors")


# ------------------------------------------------------------------------------------------------ g. refusals
def test_refusals_leave_the_handle_usable(mfx, base_case):
    W, H, S = base_case
    lib = mfx.lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    n_top = 5
    good_ptr = np.array([0, 3, 3, 7], np.uint32)
    good_idx = np.array([1, 5, 9, 0, 2, 4, COLS - 1], np.uint32)
    users = np.array([4, 0, ROWS - 1], np.uint32)
    want = expected_candidates(S[users], good_ptr, good_idx, True, n_top)
    items, scores, nel = np.zeros((3, n_top), np.uint32), np.zeros((3, n_top), F32), np.zeros(3, np.uint32)

    def call(h, ptr=good_ptr, idx=good_idx, u=users, flags=0, n=n_top, out=items, space=0):
        return lib.mfx_rec_query_candidates(h, 3, vp(u), vp(ptr), vp(idx), flags, n, vp(out), vp(scores), vp(nel), space)

    def edit(a, pos, val):
        b = a.copy()
        b[pos] = val
        return b

    cases = [
        ("strictly ascending", "slot 2", lambda h: call(h, idx=edit(good_idx, 5, 1))),        # 0 2 1: a descending pair
        ("strictly ascending", "slot 0", lambda h: call(h, idx=edit(good_idx, 1, 1))),        # 1 1: a repeated id
        ("out of range", "slot 2", lambda h: call(h, idx=edit(good_idx, 6, COLS))),
        ("non-decreasing", "slot 1", lambda h: call(h, ptr=np.array([0, 3, 2, 7], np.uint32))),
        ("non-decreasing", "slot 0", lambda h: call(h, ptr=np.array([1, 3, 3, 7], np.uint32))),
        ("n_top", "", lambda h: call(h, n=0)),
        ("n_top", "", lambda h: call(h, n=1025)),
        ("flag", "", lambda h: call(h, flags=2)),
        ("flag", "", lambda h: call(h, flags=-1)),
        ("user id", "", lambda h: call(h, u=edit(users, 1, ROWS))),
        ("cand_ptr is NULL", "", lambda h: call(h, ptr=None)),
        ("items is NULL", "", lambda h: call(h, out=None)),
        ("cand_idx is NULL", "", lambda h: call(h, idx=None)),
        ("memory space", "", lambda h: call(h, space=7)),
    ]
    with mfx.Recommender(W, H, 1) as r:
        for word, slot, f in cases:
            code = f(r.handle)
            msg = lib.mfx_last_error().decode()
            assert code == MFX_ERR_INVALID and word in msg and slot in msg, (word, slot, code, msg)
            assert call(r.handle) == 0, (word, lib.mfx_last_error().decode())
            assert_exact((items, scores, nel), want, f"after the refusal of {word}")
        # the first offending slot is the one named
        assert call(r.handle, idx=np.array([5, 1, 9, 0, 2, 4, COLS], np.uint32)) == MFX_ERR_INVALID
        assert "slot 0" in lib.mfx_last_error().decode()
        # nothing to do; empty lists need no ids; scores and counts may be left out
        assert lib.mfx_rec_query_candidates(r.handle, 0, None, None, None, 0, n_top, None, None, None, 0) == 0
        assert call(r.handle, ptr=np.zeros(4, np.uint32), idx=None) == 0 and np.all(items == PAD) and np.all(nel == 0)
        assert lib.mfx_rec_query_candidates(r.handle, 3, vp(users), vp(good_ptr), vp(good_idx), 0, n_top, vp(items), None, None, 0) == 0
        assert np.array_equal(items, want[0])
        # mfx_rec_score
        u, i, s = np.array([0, ROWS - 1], np.uint32), np.array([COLS - 1, 0], np.uint32), np.zeros(2, F32)
        for word, f in (("user id", lambda: lib.mfx_rec_score(r.handle, 2, vp(edit(u, 0, ROWS)), vp(i), vp(s), 0)),
                        ("item id", lambda: lib.mfx_rec_score(r.handle, 2, vp(u), vp(edit(i, 1, COLS)), vp(s), 0)),
                        ("scores is NULL", lambda: lib.mfx_rec_score(r.handle, 2, vp(u), vp(i), None, 0)),
                        ("memory space", lambda: lib.mfx_rec_score(r.handle, 2, vp(u), vp(i), vp(s), 5))):
            code = f()
            msg = lib.mfx_last_error().decode()
            assert code == MFX_ERR_INVALID and word in msg, (word, code, msg)
            assert lib.mfx_rec_score(r.handle, 2, vp(u), vp(i), vp(s), 0) == 0
            assert np.array_equal(s.view(np.uint32), S[u, i].view(np.uint32))
        assert lib.mfx_rec_score(r.handle, 0, None, None, None, 0) == 0


# ------------------------------------------------------------------------------------------------ h. the wrapper
def test_wrapper_canonicalises_lists(mfx, base_case):
    import torch
    W, H, S = base_case
    rng = np.random.default_rng(12)
    lens = rng.integers(0, 80, ROWS)
    ptr = np.zeros(ROWS + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    idx = rng.integers(0, COLS, ptr[-1])                   # unsorted, with repeats
    idx[rng.random(idx.size) < 0.1] = PAD
    cp, ci = canonical_lists(ptr, idx)
    A = rng.integers(0, COLS, (ROWS, 40))                  # [U, C] as an ANN index returns them, short lists padded
    A[rng.random(A.shape) < 0.2] = PAD
    ap, ai = canonical_lists(np.arange(ROWS + 1) * 40, A.reshape(-1))
    n_top = 10
    with mfx.Recommender(W, H, 1) as r:
        want = r.query_candidates(n_top, (cp, ci), canonical=True, return_counts=True)
        assert_exact(want, expected_candidates(S, cp, ci, True, n_top), "canonical form")
        assert_exact(r.query_candidates(n_top, (ptr, idx), return_counts=True), want, "unsorted lists with repeats")
        class Csr:
            csr_row_ptr, csr_col_idx = ptr, idx
        assert_exact(r.query_candidates(n_top, Csr(), return_counts=True), want, "an object with csr_row_ptr / csr_col_idx")
        tp, ti = torch.from_numpy(ptr).cuda(), torch.from_numpy(idx).cuda()
        assert_exact(r.query_candidates(n_top, (tp, ti), return_counts=True), want, "unsorted lists, tensors")
        want2 = r.query_candidates(n_top, (ap, ai), canonical=True, return_counts=True)
        assert_exact(r.query_candidates(n_top, A, return_counts=True), want2, "[U, C] array")
        assert_exact(r.query_candidates(n_top, torch.from_numpy(A).cuda(), return_counts=True), want2, "[U, C] tensor")
        with pytest.raises(mfx.MfxError, match="strictly ascending"):
            r.query_candidates(n_top, (ptr, np.where(idx == PAD, 0, idx)), canonical=True)
