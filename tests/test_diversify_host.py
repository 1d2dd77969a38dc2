"""Diversity re-ranking (mfx_rec_diversify) without a GPU: the symbols and their bindings, the refusal of a NULL handle, the
argument checks of the Python surface that raise before the library is called, and self-checks of the exact reference
in diversify_exact.py: tradeoff = 1 is the reference top-N, the tie order, negative similarities, and less alike lists
on planted clusters."""
import ctypes as C
import inspect

import numpy as np
import pytest

from cand_exact import expected_candidates, random_lists
from diversify_exact import (diversify_slot, expected_diversify, intra_list_cosine, item_gram, planted_clusters,
                             similarities)
from rec_exact import PAD, chain_scores, expected_topn
from sim_exact import COSINE, DOT, inv_norm64, item_n2

MFX_ERR_INVALID = -1  # include/mfx.h
F32 = np.float32


def bits(a):
    return np.asarray(a, F32).view(np.uint32)


def test_symbols_are_exported_with_the_declared_argument_types():
    import mfx
    from mfx import _lib
    lib = mfx.lib()                # (first: it maps the one HIP runtime the process keeps, which a bare CDLL would not)
    raw = C.CDLL(_lib.LIB_PATH)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    want = {
        "mfx_rec_diversify": [vp, i64, vp, vp, vp, vp, i32, C.c_int, C.c_float, i32, vp, vp, vp, vp, C.c_int, C.c_int],
        "mfx_rec_diversify_times": [vp, C.POINTER(C.c_double)],
    }
    for name, args in want.items():
        assert hasattr(raw, name), name
        res, got = _lib.SIGNATURES[name]
        assert res is C.c_int and list(got) == args, name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert mfx.MFX_DIV_NO_EXCLUDE == 1
    assert lib.mfx_version() == 2 == _lib.MFX_VERSION


def test_a_null_handle_is_refused():
    import mfx
    lib = mfx.lib()
    u = np.zeros(4, np.uint32)
    f = np.zeros(4, F32)
    t = (C.c_double * 3)()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for rc in (lib.mfx_rec_diversify(None, 1, None, None, vp(u), vp(u), 0, 1, 0.5, 1, vp(u), vp(f), vp(f), None, 0, 0),
               lib.mfx_rec_diversify_times(None, t)):
        assert rc == MFX_ERR_INVALID
        assert "null recommender" in lib.mfx_last_error().decode()


def test_the_python_methods_exist():
    import mfx
    R = mfx.Recommender
    d = inspect.signature(R.diversify).parameters
    assert list(d) == ["self", "n_top", "candidates", "users", "vectors", "tradeoff", "metric", "apply_exclude", "canonical",
                       "on_device", "return_values", "return_counts", "form"]
    assert [d[n].default for n in list(d)[3:]] == [None, None, 0.5, mfx.MFX_SIM_COSINE, True, False, False, False, False, 0]
    q = inspect.signature(R.query_diverse).parameters
    assert list(q) == ["self", "n_top", "pool", "users", "tradeoff", "metric", "on_device"]
    assert [q[n].default for n in list(q)[3:]] == [None, 0.5, mfx.MFX_SIM_COSINE, False]
    assert list(inspect.signature(R.diversify_times).parameters) == ["self"]


class _NoLibrary:
    """A Recommender whose handle was never made: an argument check that lets a call through fails on the NULL handle
    with MfxError, not ValueError."""
    def __new__(cls, rows=10, cols=20):
        import mfx
        r = object.__new__(mfx.Recommender)
        r.handle, r.device, r.rows, r.cols, r.k, r.layout = C.c_void_p(), 0, rows, cols, 4, 1
        return r


def test_argument_checks_raise_before_the_library_is_called():
    import mfx
    r = _NoLibrary()
    ptr, idx = np.array([0, 2, 3]), np.array([1, 5, 2])
    V = np.zeros((2, 4), F32)
    bad = [
        dict(n_top=0), dict(n_top=129),
        dict(tradeoff=-0.1), dict(tradeoff=1.5), dict(tradeoff=float("nan")), dict(tradeoff=float("inf")),
        dict(metric=2), dict(form=3), dict(form=-1),
        dict(users=[0, 1, 2]),                                                # three users, two lists
        dict(users=[0, -1]),
        dict(candidates=(ptr, np.array([1, -5, 2]))),
        dict(candidates=(np.array([0, 3, 2]), idx)),                          # ptr decreases
        dict(candidates=(np.arange(12), np.zeros(11, np.int64))),             # 11 lists without users, 10 rows
        dict(vectors=V),                                                      # vectors need apply_exclude=False
        dict(vectors=V, users=[0, 1], apply_exclude=False),                   # users and vectors
        dict(vectors=np.zeros((2, 5), F32), apply_exclude=False),             # not [U, k]
        dict(vectors=np.zeros((3, 4), F32), apply_exclude=False),             # three vectors, two lists
        dict(vectors=np.zeros(4, F32), apply_exclude=False),                  # not 2-D
    ]
    for kw in bad:
        kw.setdefault("n_top", 3)
        kw.setdefault("candidates", (ptr, idx))
        with pytest.raises(ValueError):
            r.diversify(**kw)
    for kw in (dict(n_top=0, pool=10), dict(n_top=129, pool=200), dict(n_top=5, pool=4), dict(n_top=5, pool=1025)):
        with pytest.raises(ValueError):
            r.query_diverse(**kw)
    with pytest.raises(mfx.MfxError):                                         # a call that passes the checks reaches the library
        r.diversify(3, (ptr, idx))
    with pytest.raises(mfx.MfxError):
        r.diversify(3, (ptr, idx), vectors=V, apply_exclude=False)


# ------------------------------------------------------------------------------------------------ the reference
@pytest.fixture(scope="module")
def small_model():
    rng = np.random.default_rng(21)
    rows, cols, k = 12, 80, 7
    W = rng.standard_normal((rows, k)).astype(F32)
    H = rng.standard_normal((cols, k)).astype(F32)
    return W, H, chain_scores(W, H, np.arange(rows)), item_gram(H), inv_norm64(item_n2(H))


@pytest.mark.parametrize("metric", [DOT, COSINE])
def test_reference_tradeoff_one_is_the_reference_topn(small_model, metric):
    W, H, S, G, c = small_model
    rng = np.random.default_rng(3)
    S = S.copy()
    S[rng.random(S.shape) < 0.05] = np.nan
    S[:, 5] = S[:, 9]                                       # equal scores: the item id decides
    eligible = rng.random(S.shape) < 0.8
    ptr, idx = random_lists(rng, rng.integers(0, 40, S.shape[0]), S.shape[1])
    for n_top in (1, 7, 50):
        items, scores, values, n_el = expected_diversify(S, ptr, idx, eligible, G, n_top, 1.0, metric, c)
        wi, ws, wn = expected_candidates(S, ptr, idx, eligible, n_top)
        assert np.array_equal(items, wi) and np.array_equal(bits(scores), bits(ws)) and np.array_equal(n_el, wn)
        assert np.array_equal(bits(values), bits(ws))       # value = rel, and -inf at the padding
    full = expected_topn(S, eligible, 5)                    # the whole catalogue as the list
    ptr = (np.arange(S.shape[0] + 1) * S.shape[1]).astype(np.uint32)
    idx = np.tile(np.arange(S.shape[1], dtype=np.uint32), S.shape[0])
    got = expected_diversify(S, ptr, idx, eligible, G, 5, 1.0, metric, c)
    assert np.array_equal(got[0], full[0]) and np.array_equal(bits(got[1]), bits(full[1]))


def test_reference_tie_order():
    # items 0, 1, 2 share one row of H, item 3 is orthogonal to them: equal rel and equal similarities, the id decides
    H = np.array([[1, 0], [1, 0], [1, 0], [0, 1]], F32)
    G, c = item_gram(H), inv_norm64(item_n2(H))
    rel = np.array([2, 2, 2, 1], F32)
    items, scores, values = diversify_slot(rel, np.arange(4), G, 4, 0.5, COSINE, c)
    # step 1: values 1 1 1 .5 -> item 0; then D = 1 for 1 and 2, 0 for 3: values .5 .5 .5 -> rel decides: 1, then 2, then 3
    assert items.tolist() == [0, 1, 2, 3] and values.tolist() == [1.0, 0.5, 0.5, 0.5]
    # equal values, different rel: the greater rel first, although its id is greater
    rel = np.array([1, 3, 1, 2], F32)
    items, _, values = diversify_slot(rel, np.arange(4), G, 4, 0.0, COSINE, c)  # tradeoff 0: every value is -D
    assert items.tolist() == [1, 3, 0, 2] and bits(values).tolist() == bits([0.0, 0.0, -1.0, -1.0]).tolist()
    # -0 == +0 among the rels, NaN values count as -inf: a = 0 times rel = inf is NaN
    rel = np.array([-0.0, 0.0, np.inf, -0.0], F32)
    items, scores, values = diversify_slot(rel, np.array([4, 5, 6, 7]), np.zeros((8, 8), F32), 4, 0.0, DOT)
    assert items.tolist() == [4, 5, 7, 6] and np.isnan(values[3]) and np.isposinf(scores[3])
    # padding
    items, scores, values = diversify_slot(rel[:1], np.array([9]), np.zeros((10, 10), F32), 3, 0.5, DOT)
    assert items.tolist() == [9, PAD, PAD] and np.all(np.isneginf(scores[1:])) and np.all(np.isneginf(values[1:]))


def test_reference_negative_similarities_leave_d_at_zero():
    H = np.array([[1, 0], [-1, 1], [-1, -1], [0.6, 0.8]], F32)   # 1 and 2 oppose 0 and are orthogonal to each other
    G, c = item_gram(H), inv_norm64(item_n2(H))
    assert similarities(G, 0, np.array([1, 2]), COSINE, c).max() < 0
    rel = np.array([3, 1, 2, 0.5], F32)
    for metric in (DOT, COSINE):
        items, _, values = diversify_slot(rel, np.arange(4), G, 3, 0.5, metric, c)
        # after item 0 the opposed items 1 and 2 keep D = 0 (value = rel / 2, no bonus); item 3 pays for its likeness
        assert items.tolist() == [0, 2, 1] and values.tolist() == [1.5, 1.0, 0.5]
    # a NaN similarity leaves D as it was
    Gn = G.copy()
    Gn[0, 3] = Gn[3, 0] = np.nan
    items, _, values = diversify_slot(np.array([3, 1, 2, 2.5], F32), np.arange(4), Gn, 2, 0.5, DOT)
    assert items.tolist() == [0, 3] and values.tolist() == [1.5, 1.25]


def test_reference_lists_on_planted_clusters_are_less_alike():
    """300 items around 6 centres (noise 0.3), k = 16, 40 users between two centres, the exact top 50 as the pool, N = 10:
    the mean pairwise cosine inside the lists falls with the tradeoff, by at least 0.02 between 1 and 0.3."""
    W, H = planted_clusters(seed=7)    # (seeds 0 .. 11 give gaps of 0.015 .. 0.062; this one: 0.877 against 0.838, and 0.636 at 0)
    S = chain_scores(W, H, np.arange(W.shape[0]))
    G, c = item_gram(H), inv_norm64(item_n2(H))
    pool = np.sort(expected_topn(S, True, 50)[0].astype(np.int64), axis=1)
    ptr, idx = np.arange(W.shape[0] + 1) * 50, pool.reshape(-1)
    cos = {t: intra_list_cosine(expected_diversify(S, ptr, idx, True, G, 10, t, COSINE, c)[0], H) for t in (1.0, 0.3, 0.0)}
    print("intra-list mean cosine by tradeoff:", cos)
    assert cos[1.0] - cos[0.3] >= 0.02, cos
    assert cos[0.0] < cos[0.3], cos
