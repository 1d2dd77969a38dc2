"""Candidate-list re-ranking and pair scoring (mfx_rec_query_candidates, mfx_rec_score) without a GPU: the symbols and
their bindings, the refusal of a NULL handle, self-checks of the exact reference in cand_exact.py, the wrapper's
canonicalisation against numpy, and the argument checks that raise before the library is called."""
import ctypes as C
import inspect

import numpy as np
import pytest

from cand_exact import canonical_lists, expected_candidates, random_lists, whole_catalogue
from rec_exact import PAD, expected_topn

MFX_ERR_INVALID = -1  # include/mfx.h
F32 = np.float32


def test_symbols_are_exported_with_the_declared_argument_types():
    import mfx
    from mfx import _lib
    lib = mfx.lib()                # (first: it maps the one HIP runtime the process keeps, which a bare CDLL would not)
    raw = C.CDLL(_lib.LIB_PATH)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    want = {
        "mfx_rec_query_candidates": [vp, i64, vp, vp, vp, i32, i32, vp, vp, vp, C.c_int],
        "mfx_rec_score": [vp, i64, vp, vp, vp, C.c_int],
        "mfx_rec_candidates_times": [vp, C.POINTER(C.c_double)],
    }
    for name, args in want.items():
        assert hasattr(raw, name), name
        res, got = _lib.SIGNATURES[name]
        assert res is C.c_int and list(got) == args, name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert mfx.MFX_CAND_NO_EXCLUDE == 1
    assert lib.mfx_version() == 2 == _lib.MFX_VERSION


def test_a_null_handle_is_refused():
    import mfx
    lib = mfx.lib()
    u = np.zeros(4, np.uint32)
    f = np.zeros(4, F32)
    t = (C.c_double * 3)()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for rc in (lib.mfx_rec_query_candidates(None, 1, None, vp(u), vp(u), 0, 1, vp(u), vp(f), None, 0),
               lib.mfx_rec_score(None, 4, vp(u), vp(u), vp(f), 0),
               lib.mfx_rec_candidates_times(None, t)):
        assert rc == MFX_ERR_INVALID
        assert "null recommender" in lib.mfx_last_error().decode()


def test_the_python_methods_exist():
    import mfx
    R = mfx.Recommender
    q = inspect.signature(R.query_candidates).parameters
    assert list(q) == ["self", "n_top", "candidates", "users", "apply_exclude", "canonical", "on_device", "return_counts"]
    assert [q[n].default for n in list(q)[3:]] == [None, True, False, False, False]
    s = inspect.signature(R.score).parameters
    assert list(s) == ["self", "users", "items", "on_device"] and s["on_device"].default is False
    assert list(inspect.signature(R.candidates_times).parameters) == ["self"]


# ------------------------------------------------------------------------------------------------ the reference
def special_scores(rng, U, cols):
    S = rng.integers(-3, 4, (U, cols)).astype(F32)        # many ties
    S[rng.random((U, cols)) < 0.1] = -0.0
    S[rng.random((U, cols)) < 0.1] = 0.0
    S[rng.random((U, cols)) < 0.05] = np.inf
    S[rng.random((U, cols)) < 0.05] = -np.inf
    S[rng.random((U, cols)) < 0.08] = np.nan
    return S


@pytest.mark.parametrize("seed", [0, 1])
def test_reference_whole_catalogue_list_is_the_reference_topn(seed):
    rng = np.random.default_rng(seed)
    U, cols = 9, 61
    S = special_scores(rng, U, cols)
    eligible = rng.random((U, cols)) < 0.7
    ptr, idx = whole_catalogue(U, cols)
    for n_top in (1, 7, cols + 3):
        items, scores, n_el = expected_candidates(S, ptr, idx, eligible, n_top)
        wi, ws = expected_topn(S, eligible, n_top)
        assert np.array_equal(items, wi) and np.array_equal(scores.view(np.uint32), ws.view(np.uint32))
        assert np.array_equal(n_el, (eligible & ~np.isnan(S)).sum(1))


def test_reference_ties_order_by_item_and_lists_pad():
    S = np.array([[1.0, 2.0, 2.0, -0.0, 0.0, np.nan, 2.0, -np.inf]], F32)
    ptr, idx = np.array([0, 7], np.uint32), np.array([1, 2, 3, 4, 5, 6, 7], np.uint32)    # item 0 is no candidate
    eligible = np.array([[True, True, True, True, True, True, False, True]])              # item 6 is excluded
    items, scores, n_el = expected_candidates(S, ptr, idx, eligible, 7)
    assert items[0].tolist() == [1, 2, 3, 4, 7, PAD, PAD]                                 # 2 = 2 by id; -0 = +0 by id; NaN dropped
    assert np.array_equal(scores[0].view(np.uint32), np.array([2, 2, -0.0, 0.0, -np.inf, -np.inf, -np.inf], F32).view(np.uint32))
    assert n_el.tolist() == [5]
    items, _, n_el = expected_candidates(S, np.array([0, 0], np.uint32), idx[:0], True, 3)  # an empty list
    assert items[0].tolist() == [PAD] * 3 and n_el.tolist() == [0]
    # a slot's answer depends on its own list only
    rng = np.random.default_rng(5)
    S = special_scores(rng, 6, 40)
    ptr, idx = random_lists(rng, [0, 1, 5, 40, 17, 3], 40)
    full = expected_candidates(S, ptr, idx, True, 6)
    for q in range(6):
        one = expected_candidates(S[q:q + 1], np.array([0, ptr[q + 1] - ptr[q]], np.uint32), idx[ptr[q]:ptr[q + 1]], True, 6)
        assert all(np.array_equal(a[q:q + 1].view(np.uint32), b.view(np.uint32)) for a, b in zip(full, one))


# ------------------------------------------------------------------------------------------------ the wrapper's canonical form
def messy_lists(rng, U, cols):
    lens = rng.integers(0, 30, U)
    lens[::5] = 0
    ptr = np.zeros(U + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    idx = rng.integers(0, cols, ptr[-1])                   # unsorted, with repeats
    idx[rng.random(idx.size) < 0.15] = PAD
    return ptr, idx


def test_canonicalisation_agrees_with_numpy_unique_per_row():
    from mfx import api
    rng = np.random.default_rng(11)
    ptr, idx = messy_lists(rng, 41, 50)
    want_ptr, want_idx = canonical_lists(ptr, idx)
    for q in range(41):                                    # the twin itself, against numpy
        r = np.unique(idx[ptr[q]:ptr[q + 1]])
        assert np.array_equal(want_idx[want_ptr[q]:want_ptr[q + 1]], r[r != PAD])
    got_ptr, got_idx = api._canonical_lists_np(ptr, idx)
    assert np.array_equal(got_ptr, want_ptr) and np.array_equal(got_idx, want_idx)
    assert (np.diff(want_ptr) == 0).sum() >= 9 and want_idx.size < idx.size
    # a [U, C] array of equal-length lists
    A = rng.integers(0, 50, (7, 12))
    A[A > 44] = PAD
    p2, i2 = api._candidate_lists(A)
    got = api._canonical_lists_np(api._ids_np(p2, "p"), api._ids_np(i2, "i"))
    want = canonical_lists(np.arange(8) * 12, A.reshape(-1))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    empty = api._canonical_lists_np(np.zeros(1, np.int64), np.zeros(0, np.int64))
    assert empty[0].tolist() == [0] and empty[1].size == 0


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
    bad = [
        dict(candidates=(ptr, idx), users=[0, 1, 2]),                         # three users, two lists
        dict(candidates=(np.zeros(0, np.int64), idx)),                        # no row pointers at all
        dict(candidates=(ptr, np.array([1, -5, 2]))),                         # a negative id
        dict(candidates=(ptr, np.array([1, 2 ** 32, 2]))),                    # an id of 33 bits
        dict(candidates=(ptr, idx), users=[0, -1]),
        dict(candidates=(ptr, idx), users=[0, 2 ** 32]),
        dict(candidates=(np.array([0, 2, 4]), idx)),                          # ptr ends past idx
        dict(candidates=(np.array([1, 2, 3]), idx)),                          # ptr does not start at 0
        dict(candidates=(np.array([0, 3, 2]), idx)),                          # ptr decreases
        dict(candidates=(ptr.reshape(3, 1), idx)),                            # ptr is not 1-D
        dict(candidates=(ptr, idx.astype(np.float32))),                       # ids are not integers
        dict(candidates=np.zeros((2, 3, 4), np.int64)),                       # lists as an array: 2-D only
        dict(candidates=(ptr, idx, idx)),
        dict(candidates=(np.arange(12), np.zeros(11, np.int64))),             # 11 lists without users, 10 rows
        dict(candidates=(ptr, idx), n_top=0),
        dict(candidates=(ptr, idx), n_top=1025),
    ]
    for kw in bad:
        kw.setdefault("n_top", 3)
        with pytest.raises(ValueError):
            r.query_candidates(**kw)
    for users, items in (([0, 1], [1]), ([0, -1], [1, 2]), ([0, 1], [1, 2 ** 32]), ([[0, 1]], [[1, 2]]), ([0.5], [1])):
        with pytest.raises(ValueError):
            r.score(users, items)
    with pytest.raises(mfx.MfxError):                                         # a call that passes the checks reaches the library
        r.query_candidates(3, (ptr, idx))
    with pytest.raises(mfx.MfxError):
        r.score([0, 1], [1, 2])
