"""Catalogue ranks and full-rank evaluation (mfx_rec_rank, mfx_rec_evaluate) without a GPU: the symbols, their bindings,
the refusal of a NULL handle, the Python surface, and self-checks of the exact reference in rank_exact.py."""
import ctypes as C
import inspect

import numpy as np
import pytest

from rank_exact import expected_ranks, mrr_auc
from rec_exact import PAD, expected_topn

MFX_ERR_INVALID = -1  # include/mfx.h
NEW = ("mfx_rec_rank", "mfx_rec_evaluate")
F32 = np.float32


def test_symbols_are_exported_and_bound():
    import mfx
    from mfx import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW + ("mfx_rec_rank_times",):
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        res, args = _lib.SIGNATURES[name]
        fn = getattr(mfx.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW] == [9, 11]


def test_the_abi_revision_is_still_2():
    import mfx
    from mfx import _lib
    assert mfx.lib().mfx_version() == 2 == _lib.MFX_VERSION


def test_a_null_handle_is_refused():
    import mfx
    lib = mfx.lib()
    u = np.zeros(4, np.uint32)
    out = np.zeros(4, np.uint32)
    f = np.ones(4, F32)
    cut = np.array([10], np.int32)
    m = (C.c_double * 4)()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    coo = _lib_coo(mfx, u, u, f)
    for rc in (lib.mfx_rec_rank(None, 4, vp(u), vp(u), vp(out), None, None, 0, 0),
               lib.mfx_rec_evaluate(None, C.byref(coo), 0.0, 1, vp(cut), m, None, None, None, None, 0),
               lib.mfx_rec_rank_times(None, m)):
        assert rc == MFX_ERR_INVALID
        assert "null recommender" in lib.mfx_last_error().decode()


def _lib_coo(mfx, r, c, v):
    from mfx import _lib
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    return _lib.mfx_coo(len(v), vp(r), vp(c), vp(v))


def test_the_python_methods_and_constant_exist():
    import mfx
    R = mfx.Recommender
    rk = inspect.signature(R.rank_of).parameters
    assert list(rk) == ["self", "users", "items", "item_slices", "on_device"]
    assert (rk["item_slices"].default, rk["on_device"].default) == (0, False)
    ev = inspect.signature(R.evaluate).parameters
    assert list(ev) == ["self", "T", "cutoffs", "min_rating"]
    assert ev["cutoffs"].default == (10,) and ev["min_rating"].default == float("-inf")
    assert mfx.PAD_RANK == 0xFFFFFFFF == PAD


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reference_rank_is_the_position_in_the_reference_list(seed):
    """expected_ranks == r iff expected_topn(S, eligible, cols)[0][u, r] == i, and PAD iff i is absent, for every (u, i)."""
    rng = np.random.default_rng(seed)
    U, cols = 23, 61
    S = rng.integers(-3, 4, (U, cols)).astype(F32)        # many ties
    S[rng.random((U, cols)) < 0.1] = -0.0
    S[rng.random((U, cols)) < 0.1] = 0.0
    S[rng.random((U, cols)) < 0.05] = np.inf
    S[rng.random((U, cols)) < 0.05] = -np.inf
    S[rng.random((U, cols)) < 0.08] = np.nan
    eligible = rng.random((U, cols)) < 0.7
    eligible[3] = False                                   # nothing eligible
    eligible[4] = True
    S[5] = np.nan
    uu, ii = np.divmod(np.arange(U * cols), cols)
    ranks, scores, n_el = expected_ranks(S, eligible, uu, ii)
    assert np.array_equal(scores.view(np.uint32), S.reshape(-1).view(np.uint32))
    items = expected_topn(S, eligible, cols)[0]
    pos = np.full((U, cols), PAD, np.uint32)
    for u in range(U):
        real = items[u] != PAD
        pos[u, items[u, real]] = np.nonzero(real)[0]
        assert np.all(n_el[uu == u] == real.sum())
    assert np.array_equal(ranks.reshape(U, cols), pos)
    assert (ranks == PAD).any() and (ranks != PAD).any() and np.all(ranks[uu == 3] == PAD) and np.all(ranks[uu == 5] == PAD)
    # a subset in another order, with repeats, gives the same per-pair answers
    sel = rng.integers(0, U * cols, 500)
    sub = expected_ranks(S, eligible, uu[sel], ii[sel])
    assert np.array_equal(sub[0], ranks[sel]) and np.array_equal(sub[2], n_el[sel])


def test_mrr_and_auc_by_hand():
    # user 0: targets at ranks 0 and 3 of 10 eligible items: RR 1; neg 8; AUC (8-0)/8 and (8-(3-1))/8 -> 0.875
    # user 1: one ineligible target and one at rank 4 of 5: RR 1/5; neg 4; AUC (4-4)/4 = 0
    # user 2: the only eligible item is its target (plus an ineligible one): RR 1; neg 0: not in the AUC mean
    users = [0, 0, 1, 1, 2, 2]
    ranks = [0, 3, PAD, 4, 0, PAD]
    n_el = [10, 10, 5, 5, 1, 1]
    mrr, auc, kept, auc_kept = mrr_auc(users, ranks, n_el)
    assert (kept, auc_kept) == (3, 2)
    assert abs(mrr - (1.0 + 0.2 + 1.0) / 3) < 1e-15
    assert abs(auc - (0.875 + 0.0) / 2) < 1e-15
    # a user whose targets are all ineligible: RR 0, not in the AUC mean; the order of the pairs plays no part
    mrr, auc, kept, auc_kept = mrr_auc([7, 0, 7, 0], [PAD, 3, PAD, 0], [4, 10, 4, 10])
    assert (kept, auc_kept) == (2, 1) and abs(mrr - 0.5) < 1e-15 and abs(auc - 0.875) < 1e-15
    assert mrr_auc([], [], []) == (0.0, 0.0, 0, 0)
