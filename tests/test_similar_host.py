"""Item-to-item similarity and the item filter (mfx_rec_set_item_filter, mfx_rec_similar_setup, mfx_rec_item_norms,
mfx_rec_similar) without a GPU: the symbols, their bindings, the refusal of a NULL handle, the Python surface, and
self-checks of the exact reference in sim_exact.py."""
import ctypes as C
import inspect

import numpy as np
import pytest

import sim_exact
from rec_exact import chain_scores

MFX_ERR_INVALID = -1  # include/mfx.h
NEW = ("mfx_rec_set_item_filter", "mfx_rec_similar_setup", "mfx_rec_item_norms", "mfx_rec_similar")
F32 = np.float32


def test_symbols_are_exported_and_bound():
    import mfx
    from mfx import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        res, args = _lib.SIGNATURES[name]
        fn = getattr(mfx.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW] == [3, 1, 4, 10]
    assert (mfx.MFX_SIM_DOT, mfx.MFX_SIM_COSINE) == (0, 1) == (_lib.MFX_SIM_DOT, _lib.MFX_SIM_COSINE)


def test_the_abi_revision_is_still_2():
    import mfx
    from mfx import _lib
    assert mfx.lib().mfx_version() == 2 == _lib.MFX_VERSION


def test_a_null_handle_is_refused():
    import mfx
    lib = mfx.lib()
    keep = np.ones(4, np.uint8)
    out = np.zeros(4, np.uint32)
    n2 = np.zeros(4, F32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for rc in (lib.mfx_rec_set_item_filter(None, vp(keep), 0), lib.mfx_rec_similar_setup(None),
               lib.mfx_rec_item_norms(None, vp(n2), None, 0),
               lib.mfx_rec_similar(None, 1, None, mfx.MFX_SIM_COSINE, 1, 4, vp(out), None, 0, 0)):
        assert rc == MFX_ERR_INVALID
        assert "null recommender" in lib.mfx_last_error().decode()


def test_the_python_methods_and_keywords_exist():
    import mfx
    R = mfx.Recommender
    assert list(inspect.signature(R.set_item_filter).parameters) == ["self", "keep"]
    assert list(inspect.signature(R.similar_setup).parameters) == ["self"]
    assert list(inspect.signature(R.item_norms).parameters) == ["self"]
    sim = inspect.signature(R.similar_items).parameters
    assert list(sim) == ["self", "n_top", "items", "metric", "exclude_self", "item_slices", "on_device"]
    assert (sim["items"].default, sim["metric"].default, sim["exclude_self"].default, sim["item_slices"].default,
            sim["on_device"].default) == (None, mfx.MFX_SIM_COSINE, True, 0, False)


@pytest.mark.parametrize("k", [1, 3, 17])
def test_reference_n2_is_the_diagonal_of_the_chain(k):
    rng = np.random.default_rng(k)
    H = (rng.standard_normal((300, k)) * 2.0 ** rng.integers(-70, 60, (300, 1))).astype(F32)
    H[7] = 0.0
    S = chain_scores(H, H, np.arange(300))
    n2 = sim_exact.item_n2(H)
    assert np.array_equal(n2.view(np.uint32), np.diagonal(S).view(np.uint32))
    c = sim_exact.inv_norm64(n2)
    assert c[7] == 0 and np.all(c[~np.isfinite(n2)] == 0) and np.all(c[np.isfinite(n2) & (n2 > 0)] > 0)


def test_reference_excludes_self_and_filtered_items_and_pads():
    rng = np.random.default_rng(5)
    H = rng.standard_normal((40, 4)).astype(F32)
    H[11] = H[3]
    q = np.array([3, 3, 11, 20])
    keep = np.ones(40, bool)
    keep[[20, 25]] = False
    S = chain_scores(H, H, q)
    c = sim_exact.inv_norm64(sim_exact.item_n2(H))
    items, scores = sim_exact.expected_similar(S, q, 40, sim_exact.COSINE, c, keep, True)
    for s, qq in enumerate(q):
        real = items[s][items[s] != sim_exact.PAD]
        assert qq not in real and 25 not in real and 20 not in real
        assert len(real) == 40 - 2 - (0 if qq == 20 else 1) and np.all(np.isneginf(scores[s, len(real):]))
    assert items[0, 0] == 11 and items[2, 0] == 3  # the duplicate row stays and is the nearest
    with_self = sim_exact.expected_similar(S, q, 40, sim_exact.DOT, None, None, False)[0]
    assert all(qq in with_self[s] for s, qq in enumerate(q))


@pytest.mark.parametrize("seed,k", [(0, 2), (1, 3), (2, 8)])
def test_the_collinear_ramp_separates_key_order_from_score_order(seed, k):
    cols, n_top = 6007, 200
    H = sim_exact.collinear_ramp(cols, k, seed)
    q = np.random.default_rng(100 + seed).integers(0, cols, 64)
    c = sim_exact.inv_norm64(sim_exact.item_n2(H))
    items, scores, keys = sim_exact.expected_similar(chain_scores(H, H, q), q, n_top, sim_exact.COSINE, c, with_keys=True)
    pairs = sim_exact.key_order_pairs(items, scores, keys)
    print("key-order pairs:", pairs)
    assert pairs >= 1
