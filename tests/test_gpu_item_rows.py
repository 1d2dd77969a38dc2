"""GPU tests of what mfx_knn_recommend, mfx_slim_recommend and mfx_ease_recommend have in common: one argument list, one
order of checks, one set of refusal texts, optional outputs, two time slots.  The three models are made from given lists or
weights on 70 items with small integer values, so every sum is exact; the results are compared bit for bit with the exact
references of tests/knn_exact.py, slim_exact.py and ease_exact.py."""
import ctypes as C

import numpy as np
import pytest

import ease_exact as ex
import knn_exact as kx
import slim_exact as sx

pytestmark = pytest.mark.gpu

MFX_ERR_INVALID = -1  # include/mfx.h
F = np.float32
COLS, K = 70, 3
MODELS = ("knn", "slim", "ease")
RECOMMEND_SLOTS = {"knn": (2, 3), "slim": (3, 4), "ease": (4, 5)}  # of mfx_*_times: the checks and the pass of recommend
N_SLOTS = {"knn": 4, "slim": 5, "ease": 6}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _lists():
    """K = 3 distinct ids per item, never the item itself, weights in -3 .. 3; item 5 has one pad, item 9 has no list."""
    rng = np.random.default_rng(7)
    S = np.empty((COLS, K), np.uint32)
    for i in range(COLS):
        S[i] = rng.choice(np.delete(np.arange(COLS), i), K, replace=False)
    w = rng.integers(-3, 4, (COLS, K)).astype(F)
    S[5, 2:], S[9, :] = kx.PAD, kx.PAD
    return S, w


def _dense():
    """B [70][70] with integer weights in -3 .. 3 and a zero diagonal."""
    B = np.random.default_rng(8).integers(-3, 4, (COLS, COLS)).astype(F)
    np.fill_diagonal(B, 0)
    return B


def _rows():
    """Four rows: empty, one item, 66 items (values 1 .. 3), and one that holds the item 70 >= cols."""
    rng = np.random.default_rng(9)
    long_row = np.sort(rng.choice(COLS, 66, replace=False))
    idx = np.concatenate([[17], long_row, [3, COLS]]).astype(np.uint32)
    val = rng.integers(1, 4, idx.size).astype(F)
    return np.array([0, 0, 1, 67, 69], np.uint32), idx, val


PTR4, IDX4, VAL4 = _rows()
PTR, IDX, VAL = PTR4[:4], IDX4[:67], VAL4[:67]  # the three well-formed rows


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1
    return m


def make(mfx, name):
    """(model, the reference's recommend with the model bound)."""
    if name == "ease":
        B = _dense()
        return mfx.Ease.from_weights(B), lambda *a: ex.recommend(B, *a)
    S, w = _lists()
    if name == "slim":
        return mfx.Slim.from_lists(S, w), lambda *a: sx.recommend(S, w, *a)
    sim = np.where(S == kx.PAD, F(-np.inf), w)
    return mfx.ItemKnn.from_lists(S, sim), lambda *a: kx.recommend(S, sim, *a)


@pytest.fixture(scope="module", params=MODELS)
def model(request, mfx):
    m, ref = make(mfx, request.param)
    want = {(n_top, keep): ref(PTR, IDX, VAL, n_top, keep) for n_top in (1, 5) for keep in (False, True)}
    yield request.param, m, want
    m.close()


def raw(mfx, name, handle, nusers, nnz, ptr, idx, val, n_top, flags, tile, items, scores, bad):
    """The C call on host arrays (None: NULL) -> (return code, mfx_last_error())."""
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = getattr(mfx.lib(), f"mfx_{name}_recommend")(handle, nusers, nnz, p(ptr), p(idx), p(val), n_top, flags, tile, p(items), p(scores),
                                                     None if bad is None else C.byref(bad), 0)
    return rc, mfx.lib().mfx_last_error().decode()


def test_rows_bit_for_bit(mfx, model):
    """Two tiles (64 + 6 items) and one, n_top 1 and 5, the row's items dropped and kept, host arrays and device tensors."""
    import torch
    name, m, want = model
    dev = [torch.from_numpy(a.view(np.int32)).cuda() for a in (PTR, IDX)] + [torch.from_numpy(VAL).cuda()]
    for (n_top, keep), (w_items, w_scores, w_bad) in want.items():
        assert w_bad == 0 and np.all(w_items[0] == kx.PAD)  # the empty row: pads, and not bad
        for tile in (64, 0):
            items, scores = m.recommend((PTR, IDX, VAL), n_top, keep_seen=keep, tile_items=tile)
            assert m.bad_rows == 0 and items.dtype == np.uint32 and scores.dtype == F
            assert np.array_equal(items, w_items) and np.array_equal(bits(scores), bits(w_scores)), (name, n_top, keep, tile)
            ti, ts = m.recommend(tuple(dev), n_top, keep_seen=keep, tile_items=tile)
            assert m.bad_rows == 0 and ti.is_cuda and ts.is_cuda
            assert np.array_equal(ti.cpu().numpy().view(np.uint32), w_items), (name, n_top, keep, tile)
            assert np.array_equal(bits(ts.cpu().numpy()), bits(w_scores)), (name, n_top, keep, tile)
    if name != "ease":  # the sums are on the grid: the rows' own items are among the candidates only when kept
        seen = set(IDX[1:].tolist())
        assert not seen & set(want[(5, False)][0][2].tolist()) and seen & set(want[(5, True)][0][2].tolist())


def test_optional_outputs_and_no_rows(mfx, model):
    name, m, want = model
    w_items = want[(5, False)][0]
    for tile in (64, 0):
        items, scores = np.full((3, 5), 123, np.uint32), np.full((3, 5), 7, F)
        bad = C.c_int64(99)
        assert raw(mfx, name, m.handle, 3, 67, PTR, IDX, VAL, 5, 0, tile, items, None, bad)[0] == 0  # scores = NULL
        assert np.array_equal(items, w_items) and bad.value == 0
        items[:] = 123
        assert raw(mfx, name, m.handle, 3, 67, PTR, IDX, VAL, 5, 0, tile, items, scores, None)[0] == 0  # bad_rows = NULL
        assert np.array_equal(items, w_items) and np.array_equal(bits(scores), bits(want[(5, False)][1]))
    bad = C.c_int64(99)
    assert raw(mfx, name, m.handle, 0, 0, None, None, None, 5, 0, 0, None, None, bad)[0] == 0  # no rows: nothing is read
    assert bad.value == 0
    assert raw(mfx, name, m.handle, 0, 0, None, None, None, 5, 0, 0, None, None, None)[0] == 0


def test_refusals_word_for_word(mfx, model):
    """The checks in their order -- n_top, flags, tile_items, then the rows' structure on the device -- and their texts, which
    differ between the models in the entry point's name only."""
    name, m, want = model
    fn = f"mfx_{name}_recommend"
    items, scores = np.empty((4, 5), np.uint32), np.empty((4, 5), F)
    bad = C.c_int64(0)
    call = lambda n_top=5, flags=0, tile=0, rows=(3, 67, PTR, IDX, VAL): raw(mfx, name, m.handle, *rows, n_top, flags, tile, items, scores, bad)
    assert call(n_top=0) == (MFX_ERR_INVALID, f"{fn}: n_top must be in [1, 1024] (got 0)")
    assert call(n_top=1025) == (MFX_ERR_INVALID, f"{fn}: n_top must be in [1, 1024] (got 1025)")
    assert call(flags=2) == (MFX_ERR_INVALID, f"{fn}: unknown flag bits 0x2")
    assert call(flags=5) == (MFX_ERR_INVALID, f"{fn}: unknown flag bits 0x5")
    assert call(tile=32) == (MFX_ERR_INVALID, f"{fn}: tile_items must be 0 or a multiple of 64 up to 8192 (got 32)")
    assert call(n_top=0, flags=2, tile=32)[1] == f"{fn}: n_top must be in [1, 1024] (got 0)"  # the first check speaks
    assert call(flags=2, tile=32)[1] == f"{fn}: unknown flag bits 0x2"
    for tile in (64, 0):
        assert call(tile=tile, rows=(4, 69, PTR4, IDX4, VAL4)) == (
            MFX_ERR_INVALID, f"{fn}: row 3: its pointers must ascend from 0 to nnz and its ids be strictly ascending and below cols")
    rc, _ = call()  # the handle is as good as before
    assert rc == 0 and bad.value == 0 and np.array_equal(items[:3], want[(5, False)][0])


@pytest.mark.parametrize("name", MODELS)
def test_times_fill_the_two_recommend_slots(mfx, name):
    m, _ = make(mfx, name)
    with m:
        read = lambda: list(m.times().values())
        before = read()
        check, run = RECOMMEND_SLOTS[name]
        assert len(before) == N_SLOTS[name] and before[check] == 0 and before[run] == 0
        m.recommend((PTR, IDX, VAL), 5)
        once = read()
        m.recommend((PTR, IDX, VAL), 1, keep_seen=True, tile_items=64)
        twice = read()
    assert 0 < once[check] < twice[check] and 0 < once[run] < twice[run]  # summed over the calls
    for slot in range(N_SLOTS[name]):
        if slot not in (check, run):
            assert before[slot] == once[slot] == twice[slot]
