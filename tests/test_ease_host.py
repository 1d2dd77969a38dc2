"""EASE without a GPU: the exported symbols, the self-checks of the exact reference tests/ease_exact.py (its Gram matrix
against a separately written dense integer X^T X + lambda, the optimality condition of its fp64 model), the condition the GPU
end-to-end test relies on (the reference finds the held-out items of the planted clusters), and the argument refusals that
never reach the device."""
import ctypes as C

import numpy as np
import pytest

import bpr_exact as bx
import ease_exact as ex

MFX_ERR_INVALID = -1  # include/mfx.h
F = np.float32
EASE_SYMBOLS = ("mfx_ease_gram", "mfx_ease_inverse", "mfx_ease_weights_from_inverse", "mfx_ease_train", "mfx_ease_create_from_weights",
                "mfx_ease_weights", "mfx_ease_recommend", "mfx_ease_times", "mfx_ease_destroy")


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    return m


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def random_matrix(mfx, rows, cols, nnz, seed, values="ratings"):
    rng = np.random.default_rng(seed)
    cells = rng.choice(rows * cols, nnz, replace=False)
    v = rng.integers(1, 6, nnz).astype(F) if values == "ratings" else rng.integers(-3, 4, nnz).astype(F)
    return mfx.dataset.from_coo(rows, cols, cells // cols, cells % cols, v)


# ------------------------------------------------------------------------------------------------ symbols
def test_symbols_are_exported_and_bound(mfx):
    from mfx import _lib
    lib = mfx.lib()
    for name in EASE_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.mfx_version() == 2
    assert mfx.MFX_EASE_INV_SIMPLE == 1
    assert callable(mfx.ease_gram) and callable(mfx.ease_inverse) and callable(mfx.ease_weights_from_inverse)
    assert hasattr(mfx.Ease, "from_weights")
    for m in ("weights", "recommend", "times", "close", "__enter__", "__exit__"):
        assert hasattr(mfx.Ease, m), m


# ------------------------------------------------------------------------------------------------ the reference itself
def test_reference_gram_equals_dense_integer_gram_plus_lambda_and_is_symmetric(mfx):
    """Small-integer values: every term is an integer, exact on the 2^-36 grid, so G is the dense X^T X with lambda added to
    the diagonal, every entry exact in fp32."""
    X = random_matrix(mfx, 37, 29, 400, 5, "small_int")
    ptr = X.csr_row_ptr.astype(np.int64)
    D = np.zeros((X.rows, X.cols), np.int64)
    for u in range(X.rows):
        for e in range(ptr[u], ptr[u + 1]):
            D[u, X.csr_col_idx[e]] = int(X.csr_val[e])
    for lam in (3.0, 0.5):
        G = ex.gram(X, lam)
        assert G.shape == (29, 29) and G.dtype == F
        assert np.array_equal(G.astype(np.float64), (D.T @ D).astype(np.float64) + lam * np.eye(29))
        assert np.array_equal(bits(G), bits(G.T))
    R = mfx.knn_weights(random_matrix(mfx, 37, 29, 400, 6), "cosine")
    G = ex.gram(R, 0.25)
    assert np.array_equal(bits(G), bits(G.T))
    assert np.all(np.abs(np.diagonal(G) - 1.25) < 1e-5)  # unit columns


def test_reference_weights_are_one_division_with_a_zero_diagonal():
    rng = np.random.default_rng(2)
    A = rng.standard_normal((12, 30))
    P = np.linalg.inv(A @ A.T + np.eye(12)).astype(F)
    B = ex.weights_from_inverse(P)
    assert B.dtype == F and not np.diagonal(B).any() and not np.signbit(np.diagonal(B)).any()
    for i, j in ((0, 1), (5, 3), (11, 0)):
        assert B[i, j] == F(np.float64(-P[i, j]) / np.float64(P[j, j]))  # (fp64 quotient of two fp32 rounds to the fp32 quotient)
    P[4, 4] = 0
    with pytest.raises(ValueError, match="item 4"):
        ex.weights_from_inverse(P)


def test_fp64_model_satisfies_the_optimality_condition(mfx):
    """EASE minimises ||X - X B||^2 + lambda ||B||^2 subject to diag(B) = 0: the gradient G B - X^T X = G B - G + lambda I
    vanishes off the diagonal (the diagonal carries the multipliers)."""
    X = random_matrix(mfx, 80, 33, 700, 7)
    for lam in (0.5, 20.0):
        G, P, B = ex.ease_fp64(X, lam)
        R = G @ B - G
        off = R[~np.eye(33, dtype=bool)]
        print("largest off-diagonal of G B - G", float(np.abs(off).max()), "scale", float(np.abs(G).max()))
        assert np.abs(off).max() <= 1e-10 * np.abs(G).max()
        assert not np.diagonal(B).any()


def test_reference_finds_the_held_out_items_of_the_planted_clusters():
    """Raw values, lambda = 100, the fp32 pipeline of the reference with numpy's fp32 inverse: the held-out item is in the top
    10 for >= 90 % of the users."""
    P = bx.planted_clusters()
    G = ex.gram(P, 100.0)
    B = ex.weights_from_inverse(np.linalg.inv(G).astype(F))
    ptr = P.csr_row_ptr.astype(np.int64)
    D = np.zeros((P.rows, P.cols), F)
    D[np.repeat(np.arange(P.rows), np.diff(ptr)), P.csr_col_idx.astype(np.int64)] = P.csr_val
    S = D.astype(np.float64) @ B.astype(np.float64)
    S[D != 0] = -np.inf
    top = np.argsort(-S, axis=1, kind="stable")[:, :10]
    hits = np.any(top == P.test_col[np.argsort(P.test_row)][:, None], axis=1)
    print("HR@10", hits.mean())
    assert hits.shape == (P.rows,) and hits.mean() >= 0.9, hits.mean()


def test_reference_recommend_handles_empty_bad_and_short_rows():
    B = np.array([[0, 1, -2, 0.5], [1, 0, 1, 1], [0.25, -1, 0, 0], [3, 3, 3, 0]], F)
    ptr = np.array([0, 2, 2, 3, 7], np.uint32)
    idx = np.array([0, 3, 1, 0, 1, 2, 3], np.uint32)
    val = np.array([1.0, 2.0, np.inf, 1, 1, 1, 1], F)
    items, scores, bad = ex.recommend(B, ptr, idx, val, 3)
    assert bad == 1
    assert list(items[0]) == [1, 2, ex.PAD] and list(scores[0][:2]) == [7.0, 4.0]
    assert np.all(items[1] == ex.PAD) and np.all(items[2] == ex.PAD) and np.all(items[3] == ex.PAD)
    items, scores, bad = ex.recommend(B, ptr, idx, val, 3, keep_seen=True)
    assert list(items[0]) == [1, 0, 2] and list(items[3]) == [0, 1, 2] and np.all(items[1] == ex.PAD)


# ------------------------------------------------------------------------------------------------ refusals
def _train(mfx, csx, lam=10.0, flags=0, tile=0, space=0):
    h = C.c_void_p(0x1)
    rc = mfx.lib().mfx_ease_train(C.byref(h), C.byref(csx) if csx is not None else None, lam, flags, tile, space, 0)
    return rc, h


@pytest.mark.parametrize("kw", [dict(lam=0.0), dict(lam=-1.0), dict(lam=float("nan")), dict(lam=float("inf")), dict(flags=2), dict(flags=-1),
                                dict(space=7), dict(tile=-64), dict(tile=32), dict(tile=100), dict(tile=8256)])
def test_train_and_gram_refuse_bad_arguments_before_the_device(mfx, kw):
    from mfx import api
    X = bx.small_matrix()
    csx = api._csx(X)
    rc, h = _train(mfx, csx, **kw)
    assert rc == MFX_ERR_INVALID, mfx.lib().mfx_last_error()
    assert not h.value  # the handle pointer is left null
    if "flags" not in kw:
        out = np.zeros((X.cols, X.cols), F)
        rc = mfx.lib().mfx_ease_gram(C.byref(csx), kw.get("lam", 10.0), kw.get("tile", 0), out.ctypes.data_as(C.c_void_p), kw.get("space", 0), 0)
        assert rc == MFX_ERR_INVALID, mfx.lib().mfx_last_error()


def test_train_and_gram_refuse_degenerate_matrices_and_nulls(mfx):
    from mfx import _lib, api
    X = bx.small_matrix()
    lib = mfx.lib()
    full = api._csx(X)
    fields = [f for f, _ in _lib.mfx_csx._fields_]
    out = np.zeros((X.cols, X.cols), F)
    po = out.ctypes.data_as(C.c_void_p)

    def variant(**kw):
        c = _lib.mfx_csx(*[getattr(full, f) for f in fields])
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    variants = [variant(nnz=0), variant(cols=1), variant(cols=32769), variant(rows=0)] + [variant(**{f: None}) for f in fields[3:]]
    for c in variants:
        rc, h = _train(mfx, c)
        assert rc == MFX_ERR_INVALID and not h.value
        assert lib.mfx_ease_gram(C.byref(c), 10.0, 0, po, 0, 0) == MFX_ERR_INVALID
    assert "32768" in lib.mfx_last_error().decode() or "null" in lib.mfx_last_error().decode()
    assert lib.mfx_ease_train(None, C.byref(full), 10.0, 0, 0, 0, 0) == MFX_ERR_INVALID
    rc, h = _train(mfx, None)
    assert rc == MFX_ERR_INVALID and not h.value
    assert lib.mfx_ease_gram(None, 10.0, 0, po, 0, 0) == MFX_ERR_INVALID
    assert lib.mfx_ease_gram(C.byref(full), 10.0, 0, None, 0, 0) == MFX_ERR_INVALID


def test_stand_alone_steps_refuse_bad_arguments_before_the_device(mfx):
    lib = mfx.lib()
    A = np.eye(4, dtype=F)
    out = np.zeros((4, 4), F)
    pa, po = A.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for args in ((0, pa, po, 0, 0), (-3, pa, po, 0, 0), (32769, pa, po, 0, 0), (4, None, po, 0, 0), (4, pa, None, 0, 0), (4, pa, po, 2, 0),
                 (4, pa, po, -1, 0), (4, pa, po, 0, 9)):
        assert lib.mfx_ease_inverse(*args, 0) == MFX_ERR_INVALID, args
    for args in ((1, pa, po, 0), (32769, pa, po, 0), (4, None, po, 0), (4, pa, None, 0), (4, pa, po, 3)):
        assert lib.mfx_ease_weights_from_inverse(*args, 0) == MFX_ERR_INVALID, args
    for args in ((1, pa, 0), (32769, pa, 0), (4, None, 0), (4, pa, 5)):
        h = C.c_void_p(0x1)
        assert lib.mfx_ease_create_from_weights(C.byref(h), *args, 0) == MFX_ERR_INVALID, args
        assert not h.value
    assert lib.mfx_ease_create_from_weights(None, 4, pa, 0, 0) == MFX_ERR_INVALID


def test_handle_calls_refuse_a_null_handle(mfx):
    lib = mfx.lib()
    buf = np.zeros(8, np.uint32)
    p = buf.ctypes.data_as(C.c_void_p)
    out = (C.c_double * 6)()
    bad = C.c_int64(0)
    assert lib.mfx_ease_weights(None, 0, 1, p, 0) == MFX_ERR_INVALID
    for n_top in (0, 1, 1025):
        assert lib.mfx_ease_recommend(None, 1, 0, p, None, None, n_top, 0, 0, p, p, C.byref(bad), 0) == MFX_ERR_INVALID
    assert lib.mfx_ease_times(None, out) == MFX_ERR_INVALID
    assert lib.mfx_ease_destroy(None) == 0


def test_python_front_end_refuses_malformed_input(mfx):
    with pytest.raises(ValueError):
        mfx.Ease.from_weights(np.zeros((4, 3), F))
    with pytest.raises(ValueError):
        mfx.Ease(None, 5.0, weighting="cosine", device_arrays={"rows": 1, "cols": 2})
    with pytest.raises(ValueError):
        mfx.ease_inverse(np.zeros((2, 3), F))
    with pytest.raises(ValueError):
        mfx.ease_weights_from_inverse(np.zeros(5, F))
