"""Explanations of fold-in recommendations (mfx_rec_explain) without a GPU: the symbols and their bindings, the refusal of
a NULL handle, the Python surface, and self-checks of the exact reference in explain_exact.py."""
import ctypes as C
import inspect

import numpy as np

import explain_exact as ex
import ials_ref
import ials_reg_ref

MFX_ERR_INVALID = -1  # include/mfx.h
F32 = np.float32
LAM, ALPHA, ALPHA0, NU = 0.1, 1.0, 0.3, 0.5


def test_symbols_are_exported_with_the_declared_argument_types():
    import mfx
    from mfx import _lib
    lib = mfx.lib()                # (first: it maps the one HIP runtime the process keeps, which a bare CDLL would not)
    raw = C.CDLL(_lib.LIB_PATH)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    want = {
        "mfx_rec_explain": [vp, i64, i64, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, C.c_int],
        "mfx_rec_explain_times": [vp, C.POINTER(C.c_double)],
    }
    for name, args in want.items():
        assert hasattr(raw, name), name
        res, got = _lib.SIGNATURES[name]
        assert res is C.c_int and list(got) == args, name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert lib.mfx_version() == 2 == _lib.MFX_VERSION


def test_a_null_handle_is_refused():
    import mfx
    lib = mfx.lib()
    u = np.zeros(4, np.uint32)
    f = np.zeros(4, F32)
    t = (C.c_double * 3)()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for rc in (lib.mfx_rec_explain(None, 1, 1, vp(u), vp(u), vp(f), 1, vp(u), 1, vp(u), vp(f), None, None, None, 0),
               lib.mfx_rec_explain_times(None, t)):
        assert rc == MFX_ERR_INVALID
        assert "null" in lib.mfx_last_error().decode()


def test_the_python_methods_exist():
    import mfx
    R = mfx.Recommender
    p = inspect.signature(R.explain).parameters
    assert list(p) == ["self", "rows", "targets", "n_expl", "on_device", "return_W", "return_Z", "max_ws_bytes"]
    assert [p[n].default for n in list(p)[3:]] == [10, False, False, False, 1 << 30]
    assert list(inspect.signature(R.explain_times).parameters) == ["self"]


# ------------------------------------------------------------------------------------------------ the reference
def _rows(seed, cols, sizes, repeats=True, zero_frac=0.0):
    rng = np.random.default_rng(seed)
    ptr = np.zeros(len(sizes) + 1, np.uint32)
    ptr[1:] = np.cumsum(sizes)
    idx = np.concatenate([np.sort(rng.integers(0, cols, n) if repeats else rng.choice(cols, n, replace=False)) for n in sizes]
                         + [np.zeros(0, np.int64)]).astype(np.uint32)
    val = rng.integers(1, 6, idx.size).astype(F32)
    val[rng.random(idx.size) < zero_frac] = 0.0
    return ptr, idx, val


def test_weights_per_setup():
    v = np.array([0.0, 1.0, 2.5, 5.0], F32)
    for s in ("als", "ccd"):
        b, counts = ex.weights(s, v, ALPHA, ALPHA0)
        assert b.dtype == F32 and np.array_equal(b, v) and counts.all()
    a = F32(0.7)
    b, counts = ex.weights("implicit", v, a, ALPHA0)
    assert np.array_equal(b, (F32(1) + (a * v).astype(F32)).astype(F32)) and counts.tolist() == [False, True, True, True]
    b, counts = ex.weights("reg", v, a, ALPHA0)
    assert np.array_equal(b, (F32(ALPHA0) + (a * v).astype(F32)).astype(F32)) and counts.tolist() == [False, True, True, True]


def test_systems_equal_the_dense_references_on_rows_without_repeats():
    cols, k = 60, 7
    ptr, idx, val = _rows(3, cols, [0, 1, 9, 30], repeats=False, zero_frac=0.2)
    H = (0.1 * np.random.default_rng(4).standard_normal((cols, k))).astype(F32)
    for s in range(1, 4):
        A, b = ials_ref.dense_system(ptr, idx, val, s, H, float(F32(LAM)), ALPHA)
        lo, hi = int(ptr[s]), int(ptr[s + 1])
        assert np.allclose(ex.system("implicit", ptr, idx, val, s, H, LAM, ALPHA), A, rtol=1e-13, atol=1e-15)
        assert np.allclose(ex.rhs("implicit", idx[lo:hi], val[lo:hi], H, ALPHA), b, rtol=1e-13, atol=1e-15)
        A, b = ials_reg_ref.dense_system(ptr, idx, val, s, H, LAM, ALPHA, ALPHA0, NU)
        assert np.allclose(ex.system("reg", ptr, idx, val, s, H, LAM, ALPHA, ALPHA0, NU), A, rtol=1e-13, atol=1e-15)
        # (b_e = add_rn(alpha0, w_e) is an fp32 sum, the dense reference adds in fp64: half an fp32 ulp per entry)
        scale = np.abs(H[idx[lo:hi]].astype(np.float64)).T @ (ALPHA0 + ALPHA * val[lo:hi].astype(np.float64))
        assert (np.abs(ex.rhs("reg", idx[lo:hi], val[lo:hi], H, ALPHA, ALPHA0) - b) <= 2.0 ** -24 * scale + 1e-15).all()
        Hj = H[idx[lo:hi]].astype(np.float64)
        assert np.allclose(ex.system("als", ptr, idx, val, s, H, LAM), Hj.T @ Hj + float(F32(LAM)) * np.eye(k))
        assert np.allclose(ex.system("ccd", ptr, idx, val, s, H, LAM), Hj.T @ Hj + float(F32(LAM) * F32(hi - lo)) * np.eye(k))


def test_contributions_of_a_row_sum_to_the_score_in_fp64():
    cols, k = 80, 12
    ptr, idx, val = _rows(5, cols, [1, 2, 7, 40, 80], zero_frac=0.15)
    H = (0.1 * np.random.default_rng(6).standard_normal((cols, k))).astype(F32)
    H64 = H.astype(np.float64)
    for setup in ex.SETUPS:
        for s in range(5):
            lo, hi = int(ptr[s]), int(ptr[s + 1])
            A = ex.system(setup, ptr, idx, val, s, H, LAM, ALPHA, ALPHA0, NU)
            w = np.linalg.solve(A, ex.rhs(setup, idx[lo:hi], val[lo:hi], H, ALPHA, ALPHA0))
            b, counts = ex.weights(setup, val[lo:hi], ALPHA, ALPHA0)
            for i in (0, int(idx[lo]), cols - 1):
                z = np.linalg.solve(A, H64[i])
                c = np.where(counts, b.astype(np.float64), 0.0) * (H64[idx[lo:hi]] @ z)
                total = float(H64[i] @ w)
                assert abs(c.sum() - total) <= 1e-12 * max(abs(total), np.abs(c).sum()), (setup, s, i)


def test_chain_is_the_fma_chain_and_the_product_rounds_once():
    rng = np.random.default_rng(7)
    z = rng.standard_normal(9).astype(F32)
    Hr = rng.standard_normal((5, 9)).astype(F32)
    d = ex.chain(z, Hr)
    assert d.dtype == F32
    for e in range(5):
        acc = np.zeros(1, F32)
        for c in range(9):  # one entry at a time, c ascending
            acc = ex.fmaf32(z[c:c + 1], Hr[e, c:c + 1], acc)
        assert acc.view(np.uint32)[0] == d[e:e + 1].view(np.uint32)[0]
    b = rng.standard_normal(5).astype(F32)
    H = Hr
    c = ex.contributions(z, H, np.arange(5), b)
    assert np.array_equal(c.view(np.uint32), (b * d).astype(F32).view(np.uint32))


def test_order_ties_by_position_zeros_nan_and_padding():
    idx_row = np.array([4, 4, 9, 9, 11, 30, 31], np.uint32)
    c = np.array([1.0, 1.0, -0.0, 0.0, np.nan, 5.0, 1.0], F32)
    counts = np.array([1, 1, 1, 1, 1, 0, 1], bool)
    items, contrib, pos = ex.ranked(idx_row, c, counts, 8)
    assert pos.tolist() == [0, 1, 6, 2, 3]                 # ties by position; -0 and +0 tie; NaN and the non-entry dropped
    assert items.tolist() == [4, 4, 31, 9, 9] + [ex.PAD] * 3
    assert contrib[:5].tolist() == [1.0, 1.0, 1.0, 0.0, 0.0] and np.signbit(contrib[3]) and not np.signbit(contrib[4])
    assert np.isneginf(contrib[5:]).all()
    items, contrib, pos = ex.ranked(idx_row, c, counts, 2)
    assert items.tolist() == [4, 4] and pos.tolist() == [0, 1]
    items, contrib, pos = ex.ranked(idx_row, c, counts, 0)
    assert items.size == 0 and contrib.size == 0


def test_explicit_zeros_do_not_count_in_the_implicit_models():
    cols, k = 20, 4
    H = (0.1 * np.random.default_rng(8).standard_normal((cols, k))).astype(F32)
    ptr = np.array([0, 4], np.uint32)
    idx = np.array([1, 5, 5, 7], np.uint32)
    val = np.array([0.0, 2.0, 0.0, 3.0], F32)
    targets = np.array([[3, ex.PAD]], np.uint32)
    Z = (0.1 * np.random.default_rng(9).standard_normal((1, 2, k))).astype(F32)
    for setup, n in (("als", 4), ("ccd", 4), ("implicit", 2), ("reg", 2)):
        items, contrib = ex.expected(setup, ptr, idx, val, targets, Z, H, 6, ALPHA, ALPHA0)
        got = items[0, 0][items[0, 0] != ex.PAD]
        assert got.size == n and (n == 4 or sorted(got.tolist()) == [5, 7]), setup
        assert (items[0, 1] == ex.PAD).all() and np.isneginf(contrib[0, 1]).all()   # a padding target
    val0 = np.zeros(4, F32)
    items, _ = ex.expected("implicit", ptr, idx, val0, targets, Z, H, 6, ALPHA, ALPHA0)
    assert (items == ex.PAD).all()
    assert not ex.rhs("implicit", idx, val0, H, ALPHA).any()  # and w = 0
