"""Hybrid BPR without a GPU: the self-checks of the exact reference of tests/hyb_exact.py (identity features are BPR, the
embedding chain against a float64 sum), mfx.hyb_features, the exports and the refusals of the new entry points that never
reach the device."""
import ctypes as C

import numpy as np
import pytest

import bpr_exact as bx
import hyb_exact as hx

MFX_ERR_INVALID = -1  # include/mfx.h
F = np.float32
U = 2.0 ** -24  # the unit roundoff of fp32
NAMES = ("mfx_hyb_create", "mfx_hyb_set_embeddings", "mfx_hyb_get_embeddings", "mfx_hyb_get_factors", "mfx_hyb_steps", "mfx_hyb_epochs",
         "mfx_hyb_position", "mfx_hyb_kernel_times", "mfx_hyb_destroy", "mfx_hyb_embed", "mfx_hyb_apply")


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    return m


@pytest.fixture(autouse=True)
def _library_has_hyb(mfx):
    """tests/hyb_exact.py restates the contract of the library's hybrid entry points: without them it has no subject."""
    assert all(hasattr(mfx.lib(), name) for name in NAMES)


@pytest.fixture(scope="module")
def R():
    return bx.small_matrix()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ the reference itself
def test_step_with_identity_features_is_the_bpr_step(R):
    """G is a multiple of 2^-36, fp32(1 * G) = G truncates to itself, the feature's sum is G's integer, rounding it again
    returns G, and m_f = m_r: every bit of W, H and the counts.  The batch names rows more than once, holds an
    i == j slot and meets a -0 in H, which the embedding must hand through (a chain from +0 would return +0)."""
    k, n = 7, 300
    W, H = bx.initial_factors(R.rows, R.cols, k, 1)
    H[3, 2] = F(-0.0)
    H[9] = F(-0.0)
    u, i, j, s = bx.triples(R, 4, 0, n)
    j[5] = i[5]  # a row touched twice by one slot
    s[5] = False
    u[7], i[7], j[7], s[7] = u[6], i[6], j[6], s[6]  # a triple named twice
    i[8] = 9
    assert len(np.unique(u)) < n and len(np.unique(i)) < n
    Fu, Fi = hx.identity(R.rows), hx.identity(R.cols)
    assert same_bits(hx.embed(Fi, H), H) and same_bits(hx.embed(Fu, W), W)
    assert np.signbit(hx.embed(Fi, H)[3, 2])
    want = bx.step(W, H, u, i, j, s, 0.05, 0.01)
    got = hx.step(Fu, Fi, W, H, u, i, j, s, 0.05, 0.01, counts=True)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and got[2] == want[2]
    assert not same_bits(got[0], W) and not same_bits(got[1], H)
    live = ~s
    assert np.array_equal(got[3], np.bincount(u[live], minlength=R.rows))
    assert np.array_equal(got[4], np.bincount(i[live], minlength=R.cols) + np.bincount(j[live], minlength=R.cols))


def test_embedding_is_within_the_first_order_bound_of_the_float64_sum():
    """The chain of a row of n entries rounds n times: the first product once, every fmaf once.  Term e passes through the
    roundings e .. n - 1 (term 0 through all n), so with u = 2^-24
        |computed - exact| <= ((1 + u)^n - 1) * sum_e |v_e| |E[f_e][c]| <= n u / (1 - n u) * sum <= (n + 1) u * sum,
    the last step because n^2 u <= 1 - n u for n <= 1024 (2^20 * 2^-24 = 1/16).  The products are exact in float64 and the
    float64 sum of at most 1024 of them carries a relative error below 1024 * 2^-53, far below u.  No term here is small
    enough to round into the subnormal range, where the relative bound would not hold."""
    rng = np.random.default_rng(0)
    nf, k = 1500, 5
    lengths = [0, 1, 2, 3, 63, 64, 65, 1023, 1024]
    rows, ids, vals = [], [], []
    for r, n in enumerate(lengths):
        rows += [r] * n
        ids += sorted(rng.choice(nf, n, replace=False).tolist())
        vals += (rng.random(n) * 2 - 1).tolist()
    Fm = hx.features(len(lengths), nf, rows, ids, vals)
    E = rng.standard_normal((nf, k)).astype(F)
    got = hx.embed(Fm, E)
    assert got.dtype == F and np.all(bits(got[0]) == 0)
    ptr = Fm.ptr.astype(np.int64)
    worst = 0.0
    for r, n in enumerate(lengths):
        v = Fm.val[ptr[r]:ptr[r + 1]].astype(np.float64)[:, None]
        x = E[Fm.idx[ptr[r]:ptr[r + 1]]].astype(np.float64)
        exact, scale = (v * x).sum(0), (np.abs(v) * np.abs(x)).sum(0)
        err = np.abs(got[r].astype(np.float64) - exact)
        bound = (n + 1) * U * scale
        assert np.all(err <= bound), (n, err, bound)
        if n:
            worst = max(worst, float((err / bound).max()))
    print("worst error / bound", worst)
    assert worst > 0  # (fp32 against fp64: two different computations)
    # a row of one entry is the single product, a row of the identity the table's bits
    assert same_bits(got[1], Fm.val[0] * E[Fm.idx[0]])


def test_hyb_features_builds_identity_and_tags_with_rows_that_sum_to_one(mfx):
    """[I | tags]: feature r for row r, then n + t; a pair named twice counts once; every entry float32(1 / entries of the
    row), so the row's sum is within one rounding per entry of 1: |sum - 1| <= n u (each entry errs by at most u / n
    relative to 1 / n ... times n entries; the float64 sum of the fp32 values adds nothing visible)."""
    n, n_tags = 6, 4
    tr = [0, 0, 0, 2, 2, 5, 5, 5, 5]
    tt = [3, 1, 3, 0, 2, 0, 1, 2, 3]
    Fm = mfx.hyb_features(n, tr, tt, n_tags)
    assert (Fm.n, Fm.nf) == (n, n + n_tags)
    assert Fm.ptr.tolist() == [0, 3, 4, 7, 8, 9, 14]
    assert Fm.idx.tolist() == [0, 7, 9, 1, 2, 6, 8, 3, 4, 5, 6, 7, 8, 9]
    ptr = Fm.ptr.astype(np.int64)
    for r in range(n):
        v = Fm.val[ptr[r]:ptr[r + 1]]
        assert np.all(v == F(1.0 / v.size)) and abs(v.astype(np.float64).sum() - 1.0) <= v.size * U
    raw = mfx.hyb_features(n, tr, tt, n_tags, normalize=False)
    assert np.all(raw.val == 1) and raw.idx.tolist() == Fm.idx.tolist()
    tags = mfx.hyb_features(n, tr, tt, n_tags, identity=False)
    assert tags.nf == n_tags and tags.ptr.tolist() == [0, 2, 2, 4, 4, 4, 8] and tags.idx.tolist() == [1, 3, 0, 2, 0, 1, 2, 3]
    ident = mfx.hyb_features(n)
    want = hx.identity(n)
    assert ident.nf == n and all(np.array_equal(getattr(ident, f), getattr(want, f)) for f in ("ptr", "idx", "val"))
    thirds = mfx.hyb_features(1, [0, 0], [0, 1], 2)
    assert thirds.val.tolist() == [F(1.0 / 3.0)] * 3
    with pytest.raises(AssertionError):
        mfx.hyb_features(n, [6], [0], n_tags)
    with pytest.raises(AssertionError):
        mfx.hyb_features(n, [0], [4], n_tags)


def test_exports_and_signatures(mfx):
    from mfx import _lib
    lib = mfx.lib()
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert C.sizeof(_lib.mfx_features) == 40
    assert [len(_lib.SIGNATURES[n][1]) for n in ("mfx_hyb_create", "mfx_hyb_embed", "mfx_hyb_apply")] == [9, 5, 16]
    for name in ("HybridSolver", "HybFeatures", "hyb_features", "hyb_embed", "hyb_apply"):
        assert hasattr(mfx, name)
    assert lib.mfx_version() == 2


# ------------------------------------------------------------------------------------------------ refusals without a device
def _create(mfx, R, k=8, lam=0.01, lr=0.05, batch=64, csx=None, fu=None, fi=None):
    from mfx import api
    p = mfx.parameter()
    p.k, p.lambda_ = k, lam
    cp = p.to_c()
    cp.k = k & 0xFFFFFFFF
    h = C.c_void_p()
    csx = api._csx(R) if csx is None else csx
    rc = mfx.lib().mfx_hyb_create(C.byref(h), C.byref(csx), None if fu is None else C.byref(fu), None if fi is None else C.byref(fi),
                                  C.byref(cp), lr, batch, 0, 0)
    assert not h.value
    return rc


@pytest.mark.parametrize("kw", [dict(k=0), dict(k=1025), dict(batch=0), dict(batch=(1 << 20) + 1), dict(batch=-1), dict(lr=-0.1),
                                dict(lr=float("nan")), dict(lr=float("inf")), dict(lam=-1.0), dict(lam=float("nan")),
                                dict(lam=float("inf"))])
def test_create_refuses_bad_arguments_before_the_device(mfx, R, kw):
    assert _create(mfx, R, **kw) == MFX_ERR_INVALID, mfx.lib().mfx_last_error()
    assert b"mfx_hyb_create" in mfx.lib().mfx_last_error()


def test_create_refuses_degenerate_matrices_features_and_nulls(mfx, R):
    from mfx import api
    lib = mfx.lib()
    for field, value in (("nnz", 0), ("cols", 1), ("csr_col_idx", None), ("csr_row_ptr", None)):
        broken = api._csx(R)
        setattr(broken, field, value)
        assert _create(mfx, R, csx=broken) == MFX_ERR_INVALID, field
    good_u, good_i = hx.identity(R.rows), hx.identity(R.cols)
    for side, good, n in (("fu", good_u, R.rows), ("fi", good_i, R.cols)):
        for field, value, word in (("n", n + 1, b"rows"), ("n", n - 1, b"rows"), ("nf", 0, b"nf"), ("nf", 0xFFFFFFFF, b"nf"), ("ptr", None, b"ptr")):
            c = good.to_c()
            setattr(c, field, value)
            assert _create(mfx, R, **{side: c}) == MFX_ERR_INVALID, (side, field, value)
            assert word in lib.mfx_last_error() and (b"user" if side == "fu" else b"item") in lib.mfx_last_error()
    # the sides are not interchangeable: the user matrix in the item's place has the wrong number of rows
    assert _create(mfx, R, fi=good_u.to_c()) == MFX_ERR_INVALID
    cp, csx, h = mfx.parameter().to_c(), api._csx(R), C.c_void_p()
    assert lib.mfx_hyb_create(None, C.byref(csx), None, None, C.byref(cp), 0.05, 64, 0, 0) == MFX_ERR_INVALID
    assert lib.mfx_hyb_create(C.byref(h), None, None, None, C.byref(cp), 0.05, 64, 0, 0) == MFX_ERR_INVALID
    assert lib.mfx_hyb_create(C.byref(h), C.byref(csx), None, None, None, 0.05, 64, 0, 0) == MFX_ERR_INVALID
    assert lib.mfx_hyb_create(C.byref(h), C.byref(csx), None, None, C.byref(cp), 0.05, 64, 0, 7) == MFX_ERR_INVALID  # memory space
    for fn in (lib.mfx_hyb_set_embeddings, lib.mfx_hyb_get_embeddings, lib.mfx_hyb_get_factors):
        assert fn(None, None, None, 0) == MFX_ERR_INVALID
    assert lib.mfx_hyb_steps(None, 1, None, None) == MFX_ERR_INVALID
    assert lib.mfx_hyb_epochs(None, 1, None, None) == MFX_ERR_INVALID
    assert lib.mfx_hyb_position(None, None) == MFX_ERR_INVALID
    assert lib.mfx_hyb_kernel_times(None, None) == MFX_ERR_INVALID
    assert lib.mfx_hyb_destroy(None) == 0


def test_operators_refuse_bad_arguments_before_the_device(mfx, R):
    Eu, Ei = bx.initial_factors(R.rows, R.cols, 3, 0)
    z = np.zeros(2, np.uint32)
    for kw in (dict(lr=-1.0), dict(lr=float("nan")), dict(lam=-1.0), dict(lam=float("inf"))):
        with pytest.raises(mfx.MfxError, match="mfx_hyb_apply"):
            mfx.hyb_apply(R.rows, R.cols, Eu, Ei, z, z, z, **{"lr": 0.05, "lam": 0.01, **kw})
    with pytest.raises(mfx.MfxError, match="2\\^20"):
        big = np.zeros((1 << 20) + 1, np.uint32)
        mfx.hyb_apply(R.rows, R.cols, Eu, Ei, big, big, big, 0.05, 0.01)
    Ek = np.zeros((R.rows, 1025), F)
    with pytest.raises(mfx.MfxError, match="k must be"):
        mfx.hyb_apply(R.rows, R.rows, Ek, Ek, z, z, z, 0.05, 0.01)
    with pytest.raises(mfx.MfxError, match="k must be"):
        mfx.hyb_embed(hx.identity(R.rows), Ek)
    # a feature matrix of another number of rows than the side, straight through the C ABI
    lib = mfx.lib()
    wrong = hx.identity(R.rows + 1).to_c()
    wrong.nf = R.rows
    stats = (C.c_int64 * 4)()
    args = (R.rows, R.cols, 3, C.byref(wrong), None, Eu.ctypes.data, Ei.ctypes.data, 2, z.ctypes.data_as(C.POINTER(C.c_uint32)),
            z.ctypes.data_as(C.POINTER(C.c_uint32)), z.ctypes.data_as(C.POINTER(C.c_uint32)), None, 0.05, 0.01, stats, 0)
    assert lib.mfx_hyb_apply(*args) == MFX_ERR_INVALID and b"user features" in lib.mfx_last_error()
    bad = hx.identity(4).to_c()
    bad.nf = 0
    assert lib.mfx_hyb_embed(C.byref(bad), Eu.ctypes.data, 3, Ei.ctypes.data, 0) == MFX_ERR_INVALID and b"nf" in lib.mfx_last_error()
    assert lib.mfx_hyb_embed(None, Eu.ctypes.data, 3, Ei.ctypes.data, 0) == MFX_ERR_INVALID
    # no rows: nothing to do, no device needed
    none = hx.features(0, 5, [], [], [])
    assert mfx.hyb_embed(none, np.zeros((5, 3), F)).shape == (0, 3)
