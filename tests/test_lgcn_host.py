"""LightGCN without a GPU: the self-checks of the exact reference of tests/lgcn_exact.py (layers = 0 is BPR, the propagation
against a float64 dense product, the 1024-entry segment rule against a scalar restatement) and the refusals of the new
entry points that never reach the device."""
import ctypes as C

import numpy as np
import pytest

import bpr_exact as bx
import lgcn_exact as lx
from rec_exact import fmaf32

MFX_ERR_INVALID = -1  # include/mfx.h
F = np.float32
U = 2.0 ** -24  # the unit roundoff of fp32
NAMES = ("mfx_lgcn_create", "mfx_lgcn_set_base", "mfx_lgcn_get_base", "mfx_lgcn_get_factors", "mfx_lgcn_steps", "mfx_lgcn_epochs",
         "mfx_lgcn_position", "mfx_lgcn_kernel_times", "mfx_lgcn_destroy", "mfx_lgcn_propagate", "mfx_lgcn_apply")


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    return m


@pytest.fixture(autouse=True)
def _library_has_lgcn(mfx):
    """tests/lgcn_exact.py restates the contract of the library's LightGCN entry points: without them it has no subject."""
    assert all(hasattr(mfx.lib(), name) for name in NAMES)


@pytest.fixture(scope="module")
def R():
    return bx.small_matrix()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ the reference itself
def test_step_without_layers_is_the_bpr_step(R):
    k, n = 7, 300
    W, H = bx.initial_factors(R.rows, R.cols, k, 1)
    u, i, j, s = bx.triples(R, 4, 0, n)
    j[5] = i[5]  # a row touched twice by one slot
    s[5] = False
    want = bx.step(W, H, u, i, j, s, 0.05, 0.01)
    got = lx.step(R, W, H, u, i, j, s, 0, 0.05, 0.01)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and got[2] == want[2]
    assert not same_bits(got[0], W)
    Wp, Hp = lx.propagate(R, W, H, 0)
    assert same_bits(Wp, W) and same_bits(Hp, H)


def test_propagation_is_within_fp32_rounding_of_the_dense_float64_product(R):
    """E^l against A^l E^0 in float64, A = D_u^-1/2 P D_i^-1/2 on the bipartite graph (P the 0 / 1 pattern).

    One half-pass computes, per destination row r of n entries, fl(s_r * chain) with chain the n-term FMA chain of
    s_e * x_e.  The chain rounds n times, the final multiply once, and each of s_r, s_e is the fp32 rounding of the exact
    1 / sqrt(d): with u = 2^-24 every term carries a factor (1 + d_1) .. (1 + d_m), m <= n + 3, so
        |computed - exact| <= ((1 + u)^(n + 3) - 1) * sum_e |s_r s_e x_e|  <=  1.01 (n + 3) u * (A |X|)[r]
    for n + 3 <= 63 (the longest row here has 40 + 3 terms; 1.01 covers the second order).  The error of layer l then obeys
    err_l <= A err_{l-1} + 1.01 (n + 3) u A |E^{l-1}|, and since A has no negative entry, by induction
        err_l <= 1.01 l (n_max + 3) u (1 + tiny) * (A^l |E^0|)   (entrywise),
    tiny from |E^{l-1}| <= (1 + l (n_max + 3) u) A^{l-1} |E^0|: below 1e-4 here.  The mean adds L additions, one multiply and
    the rounding of c_L: (L + 2) u relative to the sum of the absolute layers."""
    k, layers = 5, 3
    W0, H0 = bx.initial_factors(R.rows, R.cols, k, 2)
    P = np.zeros((R.rows, R.cols))
    P[np.repeat(np.arange(R.rows), np.diff(R.csr_row_ptr.astype(np.int64))), R.csr_col_idx] = 1.0
    du, di = P.sum(1), P.sum(0)
    n_max = int(max(du.max(), di.max()))
    assert n_max + 3 <= 63
    with np.errstate(divide="ignore"):
        A = P * np.where(du > 0, 1 / np.sqrt(du), 0.0)[:, None] * np.where(di > 0, 1 / np.sqrt(di), 0.0)[None, :]
    E = lx.layers_of(R, W0, H0, layers)
    Wl, Hl = W0.astype(np.float64), H0.astype(np.float64)
    Wa, Ha = np.abs(Wl), np.abs(Hl)
    sumW, sumH, absW, absH = Wl.copy(), Hl.copy(), Wa.copy(), Ha.copy()
    for l in range(1, layers + 1):
        Wl, Hl = A @ Hl, A.T @ Wl
        Wa, Ha = A @ Ha, A.T @ Wa
        bound = 1.01 * l * (n_max + 3) * U * (1 + 1e-4)
        for got, want, scale in ((E[l][0], Wl, Wa), (E[l][1], Hl, Ha)):
            err = np.abs(got.astype(np.float64) - want)
            print("layer", l, "worst error / bound", float((err / np.maximum(bound * scale, 1e-300)).max()))
            assert np.all(err <= bound * scale)
            assert np.any(err > 0)  # (fp32 against fp64: the test compares two different computations)
        sumW += Wl; sumH += Hl; absW += Wa; absH += Ha
    Wf, Hf = lx.propagate(R, W0, H0, layers)
    bound = (1.01 * layers * (n_max + 3) * (1 + 1e-4) + (layers + 2)) * U
    for got, want, scale in ((Wf, sumW, absW), (Hf, sumH, absH)):
        assert np.all(np.abs(got.astype(np.float64) - want / (layers + 1)) <= bound * scale / (layers + 1))
    # empty rows give +0 layers and the base over L + 1
    empty = np.nonzero(du == 0)[0]
    for r in empty:
        assert np.all(bits(E[1][0][r]) == 0)


def _row_by_scalars(s, x):
    """One coordinate of one row, written entry by entry: chains of 1024 from +0, their sums added left to right."""
    sums = []
    for lo in range(0, len(x), lx.SEGMENT):
        acc = np.zeros(1, F)
        for e in range(lo, min(lo + lx.SEGMENT, len(x))):
            acc = fmaf32(s[e:e + 1], x[e:e + 1], acc)
        sums.append(acc[0])
    total = sums[0]
    for t in sums[1:]:
        total = F(total + t)
    return total


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2048, 2049])
def test_segment_rule_at_the_boundaries(n):
    """A row of n entries: half_pass equals the scalar restatement; up to 1024 entries that is the single chain, and with two
    whole segments it is not (at 1025 the second segment is one product, which rounds like the chain's last step almost always)."""
    rng = np.random.default_rng(n)
    m, k = n + 3, 2
    ids = rng.permutation(m)[:n]
    ptr = np.array([0, n, n], np.int64)  # the row under test and an empty row
    X = rng.standard_normal((m, k)).astype(F)
    s_src = (rng.random(m).astype(F) + F(0.5))
    s_dst = np.array([0.37, 0.0], F)
    got = lx.half_pass(ptr, ids, s_src, s_dst, X)
    assert got.shape == (2, k) and np.all(bits(got[1]) == 0)
    one_chain = np.zeros(k, F)
    for e in ids:
        one_chain = fmaf32(s_src[e], X[e], one_chain)
    differs = False
    for c in range(k):
        want = F(s_dst[0] * _row_by_scalars(s_src[ids], X[ids, c]))
        assert bits(got[0, c]) == bits(want)
        differs |= bits(F(s_dst[0] * one_chain[c])) != bits(want)
    assert n < 2 * lx.SEGMENT or differs
    if n <= lx.SEGMENT:
        assert same_bits(got[0], s_dst[0] * one_chain)


def test_scales_and_segment_matrix():
    s = lx.scales(np.array([0, 0, 1, 5, 14]))
    assert s.dtype == F and s.tolist() == [0.0, 1.0, F(0.5), F(1.0 / 3.0)]
    S = lx.segment_matrix()
    assert S.rows == S.cols == 3100 and 20_000 <= S.nnz <= 23_000
    assert np.any(np.diff(S.csr_row_ptr.astype(np.int64)) == 0) and np.any(np.diff(S.csc_col_ptr.astype(np.int64)) == 0)


# ------------------------------------------------------------------------------------------------ refusals without a device
def _create(mfx, R, k=8, lam=0.01, lr=0.05, batch=64, layers=2, csx=None):
    from mfx import api
    p = mfx.parameter()
    p.k, p.lambda_ = k, lam
    cp = p.to_c()
    cp.k = k & 0xFFFFFFFF
    h = C.c_void_p()
    csx = api._csx(R) if csx is None else csx
    rc = mfx.lib().mfx_lgcn_create(C.byref(h), C.byref(csx), C.byref(cp), lr, batch, layers, 0, 0)
    assert not h.value
    return rc


@pytest.mark.parametrize("kw", [dict(k=0), dict(k=1025), dict(batch=0), dict(batch=(1 << 20) + 1), dict(batch=-1), dict(lr=-0.1),
                                dict(lr=float("nan")), dict(lr=float("inf")), dict(lam=-1.0), dict(lam=float("nan")),
                                dict(lam=float("inf")), dict(layers=-1), dict(layers=9)])
def test_create_refuses_bad_arguments_before_the_device(mfx, R, kw):
    assert _create(mfx, R, **kw) == MFX_ERR_INVALID, mfx.lib().mfx_last_error()
    assert b"mfx_lgcn_create" in mfx.lib().mfx_last_error()


def test_create_refuses_degenerate_matrices_and_nulls(mfx, R):
    from mfx import api
    lib = mfx.lib()
    for field, value in (("nnz", 0), ("cols", 1), ("csr_col_idx", None), ("csc_row_idx", None), ("csc_col_ptr", None)):
        broken = api._csx(R)
        setattr(broken, field, value)
        assert _create(mfx, R, csx=broken) == MFX_ERR_INVALID, field
    cp, csx, h = mfx.parameter().to_c(), api._csx(R), C.c_void_p()
    assert lib.mfx_lgcn_create(None, C.byref(csx), C.byref(cp), 0.05, 64, 2, 0, 0) == MFX_ERR_INVALID
    assert lib.mfx_lgcn_create(C.byref(h), None, C.byref(cp), 0.05, 64, 2, 0, 0) == MFX_ERR_INVALID
    assert lib.mfx_lgcn_create(C.byref(h), C.byref(csx), None, 0.05, 64, 2, 0, 0) == MFX_ERR_INVALID
    assert lib.mfx_lgcn_create(C.byref(h), C.byref(csx), C.byref(cp), 0.05, 64, 2, 0, 7) == MFX_ERR_INVALID  # memory space
    for fn in (lib.mfx_lgcn_set_base, lib.mfx_lgcn_get_base, lib.mfx_lgcn_get_factors):
        assert fn(None, None, None, 0) == MFX_ERR_INVALID
    assert lib.mfx_lgcn_steps(None, 1, None, None) == MFX_ERR_INVALID
    assert lib.mfx_lgcn_epochs(None, 1, None, None) == MFX_ERR_INVALID
    assert lib.mfx_lgcn_position(None, None) == MFX_ERR_INVALID
    assert lib.mfx_lgcn_kernel_times(None, None) == MFX_ERR_INVALID
    assert lib.mfx_lgcn_destroy(None) == 0


def test_operators_refuse_bad_arguments_before_the_device(mfx, R):
    W, H = bx.initial_factors(R.rows, R.cols, 3, 0)
    z = np.zeros(2, np.uint32)
    for kw in (dict(lr=-1.0), dict(lr=float("nan")), dict(lam=-1.0), dict(lam=float("inf")), dict(layers=-1), dict(layers=9)):
        with pytest.raises(mfx.MfxError, match="mfx_lgcn_apply"):
            mfx.lgcn_apply(R, W, H, z, z, z, **{"layers": 2, "lr": 0.05, "lam": 0.01, **kw})
    with pytest.raises(mfx.MfxError, match="2\\^20"):
        big = np.zeros((1 << 20) + 1, np.uint32)
        mfx.lgcn_apply(R, W, H, big, big, big, 2, 0.05, 0.01)
    for layers in (-1, 9):
        with pytest.raises(mfx.MfxError, match="layers must be"):
            mfx.lgcn_propagate(R, W, H, layers)
    Wk, Hk = np.zeros((R.rows, 1025), F), np.zeros((R.cols, 1025), F)
    with pytest.raises(mfx.MfxError, match="k must be"):
        mfx.lgcn_propagate(R, Wk, Hk, 1)
    with pytest.raises(mfx.MfxError, match="k must be"):
        mfx.lgcn_apply(R, Wk, Hk, z, z, z, 1, 0.05, 0.01)
