"""Exact CPU reference of EASE (mfx_ease_*): the contract of include/mfx.h ("EASE") restated in numpy.

The Gram matrix is slim_exact.gram_sums (the item-kNN similarities, fp32 terms cut to the 2^-36 grid, int64 sums) rounded to
fp32, with fp32(d_i + lambda) on the diagonal; a weight is one correctly rounded fp32 division of two entries of the inverse;
a score is the fp32 fused multiply-add chain over the row's entries in stored order (rec_exact.fmaf32), ranked by
rec_exact.expected_topn.  The inverse itself has no bit-exact restatement here: the library's two schedules are compared with
each other and with mfx_spd_inverse, and with ease_fp64 within a bound.  Nothing here calls the library."""
import numpy as np

import knn_exact as kx
import slim_exact as sx
from rec_exact import PAD, expected_topn, fmaf32

_F = np.float32
MAX_COLS = 32768
MAX_ENTRIES = kx.MAX_ENTRIES


def gram(X, lam):
    """fp32 [cols][cols]: G_ij = the fp32 of the integer sum for i != j, G_ii = fp32(fp32(d_i) + lambda).  Raises kx.BadTerm
    with the smallest item that has a bad term or an over-long column."""
    sums = sx.gram_sums(X)
    G = np.ascontiguousarray(kx.from_fixed(sums), _F)
    d = kx.from_fixed(np.diagonal(sums).copy()).astype(_F)
    g = d + _F(lam)
    assert g.dtype == _F
    G[np.arange(X.cols), np.arange(X.cols)] = g
    return G


def weights_from_inverse(P):
    """fp32 [n][n]: B_ij = fp32(-P_ij / P_jj) (one division, correctly rounded), B_ii = +0.  Raises ValueError naming the
    smallest j whose P_jj is not finite or not > 0."""
    P = np.asarray(P, _F)
    d = np.diagonal(P).copy()
    bad = ~((d > 0) & np.isfinite(d))
    if bad.any():
        raise ValueError(f"item {int(np.argmax(bad))}")
    with np.errstate(all="ignore"):
        B = (-P) / d[None, :]
    assert B.dtype == _F
    np.fill_diagonal(B, _F(0))
    return B


def scores(B, idx, val):
    """fp32 [cols]: s_j = +0, then s_j = fma(x_e, B[i_e][j], s_j) over the entries in stored order."""
    B = np.asarray(B, _F)
    s = np.zeros(B.shape[1], _F)
    for i, x in zip(np.asarray(idx, np.int64), np.asarray(val, _F)):
        s = fmaf32(x, B[i], s)
    return s


def recommend(B, ptr, idx, val, n_top, keep_seen=False):
    """(items uint32 [U][n_top], scores fp32 [U][n_top], bad_rows) of the CSR rows (ptr, idx, val) on the weights B."""
    B = np.asarray(B, _F)
    cols = B.shape[0]
    ptr = np.asarray(ptr, np.int64)
    n = len(ptr) - 1
    items = np.full((n, n_top), PAD, np.uint32)
    out = np.full((n, n_top), -np.inf, _F)
    bad_rows = 0
    for r in range(n):
        i = np.asarray(idx[ptr[r]:ptr[r + 1]], np.int64)
        x = np.asarray(val[ptr[r]:ptr[r + 1]], _F)
        if len(i) > MAX_ENTRIES or not np.isfinite(x).all():
            bad_rows += 1
            continue
        if len(i) == 0:
            continue  # pads, and not bad
        eligible = np.ones(cols, bool)
        if not keep_seen:
            eligible[i] = False
        it, sc = expected_topn(scores(B, i, x)[None, :], eligible[None, :], n_top)
        items[r], out[r] = it[0], sc[0]
    return items, out, bad_rows


def ease_fp64(X, lam):
    """The model in fp64 from the dense matrix of X: (G, P, B) with G = X^T X + lambda I, P = G^-1, B = I - P diag(P)^-1."""
    D = np.zeros((X.rows, X.cols), np.float64)
    ptr = X.csr_row_ptr.astype(np.int64)
    rows = np.repeat(np.arange(X.rows), np.diff(ptr))
    D[rows, X.csr_col_idx.astype(np.int64)] = X.csr_val.astype(np.float64)
    G = D.T @ D + float(lam) * np.eye(X.cols)
    P = np.linalg.inv(G)
    B = -P / np.diagonal(P)[None, :]
    np.fill_diagonal(B, 0.0)
    return G, P, B
