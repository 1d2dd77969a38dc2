"""numpy fp64 reference of explicit ALS by block subspace sweeps (include/mfx.h, mfx_als_block_create).

One half-sweep = for every segment, from its current row y and the scores s_j = <x_j, y> of its entries, one pass
over the blocks [b d, min(k, (b + 1) d)) in ascending order; a step is the exact minimiser of the segment's objective
    f(y) = sum_j (r_j - <x_j, y>)^2 + rho |y|^2
over the block with the rest of y fixed.  rho = lambda (reg 0) or fp32(lambda * n) for a segment of n stored entries
(reg 1).  Every stored entry counts, explicit zeros and negative values included; an empty segment gives y = 0."""
import numpy as np


def rho_of(lam, n, reg):
    return float(np.float32(lam) * np.float32(n)) if reg else float(np.float32(lam))


def dense_system(ptr, idx, val, s, X, lam, reg):
    """(A, b) of segment s in fp64: A = sum x x^T + rho I, b = sum r x."""
    lo, hi = int(ptr[s]), int(ptr[s + 1])
    Xj = np.asarray(X, np.float64)[np.asarray(idx[lo:hi], np.int64)]
    return Xj.T @ Xj + rho_of(lam, hi - lo, reg) * np.eye(Xj.shape[1]), Xj.T @ np.asarray(val[lo:hi], np.float64)


def backward_error(A, y, b):
    """|A y - b| / (|A| |y| + |b|) in 2-norms (tests/ials_ref.py's measure)."""
    y = np.asarray(y, np.float64)
    return float(np.linalg.norm(A @ y - b) / (np.linalg.norm(A, 2) * np.linalg.norm(y) + np.linalg.norm(b)))


def block_sweep(ptr, idx, val, X, Y_in, lam, d, reg):
    X = np.asarray(X, np.float64); k = X.shape[1]
    Y = np.array(Y_in, np.float64)
    for s in range(len(ptr) - 1):
        lo, hi = int(ptr[s]), int(ptr[s + 1])
        if hi == lo: Y[s] = 0; continue
        r, Xj, rho = np.asarray(val[lo:hi], np.float64), X[np.asarray(idx[lo:hi], np.int64)], rho_of(lam, hi - lo, reg)
        y = Y[s].copy(); sc = Xj @ y
        for b0 in range(0, k, d):
            b1 = min(k, b0 + d); Xb = Xj[:, b0:b1]
            A = Xb.T @ Xb + rho * np.eye(b1 - b0)
            z = np.linalg.solve(A, Xb.T @ (r - sc) - rho * y[b0:b1])
            y[b0:b1] += z; sc += Xb @ z
        Y[s] = y
    return Y


def iteration(R, H, W, lam, d, reg):
    """One full iteration: W-half over H from W, then H-half over the new W from H (fp64)."""
    W = block_sweep(R.csr_row_ptr, R.csr_col_idx, R.csr_val, H, W, lam, d, reg)
    H = block_sweep(R.csc_col_ptr, R.csc_row_idx, R.csc_val, W, H, lam, d, reg)
    return W, H


def objective(R, W, H, lam, reg):
    """The training objective in fp64: sum over stored pairs of (r - <w, h>)^2 plus the regulariser, lambda (|W|^2 + |H|^2)
    at reg 0 and lambda (sum_u n_u |w_u|^2 + sum_i n_i |h_i|^2) at reg 1 (the CCD++ objective)."""
    W, H = np.asarray(W, np.float64), np.asarray(H, np.float64)
    nr, nc = np.diff(R.csr_row_ptr.astype(np.int64)), np.diff(R.csc_col_ptr.astype(np.int64))
    rows = np.repeat(np.arange(R.rows), nr)
    cols = np.asarray(R.csr_col_idx, np.int64)
    e = np.asarray(R.csr_val, np.float64) - np.einsum("ij,ij->i", W[rows], H[cols])
    wr = np.array([rho_of(lam, n, reg) for n in nr]) if reg else np.full(R.rows, rho_of(lam, 0, 0))
    wc = np.array([rho_of(lam, n, reg) for n in nc]) if reg else np.full(R.cols, rho_of(lam, 0, 0))
    return float(e @ e + wr @ (W * W).sum(1) + wc @ (H * H).sum(1))


def test_rmse(T, W, H):
    W, H = np.asarray(W, np.float64), np.asarray(H, np.float64)
    e = np.asarray(T.test_val, np.float64) - np.einsum("ij,ij->i", W[np.asarray(T.test_row, np.int64)], H[np.asarray(T.test_col, np.int64)])
    return float(np.sqrt(e @ e / len(e)))


test_rmse.__test__ = False  # not a pytest test
