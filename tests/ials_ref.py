"""numpy fp64 reference of implicit-feedback ALS (include/mfx.h, mfx_ials_create).

Preference p = (r > 0), confidence c = 1 + w with w = fp32(alpha * r).  Every per-segment system is solved in the
DENSE form, (X^T C_s X + lambda I) y = X^T C_s p_s over ALL rows of X, without the X^T X shortcut the library uses,
so a base Gramian over the wrong rows, or one added twice, shows up as a wrong solution."""
import numpy as np


def weights(val, alpha):
    """w = fp32(alpha * r) as the library forms it, widened to fp64."""
    return (np.float32(alpha) * np.asarray(val, np.float32)).astype(np.float64)


def dense_segment(ptr, idx, val, s, nrows_x, alpha):
    """Confidence c [nrows_x] and preference p [nrows_x] of segment s over all rows of X."""
    lo, hi = int(ptr[s]), int(ptr[s + 1])
    c = np.ones(nrows_x)
    p = np.zeros(nrows_x)
    j = np.asarray(idx[lo:hi], np.int64)
    v = np.asarray(val[lo:hi], np.float32)
    w = weights(v, alpha)
    pos = v > 0
    c[j[pos]] = 1.0 + w[pos]  # an explicit zero is no entry: c = 1, p = 0
    p[j[pos]] = 1.0
    return c, p


def dense_system(ptr, idx, val, s, X, lam, alpha):
    """(A, b) of segment s in the dense form: A = X^T C X + lambda I, b = X^T C p."""
    X = np.asarray(X, np.float64)
    c, p = dense_segment(ptr, idx, val, s, X.shape[0], alpha)
    A = (X * c[:, None]).T @ X + lam * np.eye(X.shape[1])
    b = X.T @ (c * p)
    return A, b


def shortcut_system(ptr, idx, val, s, X, lam, alpha):
    """The same system as the library forms it: X^T X + lambda I + sum_j w_j x_j x_j^T, sum_{r_j > 0} (1 + w_j) x_j."""
    X = np.asarray(X, np.float64)
    lo, hi = int(ptr[s]), int(ptr[s + 1])
    j = np.asarray(idx[lo:hi], np.int64)
    v = np.asarray(val[lo:hi], np.float32)
    w = weights(v, alpha)
    Xj = X[j]
    A = X.T @ X + lam * np.eye(X.shape[1]) + (Xj * w[:, None]).T @ Xj
    b = Xj.T @ np.where(v > 0, 1.0 + w, 0.0)
    return A, b


def half(ptr, idx, val, X, lam, alpha):
    """Y [nseg][k]: every segment's dense system solved in fp64 (empty segments: y = 0)."""
    nseg, k = len(ptr) - 1, X.shape[1]
    Y = np.zeros((nseg, k))
    for s in range(nseg):
        if ptr[s + 1] == ptr[s]:
            continue
        A, b = dense_system(ptr, idx, val, s, X, lam, alpha)
        Y[s] = np.linalg.solve(A, b)
    return Y


def iteration(R, H, lam, alpha):
    """One full iteration: W over H on the CSR rows, then H over the new W on the CSC columns (fp64)."""
    W = half(R.csr_row_ptr, R.csr_col_idx, R.csr_val, H, lam, alpha)
    H = half(R.csc_col_ptr, R.csc_row_idx, R.csc_val, W, lam, alpha)
    return W, H


def dense_loss(R, W, H, lam, alpha, scores=None):
    """sum over ALL rows x cols pairs of c (p - s)^2 + lambda (|W|^2 + |H|^2), fp64.  scores: s [rows][cols] (default
    the fp64 product W H^T)."""
    W = np.asarray(W, np.float64)
    H = np.asarray(H, np.float64)
    S = W @ H.T if scores is None else np.asarray(scores, np.float64)
    C = np.ones_like(S)
    P = np.zeros_like(S)
    r = np.repeat(np.arange(R.rows), np.diff(R.csr_row_ptr.astype(np.int64)))
    c = R.csr_col_idx.astype(np.int64)
    v = R.csr_val.astype(np.float32)
    pos = v > 0
    C[r[pos], c[pos]] = 1.0 + weights(v[pos], alpha)
    P[r[pos], c[pos]] = 1.0
    return float(np.sum(C * (P - S) ** 2) + lam * (np.sum(W * W) + np.sum(H * H)))


def shortcut_loss(R, W, H, lam, alpha, scores=None):
    """The library's formula: sum over the entries of [c (p - s)^2 - s^2] + <W^T W, H^T H>_F + lambda (|W|^2 + |H|^2)."""
    W = np.asarray(W, np.float64)
    H = np.asarray(H, np.float64)
    r = np.repeat(np.arange(R.rows), np.diff(R.csr_row_ptr.astype(np.int64)))
    c = R.csr_col_idx.astype(np.int64)
    v = R.csr_val.astype(np.float32)
    pos = v > 0
    r, c, w = r[pos], c[pos], weights(v[pos], alpha)
    s = np.einsum("ij,ij->i", W[r], H[c]) if scores is None else np.asarray(scores, np.float64)[r, c]
    ent = np.sum((1.0 + w) * (1.0 - s) ** 2 - s * s)
    return float(ent + np.sum((W.T @ W) * (H.T @ H)) + lam * (np.sum(W * W) + np.sum(H * H)))


def backward_error(A, y, b):
    """Normwise backward error |A y - b| / (|A| |y| + |b|) (2-norms, fp64)."""
    A = np.asarray(A, np.float64)
    y = np.asarray(y, np.float64)
    num = np.linalg.norm(A @ y - b)
    den = np.linalg.norm(A, 2) * np.linalg.norm(y) + np.linalg.norm(b)
    return float(num / den) if den > 0 else float(num)
