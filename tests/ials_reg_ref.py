"""numpy fp64 reference of implicit ALS with an unobserved weight alpha0 and a frequency-scaled regulariser
(include/mfx.h, mfx_ials_create_reg / mfx_ials_block_create_reg).

For a segment s over the fixed factor X with N rows, n_s = its stored entries with r > 0 and w = fp32(alpha r):
    f_s(y) = sum_{r_j > 0} [(alpha0 + w_j)(1 - s_j)^2 - alpha0 s_j^2] + alpha0 y^T X^T X y + rho_s |y|^2
    rho_s  = fp32(lambda (n_s + alpha0 N)^nu)
Conventions of tests/ials_ref.py: an explicit zero is no entry, an empty segment gives y = 0, every system is formed
in the DENSE form over all rows of X (confidence alpha0 off the entries, alpha0 + w on them), no X^T X shortcut."""
import numpy as np

import ials_ref


def rho(ptr, val, N, lam, alpha0, nu):
    """rho [nseg] as the library forms it: fp64 throughout, rounded once to fp32 (returned widened to fp64).
    lam and alpha0 are the fp32 values the C ABI receives."""
    ptr = np.asarray(ptr, np.int64)
    v = np.asarray(val, np.float32)
    cs = np.concatenate([[0], np.cumsum(v > 0)])
    n = (cs[ptr[1:]] - cs[ptr[:-1]]).astype(np.float64)
    lam64, a064, nu64 = float(np.float32(lam)), float(np.float32(alpha0)), float(np.float32(nu))
    return (lam64 * np.power(n + a064 * float(N), nu64)).astype(np.float32).astype(np.float64)


def dense_segment(ptr, idx, val, s, nrows_x, alpha, alpha0):
    """Confidence c [nrows_x] and preference p [nrows_x] of segment s over all rows of X."""
    lo, hi = int(ptr[s]), int(ptr[s + 1])
    c = np.full(nrows_x, float(np.float32(alpha0)))
    p = np.zeros(nrows_x)
    j = np.asarray(idx[lo:hi], np.int64)
    v = np.asarray(val[lo:hi], np.float32)
    w = ials_ref.weights(v, alpha)
    pos = v > 0
    c[j[pos]] = float(np.float32(alpha0)) + w[pos]
    p[j[pos]] = 1.0
    return c, p


def dense_system(ptr, idx, val, s, X, lam, alpha, alpha0, nu, rho_s=None):
    """(A, b) of segment s in the dense form: A = X^T C X + rho_s I, b = X^T C p."""
    X = np.asarray(X, np.float64)
    if rho_s is None:
        rho_s = rho(ptr, val, X.shape[0], lam, alpha0, nu)[s]
    c, p = dense_segment(ptr, idx, val, s, X.shape[0], alpha, alpha0)
    A = (X * c[:, None]).T @ X + rho_s * np.eye(X.shape[1])
    b = X.T @ (c * p)
    return A, b


def half(ptr, idx, val, X, lam, alpha, alpha0, nu):
    """Y [nseg][k]: every segment's dense system solved in fp64 (empty segments: y = 0)."""
    nseg, k = len(ptr) - 1, X.shape[1]
    rh = rho(ptr, val, X.shape[0], lam, alpha0, nu)
    Y = np.zeros((nseg, k))
    for s in range(nseg):
        if ptr[s + 1] == ptr[s]:
            continue
        A, b = dense_system(ptr, idx, val, s, X, lam, alpha, alpha0, nu, rh[s])
        Y[s] = np.linalg.solve(A, b)
    return Y


def segment_objective(ptr, idx, val, s, X, y, lam, alpha, alpha0, nu):
    """f_s(y) in the dense form (up to the constant sum of c p): sum over all rows of c (p - <x, y>)^2 + rho_s |y|^2."""
    X = np.asarray(X, np.float64)
    c, p = dense_segment(ptr, idx, val, s, X.shape[0], alpha, alpha0)
    r = rho(ptr, val, X.shape[0], lam, alpha0, nu)[s]
    return float(np.sum(c * (p - X @ y) ** 2) + r * np.dot(y, y))


def block_sweep(ptr, idx, val, X, Y_in, lam, alpha, alpha0, nu, d, S=None):
    """One half-sweep of block subspace sweeps from Y_in: for every segment one pass over the blocks of d coordinates.
    S: X^T X in fp64 when the caller has it already (left unchanged)."""
    X = np.asarray(X, np.float64)
    k = X.shape[1]
    a0 = float(np.float32(alpha0))
    G0 = a0 * (X.T @ X if S is None else S)
    rh = rho(ptr, val, X.shape[0], lam, alpha0, nu)
    Y = np.array(Y_in, np.float64)
    for s in range(len(ptr) - 1):
        lo, hi = int(ptr[s]), int(ptr[s + 1])
        if hi == lo:
            Y[s] = 0
            continue
        v = np.asarray(val[lo:hi], np.float32)
        w = ials_ref.weights(v, alpha)
        pos = v > 0
        a, c1, Xj = np.where(pos, w, 0.0), np.where(pos, a0 + w, 0.0), X[np.asarray(idx[lo:hi], np.int64)]
        y = Y[s].copy()
        sc = Xj @ y
        for b0 in range(0, k, d):
            b1 = min(k, b0 + d)
            Xb = Xj[:, b0:b1]
            g = Xb.T @ (a * sc - c1) + G0[b0:b1] @ y + rh[s] * y[b0:b1]
            A = (Xb * a[:, None]).T @ Xb + G0[b0:b1, b0:b1] + rh[s] * np.eye(b1 - b0)
            dl = np.linalg.solve(A, g)
            y[b0:b1] -= dl
            sc -= Xb @ dl
        Y[s] = y
    return Y


def iteration(R, H, lam, alpha, alpha0, nu, W=None, d=None):
    """One full iteration (fp64): W over H on the CSR rows, then H over the new W on the CSC columns.  d = None: the
    exact solves; else block sweeps of d coordinates from W (None = zeros) and H."""
    if d is None:
        W = half(R.csr_row_ptr, R.csr_col_idx, R.csr_val, H, lam, alpha, alpha0, nu)
        H = half(R.csc_col_ptr, R.csc_row_idx, R.csc_val, W, lam, alpha, alpha0, nu)
        return W, H
    if W is None:
        W = np.zeros((R.rows, H.shape[1]))
    W = block_sweep(R.csr_row_ptr, R.csr_col_idx, R.csr_val, H, W, lam, alpha, alpha0, nu, d)
    H = block_sweep(R.csc_col_ptr, R.csc_row_idx, R.csc_val, W, H, lam, alpha, alpha0, nu, d)
    return W, H


def _reg_term(R, W, H, lam, alpha0, nu):
    ru = rho(R.csr_row_ptr, R.csr_val, R.cols, lam, alpha0, nu)
    ri = rho(R.csc_col_ptr, R.csc_val, R.rows, lam, alpha0, nu)
    return float(np.sum(ru * np.sum(W * W, axis=1)) + np.sum(ri * np.sum(H * H, axis=1)))


def dense_loss(R, W, H, lam, alpha, alpha0, nu, scores=None):
    """sum over ALL rows x cols pairs of c (p - s)^2 + sum_u rho_u |w_u|^2 + sum_i rho_i |h_i|^2, fp64."""
    W = np.asarray(W, np.float64)
    H = np.asarray(H, np.float64)
    S = W @ H.T if scores is None else np.asarray(scores, np.float64)
    a0 = float(np.float32(alpha0))
    Cm = np.full_like(S, a0)
    P = np.zeros_like(S)
    r = np.repeat(np.arange(R.rows), np.diff(R.csr_row_ptr.astype(np.int64)))
    c = R.csr_col_idx.astype(np.int64)
    v = R.csr_val.astype(np.float32)
    pos = v > 0
    Cm[r[pos], c[pos]] = a0 + ials_ref.weights(v[pos], alpha)
    P[r[pos], c[pos]] = 1.0
    return float(np.sum(Cm * (P - S) ** 2)) + _reg_term(R, W, H, lam, alpha0, nu)


def shortcut_loss(R, W, H, lam, alpha, alpha0, nu, scores=None):
    """The library's formula: sum over the entries of [(alpha0 + w)(1 - s)^2 - alpha0 s^2] + alpha0 <W^T W, H^T H>_F +
    the regularisers."""
    W = np.asarray(W, np.float64)
    H = np.asarray(H, np.float64)
    a0 = float(np.float32(alpha0))
    r = np.repeat(np.arange(R.rows), np.diff(R.csr_row_ptr.astype(np.int64)))
    c = R.csr_col_idx.astype(np.int64)
    v = R.csr_val.astype(np.float32)
    pos = v > 0
    r, c, w = r[pos], c[pos], ials_ref.weights(v[pos], alpha)
    s = np.einsum("ij,ij->i", W[r], H[c]) if scores is None else np.asarray(scores, np.float64)[r, c]
    ent = np.sum((a0 + w) * (1.0 - s) ** 2 - a0 * s * s)
    return float(ent + a0 * np.sum((W.T @ W) * (H.T @ H))) + _reg_term(R, W, H, lam, alpha0, nu)


backward_error = ials_ref.backward_error
