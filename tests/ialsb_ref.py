"""numpy fp64 reference of implicit ALS by block subspace sweeps (include/mfx.h, mfx_ials_block_create).

One half-sweep = for every segment, from its current row y and the scores s_j = <x_j, y> of its entries, one pass
over the blocks [b d, min(k, (b + 1) d)) in ascending order; a step is the exact minimiser of the segment's objective
over the block with the rest of y fixed.  Conventions of tests/ials_ref.py (w = fp32(alpha r), an explicit zero is no
entry, an empty segment gives y = 0)."""
import numpy as np

import ials_ref


def block_sweep(ptr, idx, val, X, Y_in, lam, alpha, d):
    X = np.asarray(X, np.float64); k = X.shape[1]
    G = X.T @ X + lam * np.eye(k); Y = np.array(Y_in, np.float64)
    for s in range(len(ptr) - 1):
        lo, hi = int(ptr[s]), int(ptr[s + 1])
        if hi == lo: Y[s] = 0; continue
        v = np.asarray(val[lo:hi], np.float32); w = ials_ref.weights(v, alpha); pos = v > 0
        a, c1, Xj = np.where(pos, w, 0.0), np.where(pos, 1.0 + w, 0.0), X[np.asarray(idx[lo:hi], np.int64)]
        y = Y[s].copy(); sc = Xj @ y
        for b0 in range(0, k, d):
            b1 = min(k, b0 + d); Xb = Xj[:, b0:b1]
            g = Xb.T @ (a * sc - c1) + G[b0:b1] @ y
            A = (Xb * a[:, None]).T @ Xb + G[b0:b1, b0:b1]
            dl = np.linalg.solve(A, g); y[b0:b1] -= dl; sc -= Xb @ dl
        Y[s] = y
    return Y


def iteration(R, H, W, lam, alpha, d):
    """One full iteration: W-half over H from W, then H-half over the new W from H (fp64)."""
    W = block_sweep(R.csr_row_ptr, R.csr_col_idx, R.csr_val, H, W, lam, alpha, d)
    H = block_sweep(R.csc_col_ptr, R.csc_row_idx, R.csc_val, W, H, lam, alpha, d)
    return W, H
