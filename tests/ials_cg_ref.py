"""numpy fp64 reference of implicit ALS by preconditioned conjugate gradients (include/mfx.h, mfx_ials_cg_create).

A half-sweep over the fixed side X is foldin_cg_ref.rows(IMPLICIT, ...) on the segments of the side being solved: every row
from its current value (None = cold, from zero) by at most `steps` steps of conjugate gradients preconditioned by the fp64
inverse of G = X^T X + lambda I, a row stopping once |b - A y| <= tol |b|.  An iteration is the W-half over H on the CSR
rows, then the H-half over the new W on the CSC columns, both warm from the current factors."""
import numpy as np

import foldin_cg_ref


def half(ptr, idx, val, X, lam, alpha, Y_init, steps, tol):
    """(Y [nseg][k] fp64, steps_done [nseg])."""
    return foldin_cg_ref.rows(foldin_cg_ref.IMPLICIT, ptr, idx, val, np.asarray(X, np.float64), lam, alpha, Y_init, steps, tol)


def iteration(R, H, W, lam, alpha, steps, tol):
    """(W, H, (steps of the W-half, steps of the H-half)); W None = the W-half starts cold."""
    W, cw = half(R.csr_row_ptr, R.csr_col_idx, R.csr_val, H, lam, alpha, W, steps, tol)
    H, ch = half(R.csc_col_ptr, R.csc_row_idx, R.csc_val, W, lam, alpha, H, steps, tol)
    return W, H, (cw, ch)
