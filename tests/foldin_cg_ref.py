"""numpy fp64 reference of fold-in by preconditioned conjugate gradients (include/mfx.h, mfx_rec_fold_in_cg_setup), and the
inputs that tests/test_foldin_cg_host.py pins it on and tests/test_gpu_foldin_cg.py runs the library on.

Row u over its counting entries e (implicit: r_e > 0; explicit: every entry), H the handle's fp32 factors widened:
    implicit:  A p = G p + sum_e w_e <h_e, p> h_e,  b = sum_e fp32(1 + w_e) h_e,  w_e = fp32(alpha r_e),  M^-1 = G^-1
    explicit:  A p = rho p + sum_e <h_e, p> h_e,    b = sum_e r_e h_e,  rho = lambda (ALS) or fp32(lambda n) (CCD),  M^-1 = I
    y = W_init[u] or 0;  r = b - A y;  z = M^-1 r;  p = z;  gamma = <r, z>
    step:  q = A p;  a = gamma / <p, q>;  y += a p;  r -= a q;  [stop test];  z = M^-1 r;  gamma' = <r, z>;  p = z + (gamma'/gamma) p
G = H^T H + lambda I and its inverse are fp64.  A row without counting entries or with b = 0 is 0 after 0 steps.  tol > 0: the
row stops once |r| <= tol |b|, tested before the first step too, the step that reaches it counted; tol = 0: `steps` steps
unless gamma becomes exactly 0."""
import functools

import numpy as np

import alsb_ref
import ials_ref
from solve_sweep import segments

ALS, CCD, IMPLICIT = 0, 2, 3  # include/mfx.h: MFX_FOLD_ALS, MFX_FOLD_CCD, MFX_FOLD_IMPLICIT
SIZES = [0, 1, 3, 0, 17, 250, 2048, 2049, 2100, 5000, 1]  # tests/test_gpu_ials.py
COLS, LAM = 6000, 0.1
KS = [37, 64, 130, 160, 256, 1024]
ALPHAS = [0.0, 1.0, 40.0]


def base(H, lam):
    """(G, G^-1) in fp64."""
    H = np.asarray(H, np.float64)
    G = H.T @ H + float(np.float32(lam)) * np.eye(H.shape[1])
    return G, np.linalg.inv(G)


def row_system(model, ptr, idx, val, u, H, lam, alpha):
    """(Hj, c, b, rho): A p = [G or rho] p + Hj^T (c * (Hj p)) over the counting entries; None for a row without any."""
    lo, hi = int(ptr[u]), int(ptr[u + 1])
    j = np.asarray(idx[lo:hi], np.int64)
    v = np.asarray(val[lo:hi], np.float32)
    if model == IMPLICIT:
        w32 = np.float32(alpha) * v
        pos = v > 0
        if not pos.any():
            return None
        Hj = np.asarray(H, np.float64)[j[pos]]
        return Hj, w32[pos].astype(np.float64), Hj.T @ (np.float32(1) + w32[pos]).astype(np.float64), 0.0
    if hi == lo:
        return None
    Hj = np.asarray(H, np.float64)[j]
    return Hj, np.ones(hi - lo), Hj.T @ v.astype(np.float64), alsb_ref.rho_of(lam, hi - lo, model == CCD)


def rows(model, ptr, idx, val, H, lam, alpha, W_init, steps, tol, precondition=True, base_pair=None):
    """(Y [U][k] fp64, steps_done [U]).  precondition=False: the implicit model with M = I (what the preconditioner buys)."""
    U, k = len(ptr) - 1, H.shape[1]
    Y, done = np.zeros((U, k)), np.zeros(U, np.int64)
    G = Ginv = None
    if model == IMPLICIT:
        G, Ginv = base_pair if base_pair is not None else base(H, lam)
    for u in range(U):
        sysu = row_system(model, ptr, idx, val, u, H, lam, alpha)
        if sysu is None:
            continue
        Hj, c, b, rho = sysu
        bn = np.linalg.norm(b)
        if bn == 0:
            continue
        mul = (lambda p: G @ p + Hj.T @ (c * (Hj @ p))) if model == IMPLICIT else (lambda p: rho * p + Hj.T @ (Hj @ p))
        pre = (lambda r: Ginv @ r) if model == IMPLICIT and precondition else (lambda r: r.copy())
        y = np.zeros(k) if W_init is None else np.array(W_init[u], np.float64)
        r = b - mul(y) if W_init is not None else b.copy()
        if tol > 0 and np.linalg.norm(r) <= tol * bn:
            Y[u] = y
            continue
        z = pre(r)
        p, gamma = z.copy(), r @ z
        for _ in range(steps):
            if gamma == 0:
                break
            q = mul(p)
            a = gamma / (p @ q)
            y += a * p
            r -= a * q
            done[u] += 1
            if tol > 0 and np.linalg.norm(r) <= tol * bn:
                break
            z = pre(r)
            g2 = r @ z
            p = z + (g2 / gamma) * p
            gamma = g2
        Y[u] = y
    return Y, done


# ------------------------------------------------------------------------------------------------ the tests' inputs
@functools.lru_cache(maxsize=None)
def inputs(k, cols=COLS, sizes=tuple(SIZES)):
    """(ptr, idx, val, H, W0) of tests/test_gpu_ialsb.py at rank k: the same seeds and draws."""
    ptr, idx, val = segments(100 + k, cols, list(sizes))
    H = (np.random.default_rng(k).standard_normal((cols, k)) / np.sqrt(k)).astype(np.float32)
    W0 = (0.1 * np.random.default_rng(1000 + k).standard_normal((len(sizes), k))).astype(np.float32)
    return ptr, idx, val, H, W0


def explicit_values(val):
    """Values for the explicit models: -2 .. 3, zeros and negatives included."""
    return (np.asarray(val, np.float32) - np.float32(2)).astype(np.float32)


def dense(model, ptr, idx, val, u, H, lam, alpha):
    """(A, b) of row u from the dense systems of tests/ials_ref.py (implicit) / tests/alsb_ref.py (explicit)."""
    if model == IMPLICIT:
        return ials_ref.dense_system(ptr, idx, val, u, H, lam, alpha)
    return alsb_ref.dense_system(ptr, idx, val, u, H, lam, model == CCD)


def counting(model, k, alpha, cols=COLS, sizes=tuple(SIZES)):
    """The rows with a right-hand side: every other row is 0 after 0 steps."""
    return [u for u, s in dense_solutions(model, k, alpha, cols, sizes).items() if s[1].any()]


def spectrum(A):
    """(2-norm, 2-norm condition number) of a symmetric positive definite matrix, from its eigenvalues."""
    ev = np.linalg.eigvalsh(A)
    return float(ev[-1]), float(ev[-1] / ev[0]) if ev[0] > 0 else float("inf")


@functools.lru_cache(maxsize=None)
def dense_solutions(model, k, alpha, cols=COLS, sizes=tuple(SIZES)):
    """{u: (A, b, y*, cond A, |A|)} of the non-empty rows of inputs(k, cols, sizes); the explicit models on explicit_values."""
    ptr, idx, val, H, _ = inputs(k, cols, sizes)
    if model != IMPLICIT:
        val = explicit_values(val)
    out = {}
    for u, n in enumerate(sizes):
        if n:
            A, b = dense(model, ptr, idx, val, u, H, LAM, alpha)
            norm, cn = spectrum(A)
            out[u] = (A, b, np.linalg.solve(A, b), cn, norm)
    return out


def errors(model, k, alpha, Y, cols=COLS, sizes=tuple(SIZES)):
    """(worst relative error, worst normwise backward error, worst condition number) of the rows Y against dense_solutions; a row
    with b = 0 (no counting entry: an implicit row of explicit zeros) must be exactly zero."""
    rel = be = cn = 0.0
    for u, (A, b, y, c, norm) in dense_solutions(model, k, alpha, cols, sizes).items():
        cn = max(cn, c)
        if not b.any():
            assert not np.any(Y[u]), u
            continue
        rel = max(rel, float(np.linalg.norm(Y[u] - y) / np.linalg.norm(y)))
        yu = np.asarray(Y[u], np.float64)  # ials_ref.backward_error with |A| taken from the eigenvalues (one decomposition per system)
        be = max(be, float(np.linalg.norm(A @ yu - b) / (norm * np.linalg.norm(yu) + np.linalg.norm(b))))
    return rel, be, cn
