"""Exact host reference of mfx_rec_explain (include/mfx.h): the weights per setup, the fp64 systems, the contributions
from given Z bits and their order.

The fold-in row is w = A^-1 sum_e b_e h_e, so the score of a target i splits over the row's entries:
<h_i, w> = sum_e b_e <h_e, z>, z = A^-1 h_i.  Given the fp32 bits of z (Z_out) a contribution is fully determined:
d = the fp32 fma chain over c ascending from +0 of z[c] * H[j_e][c] (rec_exact.fmaf32), c_e = fp32(b_e * d).

Systems are formed in fp64 over the row's entries with REPEATS counted (two entries with the same item id are two
entries), from the pieces of tests/ials_ref.py and tests/ials_reg_ref.py: their weights and rho; for rows without
repeated ids the systems equal ials_ref.dense_system / ials_reg_ref.dense_system (tests/test_explain_host.py)."""
import numpy as np

import ials_ref
import ials_reg_ref
from rec_exact import fmaf32

PAD = 0xFFFFFFFF
F32 = np.float32
SETUPS = ("als", "ccd", "implicit", "reg")


def weights(setup, val, alpha=0.0, alpha0=1.0):
    """(b fp32 [n], counts bool [n]) of the entries of a row: the rhs weight of each entry and whether it is an entry."""
    v = np.asarray(val, F32)
    if setup in ("als", "ccd"):
        return v.copy(), np.ones(v.shape, bool)
    w = F32(alpha) * v                                   # fp32(alpha r)
    a0 = F32(1.0) if setup == "implicit" else F32(alpha0)
    return (a0 + w).astype(F32), v > 0                   # add_rn(a0, w)


def system(setup, ptr, idx, val, s, H, lam, alpha=0.0, alpha0=1.0, nu=0.0):
    """A [k][k] fp64 of row s: what the fold-in of `setup` factors.  lam, alpha, alpha0, nu: the fp32 values of the C ABI."""
    H64 = np.asarray(H, np.float64)
    k = H64.shape[1]
    lo, hi = int(ptr[s]), int(ptr[s + 1])
    j = np.asarray(idx[lo:hi], np.int64)
    v = np.asarray(val[lo:hi], F32)
    Hj = H64[j]
    lam64 = float(F32(lam))
    if setup == "als":
        return Hj.T @ Hj + lam64 * np.eye(k)
    if setup == "ccd":
        return Hj.T @ Hj + float(F32(lam) * F32(hi - lo)) * np.eye(k)
    w = ials_ref.weights(v, alpha)
    S = (Hj * w[:, None]).T @ Hj
    if setup == "implicit":
        return H64.T @ H64 + lam64 * np.eye(k) + S
    rho = ials_reg_ref.rho(ptr, val, H64.shape[0], lam, alpha0, nu)[s]
    return float(F32(alpha0)) * (H64.T @ H64) + rho * np.eye(k) + S


def rhs(setup, idx_row, val_row, H, alpha=0.0, alpha0=1.0):
    """b [k] fp64 = sum over the counting entries of b_e h_e."""
    b, counts = weights(setup, val_row, alpha, alpha0)
    Hj = np.asarray(H, np.float64)[np.asarray(idx_row, np.int64)]
    return Hj.T @ np.where(counts, b.astype(np.float64), 0.0)


def chain(z, Hrows):
    """fp32 [n]: the fma chain over c ascending from +0 of z[c] * Hrows[e][c]."""
    z = np.asarray(z, F32)
    Hrows = np.asarray(Hrows, F32)
    acc = np.zeros(Hrows.shape[0], F32)
    for c in range(z.shape[0]):
        acc = fmaf32(z[c], Hrows[:, c], acc)
    return acc


def contributions(z, H, idx_row, b):
    """fp32 [n]: c_e = fp32(b_e * d_e) of every entry of the row, counting or not, from the bits of z."""
    d = chain(z, np.asarray(H, F32)[np.asarray(idx_row, np.int64)])
    with np.errstate(all="ignore"):
        return (np.asarray(b, F32) * d).astype(F32)


def ranked(idx_row, c, counts, n_expl):
    """(items uint32 [n_expl], contrib fp32 [n_expl], positions int64 [<= n_expl]): the counting entries by c descending,
    then position ascending (-0 == +0), NaN dropped, padded with (PAD, -inf)."""
    c = np.asarray(c, F32)
    ok = np.asarray(counts, bool) & ~np.isnan(c)
    pos = np.nonzero(ok)[0]
    key = c[pos].astype(np.float64) + 0.0                # -0 -> +0: the two zeros tie
    o = pos[np.lexsort((pos, -key))][:n_expl]
    items = np.full(n_expl, PAD, np.uint32)
    contrib = np.full(n_expl, -np.inf, F32)
    items[:len(o)] = np.asarray(idx_row, np.uint32)[o]
    contrib[:len(o)] = c[o]
    return items, contrib, o


def expected(setup, ptr, idx, val, targets, Z, H, n_expl, alpha=0.0, alpha0=1.0):
    """(items [U][T][n_expl], contrib [U][T][n_expl]) that mfx_rec_explain returns given its own Z_out [U][T][k]."""
    U, T = targets.shape
    items = np.full((U, T, n_expl), PAD, np.uint32)
    contrib = np.full((U, T, n_expl), -np.inf, F32)
    for q in range(U):
        lo, hi = int(ptr[q]), int(ptr[q + 1])
        b, counts = weights(setup, val[lo:hi], alpha, alpha0)
        for t in range(T):
            if targets[q, t] == PAD:
                continue
            c = contributions(Z[q, t], H, idx[lo:hi], b)
            items[q, t], contrib[q, t], _ = ranked(idx[lo:hi], c, counts, n_expl)
    return items, contrib
