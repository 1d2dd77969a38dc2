"""numpy fp64 reference of the target solves of mfx_rec_explain_cg (include/mfx.h), the targets that
tests/test_explain_cg_host.py pins it on and tests/test_gpu_explain_cg.py runs the library on, and the checks both share.

Rows, H, lambda and the models are those of tests/foldin_cg_ref.py.  For row q and target t the system is A_q z = h_t with the
A_q and the preconditioner of the fold-in of row q; solve() is the loop of foldin_cg_ref.rows with b = h_t from z = 0.
Targets per row, T = 5: the row's first item (a random item for an empty row), three items drawn with default_rng(7), one
padding.  zero_target(): a copy of H with one further row zeroed and that row as a target, for the rule h_t = 0."""
import functools

import numpy as np

import foldin_cg_ref as ref

PAD = 0xFFFFFFFF
T = 5
ZERO_ITEM, ZERO_AT = 4321, (5, 2)  # the item whose row of H zero_target() zeroes, and the (row, position) that asks for it


@functools.lru_cache(maxsize=None)
def targets(k, cols=ref.COLS, sizes=tuple(ref.SIZES)):
    """uint32 [U][T]: first item of the row (or a random one), three random items, the padding."""
    ptr, idx, _, _, _ = ref.inputs(k, cols, sizes)
    rng = np.random.default_rng(7)
    tg = np.full((len(sizes), T), PAD, np.uint32)
    for u in range(len(sizes)):
        tg[u, 0] = idx[ptr[u]] if ptr[u + 1] > ptr[u] else rng.integers(cols)
        tg[u, 1:4] = rng.integers(0, cols, 3)
    return tg


def zero_target(k):
    """(H with row ZERO_ITEM zeroed, targets(k) with ZERO_ITEM at ZERO_AT)."""
    Hz = ref.inputs(k)[3].copy()
    Hz[ZERO_ITEM] = 0
    tz = targets(k).copy()
    tz[ZERO_AT] = ZERO_ITEM
    return Hz, tz


def solve(model, ptr, idx, val, H, lam, alpha, tg, steps, tol, base_pair=None):
    """(Z [U][T][k] fp64, steps_done [U][T]): foldin_cg_ref.rows with b = H[target], from zero.  A padding target, a row
    without counting entries and a zero target row: 0 after 0 steps."""
    U, k = len(ptr) - 1, H.shape[1]
    H64 = np.asarray(H, np.float64)
    Z, done = np.zeros(tg.shape + (k,)), np.zeros(tg.shape, np.int64)
    G = Ginv = None
    if model == ref.IMPLICIT:
        G, Ginv = base_pair if base_pair is not None else ref.base(H, lam)
    for u in range(U):
        sysu = ref.row_system(model, ptr, idx, val, u, H, lam, alpha)
        if sysu is None:
            continue
        Hj, c, _, rho = sysu
        mul = (lambda p: G @ p + Hj.T @ (c * (Hj @ p))) if model == ref.IMPLICIT else (lambda p: rho * p + Hj.T @ (Hj @ p))
        pre = (lambda r: Ginv @ r) if model == ref.IMPLICIT else (lambda r: r.copy())
        for t in range(tg.shape[1]):
            if tg[u, t] == PAD:
                continue
            b = H64[tg[u, t]]
            bn = np.linalg.norm(b)
            if bn == 0:
                continue
            y, r = np.zeros(k), b.copy()
            if tol > 0 and np.linalg.norm(r) <= tol * bn:
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
                done[u, t] += 1
                if tol > 0 and np.linalg.norm(r) <= tol * bn:
                    break
                z = pre(r)
                g2 = r @ z
                p = z + (g2 / gamma) * p
                gamma = g2
            Z[u, t] = y
    return Z, done


def live_pairs(model, k, alpha, tg, cols=ref.COLS, sizes=tuple(ref.SIZES)):
    """bool [U][T]: the pairs with a system to solve: a row with counting entries (implicit: some r > 0; explicit: any entry,
    even where the row's own right-hand side is zero) and a target that is no padding.  alpha plays no part."""
    ptr, _, val, _, _ = ref.inputs(k, cols, sizes)
    rows = [bool((val[ptr[u]:ptr[u + 1]] > 0).any()) if model == ref.IMPLICIT else n > 0 for u, n in enumerate(sizes)]
    return np.asarray(rows)[:, None] & (tg != PAD)


def errors(model, k, alpha, tg, Z, W, H, cols=ref.COLS, sizes=tuple(ref.SIZES)):
    """Worst over the live pairs, against the dense systems of foldin_cg_ref.dense_solutions, of: the relative error of Z[q][t]
    to the dense solve of A_q z = h_t; its normwise backward error |A z - h_t| / (|A| |z| + |h_t|); the split gap
    |<b, z> - <h_t, w>| over (|A| |w| + |b|) |z| + (|A| |z| + |h_t|) |w|, W [U][k] the rows (the gap is <r_w, z> - <r_z, w>, and
    each residual is at most its backward error times its bracket); the condition number.  Z, W: fp32 or fp64 arrays."""
    H64 = np.asarray(H, np.float64)
    live = live_pairs(model, k, alpha, tg, cols, sizes)
    rel, be, gap, cn = [0.0], [0.0], [0.0], [0.0]
    for u, (A, b, _, c, norm) in ref.dense_solutions(model, k, alpha, cols, sizes).items():
        ts = np.nonzero(live[u])[0]
        if not ts.size:
            continue
        cn.append(c)
        ht = H64[tg[u, ts]]
        want = np.linalg.solve(A, ht.T).T
        w = np.asarray(W[u], np.float64)
        for j, t in enumerate(ts):
            z = np.asarray(Z[u, t], np.float64)
            nz, nw, nh, nb = np.linalg.norm(z), np.linalg.norm(w), np.linalg.norm(ht[j]), np.linalg.norm(b)
            rel.append(float(np.linalg.norm(z - want[j]) / np.linalg.norm(want[j])))
            be.append(float(np.linalg.norm(A @ z - ht[j]) / (norm * nz + nh)))
            bracket = (norm * nw + nb) * nz + (norm * nz + nh) * nw
            if bracket == 0:  # an explicit row whose values are all zero: b = 0 and w = 0, nothing to split
                assert b @ z == 0 and ht[j] @ w == 0
            else:
                gap.append(float(abs(b @ z - ht[j] @ w) / bracket))
    return float(np.max(rel)), float(np.max(be)), float(np.max(gap)), float(np.max(cn))  # (np.max: a NaN is not lost)
