"""Exact CPU reference of hybrid BPR training (mfx_hyb_*): the embedding of a row through its features, one step and the
training loop in single fp32 operations.

Everything here restates the contract of include/mfx.h ("Hybrid BPR") in other words, so that the library can be checked
bit for bit.  The sampler, the score chain, the sigmoid and the fixed point are those of tests/bpr_exact.py; new are the
embedding chain (rec_exact.fmaf32, started from the first product), the rounding of a row's sums to G, the second level of
integer sums from the rows to their features and the update of a feature."""
import numpy as np

import bpr_exact as bx
from rec_exact import fmaf32

_F = np.float32
MAX_ENTRIES = 1024


def features(n, nf, rows, ids, vals):
    """The feature matrix (mfx.HybFeatures) of n rows over nf features from triplets; ids ascending inside a row."""
    from mfx import HybFeatures
    rows, ids = np.asarray(rows, np.int64), np.asarray(ids, np.int64)
    order = np.lexsort((ids, rows))
    rows, ids, vals = rows[order], ids[order], np.asarray(vals, _F)[order]
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    return HybFeatures(int(n), int(nf), ptr.astype(np.uint32), ids.astype(np.uint32), np.ascontiguousarray(vals))


def identity(n):
    """Feature r on row r with the value 1: what a NULL feature matrix stands for."""
    return features(n, n, np.arange(n), np.arange(n), np.ones(n, _F))


def embed(F, E):
    """The rows of F over the table E: per coordinate acc = fp32(v_0 * E[f_0][c]), then acc = fmaf(v_e, E[f_e][c], acc) in
    stored order; an empty row gives +0.  Walks the entry position p of all rows at once (the rows sorted by length, so the
    rows that still have a p-th entry are a prefix)."""
    E = np.asarray(E, _F)
    ptr = F.ptr.astype(np.int64)
    idx = F.idx.astype(np.int64)
    deg = np.diff(ptr)
    assert E.shape[0] == F.nf and (deg.max() if F.n else 0) <= MAX_ENTRIES
    order = np.argsort(-deg, kind="stable")
    sorted_deg = deg[order]
    out = np.zeros((F.n, E.shape[1]), _F)
    for p in range(int(deg.max()) if F.n else 0):
        rows = order[:int(np.searchsorted(-sorted_deg, -p, side="left"))]  # the rows with deg > p
        e = ptr[rows] + p
        v, x = F.val[e][:, None], E[idx[e]]
        with np.errstate(all="ignore"):
            out[rows] = v * x if p == 0 else fmaf32(v, x, out[rows])
    assert out.dtype == _F
    return out


def _spread(F, G, m, k):
    """(acc int64 [nf][k], m_f int64 [nf]): the terms fp32(v * G[r][c]) of the rows with m_r > 0 as integers, and the counts."""
    ptr = F.ptr.astype(np.int64)
    entry_row = np.repeat(np.arange(F.n, dtype=np.int64), np.diff(ptr))
    live = m[entry_row] > 0
    rows, f, v = entry_row[live], F.idx.astype(np.int64)[live], F.val[live]
    with np.errstate(all="ignore"):
        terms = v[:, None] * G[rows]
    assert terms.dtype == _F
    assert np.all(np.abs(terms) < 2.0 ** 27)  # (|G| < 64 m_r <= 2^27: the product with 2^36 stays below 2^63)
    acc = np.zeros((F.nf, k), np.int64)
    np.add.at(acc, f, bx.to_fixed(terms))
    mf = np.zeros(F.nf, np.int64)
    np.add.at(mf, f, m[rows])
    return acc, mf


def step(Fu, Fi, Eu, Ei, u, i, j, skipped, lr, lam, counts=False):
    """One step at the frozen tables Eu, Ei.  Returns (Eu', Ei', [slots, skipped, bad, correct]) and, with counts=True, also
    (m_f of the user features, m_f of the item features)."""
    Eu = np.asarray(Eu, _F)
    Ei = np.asarray(Ei, _F)
    u, i, j = (np.asarray(a, np.int64) for a in (u, i, j))
    n, k = len(u), Eu.shape[1]
    skipped = np.zeros(n, bool) if skipped is None else np.asarray(skipped, bool)
    lr, lam = _F(lr), _F(lam)
    W, H = embed(Fu, Eu), embed(Fi, Ei)
    # the step of bpr_exact.step on (W, H) up to its sums
    live = np.nonzero(~skipped)[0]
    ul, il, jl = u[live], i[live], j[live]
    x, d = bx.slot_scores(W, H, ul, il, jl)
    with np.errstate(all="ignore"):
        g = bx.sigmoid_neg(x)[:, None]
        tw = g * d
        th = g * W[ul]
        bad = ~np.isfinite(x) | np.any(np.abs(tw) >= bx.TERM_LIMIT, axis=1) | np.any(np.abs(th) >= bx.TERM_LIMIT, axis=1)
    ok = ~bad
    stats = [n, int(skipped.sum()), int(bad.sum()), int((x[ok] > 0).sum())]
    ul, il, jl = ul[ok], il[ok], jl[ok]
    fw, fh = bx.to_fixed(tw[ok]), bx.to_fixed(th[ok])
    accW = np.zeros(W.shape, np.int64)
    accH = np.zeros(H.shape, np.int64)
    np.add.at(accW, ul, fw)
    np.add.at(accH, il, fh)
    np.add.at(accH, jl, -fh)
    mW = np.bincount(ul, minlength=W.shape[0])
    mH = np.bincount(il, minlength=H.shape[0]) + np.bincount(jl, minlength=H.shape[0])
    out, mfs = [], []
    for F, E, accX, m in ((Fu, Eu, accW, mW), (Fi, Ei, accH, mH)):
        G = accX.astype(_F) * _F(2.0 ** -36)  # one rounding int64 -> fp32, then the exact scale (read where m_r > 0 only)
        acc, mf = _spread(F, G, m, k)
        with np.errstate(all="ignore"):
            a = acc.astype(_F) * _F(2.0 ** -36)
            reg = (lam * mf.astype(_F))[:, None] * E
            new = E + lr * (a - reg)
        assert new.dtype == _F
        out.append(np.where((mf > 0)[:, None], new, E))
        mfs.append(mf)
    if counts:
        return out[0], out[1], stats, mfs[0], mfs[1]
    return out[0], out[1], stats


def initial_tables(nfu, nfi, k, seed):
    """0.1 * N(0, 1) tables, Eu then Ei from one generator: what mfx.HybridSolver(init_seed=seed) draws."""
    return bx.initial_factors(nfu, nfi, k, seed)


def train(R, Fu, Fi, Eu, Ei, lr, lam, batch, seed, n_epochs, pos=0, sampler=bx.triples_np):
    """n_epochs epochs from slot `pos` (a started epoch is finished as the first).  Returns (Eu, Ei, per-epoch stats, pos)."""
    nnz = int(R.csr_row_ptr[-1])
    stats = []
    for _ in range(n_epochs):
        tot = np.zeros(4, np.int64)
        for first, cnt in bx.epoch_steps(nnz, batch, pos):
            u, i, j, s = sampler(R, seed, first, cnt)
            Eu, Ei, st = step(Fu, Fi, Eu, Ei, u, i, j, s, lr, lam)
            tot += st
            pos = first + cnt
        stats.append(tot)
    return Eu, Ei, np.array(stats), pos


def cold_start_split(held=3):
    """bx.planted_clusters() with `held` items of every cluster taken out of training altogether.  Returns (R over the same
    600 columns, the cold items ascending, the cluster of every item)."""
    from mfx import dataset as ds
    P = bx.planted_clusters()
    nc, per = 20, 30
    cluster = np.arange(P.cols) // per
    cold = np.concatenate([c * per + np.arange(held) for c in range(nc)])
    rows = np.repeat(np.arange(P.rows), np.diff(P.csr_row_ptr.astype(np.int64)))
    cols = P.csr_col_idx.astype(np.int64)
    keep = ~np.isin(cols, cold)
    R = ds.from_coo(P.rows, P.cols, rows[keep], cols[keep], np.ones(int(keep.sum()), _F))
    return R, cold, cluster


def cold_auc(W, Hcold, cold_cluster, user_cluster):
    """The mean over the users of the AUC of the user's own cluster's cold items among all cold items, by float64 scores
    (ties count a half)."""
    S = W.astype(np.float64) @ Hcold.astype(np.float64).T
    own = cold_cluster[None, :] == user_cluster[:, None]
    total = 0.0
    for r in range(S.shape[0]):
        p, q = S[r, own[r]], S[r, ~own[r]]
        total += ((p[:, None] > q[None, :]).sum() + 0.5 * (p[:, None] == q[None, :]).sum()) / (p.size * q.size)
    return total / S.shape[0]
