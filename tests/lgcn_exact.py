"""Exact CPU reference of LightGCN training (mfx_lgcn_*): the propagation half-pass, the layer mean and one step in single
fp32 operations.

Everything here restates the contract of include/mfx.h ("LightGCN") in other words, so that the library can be checked bit
for bit.  The sampler, the score chain, the sigmoid and the fixed point are those of tests/bpr_exact.py; new are the scale
tables, the 1024-entry segments of a row's FMA chain (rec_exact.fmaf32), the left-to-right sums and the base update."""
import numpy as np

import bpr_exact as bx
from rec_exact import fmaf32

_F = np.float32
SEGMENT = 1024
MAX_LAYERS = 8


def scales(ptr):
    """s = fp32(1 / sqrt((double) degree)) of the rows behind `ptr`, 0 for an empty row."""
    d = np.diff(np.asarray(ptr, np.int64)).astype(np.float64)
    with np.errstate(divide="ignore"):
        return np.where(d > 0, 1.0 / np.sqrt(d), 0.0).astype(_F)


def half_pass(ptr, idx, s_src, s_dst, X):
    """The rows of one side from the rows X of the other: per coordinate the FMA chain fmaf(s[src], X[src][c], acc) over a
    segment of 1024 entries in stored order from +0, the segment sums added left to right, the result times s_dst.  Walks the
    entry position p of all rows at once (the rows sorted by length, so the rows that still have a p-th entry are a prefix)."""
    ptr = np.asarray(ptr, np.int64)
    idx = np.asarray(idx, np.int64)
    X = np.asarray(X, _F)
    n, k = len(ptr) - 1, X.shape[1]
    deg = np.diff(ptr)
    order = np.argsort(-deg, kind="stable")
    sorted_deg = deg[order]
    longest = int(deg.max()) if n else 0
    total = np.zeros((n, k), _F)
    for seg in range(max(1, -(-longest // SEGMENT))):
        lo = seg * SEGMENT
        acc = np.zeros((n, k), _F)
        for p in range(lo, min(lo + SEGMENT, longest)):
            rows = order[:int(np.searchsorted(-sorted_deg, -p, side="left"))]  # the rows with deg > p
            src = idx[ptr[rows] + p]
            acc[rows] = fmaf32(s_src[src][:, None], X[src], acc[rows])
        if seg == 0:
            total = acc
        else:
            rows = order[:int(np.searchsorted(-sorted_deg, -lo, side="left"))]
            with np.errstate(all="ignore"):
                total[rows] = total[rows] + acc[rows]
    with np.errstate(all="ignore"):
        out = s_dst[:, None] * total
    assert out.dtype == _F
    return out


def layers_of(R, W0, H0, layers):
    """[(W^0, H^0), ..., (W^L, H^L)]: user rows of layer l + 1 from the item rows of layer l and the other way round."""
    su, si = scales(R.csr_row_ptr), scales(R.csc_col_ptr)
    out = [(np.asarray(W0, _F), np.asarray(H0, _F))]
    for _ in range(layers):
        W, H = out[-1]
        out.append((half_pass(R.csr_row_ptr, R.csr_col_idx, si, su, H), half_pass(R.csc_col_ptr, R.csc_row_idx, su, si, W)))
    return out


def propagate(R, W0, H0, layers):
    """The final embeddings of the base W0, H0."""
    assert 0 <= layers <= MAX_LAYERS
    return mean_of(layers_of(R, W0, H0, layers), layers)


def mean_of(E, layers):
    """fp32(c_L * (((E^0 + E^1) + ...) + E^L)) of the first L + 1 layers of E, c_L = fp32(1 / fp32(L + 1)); L = 0: the base itself."""
    if layers == 0:
        return E[0][0].copy(), E[0][1].copy()
    c = _F(1.0) / _F(layers + 1)
    out = []
    with np.errstate(all="ignore"):
        for side in (0, 1):
            acc = E[0][side]
            for l in range(1, layers + 1):
                acc = acc + E[l][side]
            out.append(acc * c)
    assert out[0].dtype == _F
    return out[0], out[1]


def step(R, W0, H0, u, i, j, skipped, layers, lr, lam):
    """One step at the frozen base W0, H0.  Returns (W0', H0', [slots, skipped, bad, correct])."""
    W0 = np.asarray(W0, _F)
    H0 = np.asarray(H0, _F)
    u, i, j = (np.asarray(a, np.int64) for a in (u, i, j))
    n = len(u)
    skipped = np.zeros(n, bool) if skipped is None else np.asarray(skipped, bool)
    lr, lam = _F(lr), _F(lam)
    W, H = propagate(R, W0, H0, layers)
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
    GW = np.where((mW > 0)[:, None], accW.astype(_F) * _F(2.0 ** -36), _F(0))
    GH = np.where((mH > 0)[:, None], accH.astype(_F) * _F(2.0 ** -36), _F(0))
    DW, DH = propagate(R, GW, GH, layers)
    out = []
    for X, D, m, ptr in ((W0, DW, mW, R.csr_row_ptr), (H0, DH, mH, R.csc_col_ptr)):
        deg = np.diff(np.asarray(ptr, np.int64))
        with np.errstate(all="ignore"):
            reg = (lam * m.astype(_F))[:, None] * X
            new = X + lr * (D - reg)
        assert new.dtype == _F
        upd = (m > 0) | ((deg > 0) if layers >= 1 else np.zeros(len(m), bool))
        out.append(np.where(upd[:, None], new, X))
    return out[0], out[1], stats


def train(R, W0, H0, layers, lr, lam, batch, seed, n_epochs, pos=0, sampler=bx.triples_np):
    """n_epochs epochs from slot `pos` (a started epoch is finished as the first).  Returns (W0, H0, per-epoch stats, pos)."""
    nnz = int(R.csr_row_ptr[-1])
    stats = []
    for _ in range(n_epochs):
        tot = np.zeros(4, np.int64)
        for first, cnt in bx.epoch_steps(nnz, batch, pos):
            u, i, j, s = sampler(R, seed, first, cnt)
            W0, H0, st = step(R, W0, H0, u, i, j, s, layers, lr, lam)
            tot += st
            pos = first + cnt
        stats.append(tot)
    return W0, H0, np.array(stats), pos


def segment_matrix(seed=5, n=3100, lengths=(1023, 1024, 1025, 2048, 2049, 3000), background=1500):
    """n x n with rows 0 .. 5 AND columns 0 .. 5 of exactly `lengths` entries over a sparse background elsewhere: the rows and
    columns on either side of the 1024-entry segment boundaries.  About 20 000 entries in all."""
    from mfx import dataset as ds
    rng = np.random.default_rng(seed)
    h = len(lengths)
    cells = set()
    for q, m in enumerate(lengths):
        # (the heavy rows and columns draw from the ids >= h only, so they do not change each other's lengths)
        for c in h + rng.choice(n - h, m, replace=False):
            cells.add((q, int(c)))
        for r in h + rng.choice(n - h, m, replace=False):
            cells.add((int(r), q))
    r = h + rng.integers(0, n - h, background)
    c = h + rng.integers(0, n - h, background)
    cells.update(zip(r.tolist(), c.tolist()))
    rc = np.array(sorted(cells), np.int64)
    R = ds.from_coo(n, n, rc[:, 0], rc[:, 1], np.ones(len(rc), _F))
    assert np.diff(R.csr_row_ptr.astype(np.int64))[:h].tolist() == list(lengths)
    assert np.diff(R.csc_col_ptr.astype(np.int64))[:h].tolist() == list(lengths)
    return R
