"""Exact CPU reference of SLIM on given supports (mfx_slim_*): the contract of include/mfx.h ("SLIM") restated in numpy.

The Gram entries are the item-kNN similarities of knn_exact (fp32 terms cut to the 2^-36 grid, int64 sums, the fp32 nearest to
the sum) plus the same sum over the squares on the diagonal; the solve is the covariance-update coordinate descent in fp32,
one rounding per operation in the order the contract gives (fused multiply-adds by rec_exact.fmaf32); the recommendation
adds fp32 terms as int64 over the transposed weights and ranks with knn_exact.top_lists.  gram_blocks_sparse gives the blocks
of gram_blocks from the pairs the support names alone (pair_sums), for catalogues whose dense cols x cols sums do not fit.
Nothing here calls the library."""
import numpy as np

import knn_exact as kx
from rec_exact import fmaf32

_F = np.float32
PAD = kx.PAD
MAX_K = 128


class BadSupport(ValueError):
    """A support that the library refuses: .item is the smallest item with a bad list."""

    def __init__(self, item):
        super().__init__(f"item {item}")
        self.item = item


def real_slots(S):
    """n_j of every list (pads at the tail)."""
    return (np.asarray(S, np.uint32) != PAD).sum(axis=1).astype(np.int64)


def check_support(S, cols, w=None):
    """Raises BadSupport with the smallest item whose list has an id >= cols, its own item, a duplicate, a pad before a real
    slot or (given weights) a weight of a real slot that is not finite."""
    S = np.asarray(S, np.uint32)
    K = S.shape[1]
    real = S != PAD
    ids = np.where(real, S.astype(np.int64), -1 - np.arange(K, dtype=np.int64)[None, :])  # (pads: distinct, equal to no id)
    bad = (real != (np.arange(K)[None, :] < real.sum(axis=1)[:, None])).any(axis=1)        # a pad before a real slot
    bad |= (ids >= cols).any(axis=1) | (ids == np.arange(S.shape[0])[:, None]).any(axis=1)
    bad |= (np.diff(np.sort(ids, axis=1), axis=1) == 0).any(axis=1)
    if w is not None:
        bad |= (real & ~np.isfinite(np.asarray(w, _F))).any(axis=1)
    if bad.any():
        raise BadSupport(int(np.argmax(bad)))


def diagonal(X):
    """(int64 [cols] sums of the terms fp32(x * x) of every column, the smallest item with a bad term or None)."""
    cptr = X.csc_col_ptr.astype(np.int64)
    x = X.csc_val.astype(_F)
    with np.errstate(all="ignore"):
        t = x * x
        bad = ~(t < kx.TERM_LIMIT)
    col = np.repeat(np.arange(X.cols), np.diff(cptr))
    d = np.zeros(X.cols, np.int64)
    with np.errstate(all="ignore"):
        np.add.at(d, col[~bad], kx.to_fixed(t[~bad]))
    return d, (int(col[bad].min()) if bad.any() else None)


def gram_sums(X):
    """The integer sums of the whole X^T X, int64 [cols][cols], the diagonal included (small catalogues only).  Raises
    kx.BadTerm with the smallest item that has a bad term (of a pair or of its diagonal) or an over-long column."""
    d, bad_d = diagonal(X)
    try:
        G = kx.similarity_rows(X, np.arange(X.cols))
        bad_s = None
    except kx.BadTerm as e:
        G, bad_s = None, e.item
    bad = [b for b in (bad_d, bad_s) if b is not None]
    if bad:
        raise kx.BadTerm(min(bad))
    G[np.arange(X.cols), np.arange(X.cols)] = d
    return G


def gram_blocks(X, S, sums=None):
    """fp32 [cols][K + 1][K]: rows 0 .. K - 1 the Gram matrix over S_j x S_j (d on the diagonal), row K the Gram entries of j
    against S_j; pads 0.  sums: gram_sums(X) if already at hand."""
    S = np.asarray(S, np.uint32)
    cols, K = S.shape
    assert cols == X.cols and 1 <= K <= MAX_K
    check_support(S, cols)
    G = gram_sums(X) if sums is None else sums
    B = np.zeros((cols, K + 1, K), _F)
    n = real_slots(S)
    for j in range(cols):
        ids = S[j, :n[j]].astype(np.int64)
        B[j, :n[j], :n[j]] = kx.from_fixed(G[np.ix_(ids, ids)])
        B[j, K, :n[j]] = kx.from_fixed(G[j, ids])
    return B


def pair_sums(X, a, b, chunk=1 << 22):
    """int64 [len(a)]: for every pair (a[n], b[n]) the sum of to_fixed(fp32(x_ua * x_ub)) over the users u that hold both
    items -- the entries of gram_sums(X) at (a, b) without the dense matrix.  The users of column a come from the CSC side;
    (u, b) is looked up in the sorted CSR keys u * cols + col.  Raises kx.BadTerm with the smallest item of a pair that has a
    term which is not finite or of magnitude >= 64.  chunk: entries of the columns a handled at a time."""
    a = np.asarray(a, np.int64).reshape(-1)
    b = np.asarray(b, np.int64).reshape(-1)
    assert a.shape == b.shape
    cols = np.int64(X.cols)
    cptr = X.csc_col_ptr.astype(np.int64)
    keys = np.repeat(np.arange(X.rows, dtype=np.int64), np.diff(X.csr_row_ptr.astype(np.int64))) * cols + X.csr_col_idx.astype(np.int64)
    assert np.all(np.diff(keys) > 0)
    out = np.zeros(len(a), np.int64)
    ends = np.cumsum(cptr[a + 1] - cptr[a])
    bad_item = None
    lo = 0
    while lo < len(a):
        hi = max(lo + 1, int(np.searchsorted(ends, (ends[lo - 1] if lo else 0) + chunk, side="right")))
        lens = cptr[a[lo:hi] + 1] - cptr[a[lo:hi]]
        at = np.repeat(cptr[a[lo:hi]] - (np.cumsum(lens) - lens), lens) + np.arange(lens.sum())  # every entry of the columns a
        pair = np.repeat(np.arange(lo, hi), lens)
        want = X.csc_row_idx[at].astype(np.int64) * cols + b[pair]
        pos = np.minimum(np.searchsorted(keys, want), len(keys) - 1)
        hit = keys[pos] == want
        with np.errstate(all="ignore"):
            t = X.csc_val[at][hit].astype(_F) * X.csr_val[pos[hit]].astype(_F)
            bad = ~(np.abs(t) < kx.TERM_LIMIT)
        assert t.dtype == _F
        pair = pair[hit]
        if bad.any():
            m = int(min(a[pair[bad]].min(), b[pair[bad]].min()))
            bad_item = m if bad_item is None else min(bad_item, m)
        with np.errstate(all="ignore"):
            np.add.at(out, pair[~bad], kx.to_fixed(t[~bad]))
        lo = hi
    if bad_item is not None:
        raise kx.BadTerm(bad_item)
    return out


def gram_blocks_sparse(X, S):
    """gram_blocks(X, S) without gram_sums: only the pairs that S names are summed (pair_sums, every unordered pair once:
    the terms commute), the diagonal comes from diagonal().  For catalogues whose cols x cols matrix does not fit.  A bad
    term is looked for only where S looks (and on every diagonal), an over-long column everywhere."""
    S = np.asarray(S, np.uint32)
    cols, K = S.shape
    assert cols == X.cols and 1 <= K <= MAX_K
    check_support(S, cols)
    bad = []
    counts = np.diff(X.csc_col_ptr.astype(np.int64))
    if np.any(counts > kx.MAX_ENTRIES):
        bad.append(int(np.nonzero(counts > kx.MAX_ENTRIES)[0][0]))
    d, bad_d = diagonal(X)
    if bad_d is not None:
        bad.append(bad_d)
    real = S != PAD
    ids = np.where(real, S, 0).astype(np.int64)
    j, p, t = np.nonzero(real[:, :, None] & real[:, None, :] & ~np.eye(K, dtype=bool)[None])  # the off-diagonal cells of the blocks
    gj, gp = np.nonzero(real)                                                                  # the cells of row K
    one = np.concatenate([ids[j, p], gj])
    two = np.concatenate([ids[j, t], ids[gj, gp]])
    key, inv = np.unique(np.minimum(one, two) * np.int64(cols) + np.maximum(one, two), return_inverse=True)
    try:
        sums = pair_sums(X, key // cols, key % cols)
    except kx.BadTerm as e:
        bad.append(e.item)
    if bad:
        raise kx.BadTerm(min(bad))
    v = kx.from_fixed(sums)[inv.reshape(-1)]
    B = np.zeros((cols, K + 1, K), _F)
    B[j, p, t] = v[:len(j)]
    B[gj, gp, gp] = kx.from_fixed(d[ids[gj, gp]])
    B[gj, K, gp] = v[len(j):]
    return B


def solve(blocks, n_real=None, l1=1.0, l2=10.0, sweeps=10, tol=0.0, signed=False, trace=None):
    """(w fp32 [n][K], sweeps_used int32 [n], failed) of the blocks [n][K + 1][K], all items side by side.  trace: a list that
    receives a copy of w after every sweep."""
    B = np.asarray(blocks, _F)
    N, K = B.shape[0], B.shape[2]
    assert B.shape[1] == K + 1
    n = np.full(N, K, np.int64) if n_real is None else np.minimum(np.asarray(n_real, np.int64), K)
    l1, l2, tol = _F(l1), _F(l2), _F(tol)
    slot = np.arange(K)[None, :] < n[:, None]
    w = np.zeros((N, K), _F)
    c = np.where(slot, B[:, K, :], _F(0))
    active = np.ones(N, bool)
    failed = np.zeros(N, bool)
    used = np.zeros(N, np.int32)
    with np.errstate(all="ignore"):
        for sw in range(int(sweeps)):
            m = np.zeros(N, _F)
            for a in range(K):
                d = B[:, a, a]
                den = d + l2
                go = active & (a < n) & (den > 0)
                if not go.any():
                    continue
                wa = w[:, a].copy()
                z = fmaf32(d, wa, c[:, a])
                if signed:
                    r = np.abs(z) - l1
                    t = np.copysign(np.where(r > 0, r, _F(0)), z)
                else:
                    r = z - l1
                    t = np.where(r > 0, r, _F(0))
                v = (t / den).astype(_F)
                delta = v - wa
                assert delta.dtype == _F and den.dtype == _F and r.dtype == _F
                broke = go & ~(np.abs(delta) < np.inf)
                failed |= broke
                active &= ~broke
                upd = go & ~broke & (delta != 0)
                if not upd.any():
                    continue
                cn = fmaf32(-delta[:, None], B[:, a, :], c)
                c = np.where(upd[:, None] & slot, cn, c)
                w[upd, a] = v[upd]
                m = np.where(upd, np.maximum(m, np.abs(delta)), m)
            used[active] = sw + 1
            active &= ~(m <= tol)
            if trace is not None:
                trace.append(w.copy())
            if not active.any():
                break
    w[failed] = 0
    used[failed] = 0
    return w, used, int(failed.sum())


def objective(block, n, w, l1, l2):
    """The objective of one block at w in fp64 (the constant 1/2 ||x_j||^2 left out)."""
    G = np.asarray(block[:n, :n], np.float64)
    g = np.asarray(block[-1, :n], np.float64)
    w = np.asarray(w[:n], np.float64)
    return 0.5 * w @ G @ w - g @ w + 0.5 * float(l2) * (w @ w) + float(l1) * np.abs(w).sum()


def train(X, S, l1=1.0, l2=10.0, sweeps=10, tol=0.0, signed=False, sums=None):
    """(w, sweeps_used, failed) of the model of X on the support S."""
    return solve(gram_blocks(X, S, sums), real_slots(S), l1, l2, sweeps, tol, signed)


def transpose(S, w):
    """The model by source item: (iptr int64 [cols + 1], tj uint32, tw fp32): for every i the (j, w_ij) with i in S_j, targets
    ascending; zero weights are kept."""
    S = np.asarray(S, np.uint32)
    w = np.asarray(w, _F)
    cols, K = S.shape
    j, p = np.nonzero(S != PAD)  # (row-major: j ascending)
    src = S[j, p].astype(np.int64)
    o = np.argsort(src, kind="stable")
    iptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=cols))]).astype(np.int64)
    return iptr, j[o].astype(np.uint32), w[j[o], p[o]]


def transposed_lists(S, w):
    """The transpose as item-kNN lists (ids uint32 [cols][K'], values fp32 [cols][K']) with K' the longest list; pads
    (PAD, -inf) at the tail."""
    iptr, tj, tw = transpose(S, w)
    cols = len(iptr) - 1
    Kt = max(1, int(np.diff(iptr).max()))
    ids = np.full((cols, Kt), PAD, np.uint32)
    vals = np.full((cols, Kt), -np.inf, _F)
    for i in range(cols):
        k = iptr[i + 1] - iptr[i]
        ids[i, :k] = tj[iptr[i]:iptr[i + 1]]
        vals[i, :k] = tw[iptr[i]:iptr[i + 1]]
    return ids, vals


def recommend(S, w, ptr, idx, val, n_top, keep_seen=False):
    """(items uint32 [U][n_top], scores fp32 [U][n_top], bad_rows) of the CSR rows (ptr, idx, val) on the model (S, w)."""
    iptr, tj, tw = transpose(S, w)
    cols = len(iptr) - 1
    ptr = np.asarray(ptr, np.int64)
    n = len(ptr) - 1
    items = np.full((n, n_top), PAD, np.uint32)
    scores = np.full((n, n_top), -np.inf, _F)
    bad_rows = 0
    for r in range(n):
        i = np.asarray(idx[ptr[r]:ptr[r + 1]], np.int64)
        x = np.asarray(val[ptr[r]:ptr[r + 1]], _F)
        if len(i) > kx.MAX_ENTRIES:
            bad_rows += 1
            continue
        lens = iptr[i + 1] - iptr[i]
        at = np.repeat(iptr[i] - (np.cumsum(lens) - lens), lens) + np.arange(lens.sum())
        with np.errstate(all="ignore"):
            t = np.repeat(x, lens) * tw[at]
        assert t.dtype == _F
        with np.errstate(invalid="ignore"):
            if (~(np.abs(t) < kx.TERM_LIMIT)).any():
                bad_rows += 1
                continue
        acc = np.zeros(cols, np.int64)
        np.add.at(acc, tj[at].astype(np.int64), kx.to_fixed(t))
        if not keep_seen:
            acc[i] = 0
        items[r], scores[r] = kx.top_lists(acc, n_top)
    return items, scores, bad_rows
