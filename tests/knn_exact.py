"""Exact CPU reference of the item-kNN model (mfx_knn_*): the contract of include/mfx.h ("Item-kNN") restated in numpy.

A term is one fp32 multiply, cut toward zero to a multiple of 2^-36; terms are added as int64 (wrapping, like the library's
64-bit adds); a similarity or score is the fp32 nearest to the sum; lists are ordered by value descending, then item
ascending (the `beats` order of the recommender).  Nothing here calls the library."""
import numpy as np

_F = np.float32
PAD = 0xFFFFFFFF
FIXED_ONE = 2.0 ** 36
TERM_LIMIT = _F(64.0)
MAX_ENTRIES = 1 << 21


class BadTerm(ValueError):
    """A build that the library refuses: .item is the smallest item with a bad term or an over-long column."""

    def __init__(self, item):
        super().__init__(f"item {item}")
        self.item = item


def to_fixed(t):
    """fp32 terms -> int64 multiples of 2^-36, truncated toward zero."""
    return np.trunc(np.asarray(t, _F).astype(np.float64) * FIXED_ONE).astype(np.int64)


def from_fixed(s):
    """int64 sums -> fp32: one rounding int64 -> fp32, then the exact scale."""
    return np.asarray(s, np.int64).astype(_F) * _F(2.0 ** -36)


def _bad(t):
    with np.errstate(invalid="ignore"):
        return ~(np.abs(t) < TERM_LIMIT)


def similarities(X):
    """The integer sums of every pair, int64 [cols][cols] with a zero diagonal (small matrices only).  Raises BadTerm."""
    ptr = X.csr_row_ptr.astype(np.int64)
    S = np.zeros((X.cols, X.cols), np.int64)
    bad_item = None
    counts = np.diff(X.csc_col_ptr.astype(np.int64))
    if np.any(counts > MAX_ENTRIES):
        bad_item = int(np.nonzero(counts > MAX_ENTRIES)[0][0])
    for u in range(X.rows):
        j = X.csr_col_idx[ptr[u]:ptr[u + 1]].astype(np.int64)
        x = X.csr_val[ptr[u]:ptr[u + 1]].astype(_F)
        with np.errstate(all="ignore"):
            t = x[:, None] * x[None, :]
        assert t.dtype == _F
        off = ~np.eye(len(j), dtype=bool)
        b = _bad(t) & off
        if b.any():
            m = int(j[np.nonzero(b.any(axis=1))[0]].min())
            bad_item = m if bad_item is None else min(bad_item, m)
        ok = off & ~b
        with np.errstate(all="ignore"):
            f = np.where(ok, to_fixed(np.where(ok, t, 0)), 0)
        S[np.ix_(j, j)] += f
    if bad_item is not None:
        raise BadTerm(bad_item)
    return S


def similarity_rows(X, items):
    """The integer sums of the given items only, int64 [len(items)][cols]: similarities(X)[items] without the dense
    cols x cols matrix, from the CSC column of each item and the CSR rows of its users.  Raises BadTerm with the smallest of
    the given items that has a bad term or an over-long column (given every item: the item similarities names)."""
    items = np.asarray(items, np.int64).reshape(-1)
    rptr = X.csr_row_ptr.astype(np.int64)
    cptr = X.csc_col_ptr.astype(np.int64)
    S = np.zeros((len(items), X.cols), np.int64)
    bad_item = None
    for n, i in enumerate(items):
        c0, c1 = cptr[i], cptr[i + 1]
        bad = c1 - c0 > MAX_ENTRIES
        users = X.csc_row_idx[c0:c1].astype(np.int64)
        lens = rptr[users + 1] - rptr[users]
        at = np.repeat(rptr[users] - (np.cumsum(lens) - lens), lens) + np.arange(lens.sum())  # every entry of the users' rows
        j = X.csr_col_idx[at].astype(np.int64)
        with np.errstate(all="ignore"):
            t = np.repeat(X.csc_val[c0:c1].astype(_F), lens) * X.csr_val[at].astype(_F)
        assert t.dtype == _F
        off = j != i
        b = _bad(t) & off
        bad = bad or bool(b.any())
        if bad:
            bad_item = int(i) if bad_item is None else min(bad_item, int(i))
            continue
        np.add.at(S[n], j[off], to_fixed(t[off]))
    if bad_item is not None:
        raise BadTerm(bad_item)
    return S


def top_lists(S, keep):
    """Rows of integer sums -> (ids uint32 [n][keep], values fp32 [n][keep]): the non-zero entries of a row by value
    descending, then item ascending; pads (PAD, -inf) at the tail."""
    S = np.atleast_2d(S)
    n, cols = S.shape
    ids = np.full((n, keep), PAD, np.uint32)
    vals = np.full((n, keep), -np.inf, _F)
    for r in range(n):
        j = np.nonzero(S[r])[0]
        v = from_fixed(S[r, j])
        o = np.lexsort((j, -v.astype(np.float64)))[:keep]  # (the keys are fp32: exact in fp64)
        ids[r, :len(o)] = j[o]
        vals[r, :len(o)] = v[o]
    return ids, vals


def build(X, K):
    """(nbr_idx uint32 [cols][K], nbr_sim fp32 [cols][K]) of the weighted matrix X."""
    return top_lists(similarities(X), K)


def recommend(nbr_idx, nbr_sim, ptr, idx, val, n_top, keep_seen=False):
    """(items uint32 [U][n_top], scores fp32 [U][n_top], bad_rows) of the CSR rows (ptr, idx, val) on the given lists."""
    nbr_idx = np.asarray(nbr_idx, np.uint32)
    nbr_sim = np.asarray(nbr_sim, _F)
    cols = nbr_idx.shape[0]
    ptr = np.asarray(ptr, np.int64)
    n = len(ptr) - 1
    items = np.full((n, n_top), PAD, np.uint32)
    scores = np.full((n, n_top), -np.inf, _F)
    bad_rows = 0
    for r in range(n):
        i = np.asarray(idx[ptr[r]:ptr[r + 1]], np.int64)
        x = np.asarray(val[ptr[r]:ptr[r + 1]], _F)
        if len(i) > MAX_ENTRIES:
            bad_rows += 1
            continue
        j = nbr_idx[i]                      # [n_u][K]
        real = j != PAD
        with np.errstate(all="ignore"):
            t = x[:, None] * nbr_sim[i]
        assert t.dtype == _F
        if (_bad(t) & real).any():
            bad_rows += 1
            continue
        acc = np.zeros(cols, np.int64)
        np.add.at(acc, j[real].astype(np.int64), to_fixed(t[real]))
        if not keep_seen:
            acc[i] = 0
        items[r], scores[r] = top_lists(acc, n_top)
    return items, scores, bad_rows


def weights(R, scheme, k1=1.2, b=0.75):
    """The weighting of mfx.knn_weights as (csr_val, csc_val), fp64 arithmetic and one rounding to fp32."""
    if scheme is None:
        return R.csr_val.copy(), R.csc_val.copy()
    cptr = R.csc_col_ptr.astype(np.int64)
    rptr = R.csr_row_ptr.astype(np.int64)
    c = np.diff(cptr).astype(np.float64)
    n_u = np.diff(rptr).astype(np.float64)
    nbar = n_u.sum() / R.rows
    with np.errstate(all="ignore"):
        idf = np.log(float(R.rows)) - np.log(1.0 + c)
    dense = np.zeros((R.rows, R.cols), np.float64)
    mask = np.zeros((R.rows, R.cols), bool)
    for u in range(R.rows):
        j = R.csr_col_idx[rptr[u]:rptr[u + 1]]
        dense[u, j] = R.csr_val[rptr[u]:rptr[u + 1]].astype(np.float64)
        mask[u, j] = True
    with np.errstate(all="ignore"):
        if scheme == "bm25":
            out = dense * (k1 + 1.0) / (k1 * (1.0 - b + b * n_u[:, None] / nbar) + dense) * idf[None, :]
        else:
            y = dense if scheme == "cosine" else np.sqrt(dense) * idf[None, :]
            y = np.where(mask, y, 0.0)
            norm = np.sqrt((y * y).sum(axis=0))
            out = np.where(norm[None, :] > 0, y / norm[None, :], 0.0)
    out = np.where(mask, out, 0.0).astype(_F)
    rows_of = np.repeat(np.arange(R.rows), np.diff(rptr))
    cols_of = np.repeat(np.arange(R.cols), np.diff(cptr))
    return out[rows_of, R.csr_col_idx], out[R.csc_row_idx, cols_of]
