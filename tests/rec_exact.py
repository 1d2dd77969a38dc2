"""Exact CPU reference of the top-N recommender (mfx_rec_*): fp32 fused multiply-add chains and the ranking.

The score of (u, i) is the fp32 FMA chain acc = fma(W[u,t], H[i,t], acc) over t = 0, 1, ..., k-1 from acc = +0, so the
answer to any query is fully determined and computable here bit for bit.  fmaf32 is an exactly rounded fp32 fma in
vectorised numpy: the product of two fp32 numbers is exact in fp64, TwoSum gives the sum with c as s + e exactly, and
the one case where rounding s to fp32 rounds twice -- s exactly on an fp32 midpoint with e != 0 -- is corrected one
ulp toward the sign of e."""
import numpy as np

PAD = 0xFFFFFFFF
_F32 = np.float32
_TOP = 2.0 ** 128  # where fp32 +inf sits on the fp32 grid (FLT_MAX + 1 ulp), for midpoints at the overflow threshold


def _grid64(r):
    """fp32 values as fp64, with +-inf taken as +-2^128 (the next grid point above FLT_MAX)."""
    r64 = np.asarray(r).astype(np.float64)
    return np.where(np.isinf(r64), np.copysign(_TOP, r64), r64)


def fmaf32(a, b, c):
    """Elementwise fp32 fma(a, b, c) with a single rounding (round to nearest even), broadcasting like numpy."""
    a, b, c = np.broadcast_arrays(np.asarray(a, _F32), np.asarray(b, _F32), np.asarray(c, _F32))
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b                      # exact: 24 + 24 significant bits, exponents in fp64 range
        c64 = c.astype(np.float64)
        s = p + c64
        z = s - p
        e = (p - (s - z)) + (c64 - z)                     # TwoSum: p + c == s + e exactly (finite s)
        r = s.astype(_F32)
        # s can be an fp32 midpoint only if its fp64 fraction ends in binary 1 followed by 28 zeros, or outside the
        # range where fp32 has all 24 bits (subnormal results, the top binade)
        a_s = np.abs(s)
        cand = ((s.view(np.uint64) & 0x1FFFFFFF) == 0x10000000) | (a_s < 2.0 ** -126) | (a_s >= 2.0 ** 127)
        cand &= (e != 0) & np.isfinite(s)
    idx = np.nonzero(cand)
    if idx[0].size:
        rr, ss, ee = r[idx], s[idx], e[idx]
        dd = ss - _grid64(rr)                             # which side of rr the fp64 sum lies on
        nb = np.nextafter(rr, np.where(dd > 0, _F32(np.inf), _F32(-np.inf)))
        mid = (dd != 0) & ((_grid64(rr) + _grid64(nb)) * 0.5 == ss)  # s halfway between rr and its neighbour nb
        take = mid & ((ee > 0) == (dd > 0))               # the exact value lies beyond the midpoint, on nb's side
        rr[take] = nb[take]
        r = r.copy()
        r[idx] = rr
    return r


def chain_scores(Wr, Hr, users, chunk_elems=1 << 21):
    """fp32 [len(users), cols]: the FMA chain of each (user, item) over t ascending.  Wr [rows][k], Hr [cols][k]."""
    Wr = np.asarray(Wr, _F32)
    Hr = np.asarray(Hr, _F32)
    users = np.asarray(users, np.int64)
    cols, k = Hr.shape
    HT = np.ascontiguousarray(Hr.T)
    out = np.empty((len(users), cols), _F32)
    step = max(1, chunk_elems // max(1, cols))
    for c0 in range(0, len(users), step):
        w = Wr[users[c0:c0 + step]]
        acc = np.zeros((len(w), cols), _F32)
        for t in range(k):
            acc = fmaf32(w[:, t:t + 1], HT[t][None, :], acc)
        out[c0:c0 + step] = acc
    return out


def expected_topn(S, eligible, n_top):
    """(items uint32 [U, n_top], scores float32 [U, n_top]) of scores S [U, cols]: NaN and ineligible items dropped,
    order score descending then item ascending (-0 == +0, +-inf ordinary), padded with (PAD, -inf)."""
    S = np.asarray(S, _F32)
    U, cols = S.shape
    eligible = np.broadcast_to(np.asarray(eligible, bool), S.shape)
    items = np.full((U, n_top), PAD, np.uint32)
    scores = np.full((U, n_top), -np.inf, _F32)
    key = S.astype(np.float64) + 0.0                      # -0 -> +0 so that the two zeros tie
    ar = np.arange(cols)
    for u in range(U):
        ok = eligible[u] & ~np.isnan(S[u])
        ids = ar[ok]
        o = np.lexsort((ids, -key[u, ok]))[:n_top]
        n = len(o)
        items[u, :n] = ids[o]
        scores[u, :n] = S[u, ids[o]]
    return items, scores


def eligible_mask(ex, users, cols):
    """bool [len(users), cols]: True where the item may be recommended (ex: RatingData or None)."""
    m = np.ones((len(users), cols), bool)
    if ex is not None:
        for s, u in enumerate(users):
            m[s, ex.csr_col_idx[ex.csr_row_ptr[u]:ex.csr_row_ptr[u + 1]]] = False
    return m
