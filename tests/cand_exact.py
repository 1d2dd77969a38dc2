"""Exact CPU reference of candidate-list re-ranking (mfx_rec_query_candidates): the reference top-N of rec_exact.py with the
slot's own list as one more eligibility mask, the Python twin of the wrapper's canonicalisation, and the factor and
exclusion generators the GPU tests share (those of test_gpu_rank_exact.py)."""
import numpy as np

from rec_exact import PAD, expected_topn

F32 = np.float32


def candidate_mask(cand_ptr, cand_idx, cols):
    """bool [U, cols]: True where the item is in the slot's list."""
    cand_ptr = np.asarray(cand_ptr, np.int64)
    cand_idx = np.asarray(cand_idx, np.int64)
    U = cand_ptr.size - 1
    m = np.zeros((U, cols), bool)
    for q in range(U):
        m[q, cand_idx[cand_ptr[q]:cand_ptr[q + 1]]] = True
    return m


def expected_candidates(S, cand_ptr, cand_idx, eligible, n_top):
    """(items uint32 [U, n_top], scores float32 [U, n_top], n_eligible uint32 [U]) of the slots' scores S [U, cols] (row q:
    the scores of slot q's user), the lists cand_ptr / cand_idx and the exclusion / filter mask `eligible` [U, cols] (or
    True): an item counts when it is in the slot's list, eligible and its score is not NaN."""
    S = np.asarray(S, F32)
    ok = candidate_mask(cand_ptr, cand_idx, S.shape[1]) & np.broadcast_to(np.asarray(eligible, bool), S.shape)
    items, scores = expected_topn(S, ok, n_top)
    return items, scores, (ok & ~np.isnan(S)).sum(1).astype(np.uint32)


def canonical_lists(cand_ptr, cand_idx):
    """What Recommender.query_candidates(canonical=False) hands the library, row by row: each list sorted, without
    repeats and PAD entries -> (ptr uint32 [U + 1], idx uint32)."""
    cand_ptr = np.asarray(cand_ptr, np.int64)
    cand_idx = np.asarray(cand_idx, np.int64)
    rows = []
    for q in range(cand_ptr.size - 1):
        r = np.unique(cand_idx[cand_ptr[q]:cand_ptr[q + 1]])
        rows.append(r[r != PAD])
    ptr = np.zeros(cand_ptr.size, np.int64)
    np.cumsum([len(r) for r in rows], out=ptr[1:])
    idx = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    return ptr.astype(np.uint32), idx.astype(np.uint32)


def random_lists(rng, lengths, cols):
    """Strictly ascending random lists of the given lengths -> (ptr uint32, idx uint32)."""
    lengths = np.asarray(lengths, np.int64)
    ptr = np.zeros(lengths.size + 1, np.int64)
    np.cumsum(lengths, out=ptr[1:])
    rows = [np.sort(rng.choice(cols, n, replace=False)) for n in lengths]
    idx = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    return ptr.astype(np.uint32), idx.astype(np.uint32)


def whole_catalogue(nslots, cols):
    return (np.arange(nslots + 1, dtype=np.int64) * cols).astype(np.uint32), np.tile(np.arange(cols, dtype=np.uint32), nslots)


def regime_factors(regime, rows, cols, k, seed):
    rng = np.random.default_rng(seed)
    W = rng.standard_normal((rows, k))
    H = rng.standard_normal((cols, k))
    if regime == "scaled":            # per-t scales 2^-20 .. 2^20: the rounding of each step depends on the order
        W *= 2.0 ** rng.integers(-20, 21, k)
        H *= 2.0 ** rng.integers(-20, 21, k)
    elif regime == "subnormal":       # products around 2^-136: subnormal W and H entries, subnormal sums, +-0
        ew = rng.integers(-134, -2, k)
        W *= 2.0 ** ew
        H *= 2.0 ** (-136 - ew + rng.integers(-16, 8, (cols, k)))
        W[::7] *= 2.0 ** -40          # every product underflows: the score is a signed zero
    elif regime == "huge":            # products near and beyond FLT_MAX: +-inf scores, inf - inf = NaN
        for t in {0, k // 2, k - 1}:
            W[:, t] *= 1e19 * 2.0 ** rng.integers(0, 4, rows)
            H[:, t] *= np.where(rng.random(cols) < 0.4, 1e20, 1.0)
    W, H = W.astype(F32), H.astype(F32)
    if regime == "huge":
        # An fma adds the exact product, so a chain of finite factors overflows to +-inf and stays there: it never meets
        # inf - inf.  NaN keys need infinite entries: 0 * inf, and (+inf) + (-inf) where an item has both signs.
        H[5::97, 0], H[11::97, k - 1] = np.inf, -np.inf
        W[3::13, 0], W[4::13, k - 1] = 0.0, 0.0
        if k > 1:
            H[17::97, 0], H[17::97, k - 1] = np.inf, np.inf
    return W, H


def exclusion(mfx, rng, rows, cols, n_top, S=None):
    """RatingData of mixed exclusion rows, six kinds cycling within every wave of 32 users: empty; about half the
    items; the user's own top 2 n_top items by S [rows][cols] (without S: a random half instead); every item but
    n_top / 2; every item; a random quarter of the items with duplicate indices."""
    r, c = [], []
    top = None
    if S is not None:
        top = expected_topn(S[2::6], True, 2 * n_top)[0]
    for u in range(rows):
        kind = u % 6
        if kind == 0:
            ids = np.zeros(0, np.int64)
        elif kind == 1 or (kind == 2 and top is None):
            ids = np.nonzero(rng.random(cols) < 0.5)[0]
        elif kind == 2:
            ids = top[u // 6]
            ids = np.sort(ids[ids != PAD].astype(np.int64))
        elif kind == 3:
            ids = np.setdiff1d(np.arange(cols), rng.choice(cols, n_top // 2, replace=False))
        elif kind == 4:
            ids = np.arange(cols)
        else:
            ids = rng.choice(cols, cols // 4, replace=False)
            ids = np.sort(np.repeat(ids, rng.integers(1, 4, ids.size)))
        r.append(np.full(ids.size, u, np.int64))
        c.append(ids)
    r, c = np.concatenate(r), np.concatenate(c)
    return mfx.dataset.from_coo(rows, cols, r.astype(np.uint32), c.astype(np.uint32), np.ones(r.size, F32))
