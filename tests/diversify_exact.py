"""Exact CPU reference of diversity re-ranking (mfx_rec_diversify): greedy maximal marginal relevance over a slot's
eligible candidates, every number an fp32 operation in the order include/mfx.h fixes, built on the exact fma and the score
chains of rec_exact.py and on the similarity keys of sim_exact.py.

  rel(i) = the score chain of (user, i);  a = fp32(tradeoff), b = fp32(1 - a);  D_0 = +0
  step s: value(i) = fma(-b, D(i), fp32(a * rel(i))); the pick has the greatest value (NaN as -inf), then the greater rel,
          then the smaller id (-0 == +0); D(i) = sim(pick, i) where that is greater (a NaN similarity changes nothing)
  sim:    DOT: the chain of (H[j], H[i]); COSINE: fp32(fp32(chain * c[i]) * c[j])

The chains between items do not depend on the slot, so the tests compute item_gram(H) once per H and share it."""
import numpy as np

from rec_exact import PAD, chain_scores, fmaf32
from sim_exact import COSINE, DOT, similar_keys

F32 = np.float32


def item_gram(Hr):
    """fp32 [cols, cols]: the FMA chain of (H[j], H[i]) over t ascending from +0 (symmetric: a product commutes)."""
    Hr = np.asarray(Hr, F32)
    return chain_scores(Hr, Hr, np.arange(Hr.shape[0]))


class LazyGram:
    """item_gram(H)[j, ids] computed when asked for: what a catalogue too large for the whole matrix takes in G's place."""
    def __init__(self, Hr):
        self.H = np.asarray(Hr, F32)

    def __getitem__(self, key):
        j, ids = key
        return chain_scores(self.H[j:j + 1], self.H[np.asarray(ids, np.int64)], [0])[0]


def similarities(G, j, ids, metric, c):
    """fp32 [len(ids)]: sim(j, i) for i in ids, from the chains G (item_gram or LazyGram)."""
    s = G[j, ids]
    if metric == DOT:
        return s
    key = similar_keys(s[None, :], np.asarray(c, F32)[ids], COSINE)[0]   # fp32(s * c[i])
    with np.errstate(all="ignore"):
        return (key * F32(c[j])).astype(F32)


def _order_key(x):
    """fp64 keys whose ascending order is x descending with -0 == +0 (x holds no NaN)."""
    return -(np.asarray(x, np.float64) + 0.0)


def diversify_slot(rel, ids, G, n_top, tradeoff, metric=COSINE, c=None):
    """The picks of one slot: rel fp32 [E] and ids [E] ascending, the eligible candidates -> (items uint32 [n_top], scores
    fp32 [n_top], values fp32 [n_top]) padded with (PAD, -inf, -inf)."""
    rel = np.asarray(rel, F32)
    ids = np.asarray(ids, np.int64)
    a = F32(tradeoff)
    b = F32(F32(1.0) - a)
    items = np.full(n_top, PAD, np.uint32)
    scores = np.full(n_top, -np.inf, F32)
    values = np.full(n_top, -np.inf, F32)
    D = np.zeros(ids.size, F32)
    left = np.ones(ids.size, bool)
    with np.errstate(all="ignore"):
        arel = (a * rel).astype(F32)
    for s in range(min(n_top, ids.size)):
        value = fmaf32(-b, D, arel)
        v = np.where(np.isnan(value), F32(-np.inf), value)
        pos = np.nonzero(left)[0]
        p = pos[np.lexsort((ids[pos], _order_key(rel[pos]), _order_key(v[pos])))[0]]
        items[s], scores[s], values[s] = ids[p], rel[p], value[p]
        left[p] = False
        sim = similarities(G, ids[p], ids, metric, c)
        with np.errstate(invalid="ignore"):
            D = np.where(sim > D, sim, D)
    return items, scores, values


def expected_diversify(S, cand_ptr, cand_idx, eligible, G, n_top, tradeoff, metric=COSINE, c=None):
    """(items uint32 [U, n_top], scores fp32, values fp32, n_eligible uint32 [U]) of the slots' scores S [U, cols] (row q:
    the score chains of slot q's user), the lists cand_ptr / cand_idx and the exclusion / filter mask `eligible` [U, cols]
    (or True): a candidate counts when it is eligible and its score is not NaN."""
    S = np.asarray(S, F32)
    cand_ptr = np.asarray(cand_ptr, np.int64)
    cand_idx = np.asarray(cand_idx, np.int64)
    U = cand_ptr.size - 1
    eligible = np.broadcast_to(np.asarray(eligible, bool), S.shape)
    out = (np.empty((U, n_top), np.uint32), np.empty((U, n_top), F32), np.empty((U, n_top), F32))
    counts = np.zeros(U, np.uint32)
    for q in range(U):
        ids = cand_idx[cand_ptr[q]:cand_ptr[q + 1]]
        ids = ids[eligible[q, ids] & ~np.isnan(S[q, ids])]
        counts[q] = ids.size
        for o, x in zip(out, diversify_slot(S[q, ids], ids, G, n_top, tradeoff, metric, c)):
            o[q] = x
    return out + (counts,)


def intra_list_cosine(items, Hr):
    """Mean over the slots of the mean pairwise cosine (fp64) among each slot's returned items; slots with fewer than two
    items are left out."""
    Hn = np.asarray(Hr, np.float64)
    Hn = Hn / np.linalg.norm(Hn, axis=1, keepdims=True)
    means = []
    for row in np.asarray(items):
        ids = row[row != PAD].astype(np.int64)
        if ids.size < 2:
            continue
        C = Hn[ids] @ Hn[ids].T
        means.append((C.sum() - np.trace(C)) / (ids.size * (ids.size - 1)))
    return float(np.mean(means))


def planted_clusters(seed, cols=300, centres=6, k=16, users=40, noise=0.3):
    """(W [users, k], H [cols, k]) fp32: items around Gaussian centres, users mixtures of two of them."""
    rng = np.random.default_rng(seed)
    Cn = rng.standard_normal((centres, k))
    H = Cn[rng.integers(0, centres, cols)] + noise * rng.standard_normal((cols, k))
    pair = np.array([rng.choice(centres, 2, replace=False) for _ in range(users)])
    mix = rng.uniform(0.3, 0.7, users)[:, None]
    W = mix * Cn[pair[:, 0]] + (1 - mix) * Cn[pair[:, 1]] + 0.1 * rng.standard_normal((users, k))
    return W.astype(F32), H.astype(F32)
