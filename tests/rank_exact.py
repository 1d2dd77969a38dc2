"""Exact CPU reference of the catalogue ranks of (user, item) pairs (mfx_rec_rank) and of the metrics mfx_rec_evaluate
forms from them, on top of rec_exact: the rank of a pair is the position of the item in the user's complete list --
NaN keys and ineligible items dropped, order score descending then item ascending -- and PAD when the item is not in
it.  MRR and AUC are the definitions of include/mfx.h in plain fp64 numpy."""
import numpy as np

from rec_exact import PAD

_F32 = np.float32


def expected_ranks(S, eligible, users_idx, items):
    """(ranks uint32 [P], scores float32 [P], n_eligible uint32 [P]) of the pairs (row users_idx[p] of S, items[p]).
    S [U, cols] holds the score chains (rec_exact.chain_scores) and eligible (bool, broadcast to S) says which items
    the exclusion and the filter leave to each row; the order key is the one of rec_exact.expected_topn."""
    S = np.asarray(S, _F32)
    U, cols = S.shape
    eligible = np.broadcast_to(np.asarray(eligible, bool), S.shape)
    users_idx = np.asarray(users_idx, np.int64)
    items = np.asarray(items, np.int64)
    key = S.astype(np.float64) + 0.0                      # -0 -> +0 so that the two zeros tie
    ar = np.arange(cols)
    pos = np.full((U, cols), PAD, np.uint32)
    n_el = np.zeros(U, np.uint32)
    for u in np.unique(users_idx):
        ok = eligible[u] & ~np.isnan(S[u])
        ids = ar[ok]
        o = np.lexsort((ids, -key[u, ok]))
        pos[u, ids[o]] = np.arange(len(o), dtype=np.uint32)
        n_el[u] = len(o)
    return pos[users_idx, items], S[users_idx, items], n_el[users_idx]


def mrr_auc(users, ranks, n_eligible):
    """(mrr, auc, users kept, auc users) of distinct (user, item) pairs given by their user, rank (PAD: ineligible) and
    eligible count.  MRR: mean over the users of 1 / (1 + smallest rank), 0 when every target is ineligible.  AUC_u:
    P_u the eligible targets, neg = n_eligible - |P_u|, mean over P_u of (neg - (rank_p - a_p)) / neg with a_p the number
    of other targets ranked before p; users with P_u empty or neg = 0 are left out of the AUC mean."""
    users = np.asarray(users, np.int64)
    ranks = np.asarray(ranks, np.int64)
    n_eligible = np.asarray(n_eligible, np.int64)
    rr, aucs = [], []
    for u in np.unique(users):
        m = users == u
        r = np.sort(ranks[m][ranks[m] != PAD]).astype(np.float64)
        rr.append(1.0 / (1.0 + r[0]) if r.size else 0.0)
        neg = float(n_eligible[m][0] - r.size)
        if r.size and neg > 0:
            aucs.append(float(np.mean((neg - (r - np.arange(r.size))) / neg)))
    return (float(np.mean(rr)) if rr else 0.0, float(np.mean(aucs)) if aucs else 0.0, len(rr), len(aucs))
