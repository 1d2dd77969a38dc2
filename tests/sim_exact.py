"""Exact CPU reference of item-to-item similarity and of the item filter (mfx_rec_similar, mfx_rec_set_item_filter),
built on rec_exact.py.

s(q, i) is the score chain of rec_exact.chain_scores with H[q] as the query row; n2[i] = s(i, i).  Under the cosine the
ranking key is fp32(s(q, i) * c[i]) and the returned score fp32(key * c[q]), each one fp32 multiply (one rounding,
subnormals kept), ordered by KEY descending, then item ascending.  c is whatever the caller passes: the tests of the
library pass the bits mfx_rec_item_norms returned, so the rounding of 1 / sqrt is no part of the ranking contract;
inv_norm64 is the fp64 value c has to be within 2 ulp of."""
import numpy as np

from rec_exact import PAD, expected_topn, fmaf32

F32 = np.float32
DOT, COSINE = 0, 1


def item_n2(Hr):
    """fp32 [cols]: the FMA chain of (H[i], H[i]) over t ascending from +0."""
    Hr = np.asarray(Hr, F32)
    acc = np.zeros(Hr.shape[0], F32)
    for t in range(Hr.shape[1]):
        acc = fmaf32(Hr[:, t], Hr[:, t], acc)
    return acc


def inv_norm64(n2):
    """fp64 1 / sqrt(n2) rounded to fp32; +0 where n2 is 0 or not finite."""
    n2 = np.asarray(n2, F32)
    ok = np.isfinite(n2) & (n2 > 0)
    out = np.zeros(n2.shape, F32)
    out[ok] = (1.0 / np.sqrt(n2[ok].astype(np.float64))).astype(F32)
    return out


def ulp_distance(a, b):
    """Distance in fp32 grid steps between finite, non-negative fp32 arrays."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def similar_keys(S, c, metric):
    """Ranking keys fp32 [Q, cols] of the chain scores S [Q, cols]."""
    S = np.asarray(S, F32)
    if metric == DOT:
        return S
    with np.errstate(all="ignore"):
        return (S * np.asarray(c, F32)[None, :]).astype(F32)


def similar_eligible(queries, cols, keep=None, exclude_self=True):
    """bool [Q, cols]: keep & not-self."""
    queries = np.asarray(queries, np.int64)
    m = np.ones((len(queries), cols), bool)
    if keep is not None:
        m &= np.asarray(keep).astype(bool)[None, :]
    if exclude_self:
        m[np.arange(len(queries)), queries] = False
    return m


def expected_similar(S, queries, n_top, metric=COSINE, c=None, keep=None, exclude_self=True, with_keys=False):
    """(items uint32 [Q, n_top], scores float32 [Q, n_top]) for the chain scores S [Q, cols] of query items `queries`;
    with_keys appends the ranking keys of the returned slots."""
    queries = np.asarray(queries, np.int64)
    key = similar_keys(S, c, metric)
    items, keys = expected_topn(key, similar_eligible(queries, key.shape[1], keep, exclude_self), n_top)
    scores = keys
    if metric == COSINE:
        with np.errstate(all="ignore"):
            scores = (keys * np.asarray(c, F32)[queries][:, None]).astype(F32)
        scores[items == PAD] = -np.inf
    return (items, scores, keys) if with_keys else (items, scores)


def collinear_ramp(cols, k, seed):
    """H[i] = (1, i 2^-13 u_1, ..., i 2^-13 u_{k-1}) times a per-row scale in [0.6, 1.7): nearly collinear rows, so many
    cosines land within an ulp or two of each other and different keys round to the same returned score."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(0.5, 1.0, k)
    H = np.arange(cols)[:, None] * 2.0 ** -13 * u[None, :]
    H[:, 0] = 1.0
    H *= rng.uniform(0.6, 1.7, cols)[:, None]
    return H.astype(F32)


def key_order_pairs(items, scores, keys):
    """Adjacent returned slots whose keys differ, whose returned scores are equal and whose items descend: the lists
    that ordering by the returned score would get wrong."""
    real = (items[:, :-1] != PAD) & (items[:, 1:] != PAD)
    hit = real & (keys[:, :-1] != keys[:, 1:]) & (scores[:, :-1] == scores[:, 1:]) & (items[:, :-1] > items[:, 1:])
    return int(hit.sum())
