"""Exact CPU reference of IVF retrieval (mfx_rec_ivf_probe, mfx_rec_query_ivf), made of the references already here: the
probe is the reference top-N of rec_exact.py over the score chains against the centroids, and the query is the candidate
re-ranking of cand_exact.py over the ascending union of the probed lists."""
import numpy as np

from cand_exact import expected_candidates
from rec_exact import PAD, chain_scores, expected_topn


def lists_of(assign, nlist):
    """(list_ptr uint32 [nlist + 1], list_idx uint32 [cols]) of an assignment: list l holds its items in ascending id."""
    assign = np.asarray(assign, np.int64)
    ptr = np.zeros(nlist + 1, np.int64)
    np.cumsum(np.bincount(assign, minlength=nlist), out=ptr[1:])
    return ptr.astype(np.uint32), np.argsort(assign, kind="stable").astype(np.uint32)


def expected_probe(W, centroids, users, nprobe):
    """(lists uint32 [U, nprobe], scores float32 [U, nprobe]): score descending, then list id ascending; NaN never; padded."""
    return expected_topn(chain_scores(W, centroids, users), True, nprobe)


def union_lists(probes, list_ptr, list_idx):
    """CSR (ptr uint32 [U + 1], idx uint32) of every slot's ascending union of its probed lists (PAD: no list)."""
    list_ptr = np.asarray(list_ptr, np.int64)
    rows = []
    for pr in np.asarray(probes):
        parts = [list_idx[list_ptr[l]:list_ptr[l + 1]] for l in pr if l != PAD]
        rows.append(np.sort(np.concatenate(parts)) if parts else np.zeros(0, np.uint32))
    ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=ptr[1:])
    idx = np.concatenate(rows) if rows else np.zeros(0, np.uint32)
    return ptr.astype(np.uint32), idx.astype(np.uint32)


def expected_query(S, probes, list_ptr, list_idx, eligible, n_top):
    """(items, scores, n_eligible) of the slots' scores S [U, cols] and their probed lists: expected_candidates over the unions."""
    ptr, idx = union_lists(probes, list_ptr, list_idx)
    return expected_candidates(S, ptr, idx, eligible, n_top)
