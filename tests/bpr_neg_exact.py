"""Exact CPU reference of negative sampling by trials (mfx_bpr_create_neg, mfx_bpr_apply_neg, mfx_bpr_trials): the trial
sampler in Python integers and in wrapping uint64, the two choices and one step, restated from the contract of include/mfx.h
("Negative sampling by trials") on top of bpr_exact (the sampler of the first trial, the fixed-point sums, the update)."""
import numpy as np

import bpr_exact as bx
from rec_exact import fmaf32

_F = np.float32
MASK, GOLDEN = bx.MASK, bx.GOLDEN
HARDEST, WARP = 1, 2  # MFX_BPR_NEG_* (include/mfx.h)


# ------------------------------------------------------------------------------------------------ the trials
def trial_items(cols, seed, n, m):
    """c_2 .. c_m of slot n in Python integers (trial 1 is bpr_exact.slot's j)."""
    s1 = bx.fin((seed + 2 * GOLDEN) & MASK)
    b = bx.fin((s1 + ((n + 1) & MASK) * GOLDEN) & MASK)
    return [bx.fin((b + t * GOLDEN) & MASK) % cols for t in range(2, m + 1)]


def trials(R, seed, first, count, m):
    """(u, i uint32 [count], items uint32 [count][m], member bool [count][m]), one Python integer at a time."""
    u, i = np.zeros(count, np.uint32), np.zeros(count, np.uint32)
    items, member = np.zeros((count, m), np.uint32), np.zeros((count, m), bool)
    ptr, idx = R.csr_row_ptr, R.csr_col_idx
    for s in range(count):
        n = first + s
        uu, ii, j1, _ = bx.slot(R, seed, n)
        row = set(int(x) for x in idx[int(ptr[uu]):int(ptr[uu + 1])])
        cs = [j1] + trial_items(R.cols, seed, n, m)
        u[s], i[s], items[s] = uu, ii, cs
        member[s] = [c in row for c in cs]
    return u, i, items, member


def trials_np(R, seed, first, count, m):
    """trials() in wrapping uint64 numpy arithmetic."""
    u, i, j1, s1flag = bx.triples_np(R, seed, first, count)
    items, member = np.zeros((count, m), np.int64), np.zeros((count, m), bool)
    items[:, 0], member[:, 0] = j1, s1flag
    if m > 1:
        with np.errstate(over="ignore"):
            g = np.uint64(GOLDEN)
            s1 = np.uint64(bx.fin((seed + 2 * GOLDEN) & MASK))
            n = np.uint64(first & MASK) + np.arange(count, dtype=np.uint64)
            b = bx._fin_np(s1 + (n + np.uint64(1)) * g)
            t = np.arange(2, m + 1, dtype=np.uint64)
            c = bx._fin_np(b[:, None] + t[None, :] * g) % np.uint64(R.cols)
        items[:, 1:] = c.astype(np.int64)
        ptr = R.csr_row_ptr.astype(np.int64)
        key = R.csr_col_idx.astype(np.int64) + np.repeat(np.arange(R.rows, dtype=np.int64), np.diff(ptr)) * R.cols  # ascending
        want = u.astype(np.int64)[:, None] * R.cols + items[:, 1:]
        pos = np.minimum(np.searchsorted(key, want), len(key) - 1)
        member[:, 1:] = key[pos] == want
    return u, i, items.astype(np.uint32), member


def rank_weights(cols, m):
    """The default table as numpy computes it (the library's may differ by one fp32 ulp: log is no single operation)."""
    return np.array([_F(np.log(np.float64(max(1, (cols - 1) // t)))) for t in range(1, m + 1)], _F)


# ------------------------------------------------------------------------------------------------ scores and choices
def chain(w, h):
    """The fp32 FMA chain of w . h over the last axis ascending from +0, w and h broadcast against each other."""
    w, h = np.broadcast_arrays(np.asarray(w, _F), np.asarray(h, _F))
    x = np.zeros(w.shape[:-1], _F)
    for c in range(w.shape[-1]):
        x = fmaf32(w[..., c], h[..., c], x)
    return x


def trial_scores(W, H, u, i, items):
    """(s_i [n], s_t [n][m]) at the factors W, H."""
    w, Ht = W[u], np.ascontiguousarray(H.T)
    st = np.zeros(items.shape, _F)
    for c in range(W.shape[1]):  # (the chain of `chain`, one column at a time: no [n][m][k] array)
        st = fmaf32(w[:, c][:, None], Ht[c][items], st)
    return chain(w, H[i]), st


def choose_hardest(scores, member):
    """t [n] (1-based, 0 = no eligible trial): among the trials with member = 0 a NaN ranks below every number, then the
    greater score, then the smaller t; +0 and -0 tie."""
    s = scores.astype(np.float64)
    s = np.where(np.isposinf(s), 1e300, np.where(np.isneginf(s), -1e300, s))  # (fp32 numbers lie inside +-3.5e38)
    s = np.where(np.isnan(s), -1e305, s)                                     # below -inf of fp32, above "not eligible"
    s = np.where(member, -np.inf, s)
    first_best = np.argmax(s, axis=1)  # (the first of equal maxima; -0.0 == +0.0)
    return np.where(np.all(member, axis=1), 0, first_best + 1).astype(np.int64)


def choose_warp(si, scores, member):
    """t [n]: the first trial outside the row with not (fp32(s_i - s_t) >= 1), 0 = none."""
    with np.errstate(all="ignore"):
        margin = si.astype(_F)[:, None] - scores.astype(_F)
        assert margin.dtype == _F
        viol = ~member & ~(margin >= _F(1.0))
    return np.where(viol.any(axis=1), np.argmax(viol, axis=1) + 1, 0).astype(np.int64)


def _update(W, H, ul, il, jl, tw, th, lr, lam):
    """The sums and the update of bpr_exact.step for the counted slots (ul, il, jl) with their terms tw, th."""
    fw, fh = bx.to_fixed(tw), bx.to_fixed(th)
    accW, accH = np.zeros(W.shape, np.int64), np.zeros(H.shape, np.int64)
    np.add.at(accW, ul, fw)
    np.add.at(accH, il, fh)
    np.add.at(accH, jl, -fh)
    mW = np.bincount(ul, minlength=W.shape[0])
    mH = np.bincount(il, minlength=H.shape[0]) + np.bincount(jl, minlength=H.shape[0])
    out = []
    for X, acc, m in ((W, accW, mW), (H, accH, mH)):
        a = acc.astype(_F) * _F(2.0 ** -36)
        reg = (lam * m.astype(_F))[:, None] * X
        new = X + lr * (a - reg)
        assert new.dtype == _F
        out.append(np.where((m > 0)[:, None], new, X))
    return out[0], out[1]


def step_neg(W, H, u, i, items, member, mode, rank_weight, lr, lam, scores=None):
    """One step on the trials items [n][m] at the frozen factors.  Returns (W', H', [slots, skipped, bad, correct], j, t):
    t [n] the chosen trial (0 = none) and j [n] the chosen item (0 where none was chosen).  scores: trial_scores() of the same
    arguments, for a caller that runs both modes."""
    W, H = np.asarray(W, _F), np.asarray(H, _F)
    u, i, items = (np.asarray(a, np.int64) for a in (u, i, items))
    n, m = items.shape
    member = np.zeros((n, m), bool) if member is None else np.asarray(member, bool)
    rows = np.arange(n)
    si, st = trial_scores(W, H, u, i, items) if scores is None else scores
    if mode == HARDEST:
        t = choose_hardest(st, member)
        j = np.where(t > 0, items[rows, np.maximum(t, 1) - 1], 0)
        Wn, Hn, stats = bx.step(W, H, u, i, j, t == 0, lr, lam)
        return Wn, Hn, stats, j, t
    assert mode == WARP
    lr, lam = _F(lr), _F(lam)
    rw = np.asarray(rank_weight, _F)
    bad = ~np.isfinite(si)
    t = np.where(bad, 0, choose_warp(si, st, member))
    skipped = (t == 0) & ~bad
    chosen = t > 0
    pick = np.maximum(t, 1) - 1
    j = np.where(chosen, items[rows, pick], 0)
    sj = st[rows, pick]
    g = rw[pick][:, None]
    with np.errstate(all="ignore"):
        tw = g * (H[i] - H[j])
        th = g * W[u]
        assert tw.dtype == _F and th.dtype == _F
        small = np.all(np.abs(tw) < bx.TERM_LIMIT, axis=1) & np.all(np.abs(th) < bx.TERM_LIMIT, axis=1)  # (a NaN is not below)
        bad = bad | (chosen & (~np.isfinite(sj) | ~small))
        ok = chosen & ~bad
        correct = ok & ((si - sj) > 0)
    Wn, Hn = _update(W, H, u[ok], i[ok], j[ok], tw[ok], th[ok], lr, lam)
    return Wn, Hn, [n, int(skipped.sum()), int(bad.sum()), int(correct.sum())], j, t


def train_neg(R, W, H, lr, lam, batch, seed, n_epochs, m, mode, rank_weight=None, pos=0, sampler=trials_np):
    """n_epochs epochs from slot `pos`.  Returns (W, H, per-epoch stats, pos, [slots without a chosen trial, sum of chosen t])."""
    nnz = int(R.csr_row_ptr[-1])
    rw = rank_weights(R.cols, m) if rank_weight is None else rank_weight
    stats, ts = [], np.zeros(2, np.int64)
    for _ in range(n_epochs):
        tot = np.zeros(4, np.int64)
        for first, cnt in bx.epoch_steps(nnz, batch, pos):
            u, i, items, member = sampler(R, seed, first, cnt, m)
            W, H, st, _, t = step_neg(W, H, u, i, items, member, mode, rw, lr, lam)
            tot += st
            ts += [int((t == 0).sum()), int(t.sum())]
            pos = first + cnt
        stats.append(tot)
    return W, H, np.array(stats), pos, ts
