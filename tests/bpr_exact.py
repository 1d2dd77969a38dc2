"""Exact CPU reference of BPR training (mfx_bpr_*): the sampler in Python integers and one step in single fp32 operations.

Everything here restates the contract of include/mfx.h ("BPR training") in other words, so that the library can be
checked bit for bit: the splitmix64 sampler, the fp32 FMA score chain (rec_exact.fmaf32), the sigmoid recipe, the
2^-36 fixed-point sums as integers and the one-rounding update."""
import numpy as np

from rec_exact import fmaf32

_F = np.float32
MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15

# the sigmoid recipe (include/mfx.h)
SIG_CLAMP = _F(80.0)
SIG_LOG2E = _F(1.4426950408889634)       # 0x3FB8AA3B
SIG_LN2_HI = _F(0.693359375)             # 355 / 512: n * LN2_HI is exact for |n| < 2^15
SIG_LN2_LO = _F(-2.12194440e-4)          # ln 2 - LN2_HI
SIG_POLY = tuple(_F(c) for c in (1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0, 1.0))  # c6 .. c0

FIXED_ONE = 2.0 ** 36
TERM_LIMIT = _F(64.0)


# ------------------------------------------------------------------------------------------------ sampler
def fin(z):
    """The splitmix64 finaliser on a Python integer below 2^64."""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def draw(seed, ctr):
    """Output number ctr of the stream of `seed`."""
    s0 = fin((seed + GOLDEN) & MASK)
    return fin((s0 + ((ctr + 1) & MASK) * GOLDEN) & MASK)


def slot(R, seed, n):
    """(u, i, j, skipped) of slot n."""
    ptr, idx = R.csr_row_ptr, R.csr_col_idx
    nnz = int(ptr[-1])
    p = draw(seed, (2 * n) & MASK) % nnz
    j = draw(seed, (2 * n + 1) & MASK) % R.cols
    lo, hi = 0, R.rows  # the row u with ptr[u] <= p < ptr[u + 1]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if int(ptr[mid]) <= p:
            lo = mid
        else:
            hi = mid
    u = lo
    row = idx[int(ptr[u]):int(ptr[u + 1])]
    return u, int(idx[p]), j, bool(np.any(row == j))


def triples(R, seed, first, count):
    """(u, i, j uint32 [count], skipped bool [count]) of the slots first .. first + count - 1, one Python integer at a time."""
    out = [slot(R, seed, first + t) for t in range(count)]
    u, i, j, s = (np.array(c) for c in zip(*out)) if count else ([], [], [], [])
    return np.asarray(u, np.uint32), np.asarray(i, np.uint32), np.asarray(j, np.uint32), np.asarray(s, bool)


def _fin_np(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def triples_np(R, seed, first, count):
    """triples() in wrapping uint64 numpy arithmetic (the test of the host sampler checks the two against each other)."""
    with np.errstate(over="ignore"):
        s0 = np.uint64(fin((seed + GOLDEN) & MASK))
        n = np.uint64(first & MASK) + np.arange(count, dtype=np.uint64)
        g = np.uint64(GOLDEN)
        a = _fin_np(s0 + (np.uint64(2) * n + np.uint64(1)) * g)
        b = _fin_np(s0 + (np.uint64(2) * n + np.uint64(2)) * g)
    ptr = R.csr_row_ptr.astype(np.int64)
    p = (a % np.uint64(ptr[-1])).astype(np.int64)
    j = (b % np.uint64(R.cols)).astype(np.int64)
    u = np.searchsorted(ptr, p, side="right") - 1
    i = R.csr_col_idx[p].astype(np.int64)
    key = R.csr_col_idx.astype(np.int64) + np.repeat(np.arange(R.rows, dtype=np.int64), np.diff(ptr)) * R.cols  # ascending
    want = u * R.cols + j
    pos = np.minimum(np.searchsorted(key, want), len(key) - 1)
    return u.astype(np.uint32), i.astype(np.uint32), j.astype(np.uint32), key[pos] == want


# ------------------------------------------------------------------------------------------------ one step
def sigmoid_neg(x):
    """g = 1 / (1 + e^x) of fp32 x by the recipe of include/mfx.h, every operation a single fp32 one."""
    x = np.asarray(x, _F)
    with np.errstate(all="ignore"):
        xc = np.minimum(np.maximum(x, -SIG_CLAMP), SIG_CLAMP)
        n = np.rint(xc * SIG_LOG2E)
        r = (xc - n * SIG_LN2_HI) - n * SIG_LN2_LO
        p = np.full_like(r, SIG_POLY[0])
        for c in SIG_POLY[1:]:
            p = p * r + c
        assert p.dtype == _F and r.dtype == _F
        e = np.ldexp(p, np.nan_to_num(n).astype(np.int32)).astype(_F)
        return _F(1.0) / (_F(1.0) + e)


def slot_scores(W, H, u, i, j):
    """(x [n], d [n][k]): d = fp32(H[i] - H[j]) and the FMA chain of W[u] . d over c ascending from +0."""
    with np.errstate(all="ignore"):
        d = H[i] - H[j]
        w = W[u]
        x = np.zeros(len(u), _F)
        for c in range(W.shape[1]):
            x = fmaf32(w[:, c], d[:, c], x)
    return x, d


def to_fixed(t):
    """fp32 terms -> int64 multiples of 2^-36, truncated toward zero."""
    return np.trunc(t.astype(np.float64) * FIXED_ONE).astype(np.int64)


def step(W, H, u, i, j, skipped, lr, lam):
    """One step on the slots (u, i, j, skipped) at the frozen factors W, H.  Returns (W', H', [slots, skipped, bad, correct])."""
    W = np.asarray(W, _F)
    H = np.asarray(H, _F)
    u, i, j = (np.asarray(a, np.int64) for a in (u, i, j))
    n, k = len(u), W.shape[1]
    skipped = np.zeros(n, bool) if skipped is None else np.asarray(skipped, bool)
    lr, lam = _F(lr), _F(lam)
    live = np.nonzero(~skipped)[0]
    ul, il, jl = u[live], i[live], j[live]
    x, d = slot_scores(W, H, ul, il, jl)
    with np.errstate(all="ignore"):
        g = sigmoid_neg(x)[:, None]
        tw = g * d
        th = g * W[ul]
        bad = ~np.isfinite(x) | np.any(np.abs(tw) >= TERM_LIMIT, axis=1) | np.any(np.abs(th) >= TERM_LIMIT, axis=1)
    ok = ~bad
    stats = [n, int(skipped.sum()), int(bad.sum()), int((x[ok] > 0).sum())]
    ul, il, jl = ul[ok], il[ok], jl[ok]
    fw, fh = to_fixed(tw[ok]), to_fixed(th[ok])
    accW = np.zeros(W.shape, np.int64)
    accH = np.zeros(H.shape, np.int64)
    np.add.at(accW, ul, fw)
    np.add.at(accH, il, fh)
    np.add.at(accH, jl, -fh)
    mW = np.bincount(ul, minlength=W.shape[0])
    mH = np.bincount(il, minlength=H.shape[0]) + np.bincount(jl, minlength=H.shape[0])
    out = []
    for X, acc, m in ((W, accW, mW), (H, accH, mH)):
        a = acc.astype(_F) * _F(2.0 ** -36)  # one rounding int64 -> fp32, then the exact scale
        reg = (lam * m.astype(_F))[:, None] * X
        new = X + lr * (a - reg)
        assert new.dtype == _F
        out.append(np.where((m > 0)[:, None], new, X))
    assert k == H.shape[1]
    return out[0], out[1], stats


def epoch_steps(nnz, batch, pos):
    """The slot ranges (first, count) of the steps from slot `pos` to the end of its epoch."""
    out = []
    while True:
        cnt = min(batch, nnz - pos % nnz)
        out.append((pos, cnt))
        pos += cnt
        if pos % nnz == 0:
            return out


def small_matrix(seed=3, rows=60, cols=40, nnz=503):
    """rows x cols with nnz distinct entries (mfx.dataset.from_coo: ids ascending inside a row); some rows may be empty."""
    from mfx import dataset as ds
    cells = np.random.default_rng(seed).choice(rows * cols, nnz, replace=False)
    return ds.from_coo(rows, cols, cells // cols, cells % cols, np.ones(nnz, _F))


def planted_clusters():
    """The generator of test_gpu_ials.py's end-to-end test: 20 clusters of 30 items, 2 000 users, 25 training items of the
    user's own cluster plus 2 random ones (54 000 entries), one more in-cluster item held out as the test set."""
    from mfx import dataset as ds
    rng = np.random.default_rng(11)
    nc, per, users = 20, 30, 2000
    items = nc * per
    tr_r, tr_c, te_r, te_c = [], [], [], []
    for u in range(users):
        cl = u % nc
        own = cl * per + rng.permutation(per)[:26]
        others = np.setdiff1d(np.arange(items), cl * per + np.arange(per))
        extra = rng.choice(others, 2, replace=False)
        tr = np.concatenate([own[:25], extra])
        tr_r += [u] * tr.size
        tr_c += list(tr)
        te_r.append(u)
        te_c.append(own[25])
    return ds.from_coo(users, items, np.array(tr_r), np.array(tr_c), np.ones(len(tr_r), np.float32),
                       np.array(te_r), np.array(te_c), np.ones(len(te_r), np.float32))


def initial_factors(rows, cols, k, seed):
    """0.1 * N(0, 1) factors, W then H from one generator: what mfx.BprSolver(init_seed=seed) draws."""
    rng = np.random.default_rng(seed)
    W = (0.1 * rng.standard_normal((rows, k))).astype(_F)
    H = (0.1 * rng.standard_normal((cols, k))).astype(_F)
    return W, H


def train(R, W, H, lr, lam, batch, seed, n_epochs, pos=0, sampler=triples_np):
    """n_epochs epochs from slot `pos` (a started epoch is finished as the first).  Returns (W, H, per-epoch stats, pos)."""
    nnz = int(R.csr_row_ptr[-1])
    stats = []
    for _ in range(n_epochs):
        tot = np.zeros(4, np.int64)
        for first, cnt in epoch_steps(nnz, batch, pos):
            u, i, j, s = sampler(R, seed, first, cnt)
            W, H, st = step(W, H, u, i, j, s, lr, lam)
            tot += st
            pos = first + cnt
        stats.append(tot)
    return W, H, np.array(stats), pos
