"""Order-independent inputs for the summing kernels, and integer references of what they must give (host only).

If every term and every partial sum of a segment is exactly representable in fp32, every summation order -- the
reference's left-to-right loop, a tree, a DPP scan, an MFMA chain, the scatter path's 2^-36 fixed point, fused or
separate multiply-add -- gives the same bits.  What is left of a CCD++ rank-one update is den = lambda n + h and
g / den, one correctly rounded operation each, so a path that sums differently must still equal the oracle BIT FOR BIT.

Config A (exact v-pass): ratings are small integers, the live rank of W0 holds multiples of 1/8, lambda is dyadic.
Config B (exact v-pass, u-pass and residual): the live rank of W0 is 1 everywhere, lambda = 1, every rating of column j
is c_j (a signed multiple of 1/4): g = n c_j, den = 2 n, v_j = c_j / 2; the u-pass then sums c_j^2 / 2 and c_j^2 / 4.

W0 is zero in every rank but `live`: dead ranks give v = 0 / (lambda n) = 0 and u = 0 and leave the residual alone, so
the live rank meets the pristine dyadic data at whatever position 0 <= live < k it has.  One outer iteration, one inner
iteration: after the first division nothing is dyadic any more.

preconditions() derives from the ACTUAL pattern and values that every possible partial sum fits the 24-bit significand
(and the scatter path's per-term range); the generators refuse value sets that break a bound.
"""
import numpy as np

from mfx.dataset import RatingData

SIGNIFICAND = 1 << 24      # integers up to 2^24 in magnitude are exact in fp32
SCATTER_RANGE = 1 << 27    # the scatter path's fixed point holds |term| < 2^27 / (entries of the fullest segment)
ULP_CAP = 64               # part 3: sqrt / rsq and two divisions or reciprocal multiplies, 1-2 ulp each plus a rounding:
                           # under 16 ulp; the cap leaves 4x
ULP_SENSITIVITY = 256      # ... and dropping one entry must move the checked coordinate at least this far


class BoundExceeded(ValueError):
    """A value set whose partial sums are not all exact in fp32 on the given pattern."""


# ---------------------------------------------------------------------------------------------- small helpers
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def granularity(a):
    """Largest power of two 2^-e (0 <= e <= 40) of which every entry of `a` is an integer multiple."""
    a = np.asarray(a, np.float64).ravel()
    for e in range(41):
        s = a * float(1 << e)
        if np.all(s == np.rint(s)):
            return 1.0 / float(1 << e)
    raise BoundExceeded("values are not dyadic (no granularity down to 2^-40)")


def row_of_csr(d):
    return np.repeat(np.arange(d.rows, dtype=np.int64), np.diff(d.csr_row_ptr.astype(np.int64)))


def col_of_csc(d):
    return np.repeat(np.arange(d.cols, dtype=np.int64), np.diff(d.csc_col_ptr.astype(np.int64)))


def csc_of_csr(d):
    """For every CSC position the CSR position of the same rating (both copies sorted inside their segments)."""
    rows = row_of_csr(d)
    order = np.lexsort((rows, d.csr_col_idx.astype(np.int64)))
    assert np.array_equal(rows[order], d.csc_row_idx.astype(np.int64)), "CSC copy is not in (column, row) order"
    return order


def with_values(d, csr_val):
    """`d`'s pattern with new values (given in CSR order) in both copies; the test set is kept."""
    csr_val = np.ascontiguousarray(csr_val, dtype=np.float32)
    assert csr_val.shape == (d.nnz,)
    return RatingData(d.rows, d.cols, d.csr_row_ptr, d.csr_col_idx, csr_val, d.csc_col_ptr, d.csc_row_idx,
                      np.ascontiguousarray(csr_val[csc_of_csr(d)]), d.test_row, d.test_col, d.test_val)


def segment_pattern(long_segment=0, seed=5, nvec=5000):
    """(ptr, idx, nvec, lens): the segment lengths of test_gpu_ccd.py's test_flat_kernel_long_and_degenerate_segments -- one
    segment far longer than a span, runs of 1-entry segments, empty segments, a ragged tail -- optionally extended by one
    segment of `long_segment` entries (250 000: the carries of a Netflix-length column)."""
    rng = np.random.default_rng(seed)
    lens = np.concatenate([[0, 0, 20011, 0], np.ones(700, np.int64), [3, 2, 1, 0, 5, 4099, 1, 1, 0, 257, 255, 1023],
                           rng.integers(0, 40, 300), [long_segment] if long_segment else [], [7]]).astype(np.int64)
    ptr = np.zeros(lens.size + 1, np.uint32)
    ptr[1:] = np.cumsum(lens)
    idx = rng.integers(0, nvec, int(ptr[-1])).astype(np.uint32)
    return ptr, idx, nvec, lens


# ---------------------------------------------------------------------------------------------- bounds
def units(maxlen, vmax, rmax, gv, gr, lam):
    """(g, h): maxlen * max|term| / granularity of g = sum vec r and of h = lambda n + sum vec^2, for segments of up to
    maxlen entries, |vec| <= vmax in multiples of gv, |r| <= rmax in multiples of gr."""
    return (maxlen * vmax * rmax / (gv * gr), maxlen * (vmax * vmax + abs(lam)) / min(gv * gv, granularity([lam])))


def sweep_bounds(ptr, val, vec, lam):
    """Worst partial sums of one rank-one sweep, in units of their granularity: maxlen * max|term| / granularity for
    g = sum vec r and for h = lambda n + sum vec^2 (the oracle starts h at lambda n), plus the largest term times the
    longest segment for the scatter path.  Computed from the pattern and the values, nothing is assumed."""
    lens = np.diff(np.asarray(ptr).astype(np.int64))
    maxlen = int(lens.max()) if lens.size else 0
    if maxlen == 0 or np.asarray(val).size == 0:
        return {"maxlen": maxlen, "g": 0.0, "h": 0.0, "scatter": 0.0}
    vmax, rmax = float(np.max(np.abs(vec))), float(np.max(np.abs(val)))
    g_units, h_units = units(maxlen, vmax, rmax, granularity(vec), granularity(val), lam)
    return {"maxlen": maxlen, "g": g_units, "h": h_units, "scatter": maxlen * max(vmax * rmax, vmax * vmax)}


def check_sweep(ptr, val, vec, lam, what="sweep"):
    b = sweep_bounds(ptr, val, vec, lam)
    if b["g"] > SIGNIFICAND or b["h"] > SIGNIFICAND:
        raise BoundExceeded(f"{what}: partial sums need more than 24 bits (segments of up to {b['maxlen']} entries: "
                            f"g {b['g']:.4g}, h {b['h']:.4g} units against 2^24 = {SIGNIFICAND})")
    if b["scatter"] >= SCATTER_RANGE:
        raise BoundExceeded(f"{what}: a term reaches the scatter path's 2^27 / (longest segment)")
    return b


def preconditions(data, W0, live, lam, config):
    """Raises BoundExceeded unless every partial sum of the live rank's passes is exact: the v-pass over the columns
    (configs "A" and "B") and, for config "B", the u-pass over the rows with v = c / 2.  Returns the bounds, in units of
    the granularity (bits needed = log2)."""
    if config not in ("A", "B"):
        raise ValueError(config)
    u = np.asarray(W0, np.float32)[live]
    dead = np.delete(np.asarray(W0), live, axis=0)
    if dead.size and np.any(dead != 0):
        raise BoundExceeded("the dead ranks of W0 must be zero")
    out = {"v": check_sweep(data.csc_col_ptr, data.csc_val, u, lam, "v-pass")}
    if config == "B":
        if lam != 1.0 or np.any(u != 1.0):
            raise BoundExceeded("config B needs lambda = 1 and a live rank of ones")
        cols = col_of_csc(data)
        c = np.zeros(data.cols, np.float32)
        c[cols] = data.csc_val
        if not np.array_equal(c[cols], data.csc_val):
            raise BoundExceeded("config B needs one rating value per column")
        out["u"] = check_sweep(data.csr_row_ptr, data.csr_val, c * np.float32(0.5), lam, "u-pass")
    return out


# ---------------------------------------------------------------------------------------------- generators
def live_rank(k, rows, live, values):
    W0 = np.zeros((k, rows), np.float32)
    W0[live] = values
    return W0


def config_a(d, k, live, seed=0, u_eighths=8, r_max=5, lam=0.5):
    """(data, W0, lam): ratings uniform in 1 .. r_max, live rank uniform in the multiples of 1/8 of [-u_eighths / 8,
    u_eighths / 8].  Raises BoundExceeded where the pattern's segments are too long for these value sets."""
    rng = np.random.default_rng(seed)
    data = with_values(d, rng.integers(1, r_max + 1, d.nnz).astype(np.float32))
    W0 = live_rank(k, d.rows, live, rng.integers(-u_eighths, u_eighths + 1, d.rows).astype(np.float32) / np.float32(8))
    preconditions(data, W0, live, lam, "A")
    return data, W0, float(lam)


def config_b(d, k, live, seed=0, c_quarters=16):
    """(data, W0, 1.0): every rating of column j is c_j, uniform in the non-zero multiples of 1/4 of [-c_quarters / 4,
    c_quarters / 4]; the live rank is 1."""
    rng = np.random.default_rng(seed)
    q = rng.integers(1, c_quarters + 1, d.cols) * rng.choice(np.array([-1, 1]), d.cols)
    c = q.astype(np.float32) / np.float32(4)
    data = with_values(d, c[d.csr_col_idx.astype(np.int64)])
    W0 = live_rank(k, d.rows, live, np.float32(1))
    preconditions(data, W0, live, 1.0, "B")
    return data, W0, 1.0


A_LADDER = [dict(u_eighths=8, r_max=5, lam=0.5), dict(u_eighths=8, r_max=5, lam=0.0625), dict(u_eighths=6, r_max=5, lam=0.0625),
            dict(u_eighths=4, r_max=5, lam=0.0625), dict(u_eighths=2, r_max=5, lam=0.0625), dict(u_eighths=1, r_max=3, lam=0.0625)]
B_LADDER = [dict(c_quarters=q) for q in (32, 24, 16, 8, 4)]


def fit(generator, ladder, *args, **kw):
    """The first (widest) value set of `ladder` whose bounds hold on this pattern -> (chosen set, generator's result)."""
    for choice in ladder:
        try:
            return choice, generator(*args, **kw, **choice)
        except BoundExceeded:
            continue
    raise BoundExceeded("no value set of the ladder fits this pattern")


def sweep_inputs(ptr, idx, nvec, seed=0, ladder=None):
    """Config-A inputs of one single-operator sweep over an arbitrary (ptr, idx): (val, vec, lam), the widest fitting set."""
    rng = np.random.default_rng(seed)
    raw_r, raw_u = rng.random(int(ptr[-1])), rng.random(nvec)
    for c in (ladder or A_LADDER):
        val = (1 + np.floor(raw_r * c["r_max"])).astype(np.float32)
        e = c["u_eighths"]
        vec = ((np.floor(raw_u * (2 * e + 1)) - e) / 8).astype(np.float32)
        try:
            check_sweep(ptr, val, vec, c["lam"])
        except BoundExceeded:
            continue
        return val, vec, float(c["lam"])
    raise BoundExceeded("no value set of the ladder fits this pattern")


# ---------------------------------------------------------------------------------------------- integer references
def _segment_sums(ptr, terms):
    cs = np.zeros(terms.size + 1, np.int64)
    np.cumsum(terms, out=cs[1:])
    p = np.asarray(ptr).astype(np.int64)
    return cs[p[1:]] - cs[p[:-1]]


def int_sweep(ptr, idx, val, vec, lam):
    """One rank-one sweep with g and h summed in int64 (units of their granularity) and the result formed by ONE fp32
    multiply, add and divide: out = g / (lambda * n + h), 0 for an empty segment.  Independent of the oracle."""
    ptr = np.asarray(ptr)
    n = np.diff(ptr.astype(np.int64))
    if np.asarray(val).size == 0:
        return np.zeros(n.size, np.float32)
    gv, gr = granularity(vec), granularity(val)
    iv = np.rint(np.asarray(vec, np.float64) / gv).astype(np.int64)
    ir = np.rint(np.asarray(val, np.float64) / gr).astype(np.int64)
    x = iv[np.asarray(idx).astype(np.int64)]
    G, Hs = _segment_sums(ptr, x * ir), _segment_sums(ptr, x * x)
    assert np.abs(G).max() <= SIGNIFICAND and Hs.max() <= SIGNIFICAND, "sums beyond 24 bits: preconditions() was not applied"
    g = (G.astype(np.float64) * (gv * gr)).astype(np.float32)   # exact: an integer of at most 24 bits times a power of two
    h = (Hs.astype(np.float64) * (gv * gv)).astype(np.float32)
    den = np.float32(lam) * n.astype(np.float32) + h              # fp32 multiply, fp32 add
    out = np.zeros(n.size, np.float32)
    live = n > 0
    out[live] = g[live] / den[live]                               # fp32 divide
    return out


def int_ccd_rank(data, W0, live, lam, with_u):
    """The live rank of one outer iteration at T = 1 by the integer formula: (v, u, csc residual, csr residual).  with_u
    (config B): the u-pass over the untouched ratings with the new v, and the residual r - u v as one fp32 multiply and
    one fp32 subtract; otherwise u and the residuals are None."""
    v = int_sweep(data.csc_col_ptr, data.csc_row_idx, data.csc_val, W0[live], lam)
    if not with_u:
        return v, None, None, None
    u = int_sweep(data.csr_row_ptr, data.csr_col_idx, data.csr_val, v, lam)
    csc = data.csc_val - u[data.csc_row_idx.astype(np.int64)] * v[col_of_csc(data)]
    csr = data.csr_val - v[data.csr_col_idx.astype(np.int64)] * u[row_of_csr(data)]
    return v, u, csc.astype(np.float32), csr.astype(np.float32)


def permuted_fp32_sweep(ptr, idx, val, vec, lam, rng):
    """The same sweep with every segment's terms added in a random order by a sequential fp32 accumulation (numpy's
    cumulative sum is sequential): the order-independence claim itself."""
    ptr64 = np.asarray(ptr).astype(np.int64)
    n = np.diff(ptr64)
    x = np.asarray(vec, np.float32)[np.asarray(idx).astype(np.int64)]
    val = np.asarray(val, np.float32)
    out = np.zeros(n.size, np.float32)
    for s in np.nonzero(n)[0]:
        o = rng.permutation(int(n[s])) + ptr64[s]
        g = np.cumsum(x[o] * val[o], dtype=np.float32)[-1]
        h = np.cumsum(x[o] * x[o], dtype=np.float32)[-1]
        out[s] = g / (np.float32(lam) * np.float32(n[s]) + h)
    return out


# ---------------------------------------------------------------------------------------------- negative control
def one_rating_changed(data, u, by=1.0):
    """(copy of `data` with one rating of its longest column changed by `by` in both copies, that column, its rows):
    what a single lost or doubled entry looks like to a reference.  The entry is the first one from the middle of the
    column on whose row has u != 0 (a rating that meets u = 0 contributes nothing to the column's sum)."""
    j = int(np.argmax(np.diff(data.csc_col_ptr.astype(np.int64))))
    lo, hi = int(data.csc_col_ptr[j]), int(data.csc_col_ptr[j + 1])
    p = (lo + hi) // 2
    while u[int(data.csc_row_idx[p])] == 0:
        p += 1
    i = int(data.csc_row_idx[p])
    e = data.copy()
    e.csc_val[p] += np.float32(by)
    rlo, rhi = int(e.csr_row_ptr[i]), int(e.csr_row_ptr[i + 1])
    q = rlo + int(np.nonzero(e.csr_col_idx[rlo:rhi] == j)[0][0])
    e.csr_val[q] += np.float32(by)
    return e, j, np.unique(data.csc_row_idx[lo:hi].astype(np.int64))


def relerr(a, b):
    """The existing suites' measure: largest difference relative to the largest entry of the reference vector."""
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)))) / max(1e-30, float(np.max(np.abs(b))))


# ---------------------------------------------------------------------------------------------- ALS: exact Gramians, diagonal systems
def dyadic_table(n, k, seed):
    """X [n][k] of multiples of 1/8 in [-1, 1]: products are multiples of 1/64 of magnitude at most 1."""
    return (np.random.default_rng(seed).integers(-8, 9, (n, k)).astype(np.float32) / np.float32(8))


def check_gramian(count, X):
    units = count * float(np.max(np.abs(X))) ** 2 / granularity(X) ** 2
    if units > SIGNIFICAND:
        raise BoundExceeded(f"Gramian of {count} rows needs more than 24 bits ({units:.4g} units)")
    return units


def int_gramian(idx, X):
    """sum over idx of x x^T in int64, returned as fp32 (exact under check_gramian)."""
    g = granularity(X)
    Xi = np.rint(np.asarray(X, np.float64)[np.asarray(idx).astype(np.int64)] / g).astype(np.int64)
    check_gramian(len(idx), X)
    return ((Xi.T @ Xi).astype(np.float64) * (g * g)).astype(np.float32)


def one_hot_table(n, k, seed):
    """Row i is x_i e_(i mod k) with x_i in {+-1/2, +-1}: every Gramian over rows of it -- weighted or not, the implicit
    model's base Gramian over ALL rows included -- is diagonal and exact, and so is every right-hand side."""
    rng = np.random.default_rng(seed)
    x = rng.choice(np.array([-1.0, -0.5, 0.5, 1.0], np.float32), n)
    X = np.zeros((n, k), np.float32)
    X[np.arange(n), np.arange(n) % k] = x
    return X, x


def diagonal_segments(nrows_x, sizes, seed):
    """Segments of the given sizes over distinct rows of the table; values: integers 1 .. 4 (ratings / strengths)."""
    rng = np.random.default_rng(seed)
    ptr = np.zeros(len(sizes) + 1, np.uint32)
    ptr[1:] = np.cumsum(sizes)
    idx = np.concatenate([np.sort(rng.choice(nrows_x, n, replace=False)) for n in sizes]).astype(np.uint32)
    val = rng.integers(1, 5, idx.size).astype(np.float32)
    return ptr, idx, val


def diagonal_solution(ptr, idx, val, x, k, lam, alpha=None):
    """fp64 (diag A [nseg][k], b [nseg][k], y = b / A) of the one-hot systems.  alpha None: explicit ALS,
    A = sum x^2 + lambda, b = sum r x over the segment.  alpha given: implicit ALS with weights w = alpha r (exact: alpha
    and r are dyadic), A = sum_all x^2 + sum w x^2 + lambda, b = sum (1 + w) x.  Sums are int64 in units of 1/4 resp. 1/8
    after scaling, so A and b are exact; empty segments give y = 0."""
    ptr64 = np.asarray(ptr).astype(np.int64)
    nseg = ptr64.size - 1
    x = np.asarray(x, np.float64)
    coord = np.arange(x.size) % k
    A = np.zeros((nseg, k)); b = np.zeros((nseg, k))
    base = np.zeros(k)
    if alpha is not None:
        np.add.at(base, coord, x * x)
    for s in range(nseg):
        j = np.asarray(idx[ptr64[s]:ptr64[s + 1]]).astype(np.int64)
        r = np.asarray(val[ptr64[s]:ptr64[s + 1]], np.float64)
        if alpha is None:
            np.add.at(A[s], coord[j], x[j] * x[j]); np.add.at(b[s], coord[j], r * x[j])
            A[s] += lam
        else:
            w = alpha * r
            np.add.at(A[s], coord[j], w * x[j] * x[j]); np.add.at(b[s], coord[j], (1.0 + w) * x[j])
            A[s] += base + lam
    y = b / A
    y[np.diff(ptr64) == 0] = 0.0
    return A, b, y


def ulps(got, want64):
    """|got - want| in units of the fp32 spacing at `want` (want in fp64; 0 where both are exactly 0)."""
    want64 = np.asarray(want64, np.float64)
    spacing = np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - want64) / spacing


def check_sensitivity(ptr, idx, val, x, k, lam, alpha=None):
    """Precondition of the 64-ulp check: dropping any single entry of the longest segment -- the smallest one included, x^2 =
    1/4 against a sum of at most n -- moves its coordinate of the solution by at least ULP_SENSITIVITY ulp, so a lost entry
    cannot hide under the cap.  Returns the smallest such move in ulp."""
    A, b, y = diagonal_solution(ptr, idx, val, x, k, lam, alpha)
    ptr64 = np.asarray(ptr).astype(np.int64)
    x = np.asarray(x, np.float64)
    worst = np.inf
    for s in [int(np.argmax(np.diff(ptr64)))]:
        j = np.asarray(idx[ptr64[s]:ptr64[s + 1]]).astype(np.int64)
        r = np.asarray(val[ptr64[s]:ptr64[s + 1]], np.float64)
        c = j % k
        w = r if alpha is None else alpha * r
        dA = x[j] ** 2 if alpha is None else w * x[j] ** 2
        db = r * x[j] if alpha is None else (1.0 + w) * x[j]
        moved = (b[s, c] - db) / np.where(A[s, c] - dA != 0, A[s, c] - dA, 1.0)
        worst = min(worst, float(np.min(ulps(moved, y[s, c]))))
    if worst < ULP_SENSITIVITY:
        raise BoundExceeded(f"dropping one entry moves a coordinate by only {worst:.1f} ulp (< {ULP_SENSITIVITY})")
    return worst


# ---------------------------------------------------------------------------------------------- what the GPU modules run
CCD_RANKS = [(7, 0), (7, 1), (7, 6), (1, 0)]   # (k, live): first of a pair, second of a pair, last of an odd k, k = 1


def ml1m_pattern(dataset):
    """The ML-1M-shaped synthetic of test_gpu_defer_resid.py (6040 x 3706, 10^6 ratings, empty rows and columns)."""
    return dataset.synth_ratings(6040, 3706, 1_000_000, seed=11, skew=0.9, test_frac=0.01, empty_row_frac=0.01, empty_col_frac=0.02)


def small_patterns(dataset, only=None):
    """The shapes of test_gpu_edge.py's test_hyper_sparse_shard_layouts and test_scatter_persistent_workgroup_ranges, by name
    (only: build just that one)."""
    make = {"hyper_sparse": lambda: dataset.synth_ratings(600000, 40000, 4200000, seed=21, skew=0.3, test_frac=0.002),
            "scatter_ranges": lambda: dataset.synth_ratings(3000, 2500, 60_000, seed=31, skew=0.6, test_frac=0.02,
                                                            empty_row_frac=0.02, empty_col_frac=0.02)}
    return {name: f() for name, f in make.items() if only in (None, name)}


def ccd_case(d, config, k, live):
    """(chosen value set, (data, W0, lam)) of config "A" / "B" on pattern `d`: the widest set of the ladder that fits it."""
    seed = 1000 * k + 10 * live + (config == "B")
    if config == "A":
        return fit(config_a, A_LADDER, d, k, live, seed=seed)
    return fit(config_b, B_LADDER, d, k, live, seed=seed)


ALS_LAMBDA = 0.25
IALS_ALPHAS = (0.0, 1.0, 0.5)
GRAMIAN_KS = [1, 5, 16, 32, 36, 40, 44, 60, 64, 68, 100, 128]
GRAMIAN_COUNTS = [1, 15, 16, 17, 31, 33, 777, 2047, 2048]
DIAGONAL_SIZES = [0, 1, 3, 0, 17, 250, 2048, 2049, 2100, 5000, 20000, 1]
DIAGONAL_ROWS = 30000
HALF_KS = [5, 16, 64, 100, 128]                 # als_half / ials_half (k <= 128)
BLOCK_KS, BLOCK_DS = [64, 160, 256, 1024], [16, 64, 128]
DIAGONAL_CASES = [(k, DIAGONAL_ROWS) for k in sorted(set(HALF_KS + BLOCK_KS))]
