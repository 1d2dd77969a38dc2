"""Inputs, dispatch mirror, fp64 references, checks and controls of the per-rank sweep of the conjugate-gradient kernels (host
only; used by tests/test_cg_sweep_host.py and tests/test_gpu_cg_sweep.py).

Inputs, for a rank k: foldin_cg_ref.inputs(k, 4200, sizes), so the seeds and draws are those of every other CG test
(H = standard_normal((4200, k), seed k) / sqrt(k) as fp32, rows of distinct sorted items with values 1..5 and 15 % explicit
zeros, seed 100 + k, the warm start W0 = 0.1 N(0, 1), seed 1000 + k), lambda = 0.1.  Two size sets:
    S: 12 rows (0, 1, 2, 3, 4, 5, 17, 130, 2048, 2049, 4097, 1): an empty row, the tails of kGatherRows = 4, a row that is
       exactly one chunk, one split in two and one split in three (k_cg_reduce)
    M: 140 rows, sizes cycling through 0..40 with rows 32..63 empty: two blocks of k_foldcg_dense and of the per-row kernels,
       the second with one ragged wavefront and idle ones, and one wavefront (rows 32..63) frozen from the start
Models on S: up to rank 136 the implicit model at alpha = 1 and 40, ALS and CCD on foldin_cg_ref.explicit_values; above,
implicit at alpha = 40 and ALS.  On M: implicit at alpha = 40.

Dispatch mirror: dispatch(k) restates gather() of csrc/rec_foldin_cg.hip and csrc/rec_explain_cg.hip, foldcg_dense() and
spd_inverse_launch(); the ladders and constants it rests on are read from the sources by dispatch_constants() and asserted as
they stand, so a change in a dispatcher breaks the mirror loudly instead of silently moving a rank to another instance.

References: foldin_cg_ref.rows (the method), foldin_cg_ref.dense_solutions (the dense systems), explain_cg_ref.solve /
errors (the targets); training has the same reference, ials_cg_ref.half being foldin_cg_ref.rows on the implicit model (the
host test holds the two to the bit).  Cached per (k, model, alpha, start, steps, tol) and returned read-only.
rows_batched is foldin_cg_ref.rows for the implicit model over all rows at once (set M); the host test pins it to rows().

Checks: converged / method / targets return the measured errors and the list of misses of the project's bounds, so that the GPU
test and the host controls judge an answer by the very same code.  Controls: wrong answers that the checks must refuse."""
import functools
import os
import re

import numpy as np

import explain_cg_ref as xr
import foldin_cg_ref as ref
import ials_ref
import solve_sweep as sw

CSRC = sw.CSRC
COLS, LAM = 4200, ref.LAM
S = (0, 1, 2, 3, 4, 5, 17, 130, 2048, 2049, 4097, 1)
M = tuple(0 if 32 <= u < 64 else u % 41 for u in range(140))
SPLIT_ROWS = (9, 10)                                   # rows of S split in two and in three chunks
RANGES = [(lo, lo + 16) for lo in range(1, 137, 17)]   # eight rank ranges of 17: 1..136
LARGE = [159, 160, 161, 192, 193, 224, 225, 255, 256, 257, 260, 384, 511, 512, 513, 516, 767, 1000, 1023, 1024]
M_RANKS = [3, 32, 33, 96, 128, 160, 257, 513, 1024]
EDGE_RANKS = [33, 65, 96, 129, 257, 513]
ALL_RANKS = list(range(1, 137)) + LARGE
STEPS, TOL = 64, 1e-5                                  # the converged setup
SHORT_STEPS = (1, 2, 4)                                # tol = 0: the method itself
T = 17                                                 # targets per row: a second, ragged group for TG = 16, 8 and 4
PAD_AT = 5                                             # the padding target's position; position 0 is the row's first item
ALONE = (0, 3, 4, 7, 8, 15, 16)                        # targets asked for alone, bit for bit
MAX_BACKWARD, MAX_REL, MAX_COND = sw.MAX_BACKWARD, sw.MAX_REL, sw.MAX_COND  # 3e-5, 1e-3, 1e3: test_gpu_ials.py, test_gpu_foldin_cg.py
IMPLICIT, ALS, CCD = ref.IMPLICIT, ref.ALS, ref.CCD
NAMES = {(IMPLICIT, 1.0): "implicit alpha 1", (IMPLICIT, 40.0): "implicit alpha 40", (ALS, 0.0): "ALS", (CCD, 0.0): "CCD"}


def models(k):
    """[(model, alpha)] that rank k runs on set S."""
    return [(IMPLICIT, 1.0), (IMPLICIT, 40.0), (ALS, 0.0), (CCD, 0.0)] if k <= 136 else [(IMPLICIT, 40.0), (ALS, 0.0)]


# ------------------------------------------------------------------------------------------------ dispatch mirror
@functools.lru_cache(maxsize=None)
def dispatch_constants():
    """{"fold": C ladder, "explain": (C, TG) ladder, "dense": (threshold, ND above it, column block), "spd": kSpdB,
    "chunk": kAlsChunk, "rows": kGatherRows}, read from the sources and asserted as they stand."""
    def read(name):
        with open(os.path.join(CSRC, name)) as f:
            return f.read()
    fold, expl, hpp, spd, als = (read(n) for n in ("rec_foldin_cg.hip", "rec_explain_cg.hip", "rec_foldin_cg.hpp", "spd_inverse.hip",
                                                  "als_solver.hpp"))
    per_lane = r"const\s+uint32_t\s+c\s*=\s*\(k\s*\+\s*63\)\s*/\s*64\s*;"
    assert len(re.findall(per_lane, fold)) == 1 and len(re.findall(per_lane, expl)) == 1
    f_ladder = [tuple(map(int, m)) for m in re.findall(r"if\s*\(c\s*<=\s*(\d+)\)\s*launch_gather_c<(\d+)>\(mode,", fold)]
    f_last = re.findall(r"else\s+launch_gather_c<(\d+)>\(mode,", fold)
    assert f_ladder == [(1, 1), (2, 2), (4, 4), (8, 8)] and f_last == ["16"], (f_ladder, f_last)
    assert re.findall(r"k_cg_gather<C,\s*1,\s*(\d)>\)", fold) == ["1", "2", "3"]  # one system per wavefront (TG = 1), MODE 1 .. 3
    # the first pass forms b (MODE 2) and, warm, the sum over y0 as well (MODE 3); a step is MODE 1
    assert len(re.findall(r"gather\(warm\s*\?\s*3\s*:\s*2,", fold)) == 1 and len(re.findall(r"gather\(1,", fold)) == 1
    e_ladder = [tuple(map(int, m)) for m in re.findall(r"if\s*\(c\s*<=\s*(\d+)\)\s*launch_gather<(\d+),\s*(\d+)>\(h,", expl)]
    e_last = re.findall(r"else\s+launch_gather<(\d+),\s*(\d+)>\(h,", expl)
    assert e_ladder == [(1, 1, 16), (2, 2, 16), (4, 4, 8), (8, 8, 4)] and e_last == [("16", "1")], (e_ladder, e_last)
    assert len(re.findall(r"k_cg_gather<C,\s*TG,\s*1>\)", expl)) == 1  # the same kernel, TG targets per wavefront, MODE 1
    dense = re.findall(r"switch\s*\(k\s*>\s*(\d+)\s*\?\s*(\d+)\s*:\s*\(k\s*\+\s*31\)\s*/\s*32\)", fold)
    cases = re.findall(r"case\s+(\d+):\s*hipLaunchKernelGGL\(k_foldcg_dense<(\d+)>", fold)
    default = re.findall(r"default:\s*hipLaunchKernelGGL\(k_foldcg_dense<(\d+)>", fold)
    assert dense == [("128", "4")] and cases == [("1", "1"), ("2", "2"), ("3", "3")] and default == ["4"], (dense, cases, default)
    assert len(re.findall(r"grid\(\(nseg\s*\+\s*127\)\s*/\s*128,\s*\(k\s*\+\s*127\)\s*/\s*128\),\s*block\(256\)", fold)) == 1
    assert len(re.findall(r"b0\s*=\s*blockIdx\.y\s*\*\s*128,\s*width\s*=\s*min\(128u,\s*k\s*-\s*b0\)", fold)) == 1
    assert len(re.findall(r"const\s+bool\s+vec\s*=\s*\(k\s*&\s*3\)\s*==\s*0\s*;", fold)) == 1
    assert len(re.findall(r"mok\[t\]\s*=\s*32\s*\*\s*t\s*\+\s*r31\s*<\s*width\s*;", fold)) == 1
    b = re.findall(r"constexpr\s+uint32_t\s+kSpdB\s*=\s*(\d+)\s*;", spd)
    assert b == ["32"] and len(re.findall(r"kp\s*=\s*spd_kp\(k\),\s*nb\s*=\s*kp\s*/\s*kSpdB\s*;", spd)) == 1, b
    chunk = re.findall(r"constexpr\s+uint32_t\s+kAlsChunk\s*=\s*(\d+)\s*;", als)
    rows = re.findall(r"constexpr\s+int\s+kGatherRows\s*=\s*(\d+)\s*;", hpp)
    assert chunk == ["2048"] and rows == ["4"], (chunk, rows)
    return {"fold": tuple(c for _, c in f_ladder) + (int(f_last[0]),),
            "explain": tuple((c, tg) for _, c, tg in e_ladder) + ((int(e_last[0][0]), int(e_last[0][1])),),
            "dense": (int(dense[0][0]), int(dense[0][1]), 128), "spd": int(b[0]), "chunk": int(chunk[0]), "rows": int(rows[0])}


def dispatch(k):
    """(C, TG, ND, last width, nb) of rank k: the columns per lane of both gathers, the targets per wavefront of
    explanation's k_cg_gather, the 32-column tiles of k_foldcg_dense, the width of its last column block and the blocks of the device
    inverse."""
    assert 1 <= k <= 1024, k
    d = dispatch_constants()
    c = -(-k // 64)
    C = next(x for x in d["fold"] if c <= x)
    CE, TG = next(x for x in d["explain"] if c <= x[0])
    assert C == CE
    above, nd, block = d["dense"]
    ND = nd if k > above else -(-k // 32)
    return C, TG, ND, k - block * ((k - 1) // block), -(-k // d["spd"])


def vec(k):
    """load4 of k_foldcg_dense reads 16 bytes at once"""
    return k % 4 == 0


def width_class(k):
    """(tiles of 32 columns with a column in the last column block, whether the last of them is ragged): mok[t] is mixed
    when fewer than ND tiles have one, and within a ragged tile"""
    w = dispatch(k)[3]
    return -(-w // 32), w % 32 != 0


def chunks(n):
    """work items of a row of n entries"""
    return max(1, -(-n // dispatch_constants()["chunk"]))


# ------------------------------------------------------------------------------------------------ inputs
def _frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def data(k, sizes=S):
    """(ptr, idx, val, H, W0) of rank k, read-only."""
    return _frozen(ref.inputs(k, COLS, tuple(sizes)))


@functools.lru_cache(maxsize=8)
def values(model, k, sizes=S):
    """The values the model runs on: the explicit models on foldin_cg_ref.explicit_values."""
    val = data(k, sizes)[2]
    return val if model == IMPLICIT else _frozen((ref.explicit_values(val),))[0]


@functools.lru_cache(maxsize=4)
def base_pair(k):
    return _frozen(ref.base(data(k)[3], LAM))


def live_rows(model, k, alpha):
    """The rows of S with a right-hand side."""
    return ref.counting(model, k, alpha, COLS, S)


@functools.lru_cache(maxsize=4)
def targets(k):
    """uint32 [12][T]: position 0 the row's first item (a drawn one for the empty row), PAD_AT the padding, the rest drawn
    with default_rng(7 + k)."""
    ptr, idx, _, _, _ = data(k)
    rng = np.random.default_rng(7 + k)
    tg = rng.integers(0, COLS, (len(S), T)).astype(np.uint32)
    for u in range(len(S)):
        if ptr[u + 1] > ptr[u]:
            tg[u, 0] = idx[ptr[u]]
    tg[:, PAD_AT] = xr.PAD
    return _frozen((tg,))[0]


# ------------------------------------------------------------------------------------------------ fp64 references
def method_with(pair, model, k, alpha, warm, steps, tol):
    """(Y, steps done) of foldin_cg_ref.rows on set S, cold or from W0, with the given (G, G^-1) (a control's wrong one)."""
    ptr, idx, _, H, W0 = data(k)
    return ref.rows(model, ptr, idx, values(model, k), H, LAM, alpha, W0 if warm else None, steps, tol, base_pair=pair)


@functools.lru_cache(maxsize=64)
def method(model, k, alpha, warm, steps, tol):
    """method_with the fp64 base of rank k: the reference of checks 1 to 3 (ials_cg_ref.half is this very call)."""
    return _frozen(method_with(base_pair(k) if model == IMPLICIT else None, model, k, alpha, warm, steps, tol))


@functools.lru_cache(maxsize=8)
def target_solves(model, k, alpha):
    """(Z [12][T][k], steps done [12][T]) of explain_cg_ref.solve under the converged setup."""
    ptr, idx, _, H, _ = data(k)
    pair = base_pair(k) if model == IMPLICIT else None
    return _frozen(xr.solve(model, ptr, idx, values(model, k), H, LAM, alpha, targets(k), STEPS, TOL, base_pair=pair))


def rows_batched(ptr, idx, val, H, lam, alpha, W_init, steps, tol, pair):
    """foldin_cg_ref.rows(IMPLICIT, ...) on all rows at once: the same recurrence, every row frozen on its own."""
    G, Ginv = pair
    U, k = len(ptr) - 1, H.shape[1]
    n = np.diff(ptr.astype(np.int64))
    at = np.minimum(ptr[:-1].astype(np.int64)[:, None] + np.arange(max(1, n.max()))[None, :], max(0, len(idx) - 1))
    inside = np.arange(at.shape[1])[None, :] < n[:, None]
    v = np.where(inside, np.asarray(val, np.float32)[at], np.float32(0))
    w32 = np.float32(alpha) * v
    pos = v > 0
    c = np.where(pos, w32, 0).astype(np.float64)
    Hj = np.asarray(H, np.float64)[np.asarray(idx, np.int64)[at]] * inside[:, :, None]
    b = np.einsum("unk,un->uk", Hj, np.where(pos, np.float32(1) + w32, 0).astype(np.float64))
    bn = np.linalg.norm(b, axis=1)
    mul = lambda P: P @ G + np.einsum("unk,un->uk", Hj, c * np.einsum("unk,uk->un", Hj, P))
    live = pos.any(axis=1) & (bn != 0)
    Y = np.zeros((U, k)) if W_init is None else np.where(live[:, None], np.asarray(W_init, np.float64), 0.0)
    R = b - mul(Y) if W_init is not None else b.copy()
    done = np.zeros(U, np.int64)
    act = live.copy()
    if tol > 0:
        act &= ~(np.linalg.norm(R, axis=1) <= tol * bn)
    Z = R @ Ginv
    P, gamma = Z.copy(), np.einsum("uk,uk->u", R, Z)
    for _ in range(steps):
        act &= gamma != 0
        if not act.any():
            break
        a_ = np.nonzero(act)[0]
        Q = mul(np.where(act[:, None], P, 0.0))
        a = gamma[a_] / np.einsum("uk,uk->u", P[a_], Q[a_])
        Y[a_] += a[:, None] * P[a_]
        R[a_] -= a[:, None] * Q[a_]
        done[a_] += 1
        if tol > 0:
            act[a_] = ~(np.linalg.norm(R[a_], axis=1) <= tol * bn[a_])
            a_ = np.nonzero(act)[0]
        Z = R[a_] @ Ginv
        g2 = np.einsum("uk,uk->u", R[a_], Z)
        P[a_] = Z + (g2 / gamma[a_])[:, None] * P[a_]
        gamma[a_] = g2
    return Y, done


@functools.lru_cache(maxsize=16)
def method_m(k, alpha, warm, steps, tol):
    """(Y, steps done) of the fp64 method on set M (implicit), by rows_batched."""
    ptr, idx, val, H, W0 = data(k, M)
    return _frozen(rows_batched(ptr, idx, val, H, LAM, alpha, W0 if warm else None, steps, tol, base_pair(k)))


def release(k):
    """The dense systems of a rank above 136 are up to 100 MB per model: dropped once the rank is done."""
    if k > 136:
        ref.dense_solutions.cache_clear()
        for f in (method, target_solves, base_pair, values, method_m):
            f.cache_clear()


# ------------------------------------------------------------------------------------------------ metrics and checks
def rel_error(got, want):
    return float(np.linalg.norm(np.asarray(got, np.float64) - want) / np.linalg.norm(want))


def row_errors(model, k, alpha, Y):
    """[(row, backward error, relative error)] of the rows of S with a right-hand side, against
    foldin_cg_ref.dense_solutions: the per-row values whose maxima foldin_cg_ref.errors returns (|A| from the eigenvalues;
    the host test holds it to ials_ref.backward_error)."""
    out = []
    for u, (A, b, y, _, norm) in ref.dense_solutions(model, k, alpha, COLS, S).items():
        if b.any():
            yu = np.asarray(Y[u], np.float64)
            be = float(np.linalg.norm(A @ yu - b) / (norm * np.linalg.norm(yu) + np.linalg.norm(b)))
            out.append((u, be, rel_error(yu, y)))
    return out


def converged(model, k, alpha, Y, cnt, what):
    """Check 1 on rows Y with counts cnt of the converged setup: (per-row errors, misses).  Every live row: backward error
    <= 3e-5, relative error <= 1e-3 (both against the dense system; the gate of 1e3 is asserted to skip no row), a count in
    [1, 64); a row without a right-hand side: exactly zero, count 0."""
    what = what + (NAMES[(model, alpha)], k)
    Y, cnt = np.asarray(Y), np.asarray(cnt)
    if not np.isfinite(Y).all():
        return [], [what + ("not finite",)]
    rel, be, cn = _errors(model, k, alpha, Y)
    errs = row_errors(model, k, alpha, Y)
    assert max(e[2] for e in errs) == rel and max(e[1] for e in errs) == be  # the same figures, row by row
    misses = [what + ("condition number", cn)] if not cn <= MAX_COND else []
    live = live_rows(model, k, alpha)
    for u, b_, r_ in errs:
        if not b_ <= MAX_BACKWARD:
            misses.append(what + (u, "backward error", b_))
        if not r_ <= MAX_REL:
            misses.append(what + (u, "relative error", r_))
    for u in range(len(S)):
        if u in live:
            if not 1 <= cnt[u] < STEPS:
                misses.append(what + (u, "count", int(cnt[u])))
        elif cnt[u] != 0 or np.any(Y[u]):
            misses.append(what + (u, "a row without a right-hand side is not zero after 0 steps", int(cnt[u])))
    return errs, misses


def _errors(model, k, alpha, Y):
    """foldin_cg_ref.errors, whose assertion on the rows without a right-hand side is converged()'s own finding"""
    Y = np.array(Y, np.float64)
    live = live_rows(model, k, alpha)
    Y[[u for u in range(len(S)) if u not in live]] = 0
    return ref.errors(model, k, alpha, Y, COLS, S)


def method_check(model, k, alpha, warm, steps, Y, cnt, what):
    """Check 2 on the rows after `steps` steps at tol = 0: (per-row errors (row, None, relative error to the fp64 method),
    misses).  Every live row within 1e-3 of foldin_cg_ref.rows with 1 <= count <= steps (fp32 may reach gamma = 0 a step
    before fp64); from a cold start a row of n entries with n + 1 <= steps within 1e-3 of the dense solve (the rule that sees
    a wrong preconditioner); the other rows exactly zero, count 0."""
    what = what + (NAMES[(model, alpha)], k, "W0" if warm else "zero", steps)
    Y, cnt = np.asarray(Y), np.asarray(cnt)
    if not np.isfinite(Y).all():
        return [], [what + ("not finite",)]
    want, _ = method(model, k, alpha, warm, steps, 0.0)
    live, sol = live_rows(model, k, alpha), ref.dense_solutions(model, k, alpha, COLS, S)
    errs, misses = [], []
    for u, n in enumerate(S):
        if u not in live:
            if cnt[u] != 0 or np.any(Y[u]):
                misses.append(what + (u, "a row without a right-hand side is not zero after 0 steps", int(cnt[u])))
            continue
        r_ = rel_error(Y[u], want[u])
        errs.append((u, None, r_))
        if not r_ <= MAX_REL:
            misses.append(what + (u, "distance to the fp64 method", r_))
        if not 1 <= cnt[u] <= steps:
            misses.append(what + (u, "count", int(cnt[u])))
        if not warm and n + 1 <= steps:
            d_ = rel_error(Y[u], sol[u][2])
            errs.append((u, None, d_))
            if not d_ <= MAX_REL:
                misses.append(what + (u, "n + 1 steps: distance to the dense solve", d_))
    return errs, misses


def target_check(model, k, alpha, Z, W, steps, what):
    """Check 4 on Z [12][T][k] (W [12][k]: the rows of the same call): ((relative, backward, split gap, condition), misses)
    by explain_cg_ref.errors: one dense factorisation per row for all targets, the bounds of check 1, counts in [1, 64) on
    the live pairs, exact zeros and count 0 on the others."""
    what = what + (NAMES[(model, alpha)], k)
    Z, steps = np.asarray(Z), np.asarray(steps)
    if not np.isfinite(Z).all():
        return None, [what + ("not finite",)]
    tg = targets(k)
    rel, be, gap, cn = xr.errors(model, k, alpha, tg, Z, W, data(k)[3], COLS, S)
    live = xr.live_pairs(model, k, alpha, tg, COLS, S)
    misses = []
    for name, v, bound in (("relative error", rel, MAX_REL), ("backward error", be, MAX_BACKWARD), ("split gap", gap, MAX_BACKWARD),
                           ("condition number", cn, MAX_COND)):
        if not v <= bound:
            misses.append(what + (name, v))
    if not ((steps[live] >= 1).all() and (steps[live] < STEPS).all()):
        misses.append(what + ("count", steps[live].min(), steps[live].max()))
    if steps[~live].any() or Z[~live].any():
        misses.append(what + ("a pair without a system is not zero after 0 steps",))
    return (rel, be, gap, cn), misses


class Worst(sw.Worst):
    """solve_sweep.Worst with the lines of this sweep: `cgsweep-measured` / `cgsweep-detail`."""

    def line(self, family, lo, hi):
        return sw.Worst.line(self, family, lo, hi).replace("sweep-measured", "cgsweep-measured").replace("sweep-detail", "cgsweep-detail")


# ------------------------------------------------------------------------------------------------ controls
def lost_entry(model, k, alpha, u):
    """Row u of S solved in fp64 with one counting entry lost from its sums (solve_sweep.dropped_entry's choice: the first
    from the middle on, here with a right-hand-side weight), the diagonal keeping the row's true count."""
    ptr, idx, _, H, _ = data(k)
    val = values(model, k)
    lo, hi = int(ptr[u]), int(ptr[u + 1])
    q = next(q for q in list(range(lo + (hi - lo) // 2, hi)) + list(range(lo, lo + (hi - lo) // 2)) if (val[q] > 0 if model == IMPLICIT else val[q] != 0))
    A, b, _, _, _ = ref.dense_solutions(model, k, alpha, COLS, S)[u]
    x, r = H[int(idx[q])].astype(np.float64), np.float32(val[q])
    if model == IMPLICIT:
        w = float(ials_ref.weights(r, alpha))
        return np.linalg.solve(A - w * np.outer(x, x), b - (1.0 + w) * x)
    return np.linalg.solve(A - np.outer(x, x), b - float(r) * x)


def swap_last_two(Y):
    """Every row with its last two coordinates exchanged (k >= 2)."""
    out = np.array(Y, np.float64)
    out[..., [-1, -2]] = out[..., [-2, -1]]
    return out


def lost_column_of_minv(k):
    """(G, G^-1 with its last row and column zeroed): a lost column of k_foldcg_dense or of the device inverse."""
    G, Ginv = base_pair(k)
    bad = Ginv.copy()
    bad[-1, :] = 0
    bad[:, -1] = 0
    return G, bad


def lost_coordinate_of_gp(k):
    """(G with its last row zeroed, G^-1): G p with its last coordinate lost."""
    G, Ginv = base_pair(k)
    bad = G.copy()
    bad[-1, :] = 0
    return bad, Ginv


def neighbours_target(Z, t=3):
    """Z with target t of every row answered with the solve of target t + 1."""
    out = np.array(Z, np.float64)
    out[:, t] = out[:, t + 1]
    return out
