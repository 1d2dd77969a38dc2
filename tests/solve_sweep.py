"""Inputs, dispatch mirror, fp64 references, metrics and controls of the per-rank solve sweep (host only; used by
tests/test_solve_sweep_host.py and tests/test_gpu_solve_sweep.py).

Inputs, for a rank k: X = standard_normal((8000, k), seed k) / sqrt(k) as fp32, segments of distinct sorted rows with
values 1..5 and 15 % explicit zeros (seed 100 + k), lambda = 0.1.  Two size sets:
    S: 14 segments, 10 579 entries, 17 work items, mean 622: the short class, segments unsplit, split in two and in three
    L:  5 segments, 16 385 entries, 10 work items, mean 1 638: the long class, segments unsplit, split in two and in four

Dispatch mirror: work_items / launch_class restate AlsHalf::build (csrc/als_host.hip) and launch_half (csrc/als_solver.hip); the constants
they rest on are read from the sources by dispatch_constants() and asserted, so a change in the dispatcher breaks the
mirror loudly instead of silently moving a rank to another kernel.

References: every segment's system (A, b) in fp64 with its solution and condition number, per family parameter:
    ("explicit", reg): alsb_ref.dense_system, rho = lambda (reg 0) or fp32(lambda) * fp32(n) (reg 1)
    ("implicit", alpha): the system of ials_ref.dense_system, formed as X^T X + lambda I + sum_j w_j x_j x_j^T with X^T X
    built once per k (test_solve_sweep_host.py compares it with ials_ref.dense_system itself)
Cached per (k, set, parameter); nothing returned from a cache may be written to.

Controls: fp32_solve (numpy Cholesky in fp32 on the fp32 Gramian, fp32 substitutions) shows what an honest fp32 solver
reaches; drop_one and swap_last_two are wrong answers that the bounds must refuse."""
import functools
import os
import re

import numpy as np

import alsb_ref
import ials_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-recommender_amd", "csrc")

NROWS = 8000
LAM = 0.1
S = [0, 1, 2, 3, 15, 16, 17, 33, 250, 2047, 2048, 2049, 4097, 1]
L = [2048, 2049, 6145, 2047, 4096]
SETS = {"S": S, "L": L}
RANGES = [(lo, lo + 15) for lo in range(1, 129, 16)]  # eight rank ranges of 16
MAX_BACKWARD, MAX_REL, MAX_COND = 3e-5, 1e-3, 1e3     # the bounds and the gate of test_gpu_ials.py / test_gpu_alsb.py
EXPLICIT = (("explicit", 0), ("explicit", 1))
IMPLICIT = (("implicit", 0.0), ("implicit", 1.0), ("implicit", 40.0))
CLASSES = ("N1", "G16 short", "G16 long", "G16 short-64", "G16 long-64", "N2", "N3", "N4")


def segments(seed, nrows_x, sizes, zero_frac=0.15):
    """CSR-like segments of the given sizes over distinct rows of X, strengths 1..5 with explicit zeros."""
    rng = np.random.default_rng(seed)
    ptr = np.zeros(len(sizes) + 1, np.uint32)
    ptr[1:] = np.cumsum(sizes)
    idx = np.concatenate([np.sort(rng.choice(nrows_x, n, replace=False)) for n in sizes]).astype(np.uint32)
    val = rng.integers(1, 6, idx.size).astype(np.float32)
    val[rng.random(idx.size) < zero_frac] = 0.0
    return ptr, idx, val


# ------------------------------------------------------------------------------------------------ dispatch mirror
@functools.lru_cache(maxsize=None)
def dispatch_constants():
    """(chunk, long_mean) = (kAlsChunk, the mean entries per work item from which k_als_gram16 runs its long form), read
    from the sources; the rank conditions of launch_half and the split rule of AlsHalf::build are asserted as they stand."""
    with open(os.path.join(CSRC, "als_solver.hpp")) as f:
        hpp = f.read()
    with open(os.path.join(CSRC, "als_solver.hip")) as f:
        hip = f.read()
    with open(os.path.join(CSRC, "als_host.hip")) as f:
        host = f.read()
    chunk = re.findall(r"constexpr\s+uint32_t\s+kAlsChunk\s*=\s*(\d+)\s*;", hpp)
    assert len(chunk) == 1, chunk
    longs = re.findall(r"longs\s*=\s*nnz\s*/\s*nitems\s*>=\s*(\d+)\s*,\s*full\s*=\s*a\.k\s*==\s*(\d+)\s*;", hip)
    assert len(longs) == 1, longs
    g16 = re.findall(r"if\s*\(a\.k\s*>\s*(\d+)\s*&&\s*a\.k\s*<=\s*(\d+)\s*&&\s*a\.k\s*%\s*(\d+)\s*==\s*0\s*&&\s*a\.x_rows\s*<\s*\(1u\s*<<\s*(\d+)\)", hip)
    assert len(g16) == 1, g16
    nt = re.findall(r"const\s+uint32_t\s+nt\s*=\s*\(a\.k\s*\+\s*31\)\s*/\s*32\s*;", hip)
    assert len(nt) == 1, nt
    assert re.search(r"if\s*\(hi\s*-\s*lo\s*<=\s*chunk\)", host) and re.search(r"pieces\s*=\s*\(hi\s*-\s*lo\s*\+\s*chunk\s*-\s*1\)\s*/\s*chunk\s*;", host)
    assert tuple(map(int, g16[0])) == (32, 64, 4, 24) and int(longs[0][1]) == 64, (g16, longs)
    return int(chunk[0]), int(longs[0][0])


def work_items(sizes):
    """One item per segment of at most `chunk` entries (empty ones included), ceil(n / chunk) for a longer one."""
    chunk, _ = dispatch_constants()
    return sum(1 if n <= chunk else -(-n // chunk) for n in sizes)


def is_split(n):
    return n > dispatch_constants()[0]


def launch_class(k, sizes, nrows_x=NROWS):
    """The kernel class launch_half picks for rank (or block width) k on segments of these sizes."""
    _, long_mean = dispatch_constants()
    assert 1 <= k <= 128, k
    if 32 < k <= 64 and k % 4 == 0 and nrows_x < (1 << 24) and (nrows_x + 1) * k * 4 < (1 << 32):
        longs = sum(sizes) // work_items(sizes) >= long_mean
        return "G16 " + ("long" if longs else "short") + ("-64" if k == 64 else "")
    return "N%d" % ((k + 31) // 32)


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=8)
def table(k):
    X = (np.random.default_rng(k).standard_normal((NROWS, k)) / np.sqrt(k)).astype(np.float32)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=8)
def gram(k):
    """X^T X in fp64, once per k."""
    X = table(k).astype(np.float64)
    G = X.T @ X
    G.setflags(write=False)
    return G


@functools.lru_cache(maxsize=16)
def data(k, name):
    """(ptr, idx, val, X) of rank k and size set `name`."""
    out = segments(100 + k, NROWS, SETS[name]) + (table(k),)
    for a in out:
        a.setflags(write=False)
    return out


def start(k, name):
    """Y0 = 0.1 N(0, 1) [segments][k], the warm start of the block steps."""
    return (0.1 * np.random.default_rng(1000 + k).standard_normal((len(SETS[name]), k))).astype(np.float32)


# ------------------------------------------------------------------------------------------------ fp64 references
def cond(A):
    ev = np.linalg.eigvalsh(A)
    return float(ev[-1] / ev[0]) if ev[0] > 0 else float("inf")


def _implicit_system(ptr, idx, val, s, X, G, lam, alpha):
    lo, hi = int(ptr[s]), int(ptr[s + 1])
    v = np.asarray(val[lo:hi], np.float32)
    w, pos = ials_ref.weights(v, alpha), v > 0
    Xj = X[np.asarray(idx[lo:hi], np.int64)][pos].astype(np.float64)
    A = G + lam * np.eye(G.shape[0]) + (Xj * w[pos][:, None]).T @ Xj
    return A, Xj.T @ (1.0 + w[pos])


@functools.lru_cache(maxsize=176)
def systems(k, name, family):
    """Per segment of (k, set): None for an empty one, else (A, b, y, cond) in fp64.  family: ("explicit", reg) or
    ("implicit", alpha)."""
    ptr, idx, val, X = data(k, name)
    kind, p = family
    out = []
    for s, n in enumerate(SETS[name]):
        if n == 0:
            out.append(None)
            continue
        if kind == "explicit":
            A, b = alsb_ref.dense_system(ptr, idx, val, s, X, LAM, p)
        else:
            A, b = _implicit_system(ptr, idx, val, s, X, gram(k), LAM, p)
        out.append((A, b, np.linalg.solve(A, b), cond(A)))
    return tuple(out)


def rhs_is_zero(k, name, s):
    """No non-zero rating in segment s: every family's right-hand side is exactly zero."""
    ptr, _, val, _ = data(k, name)
    return not np.any(val[int(ptr[s]):int(ptr[s + 1])])


# ------------------------------------------------------------------------------------------------ metrics
def rel_error(y_got, y_ref):
    return float(np.linalg.norm(np.asarray(y_got, np.float64) - y_ref) / max(np.linalg.norm(y_ref), 1e-30))


def segment_errors(Y, k, name, family):
    """[(s, backward error, relative error)] of the non-empty segments of Y [segments][k] against systems(k, name, family).
    Asserts the exact zeros: empty segments, and segments whose right-hand side is exactly zero (no non-zero rating: every
    solve, a one-block step from any start included, then forms b = 0 exactly and substitutes zeros)."""
    out = []
    for s, ref in enumerate(systems(k, name, family)):
        if ref is None:
            assert not np.any(Y[s]), (family, k, name, s, "empty segment")
            continue
        A, b, y, _ = ref
        if rhs_is_zero(k, name, s):
            assert not np.any(b) and not np.any(y), (family, k, name, s)
            assert not np.any(Y[s]), (family, k, name, s, "right-hand side exactly zero")
            out.append((s, 0.0, 0.0))
            continue
        out.append((s, ials_ref.backward_error(A, Y[s], b), rel_error(Y[s], y)))
    return out


def sweep_errors(Y, Yr, name):
    """[(s, None, relative error)] of a block sweep Y against its fp64 reference Yr; empty segments exactly zero."""
    out = []
    for s, n in enumerate(SETS[name]):
        if n == 0:
            assert not np.any(Y[s]) and not np.any(Yr[s]), (name, s)
            continue
        out.append((s, None, rel_error(Y[s], Yr[s])))
    return out


class Worst:
    """Running maxima of one family over a rank range, with the (rank, set, segment) where they occurred."""

    def __init__(self):
        self.backward, self.rel, self.misses, self.parts = (0.0, None), (0.0, None), [], {}

    def add(self, k, name, errors, part=None):
        """part: a label (a start, an alpha, ...) whose own maxima are kept too, for the `sweep-detail` lines"""
        if part is not None:
            self.parts.setdefault(part, Worst()).add(k, name, errors)
        for s, be, rel in errors:
            if be is not None and be >= self.backward[0]:
                self.backward = (be, (k, name, s))
            if rel is not None and rel >= self.rel[0]:
                self.rel = (rel, (k, name, s))

    def line(self, family, lo, hi):
        return (f"sweep-measured {family} ranks {lo}..{hi} max_backward={self.backward[0]:.3e} {self.backward[1]} "
                f"max_rel={self.rel[0]:.3e} {self.rel[1]}" +
                "".join("\n" + w.line(f"{family} [{part}]", lo, hi).replace("sweep-measured", "sweep-detail") for part, w in self.parts.items()))


def check_bounds(errors, what, backward=True, rel=True):
    """The misses of the project's bounds on every non-empty segment (no segment is left out: test_solve_sweep_host.py
    shows that every condition number is within the gate), as tuples what + (segment, measure, value).  Returned, not
    raised, so that a test can go through all its calls and then assert that the list of all misses is empty."""
    out = []
    for s, be, r in errors:
        if backward and not be <= MAX_BACKWARD:
            out.append(what + (s, "backward error", be))
        if rel and not r <= MAX_REL:
            out.append(what + (s, "relative error", r))
    return out


# ------------------------------------------------------------------------------------------------ controls
def _chol_solve32(A, b):
    Lo = np.linalg.cholesky(A)
    assert Lo.dtype == np.float32 and b.dtype == np.float32
    k = b.shape[0]
    z, y = np.zeros(k, np.float32), np.zeros(k, np.float32)
    for i in range(k):
        z[i] = (b[i] - Lo[i, :i] @ z[:i]) / Lo[i, i]
    for i in range(k - 1, -1, -1):
        y[i] = (z[i] - Lo[i + 1:, i] @ y[i + 1:]) / Lo[i, i]
    return y


def fp32_solve(k, name, family):
    """An honest fp32 solve of every segment: fp32 Gramian, numpy's fp32 Cholesky, fp32 substitutions."""
    ptr, idx, val, X = data(k, name)
    kind, p = family
    eye = np.eye(k, dtype=np.float32)
    Y = np.zeros((len(SETS[name]), k), np.float32)
    G = X.T @ X + np.float32(LAM) * eye if kind == "implicit" else None
    for s, n in enumerate(SETS[name]):
        if n == 0:
            continue
        lo, hi = int(ptr[s]), int(ptr[s + 1])
        Xj, v = X[idx[lo:hi].astype(np.int64)], val[lo:hi]
        if kind == "explicit":
            rho = np.float32(LAM) * np.float32(n) if p else np.float32(LAM)
            A, b = Xj.T @ Xj + rho * eye, Xj.T @ v
        else:
            w = np.float32(p) * v
            A, b = G + (Xj * w[:, None]).T @ Xj, Xj.T @ np.where(v > 0, np.float32(1) + w, np.float32(0))
        assert A.dtype == np.float32 and b.dtype == np.float32
        Y[s] = _chol_solve32(A, b)
    return Y


def dropped_entry(k, name, s):
    """Position (in the entry arrays) of segment s's first entry from the middle on with a non-zero rating, wrapping to
    the segment's start; None if the segment has fewer than two entries or no non-zero rating."""
    ptr, _, val, _ = data(k, name)
    lo, hi = int(ptr[s]), int(ptr[s + 1])
    if hi - lo < 2:
        return None
    order = list(range(lo + (hi - lo) // 2, hi)) + list(range(lo, lo + (hi - lo) // 2))
    return next((q for q in order if val[q] != 0), None)


def drop_one(k, name, family, s):
    """The fp64 solution of segment s's system with one entry lost from its sums (dropped_entry); the diagonal term keeps
    the segment's true count, as a kernel that loses an entry would.  None where dropped_entry is None."""
    q = dropped_entry(k, name, s)
    if q is None:
        return None
    _, idx, val, X = data(k, name)
    A, b, _, _ = systems(k, name, family)[s]
    x, r = X[int(idx[q])].astype(np.float64), np.float32(val[q])
    kind, p = family
    if kind == "explicit":
        return np.linalg.solve(A - np.outer(x, x), b - float(r) * x)
    w = float(ials_ref.weights(r, p))
    return np.linalg.solve(A - w * np.outer(x, x), b - (1.0 + w) * x)


def swap_last_two(y):
    """y with its last two coordinates exchanged (k >= 2)."""
    out = np.array(y, np.float64)
    out[[-1, -2]] = out[[-2, -1]]
    return out
