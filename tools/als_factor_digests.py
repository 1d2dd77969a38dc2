"""sha256 digests of the factors after a few iterations of every resident ALS solver, as one JSON line: what two builds of
libmfx.so must agree on bit for bit when a change claims to move no arithmetic.  Run it once per library (MFX_LIB_PATH
names the one to load, a fresh process each) and compare the lines.

Input: an 8000 x 8000 matrix whose rows 0..13 are the segments of set S of tests/solve_sweep.py (unsplit, split in two and
in three) and whose other rows hold 0 .. 250 entries; lambda 0.1, alpha 1, the _reg runs alpha0 = 0.5, nu = 0.5.
Runs: explicit ALS k = 64 and 100, implicit ALS k = 64 plain / reg / block / block-reg (blocks of 32), three iterations
each; explicit ALS by block sweeps k = 160, d = 64, one iteration.

    MFX_LIB_PATH=/path/to/libmfx.so python tools/als_factor_digests.py
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-recommender_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mfx
import solve_sweep as sw

N = sw.NROWS
small = [0, 1, 2, 3, 15, 16, 17, 33, 250]
sizes = list(sw.S) + [small[i % len(small)] for i in range(N - len(sw.S))]
ptr, idx, val = sw.segments(100 + 64, N, sizes)
rows = np.repeat(np.arange(N), np.diff(ptr.astype(np.int64)))
d = mfx.dataset.from_coo(N, N, rows, idx.astype(np.int64), val)
dg = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
out = {"library": mfx.LIB_PATH, "nnz": int(idx.size), "cases": {}}

def run(name, make, k, iters):
    p = mfx.parameter()
    p.k, p.lambda_ = k, sw.LAM
    s = make(p)
    s.set_factors(mfx.initial_col(N, k))
    s.iterate(iters)
    W, H = s.get_factors()
    s.close()
    assert np.isfinite(W).all() and np.isfinite(H).all(), name
    out["cases"][name] = {"W": dg(W), "H": dg(H), "absmax": float(max(np.abs(W).max(), np.abs(H).max()))}

T = mfx.test_data_of(d)
run("als_k64", lambda p: mfx.AlsSolver(d, T, p), 64, 3)
run("als_k100", lambda p: mfx.AlsSolver(d, T, p), 100, 3)
run("ials_k64", lambda p: mfx.ImplicitAlsSolver(d, p, 1.0), 64, 3)
run("ials_reg_k64", lambda p: mfx.ImplicitAlsSolver(d, p, 1.0, alpha0=0.5, nu=0.5), 64, 3)
run("ials_block_k64_d32", lambda p: mfx.ImplicitAlsSolver(d, p, 1.0, block=32), 64, 3)
run("ials_block_reg_k64_d32", lambda p: mfx.ImplicitAlsSolver(d, p, 1.0, block=32, alpha0=0.5, nu=0.5), 64, 3)
run("als_block_k160_d64", lambda p: mfx.AlsSolver(d, T, p, block=64), 160, 1)
print(json.dumps(out))
