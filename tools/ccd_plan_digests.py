"""sha256 digests of what every CCD++ schedule computes, as one JSON line: what two builds of libmfx.so must agree on bit for
bit when a change claims to move no launch and no arithmetic.  Run it once per library (MFX_LIB_PATH names the one to load, a
fresh process each) and compare the lines.

Cases: those of tests/test_gpu_ccd_plans.py (one per row of the table of schedules in DESIGN.md section 4, T = 1 and 2), each at
the test's shape (600 x 400, 20 000 ratings, k = 3) and at the ML-1M shape (6040 x 3706, 10^6 ratings, k = 8); three outer
iterations in one call, no profiling, graph = 0.  Digests: W, H, both residual copies, the RMSE trace.

    MFX_LIB_PATH=/path/to/libmfx.so python tools/ccd_plan_digests.py
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
import test_gpu_ccd_plans as tp

dg = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
out = {"library": mfx.LIB_PATH, "cases": {}}
shapes = {"test": (tp.make_data(mfx), tp.K), "ml1m": (tp.make_data(mfx, 6040, 3706, 1_000_000), 8)}
for shape, (d, k) in shapes.items():
    for case in tp.CASES:
        for T in (1, 2):
            tp.set_env(os.environ.__setitem__, lambda n: os.environ.pop(n, None), case[2])
            (W, H, csc, csr, rmse), _ = tp.solve(mfx, d, case, k, T, 0, (tp.N,))
            assert np.isfinite(W).all() and np.isfinite(H).all(), (shape, case[0], T)
            out["cases"][f"{shape}/{case[0]}/T{T}"] = {"W": dg(W), "H": dg(H), "csc": dg(csc), "csr": dg(csr), "rmse": dg(rmse),
                                                      "rmse_last": float(rmse[-1])}
print(json.dumps(out))
