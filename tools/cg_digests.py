"""sha256 digests of what the conjugate-gradient method computes for fold-in, explanation and training, as one JSON line: what
two builds of libmfx.so must agree on bit for bit when a change claims to move no arithmetic of that method.  Run it once per
library (MFX_LIB_PATH names the one to load, a fresh process each) and compare the lines.

Cases (inputs of tests/foldin_cg_ref.py and tests/explain_cg_ref.py, lambda = 0.1):
    foldin/k/model/steps:tol/start   W and the row steps of Recommender.fold_in after fold_in_cg_setup, k in 37, 64, 130, 256, 1024;
                                     implicit at alpha 0 and 40, ALS and CCD on explicit_values; cold and from W0; (64, 1e-4), (6, 0)
    explain/k/model/steps:tol/slot   Z, target_steps, totals, items, contrib of Recommender.explain_cg, k in 64, 130, 256, 1024;
                                     implicit at alpha 40 and ALS; the 5 targets of explain_cg_ref.targets and a slot of 64
                                     (tests/test_gpu_explain_cg.py, test_a_pair_does_not_depend_on_its_batch)
    train                            two iterations of ImplicitAlsSolver(cg=(8, 1e-4)), 600 x 400, k = 130: W, H, cg_stats
    ten-chunks/...                   a row of ten chunks, an empty row and a short one over 30000 columns, k = 256, implicit
                                     at alpha 40: fold-in as above, explanation with 5 and with 17 targets

    MFX_LIB_PATH=/path/to/libmfx.so python tools/cg_digests.py
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
import explain_cg_ref as xr
import foldin_cg_ref as ref
from test_gpu_ials import _params, _random_matrix

F32 = np.float32
dg = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
MODELS = [("implicit0", ref.IMPLICIT, 0.0), ("implicit40", ref.IMPLICIT, 40.0), ("als", ref.ALS, 0.0), ("ccd", ref.CCD, 0.0)]
RULES = [(64, 1e-4), (6, 0.0)]
TEN_CHUNKS = (30000, (20000, 0, 5))
PAIR_KEYS = ("Z", "target_steps", "totals", "items", "contrib")
out = {"library": os.path.relpath(mfx.LIB_PATH, ROOT), "cases": {}}


def wide_slot(tg, cols):
    """The 64-wide slot of test_a_pair_does_not_depend_on_its_batch: the row's targets among drawn ones and a padding."""
    rng = np.random.default_rng(5)
    wide = rng.integers(0, cols, (tg.shape[0], 64)).astype(np.uint32)
    wide[:, 7] = xr.PAD
    wide[:, [63, 17, 40, 5, 0]] = tg
    return wide


def run(tag, k, cols, sizes, models, explain_models, slots):
    ptr, idx, val, H, W0 = ref.inputs(k, cols, sizes)
    with mfx.Recommender(np.zeros((1, k), F32), H, 1) as r:
        for name, model, alpha in models:
            v = val if model == ref.IMPLICIT else ref.explicit_values(val)
            for steps, tol in RULES:
                r.fold_in_cg_setup(model, ref.LAM, alpha, steps=steps, tol=tol)
                for start, W_init in (("cold", None), ("warm", W0)):
                    _, _, W, cnt = r.fold_in((ptr, idx, v), W_init=W_init, return_sweeps=True)
                    out["cases"][f"{tag}foldin/{k}/{name}/{steps}:{tol}/{start}"] = {"W": dg(W), "row_steps": dg(cnt), "steps": int(cnt.sum())}
                if name in explain_models:
                    for slot, tg in slots.items():
                        e = r.explain_cg((ptr, idx, v), tg, n_expl=3, return_W=True, return_Z=True, return_steps=True)
                        d = {key: dg(e[key]) for key in PAIR_KEYS}
                        d["steps"] = int(e["target_steps"].sum())
                        out["cases"][f"{tag}explain/{k}/{name}/{steps}:{tol}/{slot}"] = d


for k in (37, 64, 130, 256, 1024):
    tg = xr.targets(k)
    run("", k, ref.COLS, tuple(ref.SIZES), MODELS, ("implicit40", "als") if k >= 64 else (), {"T5": tg, "T64": wide_slot(tg, ref.COLS)})

cols, sizes = TEN_CHUNKS
tg = xr.targets(256, cols, sizes)
tg17 = np.random.default_rng(11).integers(0, cols, (len(sizes), 17)).astype(np.uint32)
run("ten-chunks/", 256, cols, sizes, MODELS[1:2], ("implicit40",), {"T5": tg, "T17": tg17})

R = _random_matrix(5, rows=600, cols=400, density=0.05)
k = 130
s = mfx.ImplicitAlsSolver(R, _params(mfx, k, 0.1), 2.0, cg=(8, 1e-4))
s.set_factors((np.random.default_rng(k).standard_normal((R.cols, k)) * 0.1).astype(F32), None)
s.iterate(2)
W, H = s.get_factors()
out["cases"]["train"] = {"W": dg(W), "H": dg(H), "cg_stats": json.dumps(s.cg_stats(), sort_keys=True, default=int)}
s.close()
print(json.dumps(out))
