"""EASE (mfx_ease_*) at the Netflix and ML-1M shapes: training time by phase, the two schedules of the inverse side by side
with torch's inverses, the recommendation against a dense torch product, and the accuracy of the inverse.

Builds the synthetic matrix on the GPU (mfx.synth_torch, as bench.py and tools/knn_bench.py do).  Per shape:
  knn        ItemKnn at K = 20 on the same raw values: its similarity pass runs the term loops of the Gram pass;
  train      Ease at --lam: the phases of mfx_ease_times (checks, Gram pass, inverse, weights);
  inverse    mfx_ease_inverse on the library's G, grouped and simple alternated --inv-reps times in this process, and
             torch.linalg.inv and torch.cholesky_inverse (fp32) as the outside yardstick; whether the two schedules agree in
             bits; the fp64 residual |G P[:, c] - e_c|_2 on 64 sampled columns for the library and for torch.linalg.inv;
  recommend  the training rows of 1 / 64 / 1 024 / all users at n_top = 10: ms per call and the pass alone, next to torch
             dense X_batch @ B + mask + topk (in chunks of 4 096 users).
Then the planted clusters of the tests: HR@10 at lambda = 100.

With --parent-pkg DIR (a built cuda-recommender_amd tree of the parent commit): the unchanged ItemKnn build at K = 20 and Slim
train at K = 20, a fresh process per tree, parent and this tree alternated --regress-runs times.

    python tools/ease_bench.py [--lam 500] [--skip nmp] [--parent-pkg DIR] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cuda-recommender_amd")
sys.path.insert(0, os.path.join(ROOT, "tools"))
from knn_bench import matrix  # noqa: E402


def wall(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def timed_recommend(torch, m, q, reps):
    m.recommend(q, 10)
    ws, ps = [], []
    for _ in range(reps):
        t0 = m.times()["recommend_pass"]
        w, _ = wall(torch, lambda: m.recommend(q, 10))
        ws.append(w)
        ps.append((m.times()["recommend_pass"] - t0) * 1e3)
    return round(float(np.median(ws)), 4), round(float(np.median(ps)), 4)


def torch_recommend(torch, B, q, cols, chunk=4096):
    """Dense scores of the rows q = (ptr, idx, val) against B, the rows' own items masked, top 10: ms."""
    ptr, idx, val = q[0].long(), q[1].long(), q[2]
    n = ptr.numel() - 1

    def run():
        out = []
        for lo in range(0, n, chunk):
            hi = min(lo + chunk, n)
            a, b = int(ptr[lo]), int(ptr[hi])
            r = torch.repeat_interleave(torch.arange(hi - lo, device=B.device), ptr[lo + 1:hi + 1] - ptr[lo:hi])
            X = torch.zeros((hi - lo, cols), device=B.device)
            X[r, idx[a:b]] = val[a:b]
            S = X @ B
            S[r, idx[a:b]] = float("-inf")
            out.append(torch.topk(S, 10, dim=1).indices)
        return out
    run()
    return round(wall(torch, run)[0], 4)


def residuals(torch, G, P, cs):
    e = torch.zeros((G.shape[0], len(cs)), dtype=torch.float64, device=G.device)
    e[cs, torch.arange(len(cs), device=G.device)] = 1.0
    r = (G.double() @ P[:, cs].double() - e).norm(dim=0)
    return {"max": float(r.max()), "median": float(r.median())}


def shape_point(torch, mfx, a, rows, cols, nnz, batches):
    d = matrix(torch, rows, cols, nnz)
    rec = {"rows": rows, "cols": cols, "nnz": nnz, "lambda": a.lam}
    with mfx.ItemKnn(None, 20, None, device_arrays=d) as nn:
        t = nn.times()
        rec["knn_build_seconds"] = {"checks_and_work_order": round(t["build_checks"], 5), "similarity_pass": round(t["build_pass"], 5)}
    m = mfx.Ease(None, a.lam, device_arrays=d)
    t = m.times()
    rec["train_seconds"] = {k: round(t[k], 5) for k in ("train_checks", "gram_pass", "inverse", "weights")}
    rec["gram_pass_over_knn_similarity_pass"] = round(t["gram_pass"] / rec["knn_build_seconds"]["similarity_pass"], 3)
    ptr = d["csr_row_ptr"].long()
    rec["recommend"] = []
    Bt = torch.from_numpy(m.weights()).cuda()
    for n in batches:
        n = min(n, rows)
        z = int(ptr[n])
        q = (d["csr_row_ptr"][:n + 1].contiguous(), d["csr_col_idx"][:z].contiguous(), d["csr_val"][:z].contiguous())
        ms, ps = timed_recommend(torch, m, q, a.reps if n < rows else 1)
        rec["recommend"].append({"users": n, "entries": z, "ease_ms_per_call": ms, "ease_pass_ms": ps, "bad_rows": m.bad_rows,
                                 "row_read_bytes": z * cols * 4, "torch_dense_topk_ms": torch_recommend(torch, Bt, q, cols)})
    m.close()
    del Bt
    G = mfx.ease_gram(None, a.lam, device_arrays=d)
    del d
    torch.cuda.empty_cache()
    inv = {"grouped_ms": [], "simple_ms": []}
    for _ in range(a.inv_reps):
        w, Pg = wall(torch, lambda: mfx.ease_inverse(G))
        inv["grouped_ms"].append(round(w, 2))
        w, Ps = wall(torch, lambda: mfx.ease_inverse(G, simple=True))
        inv["simple_ms"].append(round(w, 2))
    inv["same_bits"] = bool(torch.equal(Pg.view(torch.int32), Ps.view(torch.int32)))
    del Ps
    cs = torch.from_numpy(np.random.default_rng(1).choice(cols, 64, replace=False)).cuda()
    inv["fp64_residual_64_columns"] = {"ease_inverse": residuals(torch, G, Pg, cs)}
    print(json.dumps({"train_seconds": rec["train_seconds"], "inverse": inv}), file=sys.stderr, flush=True)
    torch.cuda.empty_cache()
    for name, fn in (("torch_linalg_inv", lambda: torch.linalg.inv(G)), ("torch_cholesky_inverse", lambda: torch.cholesky_inverse(torch.linalg.cholesky(G)))):
        try:  # the outside yardstick: a failure of torch's own (its BLAS workspace) is recorded, not fatal
            fn()
            ms, Pt = min((wall(torch, fn) for _ in range(2)), key=lambda r: r[0])
            inv[name + "_ms"] = round(ms, 2)
            inv["fp64_residual_64_columns"][name] = residuals(torch, G, Pt, cs)
            del Pt
        except RuntimeError as e:
            inv[name + "_ms"] = None
            inv[name + "_error"] = str(e).splitlines()[0][:200]
        torch.cuda.empty_cache()
    rec["inverse"] = inv
    del G, Pg
    torch.cuda.empty_cache()
    print(json.dumps(rec), file=sys.stderr, flush=True)
    return rec


def planted(mfx):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bpr_exact as bx
    P = bx.planted_clusters()
    with mfx.Ease(P, 100.0) as m:
        return {"lambda": 100.0, "hr10_ease": round(float(mfx.topn_metrics(m.recommend(P, 10)[0], P)["hr"]), 4)}


def regress_child(a):
    sys.path.insert(0, a.regress_child)
    import torch
    import mfx
    assert os.path.dirname(os.path.dirname(os.path.abspath(mfx.__file__))) == os.path.abspath(a.regress_child)
    d = matrix(torch, a.rows, a.cols, a.nnz)
    builds, grams, solves = [], [], []
    for _ in range(3):
        with mfx.ItemKnn(None, 20, None, device_arrays=d) as nn:
            builds.append(nn.times()["build_pass"] * 1e3)
            with mfx.Slim(None, 20, support=nn, device_arrays=d) as s:
                grams.append(s.times()["gram_pass"] * 1e3)
                solves.append(s.times()["solve"] * 1e3)
    print(json.dumps({"knn_build_pass_ms": float(np.median(builds)),
                      "slim_gram_pass_ms": float(np.median(grams)), "slim_solve_ms": float(np.median(solves))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=480189)
    ap.add_argument("--cols", type=int, default=17770)
    ap.add_argument("--nnz", type=int, default=99_072_112)
    ap.add_argument("--lam", type=float, default=500.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inv-reps", type=int, default=2)
    ap.add_argument("--skip", default="", help="letters: n = Netflix shape, m = ML-1M shape, p = planted clusters")
    ap.add_argument("--parent-pkg", default=None)
    ap.add_argument("--regress-runs", type=int, default=4)
    ap.add_argument("--regress-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ease_bench.json"))
    a = ap.parse_args()
    if a.regress_child:
        return regress_child(a)
    sys.path.insert(0, PKG)
    import torch
    import mfx
    out = {"tool": "ease_bench", "values": "raw", "n_top": 10, "cus": int(torch.cuda.get_device_properties(0).multi_processor_count)}
    if "n" not in a.skip:
        out["netflix"] = shape_point(torch, mfx, a, a.rows, a.cols, a.nnz, (1, 64, 1024, a.rows))
    if "m" not in a.skip:
        out["ml1m"] = shape_point(torch, mfx, a, 6040, 3706, 1_000_000, (1, 64, 1024, 6040))
    if "p" not in a.skip:
        out["planted_clusters"] = planted(mfx)
    if a.parent_pkg:
        runs = {"parent": [], "this": []}
        for _ in range(a.regress_runs):
            for name, pkg in (("parent", os.path.abspath(a.parent_pkg)), ("this", PKG)):
                cmd = [sys.executable, os.path.abspath(__file__), "--regress-child", pkg, "--rows", str(a.rows), "--cols", str(a.cols),
                       "--nnz", str(a.nnz)]
                p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True, timeout=300)
                runs[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
        out["regression"] = {"workloads": "ItemKnn build pass and Slim train (Gram pass, solve) at K = 20, raw values", **runs}
        print(json.dumps(out["regression"]), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
