"""SLIM on kNN supports (mfx_slim_*) at the Netflix and ML-1M shapes: training time by phase, recommendation time, and
item-kNN in the same process as the yardstick.

Builds the synthetic matrix on the GPU (mfx.synth_torch, as bench.py and tools/knn_bench.py do).  For every K of --Ks:
  knn        ItemKnn on the cosine-weighted matrix: the phases of mfx_knn_times (the similarity pass runs the same term
             loops as SLIM's Gram pass);
  train      Slim on the raw values with that ItemKnn as the support, l1 = 1, l2 = 10, 10 sweeps, tol = 0: the phases of
             mfx_slim_times (checks + inverse lists, Gram pass, solve), the sweeps per item, the share of zero weights;
  recommend  the training rows of 1 / 64 / 1 024 / all users at n_top = 10, Slim and ItemKnn side by side: ms per call
             (median of --reps) and the pass alone; the number of terms each adds for all users.
Then the planted clusters of the tests: HR@10 of Slim and of ItemKnn at K = 5 and 20.

With --parent-pkg DIR (a built cuda-recommender_amd tree of the parent commit): the unchanged ItemKnn build and all-user
recommend at K = 20 and the all-user query at k = 64, a fresh process per tree, parent and this tree alternated
--regress-runs times.

    python tools/slim_bench.py [--Ks 20,100] [--parent-pkg DIR] [--regress-runs 4] [--out FILE]
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
from knn_bench import cosine, matrix  # noqa: E402


def timed_recommend(torch, m, q, reps):
    m.recommend(q, 10)
    wall, passes = [], []
    for _ in range(reps):
        t0 = m.times()
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        m.recommend(q, 10)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - w0) * 1e3)
        passes.append((m.times()["recommend_pass"] - t0["recommend_pass"]) * 1e3)
    return round(float(np.median(wall)), 4), round(float(np.median(passes)), 4)


def shape_point(torch, mfx, a, rows, cols, nnz, K, batches):
    d = matrix(torch, rows, cols, nnz)
    dc = cosine(torch, d)
    rec = {"rows": rows, "cols": cols, "nnz": nnz, "K": K, "l1": a.l1, "l2": a.l2, "sweeps": a.sweeps, "tol": 0.0,
           "workspace_bytes": cols * (K + 1) * K * 4}
    nn = mfx.ItemKnn(None, K, None, device_arrays=dc)
    t = nn.times()
    rec["knn_build_seconds"] = {"checks_and_work_order": round(t["build_checks"], 5), "similarity_pass": round(t["build_pass"], 5)}
    m = mfx.Slim(None, K, l1=a.l1, l2=a.l2, sweeps=a.sweeps, tol=0.0, support=nn, device_arrays=d)
    t = m.times()
    rec["train_seconds"] = {"checks_and_inverse_lists": round(t["train_checks"], 5), "gram_pass": round(t["gram_pass"], 5),
                            "solve": round(t["solve"], 5)}
    rec["gram_pass_over_knn_similarity_pass"] = round(t["gram_pass"] / rec["knn_build_seconds"]["similarity_pass"], 3)
    used = m.sweeps_used
    S, w = m.weights()
    real = S != 0xFFFFFFFF
    rec["sweeps_per_item"] = {"mean": round(float(used.mean()), 3), "min": int(used.min()), "max": int(used.max())}
    rec["failed"] = m.failed
    rec["real_slots"] = int(real.sum())
    rec["zero_weights_share"] = round(float((w[real] == 0).mean()), 4)
    ptr = d["csr_row_ptr"].long()
    # the terms of the all-user call: for SLIM the transposed lists of the row's items (a popular item is named by many
    # lists), for item-kNN the real slots of their own lists
    ids = nn.lists()[0]
    per_source = torch.from_numpy(np.bincount(S[real].astype(np.int64), minlength=cols)).to(ptr.device)
    per_item = torch.from_numpy((ids != 0xFFFFFFFF).sum(axis=1)).to(ptr.device)
    ci = d["csr_col_idx"].long()
    rec["terms_all_users"] = {"slim": int(per_source[ci].sum()), "knn": int(per_item[ci].sum()),
                              "longest_transposed_list": int(per_source.max())}
    rec["recommend"] = []
    for n in batches:
        n = min(n, rows)
        z = int(ptr[n])
        q = (d["csr_row_ptr"][:n + 1].contiguous(), d["csr_col_idx"][:z].contiguous(), d["csr_val"][:z].contiguous())
        qc = (q[0], q[1], dc["csr_val"][:z].contiguous())
        ms, ps = timed_recommend(torch, m, q, a.reps)
        kms, kps = timed_recommend(torch, nn, qc, a.reps)
        rec["recommend"].append({"users": n, "entries": z, "slim_ms_per_call": ms, "slim_pass_ms": ps, "slim_bad_rows": m.bad_rows,
                                 "knn_ms_per_call": kms, "knn_pass_ms": kps, "knn_bad_rows": nn.bad_rows})
    m.close()
    nn.close()
    del d, dc
    torch.cuda.empty_cache()
    print(json.dumps(rec), file=sys.stderr, flush=True)
    return rec


def planted(mfx):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bpr_exact as bx
    P = bx.planted_clusters()
    X = mfx.knn_weights(P, "cosine")
    out = []
    for K in (5, 20):
        with mfx.ItemKnn(P, K, "cosine") as nn, mfx.Slim(P, K, l1=1.0, l2=10.0, sweeps=10, support=nn) as m:
            hk = mfx.topn_metrics(nn.recommend(X, 10)[0], P)["hr"]
            hs = mfx.topn_metrics(m.recommend(P, 10)[0], P)["hr"]
        out.append({"K": K, "hr10_item_knn_cosine": round(float(hk), 4), "hr10_slim": round(float(hs), 4)})
    return out


def regress_child(a):
    sys.path.insert(0, a.regress_child)
    import torch
    import mfx
    assert os.path.dirname(os.path.dirname(os.path.abspath(mfx.__file__))) == os.path.abspath(a.regress_child)
    d = cosine(torch, matrix(torch, a.rows, a.cols, a.nnz))
    builds, recs = [], []
    q = (d["csr_row_ptr"], d["csr_col_idx"], d["csr_val"])
    for rep in range(3):
        with mfx.ItemKnn(None, 20, None, device_arrays=d) as nn:
            builds.append(nn.times()["build_pass"] * 1e3)
            for r in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                nn.recommend(q, 10)
                torch.cuda.synchronize()
                if rep or r:
                    recs.append((time.perf_counter() - t0) * 1e3)
    rp, ci = d["csr_row_ptr"].cpu().numpy().view(np.uint32), d["csr_col_idx"].cpu().numpy().view(np.uint32)
    del d, q
    ex = mfx.dataset.RatingData(a.rows, a.cols, rp, ci, np.zeros(0, np.float32), np.zeros(a.cols + 1, np.uint32),
                                np.zeros(0, np.uint32), np.zeros(0, np.float32))
    g = torch.Generator(device="cuda:0")
    g.manual_seed(64)
    W = (torch.randn(a.rows, 64, generator=g, device="cuda:0") * 0.3).contiguous()
    H = (torch.randn(a.cols, 64, generator=g, device="cuda:0") * 0.3).contiguous()
    ts = []
    with mfx.Recommender(W, H, 1, exclude=ex) as r:
        for rep in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r.query(10, on_device=True)
            torch.cuda.synchronize()
            if rep:
                ts.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"knn_build_pass_ms": float(np.median(builds)), "knn_recommend_all_ms": float(np.median(recs)),
                      "query_ms": float(np.median(ts))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=480189)
    ap.add_argument("--cols", type=int, default=17770)
    ap.add_argument("--nnz", type=int, default=99_072_112)
    ap.add_argument("--Ks", default="20,100")
    ap.add_argument("--l1", type=float, default=1.0)
    ap.add_argument("--l2", type=float, default=10.0)
    ap.add_argument("--sweeps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip", default="", help="letters: n = Netflix shape, m = ML-1M shape, p = planted clusters")
    ap.add_argument("--parent-pkg", default=None)
    ap.add_argument("--regress-runs", type=int, default=4)
    ap.add_argument("--regress-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slim_bench.json"))
    a = ap.parse_args()
    if a.regress_child:
        return regress_child(a)
    sys.path.insert(0, PKG)
    import torch
    import mfx
    out = {"tool": "slim_bench", "support": "cosine item-kNN", "values": "raw", "n_top": 10,
           "cus": int(torch.cuda.get_device_properties(0).multi_processor_count), "netflix": [], "ml1m": []}
    Ks = [int(x) for x in a.Ks.split(",") if x]
    if "n" not in a.skip:
        for K in Ks:
            out["netflix"].append(shape_point(torch, mfx, a, a.rows, a.cols, a.nnz, K, (1, 64, 1024, a.rows)))
    if "m" not in a.skip:
        for K in Ks:
            out["ml1m"].append(shape_point(torch, mfx, a, 6040, 3706, 1_000_000, K, (1, 64, 1024, 6040)))
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
        out["regression"] = {"workloads": "ItemKnn build pass and all-user recommend at K = 20 (cosine), all-user query at k = 64, n_top = 10",
                             "parent": runs["parent"], "this": runs["this"]}
        print(json.dumps(out["regression"]), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
