"""IVF retrieval (mfx_rec_ivf_setup, mfx_rec_query_ivf) next to the full query on the same handle.

Three cases, N = 10, no exclusion, factors made on the device:
  (a) 10^6 items, k = 128, items and users drawn from a mixture of 1,024 Gaussians, nlist = 1,024;
  (b) 10^6 items, k = 128, i.i.d. Gaussian factors (no cluster structure: the unflattering case), nlist = 1,024;
  (c) the Netflix shape, 480,189 x 17,770, k = 64, Gaussian factors, nlist = 128 (IVF is not expected to pay here).
Per case the ivf_build time (ivf_kmeans on the device + mfx_rec_ivf_setup), and for 1 / 64 / 1,024 users (and all users
for (c)) and nprobe in 1, 4, 16, 64: the time of query_ivf with its four phases (mfx_rec_ivf_times), the time of query
for the same users, and recall@10 against query (the mean over the batch of the share of query's items that query_ivf
returns).  Writes ONE JSON record (--out).  With --parent-pkg DIR (a built cuda-recommender_amd tree of the parent commit):
the unchanged all-user query at k = 64 and query_candidates for all users x 100 candidates on that tree and on this one,
alternated, --regress-runs fresh processes each.

    python tools/ivf_bench.py [--reps 5] [--cases a,b,c] [--iters 10] [--parent-pkg DIR] [--regress-runs 4] [--out FILE]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from candidates_bench import gen_lists  # noqa: E402
from rank_bench import exclusion, factors, timed  # noqa: E402  (the same data and timer as the rank and candidates records)

N_TOP = 10
CASES = {
    "a": dict(rows=1024, cols=1_000_000, k=128, nlist=1024, mixture=1024, what="mixture of 1024 Gaussians"),
    "b": dict(rows=1024, cols=1_000_000, k=128, nlist=1024, mixture=0, what="i.i.d. Gaussian"),
    "c": dict(rows=480189, cols=17770, k=64, nlist=128, mixture=0, what="Netflix shape, i.i.d. Gaussian"),
}


def make_factors(torch, c, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(c["k"] + c["mixture"])
    if not c["mixture"]:
        W = torch.randn(c["rows"], c["k"], generator=g, device=dev) * 0.3
        H = torch.randn(c["cols"], c["k"], generator=g, device=dev) * 0.3
        return W.contiguous(), H.contiguous()
    centres = torch.randn(c["mixture"], c["k"], generator=g, device=dev) * 0.3
    pick = lambda n: torch.randint(0, c["mixture"], (n,), generator=g, device=dev)
    W = centres[pick(c["rows"])] + 0.1 * torch.randn(c["rows"], c["k"], generator=g, device=dev)
    H = centres[pick(c["cols"])] + 0.1 * torch.randn(c["cols"], c["k"], generator=g, device=dev)
    return W.contiguous(), H.contiguous()


def recall(torch, got, want):
    """The share of want's items (padding aside) that got holds, the mean over the slots."""
    g, w = got.long(), want.long()
    hit = (w[:, :, None] == g[:, None, :]).any(2) & (w != 0xFFFFFFFF) & (w != -1)
    n = ((w != 0xFFFFFFFF) & (w != -1)).sum(1).clamp(min=1)
    return float((hit.sum(1).float() / n.float()).mean())


def run_case(torch, mfx, name, c, a):
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    W, H = make_factors(torch, c, dev)
    sync()
    out = dict(c, case=name, points=[])
    rng = np.random.default_rng(23)
    with mfx.Recommender(W, H, 1) as r:
        sync()
        t0 = time.perf_counter()
        assign, _ = r.ivf_build(H, c["nlist"], iters=a.iters, seed=0)
        sync()
        out["ivf_build_ms"] = (time.perf_counter() - t0) * 1e3
        sizes = torch.bincount(assign.long(), minlength=c["nlist"])
        out["list_sizes"] = {"min": int(sizes.min()), "median": int(sizes.median()), "max": int(sizes.max()), "empty": int((sizes == 0).sum())}
        batches = [1, 64, 1024] + ([c["rows"]] if name == "c" else [])
        for B in batches:
            u = np.arange(c["rows"]) if B == c["rows"] else np.sort(rng.choice(c["rows"], B, replace=False))
            users = torch.from_numpy(u.astype(np.uint32).view(np.int32)).to(dev)
            full = {}

            def run_full():
                full["items"] = r.query(N_TOP, users=users)[0]
            tq = timed(run_full, a.reps, sync)
            for nprobe in (1, 4, 16, 64):
                if nprobe > c["nlist"]:
                    continue
                got = {}

                def run():
                    got["items"] = r.query_ivf(N_TOP, nprobe, users=users)[0]
                t = timed(run, a.reps, sync, r.ivf_times)
                p = {"batch": B, "nprobe": nprobe, "query_ivf": t, "query": tq, "ivf_over_query": t["median_ms"] / tq["median_ms"]}
                rec = [recall(torch, got["items"][i0:i0 + 65536], full["items"][i0:i0 + 65536]) * min(65536, B - i0) for i0 in range(0, B, 65536)]
                p["recall_at_10"] = sum(rec) / B
                out["points"].append(p)
                print(json.dumps(p), file=sys.stderr, flush=True)
    return out


def regress_child(a):
    """All-user query at k = 64 and query_candidates for all users x 100 candidates on the tree a.regress_child."""
    sys.path.insert(0, a.regress_child)
    import torch
    import mfx
    assert os.path.dirname(os.path.dirname(os.path.abspath(mfx.__file__))) == os.path.abspath(a.regress_child)
    ex = exclusion(a, mfx, torch)[0]
    W, H = factors(a, 64, torch)
    sync = torch.cuda.synchronize
    with mfx.Recommender(W, H, 1, exclude=ex) as r:
        q = timed(lambda: r.query(10, on_device=True), a.reps, sync)
        ptr, idx = gen_lists(torch, W.device, a.rows, 100, a.cols, 100 + a.rows)
        c = timed(lambda: r.query_candidates(10, (ptr, idx), canonical=True), a.reps, sync)
    print(json.dumps({"query_ms": q["median_ms"], "candidates_ms": c["median_ms"]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=480189)
    ap.add_argument("--cols", type=int, default=17770)
    ap.add_argument("--nnz", type=int, default=99_072_112)
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-pkg", default=None)
    ap.add_argument("--regress-runs", type=int, default=4)
    ap.add_argument("--regress-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_bench.json"))
    a = ap.parse_args()
    if a.regress_child:
        return regress_child(a)
    sys.path.insert(0, PKG)
    import torch
    import mfx
    out = {"tool": "ivf_bench", "n_top": N_TOP, "kmeans_iters": a.iters, "cases": []}
    for name in [x for x in a.cases.split(",") if x]:
        out["cases"].append(run_case(torch, mfx, name, CASES[name], a))
        torch.cuda.empty_cache()
    if a.parent_pkg:
        runs = {"parent": [], "this": []}
        for _ in range(a.regress_runs):
            for name, pkg in (("parent", os.path.abspath(a.parent_pkg)), ("this", PKG)):
                cmd = [sys.executable, os.path.abspath(__file__), "--regress-child", pkg, "--reps", str(a.reps),
                       "--rows", str(a.rows), "--cols", str(a.cols), "--nnz", str(a.nnz)]
                p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True, timeout=600)
                runs[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
        reg = {}
        for key, what in (("query_ms", "all-user query, k = 64, N = 10"), ("candidates_ms", "query_candidates, all users x 100, k = 64, N = 10")):
            pa, th = [x[key] for x in runs["parent"]], [x[key] for x in runs["this"]]
            pm, tm, spread = float(np.median(pa)), float(np.median(th)), max(pa) - min(pa)
            reg[key] = {"workload": what, "parent_ms": pa, "this_ms": th, "parent_median_ms": pm, "this_median_ms": tm,
                        "parent_spread_ms": spread, "no_slower": bool(tm <= pm + spread)}
        out["regression"] = reg
        print(json.dumps(reg), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
