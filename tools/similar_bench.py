"""Item-to-item similarity and the item filter (mfx_rec_similar, mfx_rec_set_item_filter) at the Netflix shape.

Prints ONE JSON line:
  (i)   all-items queries over 17,770 items at k = 64 / 128, N = 10 / 100, dot and cosine, beside a torch baseline on the
        same device (normalise, chunked torch.mm, mask self, torch.topk);
  (ii)  1 / 64 / 1,024 query items over 1,000,000 items at k = 128 (cosine, N = 10);
  (iii) the all-user query of tools/recommend_bench.py (480,189 users, k = 64, N = 10, the training ratings excluded)
        without a filter and with a random 50 % filter;
  (iv)  with --parent-pkg DIR (a built cuda-recommender_amd tree of the parent commit): the unfiltered query of (iii) on
        that tree and on this one, alternated, --regress-runs fresh processes each.

    python tools/similar_bench.py [--reps 5] [--parent-pkg DIR] [--regress-runs 4] [--skip i,ii,iii]
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


def timed(fn, reps, sync):
    fn()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "reps": reps}


def user_workload(a, mfx, torch):
    """The handle of recommend_bench.py at k = 64: Netflix-shaped exclusion set, random factors."""
    from mfx import synth_torch
    dev = torch.device("cuda:0")
    d = synth_torch.synth_ratings_device(a.rows, a.cols, a.nnz, seed=1234, device="cuda:0", sigma_rows=0.5, sigma_cols=1.0)
    rp = d["csr_row_ptr"].contiguous().cpu().numpy().view(np.uint32)
    ci = d["csr_col_idx"].contiguous().cpu().numpy().view(np.uint32)
    del d
    ex = mfx.dataset.RatingData(a.rows, a.cols, rp, ci, np.zeros(0, np.float32), np.zeros(a.cols + 1, np.uint32),
                                np.zeros(0, np.uint32), np.zeros(0, np.float32))
    g = torch.Generator(device=dev)
    g.manual_seed(64)
    W = (torch.randn(a.rows, 64, generator=g, device=dev) * 0.3).contiguous()
    H = (torch.randn(a.cols, 64, generator=g, device=dev) * 0.3).contiguous()
    return mfx.Recommender(W, H, 1, exclude=ex)


def regress_child(a):
    sys.path.insert(0, a.regress_child)
    import torch
    import mfx
    assert os.path.dirname(os.path.dirname(os.path.abspath(mfx.__file__))) == os.path.abspath(a.regress_child)
    with user_workload(a, mfx, torch) as r:
        print(json.dumps(timed(lambda: r.query(10, on_device=True), a.reps, torch.cuda.synchronize)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=480189)
    ap.add_argument("--cols", type=int, default=17770)
    ap.add_argument("--nnz", type=int, default=99_072_112)
    ap.add_argument("--big-cols", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-chunk", type=int, default=4096)
    ap.add_argument("--skip", default="")
    ap.add_argument("--parent-pkg", default=None)
    ap.add_argument("--regress-runs", type=int, default=4)
    ap.add_argument("--regress-child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.regress_child:
        return regress_child(a)
    sys.path.insert(0, PKG)
    import torch
    import mfx
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    skip = set(a.skip.split(","))
    out = {"tool": "similar_bench", "rows": a.rows, "cols": a.cols, "nnz": a.nnz}

    if "i" not in skip:
        out["all_items"] = []
        for k in (64, 128):
            g = torch.Generator(device=dev)
            g.manual_seed(k)
            H = (torch.randn(a.cols, k, generator=g, device=dev) * 0.3).contiguous()
            W = torch.zeros(1, k, device=dev)
            with mfx.Recommender(W, H, 1) as r:
                r.similar_setup()
                for n_top in (10, 100):
                    case = {"k": k, "n_top": n_top, "flop": 2.0 * a.cols * a.cols * k}
                    for name, metric in (("dot", mfx.MFX_SIM_DOT), ("cosine", mfx.MFX_SIM_COSINE)):
                        case[name] = timed(lambda: r.similar_items(n_top, metric=metric, on_device=True), a.reps, sync)
                    case["cosine_over_dot"] = case["cosine"]["median_ms"] / case["dot"]["median_ms"]
                    bi = torch.empty((a.cols, n_top), dtype=torch.int64, device=dev)

                    def base():
                        Hn = H / H.norm(dim=1, keepdim=True)
                        for q0 in range(0, a.cols, a.baseline_chunk):
                            q1 = min(a.cols, q0 + a.baseline_chunk)
                            S = torch.mm(Hn[q0:q1], Hn.t())
                            S[torch.arange(q1 - q0, device=dev), torch.arange(q0, q1, device=dev)] = float("-inf")
                            bi[q0:q1] = torch.topk(S, n_top, dim=1).indices
                    case["torch_baseline"] = timed(base, a.reps, sync)
                    case["speedup_vs_torch"] = case["torch_baseline"]["median_ms"] / case["cosine"]["median_ms"]
                    got = r.similar_items(n_top, metric=mfx.MFX_SIM_COSINE, on_device=True)[0].long()
                    case["top1_agrees_with_torch"] = float((got[:, 0] == bi[:, 0]).float().mean())
                    out["all_items"].append(case)
                    print(json.dumps(case), file=sys.stderr, flush=True)

    if "ii" not in skip:
        k = 128
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        H = (torch.randn(a.big_cols, k, generator=g, device=dev) * 0.3).contiguous()
        lat = {}
        with mfx.Recommender(torch.zeros(1, k, device=dev), H, 1) as r:
            r.similar_setup()
            for nq in (1, 64, 1024):
                q = torch.from_numpy(np.random.default_rng(nq).choice(a.big_cols, nq).astype(np.int32)).to(dev)
                lat[str(nq)] = timed(lambda: r.similar_items(10, q), a.reps, sync)
        del H
        out["large_catalogue"] = {"cols": a.big_cols, "k": k, "n_top": 10, "metric": "cosine", "latency": lat}
        print(json.dumps(out["large_catalogue"]), file=sys.stderr, flush=True)

    if "iii" not in skip:
        with user_workload(a, mfx, torch) as r:
            res = {"k": 64, "n_top": 10}
            res["no_filter"] = timed(lambda: r.query(10, on_device=True), a.reps, sync)
            keep = torch.rand(a.cols, device=dev) < 0.5
            r.set_item_filter(keep)
            res["filter_50pct"] = timed(lambda: r.query(10, on_device=True), a.reps, sync)
            res["filter_over_none"] = res["filter_50pct"]["median_ms"] / res["no_filter"]["median_ms"]
        out["user_query_filter"] = res
        print(json.dumps(res), file=sys.stderr, flush=True)

    if a.parent_pkg:
        runs = {"parent": [], "this": []}
        for _ in range(a.regress_runs):
            for name, pkg in (("parent", os.path.abspath(a.parent_pkg)), ("this", PKG)):
                cmd = [sys.executable, os.path.abspath(__file__), "--regress-child", pkg, "--reps", str(a.reps),
                       "--rows", str(a.rows), "--cols", str(a.cols), "--nnz", str(a.nnz)]
                p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True, timeout=600)
                runs[name].append(json.loads(p.stdout.strip().splitlines()[-1])["median_ms"])
        pm, tm = float(np.median(runs["parent"])), float(np.median(runs["this"]))
        spread = max(runs["parent"]) - min(runs["parent"])
        out["regression"] = {"workload": "unfiltered all-user query, k = 64, N = 10", "parent_ms": runs["parent"],
                             "this_ms": runs["this"], "parent_median_ms": pm, "this_median_ms": tm,
                             "parent_spread_ms": spread, "no_slower": bool(tm <= pm + spread)}
        print(json.dumps(out["regression"]), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
