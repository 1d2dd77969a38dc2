"""Exact catalogue ranks and full-rank evaluation (mfx_rec_rank, mfx_rec_evaluate) at the Netflix shape.

A synthetic 480,189 x 17,770 matrix generated on the device is the exclude matrix; factors are random, k = 64 and 128.
Prints ONE JSON line, per k:
  (a) rank_of for one pair per user (480,189 pairs), with the device time of the three phases (target keys, counting
      pass, exclusion correction) from mfx_rec_rank_times;
  (b) rank_of for a 1.4 M-pair held-out set with about three targets per user;
  (c) evaluate with cutoffs (1, 10, 100, 1000, 10000) on that set (host arrays in, the metrics out);
  (d) a torch baseline of (a) on the same device: chunked torch.mm, mask the excluded items, compare and count;
  (e) query(n_top = 10) for all users: the pass the counting pass shares its loop with.
With --parent-pkg DIR (a built cuda-recommender_amd tree of the parent commit): the all-user query of (e) at k = 64 on
that tree and on this one, alternated, --regress-runs fresh processes each.

    python tools/rank_bench.py [--reps 5] [--ks 64,128] [--parent-pkg DIR] [--regress-runs 4] [--skip d]
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


def timed(fn, reps, sync, after=None):
    fn()
    sync()
    ts, extra = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
        if after:
            extra.append(after())
    out = {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "reps": reps}
    if extra:
        out["phases_ms"] = {k: float(np.median([e[k] for e in extra]) * 1e3) for k in extra[0]}
    return out


def exclusion(a, mfx, torch):
    """Netflix-shaped training set as the exclude matrix: (RatingData, row pointers and column ids on the device)."""
    from mfx import synth_torch
    d = synth_torch.synth_ratings_device(a.rows, a.cols, a.nnz, seed=1234, device="cuda:0", sigma_rows=0.5, sigma_cols=1.0)
    rp_d, ci_d = d["csr_row_ptr"].contiguous(), d["csr_col_idx"].contiguous()
    del d
    rp, ci = rp_d.cpu().numpy().view(np.uint32), ci_d.cpu().numpy().view(np.uint32)
    ex = mfx.dataset.RatingData(a.rows, a.cols, rp, ci, np.zeros(0, np.float32), np.zeros(a.cols + 1, np.uint32),
                                np.zeros(0, np.uint32), np.zeros(0, np.float32))
    return ex, rp_d, ci_d


def factors(a, k, torch):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(k)
    W = (torch.randn(a.rows, k, generator=g, device=dev) * 0.3).contiguous()
    H = (torch.randn(a.cols, k, generator=g, device=dev) * 0.3).contiguous()
    return W, H


def regress_child(a):
    sys.path.insert(0, a.regress_child)
    import torch
    import mfx
    assert os.path.dirname(os.path.dirname(os.path.abspath(mfx.__file__))) == os.path.abspath(a.regress_child)
    ex = exclusion(a, mfx, torch)[0]
    W, H = factors(a, 64, torch)
    with mfx.Recommender(W, H, 1, exclude=ex) as r:
        print(json.dumps(timed(lambda: r.query(10, on_device=True), a.reps, torch.cuda.synchronize)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=480189)
    ap.add_argument("--cols", type=int, default=17770)
    ap.add_argument("--nnz", type=int, default=99_072_112)
    ap.add_argument("--heldout", type=int, default=1_400_000)
    ap.add_argument("--ks", default="64,128")
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
    out = {"tool": "rank_bench", "rows": a.rows, "cols": a.cols, "nnz": a.nnz, "heldout": a.heldout, "cases": []}
    ks = [int(x) for x in a.ks.split(",") if x]

    if ks:
        ex, rp_d, ci_d = exclusion(a, mfx, torch)
        rng = np.random.default_rng(14)
        one_u = np.arange(a.rows, dtype=np.uint32)
        one_i = rng.integers(0, a.cols, a.rows).astype(np.uint32)
        held_u = np.sort(rng.integers(0, a.rows, a.heldout)).astype(np.uint32)
        held_i = rng.integers(0, a.cols, a.heldout).astype(np.uint32)
        T = mfx.TestData(a.rows, a.cols, held_u, held_i, np.ones(a.heldout, np.float32))
        to_dev = lambda x: torch.from_numpy(x.view(np.int32)).to(dev)
        d_one_u, d_one_i, d_held_u, d_held_i = (to_dev(x) for x in (one_u, one_i, held_u, held_i))
        rp_l = rp_d.long()
        ex_row = torch.repeat_interleave(torch.arange(a.rows, device=dev, dtype=torch.int32), (rp_l[1:] - rp_l[:-1]))
        rp_h = rp_l.cpu().numpy()
    for k in ks:
        W, H = factors(a, k, torch)
        case = {"k": k, "flop_per_pair": 2.0 * a.cols * k}
        with mfx.Recommender(W, H, 1, exclude=ex) as r:
            case["query_all_users_n10"] = timed(lambda: r.query(10, on_device=True), a.reps, sync)
            case["rank_one_pair_per_user"] = timed(lambda: r.rank_of(d_one_u, d_one_i), a.reps, sync, r.rank_times)
            case["rank_heldout"] = timed(lambda: r.rank_of(d_held_u, d_held_i), a.reps, sync, r.rank_times)
            cuts = (1, 10, 100, 1000, 10000)
            res = {}

            def ev():
                res.update(r.evaluate(T, cutoffs=cuts))
            case["evaluate_heldout"] = timed(ev, a.reps, sync, r.rank_times)
            case["evaluate_result"] = {x: res[x] for x in ("cutoffs", "hr", "ndcg", "mrr", "auc", "users", "auc_users")}
            case["count_pass_over_query"] = (case["rank_one_pair_per_user"]["phases_ms"]["count"]
                                             / case["query_all_users_n10"]["median_ms"])
            got = r.rank_of(d_one_u, d_one_i)[0]
        if "d" not in skip:
            base_rank = torch.empty(a.rows, dtype=torch.int64, device=dev)
            ids = torch.arange(a.cols, device=dev)

            def base():
                for u0 in range(0, a.rows, a.baseline_chunk):
                    u1 = min(a.rows, u0 + a.baseline_chunk)
                    S = torch.mm(W[u0:u1], H.t())
                    it = d_one_i[u0:u1].long()
                    t = S[torch.arange(u1 - u0, device=dev), it].clone()
                    lo, hi = int(rp_h[u0]), int(rp_h[u1])
                    S[(ex_row[lo:hi].long() - u0), ci_d[lo:hi].long()] = float("-inf")
                    before = (S > t[:, None]) | ((S == t[:, None]) & (ids[None, :] < it[:, None]))
                    base_rank[u0:u1] = before.sum(1)
            case["torch_baseline_one_pair_per_user"] = timed(base, max(1, a.reps // 2), sync)
            case["speedup_vs_torch"] = case["torch_baseline_one_pair_per_user"]["median_ms"] / case["rank_one_pair_per_user"]["median_ms"]
            ok = got != -1                                       # (int32 bits of 0xFFFFFFFF: the excluded targets)
            case["median_abs_rank_difference_to_torch"] = float((got[ok].long() - base_rank[ok]).abs().float().median())
        out["cases"].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
        del W, H

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
        out["regression"] = {"workload": "all-user query, k = 64, N = 10", "parent_ms": runs["parent"],
                             "this_ms": runs["this"], "parent_median_ms": pm, "this_median_ms": tm,
                             "parent_spread_ms": spread, "no_slower": bool(tm <= pm + spread)}
        print(json.dumps(out["regression"]), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
