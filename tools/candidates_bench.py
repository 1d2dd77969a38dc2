"""Candidate-list re-ranking and pair scoring (mfx_rec_query_candidates, mfx_rec_score) at the Netflix shape.

A synthetic 480,189 x 17,770 matrix generated on the device is the exclude matrix; factors are random, k = 64 and 128,
N = 10.  Candidate lists are random and strictly ascending (one uniform draw from each of C equal strata of the
catalogue), C = 100 and 1,000, for batches of 1 / 64 / 1,024 / all users.  Writes ONE JSON record (--out), per point:
  (a) query_candidates on device tensors, with the stream time of the phases (check + stage, score, select) from
      mfx_rec_candidates_times and the gathered bytes per second of the score phase, candidates * kt * 4 / seconds,
      as the library chooses between the two forms of the gather and with each forced (MFX_CAND_LOAD=group / lane);
  (b) a torch baseline on the same data: gather of the H rows, batched dot, mask of the excluded items, topk per row;
  (c) the full-catalogue query for the same users.
Then: a sweep of the list length up to the catalogue at k = 64 (where does the full query become the faster way?);
10^6 items at k = 128 with 1,000 candidates for 1,024 users; score() on a 1.4 M-pair set against rank_of on the same
pairs.  With --parent-pkg DIR (a built cuda-recommender_amd tree of the parent commit): the unchanged all-user query at
k = 64 on that tree and on this one, alternated, --regress-runs fresh processes each.

    python tools/candidates_bench.py [--reps 5] [--ks 64,128] [--parent-pkg DIR] [--regress-runs 4] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cuda-recommender_amd")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rank_bench import exclusion, factors, regress_child, timed  # noqa: E402  (the same data and timer as the rank record)

N_TOP = 10


def gen_lists(torch, dev, B, C, cols, seed):
    """B strictly ascending random lists of C ids below cols: (ptr int32 [B + 1], idx int32 [B * C])."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    base = ((torch.arange(C, device=dev, dtype=torch.int64) * cols) // C).to(torch.int32)
    width = max(1, cols // C)
    idx = torch.randint(0, width, (B, C), generator=g, device=dev, dtype=torch.int32).add_(base[None, :])
    ptr = (torch.arange(B + 1, device=dev, dtype=torch.int64) * C).to(torch.int32)
    return ptr, idx.reshape(-1)


def torch_baseline(torch, W, H, users, idx, C, exkey, cols, n_top):
    """Gather of the H rows, batched dot, mask of the excluded items, topk per row -> items [B, min(n_top, C)]."""
    B = users.numel()
    k = W.shape[1]
    chunk = max(1, (1 << 28) // (C * k))
    out = torch.empty((B, min(n_top, C)), dtype=torch.int64, device=W.device)
    it_all = idx.view(B, C)
    for c0 in range(0, B, chunk):
        u = users[c0:c0 + chunk].long()
        it = it_all[c0:c0 + chunk].long()
        S = torch.bmm(H[it], W[u].unsqueeze(2)).squeeze(2)
        if exkey is not None:
            key = (u[:, None] * cols + it).reshape(-1)
            pos = torch.searchsorted(exkey, key).clamp_(max=exkey.numel() - 1)
            S[(exkey[pos] == key).view_as(S)] = float("-inf")
        out[c0:c0 + chunk] = it.gather(1, S.topk(out.shape[1], dim=1).indices)
    return out


def point(torch, r, W, H, users, C, cols, exkey, reps, seed, baseline=True, both_forms=True):
    """One (batch, list length) point on handle r: query_candidates (default and both load forms forced), the torch baseline, the full query."""
    dev = W.device
    sync = torch.cuda.synchronize
    B = users.numel()
    ptr, idx = gen_lists(torch, dev, B, C, cols, seed)
    kt = r.k if r.k >= 2 else 2
    p = {"batch": B, "list_length": C, "candidates": B * C}
    res = {}
    for form in (("default", "group", "lane") if both_forms else ("default",)):
        os.environ.pop("MFX_CAND_LOAD", None)
        if form != "default":                                    # (default: the library's own choice between the two)
            os.environ["MFX_CAND_LOAD"] = form

        def run():
            res[form] = r.query_candidates(N_TOP, (ptr, idx), users=users, canonical=True)
        t = timed(run, reps, sync, r.candidates_times)
        t["gathered_GBps"] = B * C * kt * 4 / (t["phases_ms"]["score"] * 1e-3) / 1e9
        p["candidates_" + form] = t
    os.environ.pop("MFX_CAND_LOAD", None)
    if both_forms:
        p["forms_agree_bitwise"] = bool(all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(res["default"], res["group"], res["lane"])))
    p["query_full_catalogue"] = timed(lambda: r.query(N_TOP, users=users), reps, sync)
    p["candidates_over_query"] = p["candidates_default"]["median_ms"] / p["query_full_catalogue"]["median_ms"]
    if baseline:
        got = {}

        def base():
            got["items"] = torch_baseline(torch, W, H, users, idx, C, exkey, cols, N_TOP)
        p["torch_baseline"] = timed(base, max(1, reps // 2), sync)
        p["speedup_vs_torch"] = p["torch_baseline"]["median_ms"] / p["candidates_default"]["median_ms"]
        ours = res["default"][0].long()[:, :got["items"].shape[1]]
        p["top1_agreement_with_torch"] = float((ours[:, 0] == got["items"][:, 0]).float().mean())  # (torch sums in another order)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=480189)
    ap.add_argument("--cols", type=int, default=17770)
    ap.add_argument("--nnz", type=int, default=99_072_112)
    ap.add_argument("--heldout", type=int, default=1_400_000)
    ap.add_argument("--ks", default="64,128")
    ap.add_argument("--lengths", default="100,1000")
    ap.add_argument("--batches", default="1,64,1024,0", help="0 = all users")
    ap.add_argument("--sweep", default="100,300,1000,2000,4000,8000,17770")
    ap.add_argument("--sweep-all-users-max", type=int, default=4000, help="longest list of the all-user sweep (4 bytes per candidate)")
    ap.add_argument("--big-cols", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-pkg", default=None)
    ap.add_argument("--regress-runs", type=int, default=4)
    ap.add_argument("--regress-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "candidates_bench.json"))
    a = ap.parse_args()
    if a.regress_child:
        return regress_child(a)
    sys.path.insert(0, PKG)
    import torch
    import mfx
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    out = {"tool": "candidates_bench", "rows": a.rows, "cols": a.cols, "nnz": a.nnz, "n_top": N_TOP, "cases": []}
    ks = [int(x) for x in a.ks.split(",") if x]
    lengths = [int(x) for x in a.lengths.split(",") if x]
    batches = [int(x) or a.rows for x in a.batches.split(",") if x]
    rng = np.random.default_rng(15)

    def users_of(B):
        u = np.arange(a.rows) if B == a.rows else np.sort(rng.choice(a.rows, B, replace=False))
        return torch.from_numpy(u.astype(np.uint32).view(np.int32)).to(dev)

    if ks:
        ex, rp_d, ci_d = exclusion(a, mfx, torch)
        rp_l = rp_d.long()
        ex_row = torch.repeat_interleave(torch.arange(a.rows, device=dev), rp_l[1:] - rp_l[:-1])
        exkey = ex_row * a.cols + ci_d.long()                    # ascending: the rows are, and the ids within a row
        del ex_row, rp_l
    for k in ks:
        W, H = factors(a, k, torch)
        case = {"k": k, "points": []}
        with mfx.Recommender(W, H, 1, exclude=ex) as r:
            for C in lengths:
                for B in batches:
                    case["points"].append(point(torch, r, W, H, users_of(B), C, a.cols, exkey, a.reps, seed=C + B))
                    print(json.dumps(case["points"][-1]), file=sys.stderr, flush=True)
            if k == ks[0]:
                # where the full-catalogue query becomes the faster way: the first swept length at which it is
                sweep = {}
                for B in (1024, a.rows):
                    pts = []
                    for C in [int(x) for x in a.sweep.split(",") if x]:
                        if C > a.cols or (B == a.rows and C > a.sweep_all_users_max):
                            continue
                        pts.append(point(torch, r, W, H, users_of(B), C, a.cols, exkey, max(2, a.reps // 2), seed=7 * C + B,
                                         baseline=False, both_forms=False))
                        print(json.dumps(pts[-1]), file=sys.stderr, flush=True)
                    slower = [p["list_length"] for p in pts if p["candidates_over_query"] >= 1.0]
                    sweep[str(B)] = {"points": pts, "first_length_where_query_is_faster": slower[0] if slower else None}
                case["length_sweep"] = sweep
                # the scores of a held-out set: score() against rank_of (which also counts) on the same pairs
                held_u = torch.from_numpy(np.sort(rng.integers(0, a.rows, a.heldout)).astype(np.uint32).view(np.int32)).to(dev)
                held_i = torch.from_numpy(rng.integers(0, a.cols, a.heldout).astype(np.uint32).view(np.int32)).to(dev)
                sc = {}
                for form in ("group", "lane"):
                    os.environ["MFX_CAND_LOAD"] = form
                    sc["score_" + form] = timed(lambda: r.score(held_u, held_i), a.reps, sync, r.candidates_times)
                os.environ.pop("MFX_CAND_LOAD", None)
                sc["rank_of"] = timed(lambda: r.rank_of(held_u, held_i), a.reps, sync, r.rank_times)
                sc["same_bits"] = bool(torch.equal(r.score(held_u, held_i), r.rank_of(held_u, held_i)[1]))
                sc["pairs"] = a.heldout
                case["score_heldout"] = sc
                print(json.dumps(sc), file=sys.stderr, flush=True)
        out["cases"].append(case)
        del W, H
    if a.big_cols:
        k, B, C = 128, 1024, 1000
        g = torch.Generator(device=dev)
        g.manual_seed(3)
        W = (torch.randn(B, k, generator=g, device=dev) * 0.3).contiguous()
        H = (torch.randn(a.big_cols, k, generator=g, device=dev) * 0.3).contiguous()
        with mfx.Recommender(W, H, 1) as r:
            users = torch.arange(B, device=dev, dtype=torch.int32)
            out["big_catalogue"] = dict(point(torch, r, W, H, users, C, a.big_cols, None, a.reps, seed=1), k=k, cols=a.big_cols)
        print(json.dumps(out["big_catalogue"]), file=sys.stderr, flush=True)
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
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
