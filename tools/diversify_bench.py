"""Diversity re-ranking (mfx_rec_diversify) at the Netflix shape.

A synthetic 480,189 x 17,770 matrix generated on the device is the exclude matrix; factors are random, k = 64 and 128,
N = 10, cosine, tradeoff 0.5.  Candidate lists are random and strictly ascending (those of candidates_bench.py), 100 and
1,000 candidates, for batches of 1 / 64 / 1,024 users and, at 100 candidates, all users.  Writes ONE JSON record (--out),
per point:
  (a) diversify on device tensors with the stream time of the phases (check + stage, relevance, selection) from
      mfx_rec_diversify_times, as the library chooses the form of the selection kernel and with form 1 (rows staged in
      LDS; "refused" where they do not fit) and form 2 (rows re-read) forced;
  (b) the same with MFX_DIV_THREADS=256, the workgroup the library would have without its rule of one wave per 64
      candidates of the longest list;
  (c) the floor: query_candidates on the same lists at n_top = 10, the same scoring without the greedy steps;
  (d) a torch baseline on the same data: gather of the H rows, bmm for the scores and for the pool x pool cosines, then N
      batched masked argmax steps.
Then query_diverse(10, pool = 100) for all users against query(100) alone.  With --parent-pkg DIR (a built
cuda-recommender_amd tree of the parent commit): the unchanged all-user query and query_candidates for all users x 100 at
k = 64 on that tree and on this one, alternated, --regress-runs fresh processes each.

    python tools/diversify_bench.py [--reps 5] [--ks 64,128] [--parent-pkg DIR] [--regress-runs 4] [--out FILE]
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
from candidates_bench import gen_lists  # noqa: E402  (the same lists as the candidates record)
from rank_bench import exclusion, factors, timed  # noqa: E402  (the same data and timer as the rank record)

N_TOP = 10
TRADEOFF = 0.5


def torch_baseline(torch, W, H, cn, users, idx, C, exkey, cols, n_top, tradeoff):
    """Gather, bmm for the scores and the C x C cosines, n_top batched masked argmax steps -> items [B, n_top]."""
    B = users.numel()
    k = W.shape[1]
    chunk = max(1, (1 << 28) // (C * max(k, C)))
    out = torch.empty((B, n_top), dtype=torch.int64, device=W.device)
    it_all = idx.view(B, C)
    for c0 in range(0, B, chunk):
        u = users[c0:c0 + chunk].long()
        it = it_all[c0:c0 + chunk].long()
        Hg = H[it]
        rel = torch.bmm(Hg, W[u].unsqueeze(2)).squeeze(2)
        Hn = Hg * cn[it].unsqueeze(2)
        sim = torch.bmm(Hn, Hn.transpose(1, 2))
        dead = torch.zeros_like(rel, dtype=torch.bool)
        if exkey is not None:
            key = (u[:, None] * cols + it).reshape(-1)
            pos = torch.searchsorted(exkey, key).clamp_(max=exkey.numel() - 1)
            dead = (exkey[pos] == key).view_as(rel)
        D = torch.zeros_like(rel)
        ar = torch.arange(u.numel(), device=W.device)
        for s in range(n_top):
            val = tradeoff * rel - (1.0 - tradeoff) * D
            val[dead] = float("-inf")
            p = val.argmax(1)
            out[c0:c0 + chunk, s] = it[ar, p]
            dead[ar, p] = True
            D = torch.maximum(D, sim[ar, p])
    return out


def point(torch, mfx, r, W, H, cn, users, C, cols, exkey, reps, seed):
    dev = W.device
    sync = torch.cuda.synchronize
    B = users.numel()
    ptr, idx = gen_lists(torch, dev, B, C, cols, seed)
    p = {"batch": B, "list_length": C, "candidates": B * C}
    res = {}

    def measure(name, form):
        def run():
            res[name] = r.diversify(N_TOP, (ptr, idx), users=users, tradeoff=TRADEOFF, canonical=True, return_values=True, form=form)
        try:
            p[name] = timed(run, reps, sync, r.diversify_times)
        except mfx.MfxError:
            p[name] = "refused"                                  # (form 1 where the rows do not fit in LDS)

    for name, form in (("diversify_auto", 0), ("diversify_form1", 1), ("diversify_form2", 2)):
        measure(name, form)
    os.environ["MFX_DIV_THREADS"] = "256"
    measure("diversify_auto_256_threads", 0)
    os.environ.pop("MFX_DIV_THREADS", None)
    p["forms_agree_bitwise"] = bool(all(torch.equal(a, b) for name in res for a, b in zip(res["diversify_auto"], res[name])))
    p["query_candidates_floor"] = timed(lambda: r.query_candidates(N_TOP, (ptr, idx), users=users, canonical=True), reps, sync, r.candidates_times)
    p["diversify_over_floor"] = p["diversify_auto"]["median_ms"] / p["query_candidates_floor"]["median_ms"]
    got = {}

    def base():
        got["items"] = torch_baseline(torch, W, H, cn, users, idx, C, exkey, cols, N_TOP, TRADEOFF)
    p["torch_baseline"] = timed(base, max(1, reps // 2), sync)
    p["speedup_vs_torch"] = p["torch_baseline"]["median_ms"] / p["diversify_auto"]["median_ms"]
    ours = res["diversify_auto"][0].long() & 0xFFFFFFFF
    real = ours[:, -1] != 0xFFFFFFFF                             # (slots with N eligible candidates)
    p["first_pick_agreement_with_torch"] = float((ours[real, 0] == got["items"][real, 0]).float().mean())  # (torch sums in another order)
    p["all_picks_agreement_with_torch"] = float((ours[real] == got["items"][real]).all(1).float().mean())
    return p


def regress_child(a):
    sys.path.insert(0, a.regress_child)
    import torch
    import mfx
    assert os.path.dirname(os.path.dirname(os.path.abspath(mfx.__file__))) == os.path.abspath(a.regress_child)
    ex = exclusion(a, mfx, torch)[0]
    W, H = factors(a, 64, torch)
    ptr, idx = gen_lists(torch, W.device, a.rows, 100, a.cols, 100 + a.rows)
    with mfx.Recommender(W, H, 1, exclude=ex) as r:
        q = timed(lambda: r.query(10, on_device=True), a.reps, torch.cuda.synchronize)
        c = timed(lambda: r.query_candidates(10, (ptr, idx), canonical=True), a.reps, torch.cuda.synchronize)
    print(json.dumps({"query_ms": q["median_ms"], "query_candidates_ms": c["median_ms"]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=480189)
    ap.add_argument("--cols", type=int, default=17770)
    ap.add_argument("--nnz", type=int, default=99_072_112)
    ap.add_argument("--ks", default="64,128")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-pkg", default=None)
    ap.add_argument("--regress-runs", type=int, default=4)
    ap.add_argument("--regress-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diversify_bench.json"))
    a = ap.parse_args()
    if a.regress_child:
        return regress_child(a)
    sys.path.insert(0, PKG)
    import torch
    import mfx
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    out = {"tool": "diversify_bench", "rows": a.rows, "cols": a.cols, "nnz": a.nnz, "n_top": N_TOP, "tradeoff": TRADEOFF,
           "metric": "cosine", "cases": []}
    ks = [int(x) for x in a.ks.split(",") if x]
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
        cn = 1.0 / H.norm(dim=1)
        case = {"k": k, "points": []}
        with mfx.Recommender(W, H, 1, exclude=ex) as r:
            for B, C in ((a.rows, 100), (1, 100), (64, 100), (1024, 100), (1, 1000), (64, 1000), (1024, 1000)):
                case["points"].append(point(torch, mfx, r, W, H, cn, users_of(B), C, a.cols, exkey, a.reps, seed=C + B))
                print(json.dumps(case["points"][-1]), file=sys.stderr, flush=True)
            qd = {"query_diverse_10_pool_100": timed(lambda: r.query_diverse(N_TOP, 100, tradeoff=TRADEOFF, on_device=True), a.reps, sync,
                                                     r.diversify_times),
                  "query_100_alone": timed(lambda: r.query(100, on_device=True), a.reps, sync)}
            case["one_call"] = qd
            print(json.dumps(qd), file=sys.stderr, flush=True)
        out["cases"].append(case)
        del W, H

    if a.parent_pkg:
        runs = {"parent": [], "this": []}
        for _ in range(a.regress_runs):
            for name, pkg in (("parent", os.path.abspath(a.parent_pkg)), ("this", PKG)):
                cmd = [sys.executable, os.path.abspath(__file__), "--regress-child", pkg, "--reps", str(a.reps),
                       "--rows", str(a.rows), "--cols", str(a.cols), "--nnz", str(a.nnz)]
                p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True, timeout=600)
                runs[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
        out["regression"] = {"k": 64, "n_top": 10}
        for key, what in (("query_ms", "all-user query"), ("query_candidates_ms", "query_candidates, all users x 100")):
            pr, th = [x[key] for x in runs["parent"]], [x[key] for x in runs["this"]]
            pm, tm = float(np.median(pr)), float(np.median(th))
            spread = max(pr) - min(pr)
            out["regression"][key] = {"workload": what, "parent_ms": pr, "this_ms": th, "parent_median_ms": pm, "this_median_ms": tm,
                                      "parent_spread_ms": spread, "no_slower": bool(tm <= pm + spread)}
        print(json.dumps(out["regression"]), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
