"""BPR training (mfx_bpr_*) at the Netflix shape: seconds per epoch, counted triples per second, and the split by kernel.

Builds the Netflix-shaped synthetic matrix on the GPU (mfx.synth_torch, as bench.py does; every stored pair is taken as a
positive interaction) and, for every k of --ks and every batch of --batches, trains from 0.1 N(0, 1) factors: a warm-up of
--warm steps, then one whole epoch timed by the library's stream events; then --profile-steps steps on a handle made with
parameters.profile = 1, which synchronises every step and gives the split sample / gradient / scatter / apply.

The floor the result is held against: a counted slot adds 3 k terms of 8 bytes with 64-bit integer atomics, and the chip
adds about 1.3 TB/s of bytes with FLOAT atomics (the only atomic rate measured on this part; for 64-bit integer adds it is
not measured).  So the record carries the added bytes per second of the scatter kernel and of the epoch, to be read
against that figure, not a fraction of a known peak.

In the same process a torch baseline runs the same batch mathematics -- torch.randint for the draws, searchsorted for the
user and the membership, index_add_ for the three scatters -- for --torch-steps steps per point: float atomics in arrival
order, so it is NOT reproducible; its time per slot is scaled to an epoch.

With --negatives M[,M...] --loss bpr|warp[,...] every point is run once per (loss, M): negatives = 1 with loss bpr is the
uniform sampler, negatives > 1 hardest of M, loss warp WARP with the default rank weights (mfx_bpr_create_neg).  The record
then carries the trials per slot of the timed epoch from trial_stats -- by the contract's sequential definition: M for
hardest of M; for WARP the chosen trial number, or M where no trial violated -- and the gathered bytes per second of the
trials kernel, (trials + 1) * k * 4 bytes per slot over the "sample" phase of the profiled steps (which holds the sampler's
own few microseconds as well, so the figure is a little low), to be read against the rate query_candidates reaches on
gathered rows of H (GATHER_TBS).  WARP trains at --warp-lr (its rank weight, up to ln(cols - 1), multiplies the step: at the
lr of the other modes the factors leave the range of the fixed point within an epoch and the slots are counted bad).  The
kernel scores whole rounds of its lane group, so it gathers somewhat more than the sequential definition counts.  The torch
baseline runs for the uniform sampler only.

With --parent-pkg DIR (a built cuda-recommender_amd tree of the parent commit): the unchanged all-user query, one
implicit-ALS iteration and one uniform BPR epoch at batch 65 536 (k = 64), each in a fresh process per tree, parent and this tree alternated --regress-runs times.

    python tools/bpr_bench.py [--ks 64,128] [--batches 4096,65536,1048576] [--negatives 1,8,32] [--loss bpr,warp]
                              [--parent-pkg DIR] [--regress-runs 4] [--out FILE]
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
FLOAT_ATOMIC_TBS = 1.3  # chip-wide added bytes per second of global FLOAT atomic adds (the guide's figure)
GATHER_TBS = 4.7        # gathered bytes per second of H rows that query_candidates reaches (README, all users x 1 000)


def matrix(a, torch):
    from mfx import synth_torch
    return synth_torch.synth_ratings_device(a.rows, a.cols, a.nnz, seed=1234, device="cuda:0", sigma_rows=0.5, sigma_cols=1.0)


def torch_steps(torch, d, W, H, batch, steps, lr, lam):
    """`steps` batches of the same mathematics in torch; returns (seconds, counted slots)."""
    dev = W.device
    ptr = d["csr_row_ptr"].long()
    idx = d["csr_col_idx"].long()
    rows, cols, nnz = W.shape[0], H.shape[0], idx.numel()
    key = torch.repeat_interleave(torch.arange(rows, device=dev), ptr[1:] - ptr[:-1]) * cols + idx  # ascending
    g = torch.Generator(device=dev)
    g.manual_seed(1)

    def one():
        p = torch.randint(0, nnz, (batch,), generator=g, device=dev)
        j = torch.randint(0, cols, (batch,), generator=g, device=dev)
        u = torch.searchsorted(ptr, p, right=True) - 1
        i = idx[p]
        want = u * cols + j
        pos = torch.searchsorted(key, want).clamp_(max=nnz - 1)
        keep = key[pos] != want
        u, i, j = u[keep], i[keep], j[keep]
        w, hi, hj = W[u], H[i], H[j]
        dd = hi - hj
        gg = torch.sigmoid(-(w * dd).sum(1, keepdim=True))
        W.index_add_(0, u, lr * (gg * dd - lam * w))
        H.index_add_(0, i, lr * (gg * w - lam * hi))
        H.index_add_(0, j, lr * (-gg * w - lam * hj))
        return keep.sum()

    one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    counted = sum(one() for _ in range(steps))
    torch.cuda.synchronize()
    return time.perf_counter() - t0, int(counted)


def point(torch, mfx, d, a, k, batch, loss="bpr", negatives=1):
    p = mfx.parameter()
    p.k, p.lambda_ = k, a.lam
    nnz = int(d["csr_val"].numel())
    uniform = loss == "bpr" and negatives == 1
    rec = {"k": k, "batch": batch, "loss": loss, "negatives": negatives, "steps_per_epoch": -(-nnz // batch)}
    neg = {} if uniform else {"negatives": negatives, "loss": loss}
    lr = a.warp_lr if loss == "warp" else a.lr
    rec["lr"] = lr
    s = mfx.BprSolver(None, p, lr, batch, seed=1, device_arrays=d, init_seed=k, **neg)
    s.steps(min(a.warm, max(1, nnz // batch // 4)))
    s.iterate(1)  # (finishes the started epoch: more warm-up, and the next call is a whole epoch)
    ts0 = s.trial_stats()
    e = s.iterate(1)[0]
    ts1 = s.trial_stats()
    trained = None if uniform else s.get_factors()
    s.close()
    none, tsum = (ts1[key] - ts0[key] for key in ("none_chosen", "chosen_trial_sum"))
    # (WARP: a slot without a chosen trial went through all M, unless its s_i was no number -- bad slots, none in a sane run)
    trials = float(negatives) if loss == "bpr" else (tsum + none * negatives) / max(1, e["slots"])
    rec.update({"none_chosen": none, "mean_chosen_trial": round(tsum / max(1, e["slots"] - none), 3), "trials_per_slot": round(trials, 3)})
    counted = e["slots"] - e["skipped"] - e["bad"]
    rec.update({"seconds_per_epoch": round(e["seconds"], 4), "counted_triples_per_second": round(counted / e["seconds"], 1),
                "skipped": e["skipped"], "bad": e["bad"], "auc_of_the_epoch": round(e["auc"], 4),
                "added_bytes_per_counted_slot": 3 * k * 8,
                "epoch_added_tb_per_s": round(counted * 3 * k * 8 / e["seconds"] / 1e12, 4),
                "floor_seconds_per_epoch_at_float_atomic_rate": round(counted * 3 * k * 8 / (FLOAT_ATOMIC_TBS * 1e12), 4)})
    p.profile = 1
    s = mfx.BprSolver(None, p, lr, batch, seed=1, device_arrays=d, init_seed=k, **neg)
    n = min(a.profile_steps, rec["steps_per_epoch"])
    if trained is not None:  # (the trials WARP needs depend on the state of training: profile at the timed epoch's factors)
        s.set_factors(*trained)
    s.steps(min(3, n))
    t0, ts0 = s.kernel_times(), s.trial_stats()
    r = s.steps(n)
    t1, ts1 = s.kernel_times(), s.trial_stats()
    s.close()
    cnt = r["slots"] - r["skipped"] - r["bad"]
    split = {name: (t1[name] - t0[name]) / n for name in t1}
    rec["us_per_step"] = {name: round(v * 1e6, 2) for name, v in split.items()}
    rec["scatter_added_tb_per_s"] = round(cnt * 3 * k * 8 / (split["scatter"] * n) / 1e12, 4) if split["scatter"] > 0 else None
    if not uniform:
        none, tsum = (ts1[key] - ts0[key] for key in ("none_chosen", "chosen_trial_sum"))
        ptrials = float(negatives) if loss == "bpr" else (tsum + none * negatives) / max(1, r["slots"])
        gathered = r["slots"] * (ptrials + 1) * k * 4
        rec["profiled_trials_per_slot"] = round(ptrials, 3)
        rec["trials_gathered_bytes_per_slot"] = round((ptrials + 1) * k * 4, 1)
        rec["trials_gathered_tb_per_s"] = round(gathered / (split["sample"] * n) / 1e12, 4) if split["sample"] > 0 else None
        rec["gather_yardstick_tb_per_s"] = GATHER_TBS
        return rec
    W = torch.randn(int(d["rows"]), k, device="cuda:0") * 0.1
    H = torch.randn(int(d["cols"]), k, device="cuda:0") * 0.1
    ts, tc = torch_steps(torch, d, W, H, batch, min(a.torch_steps, rec["steps_per_epoch"]), a.lr, a.lam)
    rec["torch_index_add"] = {"counted_triples_per_second": round(tc / ts, 1), "seconds_per_epoch_scaled": round(ts / tc * counted, 4),
                              "reproducible": False}
    rec["ratio_to_torch"] = round(rec["seconds_per_epoch"] / rec["torch_index_add"]["seconds_per_epoch_scaled"], 3)
    return rec


def regress_child(a):
    sys.path.insert(0, a.regress_child)
    import torch
    import mfx
    assert os.path.dirname(os.path.dirname(os.path.abspath(mfx.__file__))) == os.path.abspath(a.regress_child)
    d = matrix(a, torch)
    p = mfx.parameter()
    p.k, p.lambda_ = 64, 0.05
    s = mfx.ImplicitAlsSolver(None, p, 1.0, device_arrays=d)
    s.set_factors(mfx.initial_col(a.cols, 64))
    s.iterate(1)
    ials = float(np.median([r.update_time * 1e3 for r in s.iterate(3)]))
    s.close()
    p.lambda_ = 0.01
    s = mfx.BprSolver(None, p, 0.05, 65536, seed=1, device_arrays=d, init_seed=64)  # the uniform sampler
    s.steps(20)
    s.iterate(1)
    bpr = s.iterate(1)[0]["seconds"] * 1e3
    s.close()
    rp, ci = d["csr_row_ptr"].cpu().numpy().view(np.uint32), d["csr_col_idx"].cpu().numpy().view(np.uint32)
    del d
    ex = mfx.dataset.RatingData(a.rows, a.cols, rp, ci, np.zeros(0, np.float32), np.zeros(a.cols + 1, np.uint32),
                                np.zeros(0, np.uint32), np.zeros(0, np.float32))
    g = torch.Generator(device="cuda:0")
    g.manual_seed(64)
    W = (torch.randn(a.rows, 64, generator=g, device="cuda:0") * 0.3).contiguous()
    H = (torch.randn(a.cols, 64, generator=g, device="cuda:0") * 0.3).contiguous()
    ts = []
    with mfx.Recommender(W, H, 1, exclude=ex) as r:
        for rep in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r.query(10, on_device=True)
            torch.cuda.synchronize()
            if rep:
                ts.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"query_ms": float(np.median(ts)), "ials_iteration_ms": ials, "bpr_uniform_epoch_ms": bpr}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=480189)
    ap.add_argument("--cols", type=int, default=17770)
    ap.add_argument("--nnz", type=int, default=99_072_112)
    ap.add_argument("--ks", default="64,128")
    ap.add_argument("--batches", default="4096,65536,1048576")
    ap.add_argument("--negatives", default="1", help="trials per slot, comma list; 1 with --loss bpr is the uniform sampler")
    ap.add_argument("--loss", default="bpr", help="bpr (uniform / hardest of M) and / or warp, comma list")
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--warp-lr", type=float, default=0.005)
    ap.add_argument("--lam", type=float, default=0.01)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--profile-steps", type=int, default=50)
    ap.add_argument("--torch-steps", type=int, default=20)
    ap.add_argument("--parent-pkg", default=None)
    ap.add_argument("--regress-runs", type=int, default=4)
    ap.add_argument("--regress-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bpr_bench.json"))
    a = ap.parse_args()
    if a.regress_child:
        return regress_child(a)
    sys.path.insert(0, PKG)
    import torch
    import mfx
    out = {"tool": "bpr_bench", "rows": a.rows, "cols": a.cols, "nnz": a.nnz, "lr": a.lr, "warp_lr": a.warp_lr, "lambda": a.lam,
           "float_atomic_tb_per_s_of_the_guide": FLOAT_ATOMIC_TBS, "points": []}
    ks = [int(x) for x in a.ks.split(",") if x]
    if ks:
        d = matrix(a, torch)
        for k in ks:
            for batch in (int(x) for x in a.batches.split(",") if x):
                for loss in (x for x in a.loss.split(",") if x):
                    for m in (int(x) for x in a.negatives.split(",") if x):
                        out["points"].append(point(torch, mfx, d, a, k, batch, loss, m))
                        print(json.dumps(out["points"][-1]), file=sys.stderr, flush=True)
        del d
        torch.cuda.empty_cache()
    if a.parent_pkg:
        runs = {"parent": [], "this": []}
        for _ in range(a.regress_runs):
            for name, pkg in (("parent", os.path.abspath(a.parent_pkg)), ("this", PKG)):
                cmd = [sys.executable, os.path.abspath(__file__), "--regress-child", pkg, "--rows", str(a.rows), "--cols", str(a.cols),
                       "--nnz", str(a.nnz)]
                p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True, timeout=600)
                runs[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
        out["regression"] = {"k": 64}
        for key, what in (("query_ms", "all-user query, n_top = 10"), ("ials_iteration_ms", "one implicit-ALS iteration"),
                          ("bpr_uniform_epoch_ms", "one BPR epoch, uniform sampler, batch 65 536")):
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
