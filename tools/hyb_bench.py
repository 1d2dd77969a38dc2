"""Hybrid BPR training (mfx_hyb_*) at the Netflix shape: seconds per step and per epoch against BprSolver, the split by
phase, the bytes the spread adds per second, the price of a feature that every item carries, and the time of embedding
all rows.

Builds the Netflix-shaped synthetic matrix on the GPU (mfx.synth_torch, as bench.py does; every stored pair is taken as a
positive interaction) and, for every k of --ks and batch of --batches, three configurations of the features:
  a  identities on both sides (the model is BPR bit for bit);
  b  items: identity + 1 .. 3 of 20 tags, normalised; users: identity;
  c  as b, plus one tag that every item carries.
Per point: --rounds rounds of (BprSolver --steps steps, HybridSolver --steps steps) in the same process, alternated, the
median of the rounds (--lr is the rate at 65 536 slots, scaled down in proportion for a larger batch, since the terms
of a feature that many rows carry add up over the batch); one whole epoch of either; --profile-steps steps on a handle
made with parameters.profile = 1 for the split sample / embed / gradient / scatter / spread / apply.

What the result is held against, stated beforehand.  (a) costs a BPR step plus the embed and spread passes: the embed
pass reads one table row per (slot, role) and writes one row, the spread pass adds one 8 k-byte row per touched row -- as
many atomic bytes again as k_bpr_apply would have read -- so a step of (a) should stay below twice a BPR step.  The bytes
the spread adds (8 k per entry of every touched row, the touched rows counted from the first step's triples on the host)
over the spread phase are read against the 1.09 - 1.30 TB/s that k_bpr_scatter reached.  (c) against (b)
prices the hot feature: every touched item adds into one 8 k-byte row, the shape the microarchitecture notes put an order
of magnitude below the spread rate.

With --parent-pkg DIR (the built cuda-recommender_amd directory inside a whole checkout of the parent commit): the
unchanged uniform BPR epoch and all-user query (tools/bpr_bench.py's regression child), one LightGCN step (this tool's
own child) and bench.py, each in a fresh process per tree, parent and this tree alternated --regress-runs times.

    python tools/hyb_bench.py [--ks 64,128] [--batches 65536,1048576] [--configs a,b,c] [--parent-pkg DIR] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cuda-recommender_amd")
SCATTER_TBS = (1.09, 1.30)  # added bytes per second of k_bpr_scatter


def matrix(a, torch):
    from mfx import synth_torch
    return synth_torch.synth_ratings_device(a.rows, a.cols, a.nnz, seed=1234, device="cuda:0", sigma_rows=0.5, sigma_cols=1.0)


def item_features(mfx, cols, config):
    if config == "a":
        return None
    rng = np.random.default_rng(20)
    per = rng.integers(1, 4, cols)
    rows = np.repeat(np.arange(cols), per)
    tags = np.concatenate([rng.choice(20, m, replace=False) for m in per])
    if config == "c":
        rows = np.concatenate([rows, np.arange(cols)])
        tags = np.concatenate([tags, np.full(cols, 20)])
    return mfx.hyb_features(cols, rows, tags, 21 if config == "c" else 20)


def spread_bytes(mfx, host, Fi, k, batch, seed):
    """8 k bytes per entry of every row the first step touches (skipped slots left out; bad slots do not occur here)."""
    from mfx import _lib as L
    rows, cols, rp, ci = host
    u, i, j = (np.empty(batch, np.uint32) for _ in range(3))
    sk = np.empty(batch, np.uint8)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    csx = L.mfx_csx(rows, cols, ci.size, None, None, None, vp(rp), vp(ci), None)  # (the sampler reads the CSR pointers and ids only)
    L.check(mfx.lib().mfx_bpr_triples(seed, 0, batch, C.byref(csx), u.ctypes.data_as(L.u32p), i.ctypes.data_as(L.u32p),
                                      j.ctypes.data_as(L.u32p), vp(sk)))
    sk = sk.astype(bool)
    users = np.unique(u[~sk]).size
    items = np.unique(np.concatenate([i[~sk], j[~sk]]))
    per = np.ones(cols, np.int64) if Fi is None else np.diff(Fi.ptr.astype(np.int64))
    return {"touched_users": int(users), "touched_items": int(items.size), "feature_entries_of_touched_rows": int(users + per[items].sum()),
            "atomic_bytes": int((users + per[items].sum()) * 8 * k)}


def embed_seconds(torch, mfx, s, reps=5):
    """Seconds of embedding every user and every item into device memory (mfx_hyb_get_factors, one side at a time)."""
    from mfx import _lib as L
    out = {}
    for side, n in (("users", s.rows), ("items", s.cols)):
        X = torch.empty(n, s.k, device="cuda:0")
        ptr = C.c_void_p(X.data_ptr())
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            L.check(mfx.lib().mfx_hyb_get_factors(s.handle, ptr if side == "users" else None, ptr if side == "items" else None, L.MFX_DEVICE))
            ts.append(time.perf_counter() - t0)
        out[side + "_ms"] = round(float(np.median(ts[1:])) * 1e3, 4)
        out[side + "_written_gb_per_s"] = round(n * s.k * 4 / float(np.median(ts[1:])) / 1e9, 1)
    return out


def point(torch, mfx, d, host, a, k, batch, config):
    p = mfx.parameter()
    p.k, p.lambda_ = k, a.lam
    nnz = int(d["csr_val"].numel())
    Fi = item_features(mfx, a.cols, config)
    lr = a.lr * min(1.0, 65536 / batch)  # (a batch is the sum of its slots' steps: --lr is the rate at 65 536 slots)
    rec = {"k": k, "batch": batch, "config": config, "lr": lr, "steps_per_epoch": -(-nnz // batch), "timed_steps": a.steps,
           "item_features": "identity" if Fi is None else {"nf": Fi.nf, "entries": int(Fi.ptr[-1])}}
    b = mfx.BprSolver(None, p, lr, batch, seed=1, device_arrays=d, init_seed=k)
    h = mfx.HybridSolver(None, p, lr, batch, item_features=Fi, seed=1, device_arrays=d, init_seed=k)
    b.steps(a.warm)
    h.steps(a.warm)
    tb, th = [], []
    for _ in range(a.rounds):  # alternated in the same process
        tb.append(b.steps(a.steps)["seconds"] / a.steps)
        e = h.steps(a.steps)
        th.append(e["seconds"] / a.steps)
    rec.update({"bpr_step_ms": round(float(np.median(tb)) * 1e3, 4), "hyb_step_ms": round(float(np.median(th)) * 1e3, 4),
                "step_ratio_to_bpr": round(float(np.median(th) / np.median(tb)), 3), "bad": e["bad"], "auc_of_the_steps": round(e["auc"], 4)})
    eb, eh = b.iterate(1)[0], h.iterate(1)[0]  # (finishes the started epoch: scaled to a whole one by its slots)
    rec["bpr_epoch_ms"] = round(eb["seconds"] * 1e3 * nnz / eb["slots"], 2)
    rec["hyb_epoch_ms"] = round(eh["seconds"] * 1e3 * nnz / eh["slots"], 2)
    rec["embed_all_rows"] = embed_seconds(torch, mfx, h)
    b.close()
    h.close()
    p.profile = 1
    h = mfx.HybridSolver(None, p, lr, batch, item_features=Fi, seed=1, device_arrays=d, init_seed=k)
    h.steps(2)
    t0 = h.kernel_times()
    h.steps(a.profile_steps)
    t1 = h.kernel_times()
    h.close()
    split = {name: (t1[name] - t0[name]) / a.profile_steps for name in t1}
    rec["ms_per_step"] = {name: round(v * 1e3, 4) for name, v in split.items()}
    sb = spread_bytes(mfx, host, Fi, k, batch, 1)
    rec["spread"] = dict(sb, tb_per_s=round(sb["atomic_bytes"] / split["spread"] / 1e12, 4), scatter_yardstick_tb_per_s=list(SCATTER_TBS))
    return rec


def lgcn_child(a):
    sys.path.insert(0, a.lgcn_child)
    import torch
    import mfx
    assert os.path.dirname(os.path.dirname(os.path.abspath(mfx.__file__))) == os.path.abspath(a.lgcn_child)
    d = matrix(a, torch)
    p = mfx.parameter()
    p.k, p.lambda_ = 64, 0.01
    s = mfx.LightGcnSolver(None, p, 0.05, 65536, 2, seed=1, device_arrays=d, init_seed=64)
    s.steps(2)
    ms = s.steps(5)["seconds"] / 5 * 1e3
    s.close()
    print(json.dumps({"lgcn_step_ms_k64_L2_batch65536": ms}))


def regress(a):
    shape = ["--rows", str(a.rows), "--cols", str(a.cols), "--nnz", str(a.nnz)]
    lines = []
    for run in range(a.regress_runs):
        for tree, pkg in (("parent", os.path.abspath(a.parent_pkg)), ("this", PKG)):
            jobs = (("bpr_bench --regress-child", [os.path.join(ROOT, "tools", "bpr_bench.py"), "--regress-child", pkg] + shape),
                    ("hyb_bench --lgcn-child", [os.path.abspath(__file__), "--lgcn-child", pkg] + shape),
                    # (each tree's own bench.py beside its package: the checkout of the parent commit is whole)
                    ("bench", [os.path.join(os.path.dirname(pkg), "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"]))
            for tool, cmd in jobs:
                t0 = time.perf_counter()
                r = subprocess.run([sys.executable] + cmd, stdout=subprocess.PIPE, text=True, check=True, timeout=600)
                res = json.loads(r.stdout.strip().splitlines()[-1])
                if tool == "bench":
                    res = {key: res[key] for key in ("metric", "value", "unit", "ms_per_step")}
                lines.append({"run": run, "tool": tool, "tree": tree, "seconds": round(time.perf_counter() - t0, 1), "result": res})
                print(json.dumps(lines[-1]), file=sys.stderr, flush=True)
    with open(a.ab_out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=480189)
    ap.add_argument("--cols", type=int, default=17770)
    ap.add_argument("--nnz", type=int, default=99_072_112)
    ap.add_argument("--ks", default="64,128")
    ap.add_argument("--batches", default="65536,1048576")
    ap.add_argument("--configs", default="a,b,c")
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--lam", type=float, default=1e-6)  # (lr * lambda * m_f of the tag on every item stays small at batch 2^20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--profile-steps", type=int, default=5)
    ap.add_argument("--parent-pkg", default=None)
    ap.add_argument("--regress-runs", type=int, default=4)
    ap.add_argument("--lgcn-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hyb_bench.json"))
    ap.add_argument("--ab-out", default=os.path.join(ROOT, "profiles", "hyb_bench_ab.jsonl"))
    a = ap.parse_args()
    if a.lgcn_child:
        return lgcn_child(a)
    sys.path.insert(0, PKG)
    import torch
    import mfx
    out = {"tool": "hyb_bench", "rows": a.rows, "cols": a.cols, "nnz": a.nnz, "lr": a.lr, "lambda": a.lam, "points": []}
    ks = [int(x) for x in a.ks.split(",") if x]
    if ks:
        d = matrix(a, torch)
        rp, ci = d["csr_row_ptr"].cpu().numpy().view(np.uint32), d["csr_col_idx"].cpu().numpy().view(np.uint32)
        host = (a.rows, a.cols, np.ascontiguousarray(rp), np.ascontiguousarray(ci))
        for k in ks:
            for batch in (int(x) for x in a.batches.split(",") if x):
                for config in (c for c in a.configs.split(",") if c):
                    out["points"].append(point(torch, mfx, d, host, a, k, batch, config))
                    print(json.dumps(out["points"][-1]), file=sys.stderr, flush=True)
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out, "w") as f:  # (kept up to date: a run cut short leaves its finished points)
                        f.write(json.dumps(out) + "\n")
        del d
        torch.cuda.empty_cache()
        print(json.dumps(out))
    if a.parent_pkg:
        regress(a)


if __name__ == "__main__":
    main()
