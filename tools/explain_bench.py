"""Explanations of fold-in recommendations at the Netflix shape: ms per mfx_rec_explain call next to the fold-in it sits on.

Builds the Netflix-shaped synthetic matrix on the GPU (mfx.synth_torch, as tools/foldin_bench.py does) and a random H in a
recommender handle set up for MFX_FOLD_IMPLICIT.  The query rows are training rows: 1, 64 and 1 024 seeded random users and
all 480 189 rows in order, as device tensors.  The targets of a row are the items of fold_in(n_top = 10) for it,
n_expl = 10.  Per k and batch, alternated in one process, warm: fold_in(n_top = 10) (the work an explanation sits on top
of) and explain, ms per call (median / min / max of --reps, host clock around the call, which ends in a stream
synchronisation) with the phases of mfx_rec_fold_in_times / mfx_rec_explain_times of the median call (explain with
max_ws_bytes large enough for one piece: Z of all users is 1.2 GB at k = 64, 2.5 GB at k = 128).  For the 1 024-user
batch also a torch baseline on the device: padded gather of the rows of H, the batched systems by bmm, cholesky,
cholesky_solve against the target rows, bmm for the contributions, topk.

With --parent-pkg DIR (a built cuda-recommender_amd tree of the parent commit): the unchanged all-user fold_in(n_top = 10)
and query(10) at k = 64 on that tree and on this one, alternated, --regress-runs fresh processes each.

With --cg [--k 256]: mfx_rec_explain_cg instead, after fold_in_cg_setup(MFX_FOLD_IMPLICIT, tol = 1e-4) at alpha = 1 and
alpha = 40: the same batches, targets and n_expl; per batch fold_in(n_top = 10) and explain_cg under the same setup,
alternated, with their phases, the step counts, and the solve phase per target relative to fold-in's solve:
(explain_cg solve - fold_in solve) / n_targets / fold_in solve -- below 1 where the targets of a slot share the gathered rows.
With --parent-pkg the unchanged paths are the all-user query(10) at k = 64 and the all-user cg fold-in at --k.

Prints ONE JSON line (also to --out FILE).

    python tools/explain_bench.py [--reps 5] [--ks 64,128] [--cg [--k 256]] [--parent-pkg DIR] [--regress-runs 4] [--out FILE]
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
ROWS, COLS, NNZ = 480189, 17770, 99_072_112
LAM, ALPHA, N_TOP, N_EXPL = 0.05, 1.0, 10, 10
CG_TOL, CG_ALPHAS = 1e-4, (1.0, 40.0)


def timed(fn, reps, sync):
    fn()
    sync()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def stats(ms):
    return {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}


def data(seed, k, torch, dev):
    from mfx import synth_torch
    d = synth_torch.synth_ratings_device(ROWS, COLS, NNZ, seed=seed, device="cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(k)
    H = (torch.randn(int(d["cols"]), k, generator=g, device=dev) * 0.3).contiguous()
    return d, H


def regress_child(a):
    """All-user fold_in(n_top = 10) and query(10) at k = 64 with the package in a.regress_child: one JSON line."""
    sys.path.insert(0, a.regress_child)
    import torch
    import mfx
    dev = torch.device("cuda:0")
    d, H = data(a.seed, 64, torch, dev)
    q = (d["csr_row_ptr"], d["csr_col_idx"], d["csr_val"])
    gw = torch.Generator(device=dev)
    gw.manual_seed(7)
    W = (torch.randn(int(d["rows"]), 64, generator=gw, device=dev) * 0.3).contiguous()
    with mfx.Recommender(W, H, 1) as r:
        r.fold_in_setup(mfx.MFX_FOLD_IMPLICIT, LAM, ALPHA)
        fold = timed(lambda: r.fold_in(q, N_TOP), a.reps, torch.cuda.synchronize)
        query = timed(lambda: r.query(N_TOP, on_device=True), a.reps, torch.cuda.synchronize)
    print(json.dumps({"fold_in_ms": float(np.median(fold)), "query_ms": float(np.median(query))}))
    return 0


def cg_regress_child(a):
    """All-user query(10) at k = 64 and all-user cg fold_in(n_top = 10) at k = a.k, tol = 1e-4, with the package in
    a.regress_child: one JSON line."""
    sys.path.insert(0, a.regress_child)
    import torch
    import mfx
    dev = torch.device("cuda:0")
    d, H = data(a.seed, 64, torch, dev)
    gw = torch.Generator(device=dev)
    gw.manual_seed(7)
    W = (torch.randn(int(d["rows"]), 64, generator=gw, device=dev) * 0.3).contiguous()
    with mfx.Recommender(W, H, 1) as r:
        query = timed(lambda: r.query(N_TOP, on_device=True), a.reps, torch.cuda.synchronize)
    del W, H
    q = (d["csr_row_ptr"], d["csr_col_idx"], d["csr_val"])
    g = torch.Generator(device=dev)
    g.manual_seed(a.k)
    H = (torch.randn(int(d["cols"]), a.k, generator=g, device=dev) * 0.3).contiguous()
    with mfx.Recommender(torch.zeros(1, a.k, device=dev), H, 1) as r:
        r.fold_in_cg_setup(mfx.MFX_FOLD_IMPLICIT, LAM, ALPHA, steps=64, tol=CG_TOL)
        fold = timed(lambda: r.fold_in(q, N_TOP), a.reps, torch.cuda.synchronize)
    print(json.dumps({"fold_in_ms": float(np.median(fold)), "query_ms": float(np.median(query))}))
    return 0


def cg_points(a, mfx, torch, dev, H, batches, alpha):
    """fold_in(n_top = 10) and explain_cg under one cg setup, alternated, per batch."""
    sync = torch.cuda.synchronize
    points = []
    with mfx.Recommender(torch.zeros(1, a.k, device=dev), H, 1) as r:
        r.fold_in_cg_setup(mfx.MFX_FOLD_IMPLICIT, LAM, alpha, steps=64, tol=CG_TOL)
        for name, q in batches.items():
            targets = r.fold_in(q, N_TOP)[0]
            call = lambda: r.explain_cg(q, targets, N_EXPL, return_steps=True, max_ws_bytes=1 << 40)
            fold, expl, fsplit, esplit = [], [], [], []
            r.fold_in(q, N_TOP)
            res = call()
            sync()
            for _ in range(a.reps):                          # alternated
                t0 = time.perf_counter()
                r.fold_in(q, N_TOP)
                sync()
                fold.append((time.perf_counter() - t0) * 1e3)
                fsplit.append(r.fold_in_times())
                t0 = time.perf_counter()
                call()
                sync()
                expl.append((time.perf_counter() - t0) * 1e3)
                esplit.append(r.explain_times())
            fm, em = int(np.argsort(fold)[len(fold) // 2]), int(np.argsort(expl)[len(expl) // 2])
            ts, rs = res["target_steps"].float(), res["row_steps"].float()
            pt = {"batch": name, "users": int(q[0].numel()) - 1, "nnz": int(q[1].numel()), "alpha": alpha,
                  "fold_in": dict(stats(fold), phases_ms={key: round(v * 1e3, 3) for key, v in fsplit[fm].items()}),
                  "explain_cg": dict(stats(expl), phases_ms={key: round(v * 1e3, 3) for key, v in esplit[em].items()}),
                  "row_steps_mean_max": [round(float(rs.mean()), 3), int(rs.max())],
                  "target_steps_mean_max": [round(float(ts.mean()), 3), int(ts.max())]}
            fs, es = pt["fold_in"]["phases_ms"]["solve"], pt["explain_cg"]["phases_ms"]["solve"]
            pt["explain_cg_over_fold_in"] = round(pt["explain_cg"]["ms_median"] / pt["fold_in"]["ms_median"], 3)
            pt["target_solve_per_target_over_fold_in_solve"] = round((es - fs) / N_TOP / fs, 3)
            points.append(pt)
            print(json.dumps(pt), file=sys.stderr, flush=True)
    return points


def torch_explain(torch, H, G, q, targets):
    """The same answer from torch ops on the device for one batch: (items, contrib) [U, T, n_expl]."""
    ptr, idx, val = q
    U = ptr.numel() - 1
    lens = (ptr[1:] - ptr[:-1]).long()
    L = int(lens.max())
    pos = torch.arange(L, device=H.device)[None, :]
    live = pos < lens[:, None]
    src = (ptr[:-1].long()[:, None] + pos).clamp(max=idx.numel() - 1)
    ids = torch.where(live, idx.long()[src], torch.zeros_like(src))
    r = torch.where(live, val[src], torch.zeros_like(val[src]))
    Hg = H[ids] * live[:, :, None]                          # [U, L, k]
    w = ALPHA * r
    A = G[None] + torch.bmm((Hg * w[:, :, None]).transpose(1, 2), Hg)
    Lc = torch.linalg.cholesky(A)
    Ht = H[targets.long().clamp(min=0)]                     # [U, T, k]
    Z = torch.cholesky_solve(Ht.transpose(1, 2), Lc)        # [U, k, T]
    c = torch.bmm(Hg, Z) * (1.0 + w)[:, :, None]            # [U, L, T]
    c = torch.where((live & (r > 0))[:, :, None], c, torch.full_like(c, float("-inf")))
    top = torch.topk(c.transpose(1, 2), min(N_EXPL, L), dim=2)
    return torch.gather(ids[:, None, :].expand(-1, targets.shape[1], -1), 2, top.indices), top.values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ks", default="64,128")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--cg", action="store_true", help="mfx_rec_explain_cg under fold_in_cg_setup at rank --k")
    ap.add_argument("--k", type=int, default=256)
    ap.add_argument("--parent-pkg", default=None)
    ap.add_argument("--regress-runs", type=int, default=4)
    ap.add_argument("--regress-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.regress_child:
        return cg_regress_child(a) if a.cg else regress_child(a)
    sys.path.insert(0, PKG)
    import torch
    import mfx
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    out = {"tool": "explain_bench", "workload": f"{ROWS}x{COLS} nnz={NNZ}", "model": "IMPLICIT", "lambda": LAM, "alpha": ALPHA,
           "n_targets": N_TOP, "n_expl": N_EXPL, "reps": a.reps, "query_arrays": "device", "cases": []}
    if a.cg:
        out.update(tool="explain_bench --cg", alpha=list(CG_ALPHAS), k=a.k, steps=64, tol=CG_TOL)
    for k in [a.k] if a.cg else [int(x) for x in a.ks.split(",") if x]:
        d, H = data(a.seed, k, torch, dev)
        rows = int(d["rows"])
        rp, ci, cv = d["csr_row_ptr"], d["csr_col_idx"], d["csr_val"]
        rp_h = rp.cpu().numpy().astype(np.int64)

        def batch(users):
            lo, hi = rp_h[users], rp_h[users + 1]
            ptr = np.zeros(len(users) + 1, np.int64)
            ptr[1:] = np.cumsum(hi - lo)
            pos = torch.from_numpy(np.concatenate([np.arange(x, y) for x, y in zip(lo, hi)])).to(dev)
            return torch.from_numpy(ptr.astype(np.int32)).to(dev), ci[pos].contiguous(), cv[pos].contiguous()

        batches = {str(n): batch(np.sort(np.random.default_rng(n).choice(rows, n, replace=False))) for n in (1, 64, 1024)}
        batches["all"] = (rp, ci, cv)
        case = {"k": k, "points": []}
        if a.cg:
            for alpha in CG_ALPHAS:
                case["points"] += cg_points(a, mfx, torch, dev, H, batches, alpha)
            out["cases"].append(case)
            break
        with mfx.Recommender(torch.zeros(1, k, device=dev), H, 1) as r:
            r.fold_in_setup(mfx.MFX_FOLD_IMPLICIT, LAM, ALPHA)
            for name, q in batches.items():
                targets = r.fold_in(q, N_TOP)[0]
                fold, expl, fsplit, esplit = [], [], [], []
                r.fold_in(q, N_TOP)
                r.explain(q, targets, N_EXPL, max_ws_bytes=1 << 40)
                sync()
                for _ in range(a.reps):                      # alternated
                    t0 = time.perf_counter()
                    r.fold_in(q, N_TOP)
                    sync()
                    fold.append((time.perf_counter() - t0) * 1e3)
                    fsplit.append(r.fold_in_times())
                    t0 = time.perf_counter()
                    res = r.explain(q, targets, N_EXPL, max_ws_bytes=1 << 40)
                    sync()
                    expl.append((time.perf_counter() - t0) * 1e3)
                    esplit.append(r.explain_times())
                fm, em = int(np.argsort(fold)[len(fold) // 2]), int(np.argsort(expl)[len(expl) // 2])
                pt = {"batch": name, "users": int(q[0].numel()) - 1, "nnz": int(q[1].numel()),
                      "fold_in": dict(stats(fold), phases_ms={key: round(v * 1e3, 3) for key, v in fsplit[fm].items()}),
                      "explain": dict(stats(expl), phases_ms={key: round(v * 1e3, 3) for key, v in esplit[em].items()})}
                pt["explain_solve_over_fold_in_solve"] = round(pt["explain"]["phases_ms"]["solve"] / pt["fold_in"]["phases_ms"]["solve"], 3)
                if name == "1024":
                    G = (H.double().T @ H.double()).float() + LAM * torch.eye(k, device=dev)
                    tms = timed(lambda: torch_explain(torch, H, G, q, targets), a.reps, sync)
                    ti, tc = torch_explain(torch, H, G, q, targets)
                    first = res["items"][:, :, 0].long() & 0xFFFFFFFF
                    live = first != 0xFFFFFFFF
                    pt["torch_baseline"] = dict(stats(tms), speedup_vs_torch=round(float(np.median(tms)) / pt["explain"]["ms_median"], 2),
                                                first_item_agrees=round(float((ti[:, :, 0][live] == first[live]).float().mean()), 4))
                case["points"].append(pt)
                print(json.dumps(pt), file=sys.stderr, flush=True)
        out["cases"].append(case)
        del d, H, rp, ci, cv, batches
        torch.cuda.empty_cache()
    if a.parent_pkg:
        runs = {"parent": [], "this": []}
        for _ in range(a.regress_runs):
            for name, pkg in (("parent", os.path.abspath(a.parent_pkg)), ("this", PKG)):
                cmd = [sys.executable, os.path.abspath(__file__), "--regress-child", pkg, "--reps", str(a.reps), "--seed", str(a.seed)]
                cmd += ["--cg", "--k", str(a.k)] if a.cg else []
                p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True, timeout=300)
                runs[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
        reg = {"workload": f"all users, N = 10: query at k = 64, cg fold-in (IMPLICIT, tol = {CG_TOL}) at k = {a.k}" if a.cg
               else "all users, k = 64, N = 10, IMPLICIT"}
        for key in ("fold_in_ms", "query_ms"):
            pv, tv = [x[key] for x in runs["parent"]], [x[key] for x in runs["this"]]
            spread = max(pv) - min(pv)
            reg[key] = {"parent": pv, "this": tv, "parent_median": float(np.median(pv)), "this_median": float(np.median(tv)),
                        "parent_spread": spread, "no_slower": bool(np.median(tv) <= np.median(pv) + spread),
                        "ranges_overlap": bool(min(tv) <= max(pv) and min(pv) <= max(tv))}
        out["regression"] = reg
        print(json.dumps(reg), file=sys.stderr, flush=True)
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
