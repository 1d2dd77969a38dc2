"""Fold-in recommendation at the Netflix shape: ms per batch of query users, split into host build / solve / score.

Builds the Netflix-shaped synthetic matrix on the GPU (mfx.synth_torch, as tools/ials_bench.py does) and a random H
(k = 64) in a recommender handle.  The query rows are training rows of that matrix, so every batch is one the trainers
themselves solve: 1, 64 and 1 024 seeded random users, and all 480 189 rows in order.  Query arrays are device tensors.
For models ALS and IMPLICIT at N = 10 it prints ONE JSON line: per (model, batch) the median / min / max ms per
mfx_rec_fold_in call over --reps (host clock around the call, which ends in a stream synchronisation) and the split of
the median call into host build (query copies, checks, the host-side split into work items), solve and score, as
mfx_rec_fold_in_times reports it.

With --block D the model is fold-in by block subspace sweeps instead (mfx_rec_fold_in_block_setup, any k <= 1024, D = 0: the
default block): at most --sweeps sweeps per row from w = 0, stopped per row by --tol when it is > 0.  Each run then also
reports the sweeps the slowest row took, the mean over the non-empty rows, and the share of row-sweeps that were spent
on rows already frozen (every sweep runs over the whole batch).

--explicit (with --block) runs the sweeps on the explicit objective (mfx_rec_fold_in_block_setup_als, --reg 0 / 1).

--alpha0 A --nu V (either one; a lone alpha0 means nu = 0, a lone nu means alpha0 = 1) run the implicit model, direct or with
--block, on the objective with an unobserved weight and a frequency-scaled regulariser (mfx_rec_fold_in_setup_reg /
mfx_rec_fold_in_block_setup_reg); without --block the model is then IMPLICIT_REG alone.  Not with --explicit.

--cg runs fold-in by preconditioned conjugate gradients (mfx_rec_fold_in_cg_setup; --steps S, --tol T, --explicit --reg R
for the explicit objectives): the same batches and the same record, the step statistics in the fields of the sweep
statistics (steps_max, steps_mean, frozen_row_steps_share).  Its workspace is 20 k bytes per row on top of the rows
themselves: the all-user batch is cut into equal pieces of at most --max-ws-bytes of workspace, the cut is printed and the
times of the pieces are summed.

--accuracy N (with --block or --cg, the implicit objective): for N seeded users the relative distance |w - w*| / |w*| of the
rows the setup returns to the fp64 dense solve of the same rows (G = H^T H + lambda I in fp64), worst and median.

    python tools/foldin_bench.py [--reps 5] [--k 64] [--n-top 10] [--block D --sweeps S --tol T [--explicit [--reg R]]]
                                 [--cg --steps S --tol T [--explicit [--reg R]]] [--alpha0 A --nu V] [--accuracy N]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-recommender_amd"))

ROWS, COLS, NNZ = 480189, 17770, 99_072_112


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--n-top", type=int, default=10)
    ap.add_argument("--lam", type=float, default=0.05)
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--block", type=int, default=None, help="fold-in by block sweeps with blocks of D coordinates (0: default)")
    ap.add_argument("--sweeps", type=int, default=8)
    ap.add_argument("--tol", type=float, default=0.0)
    ap.add_argument("--cg", action="store_true", help="fold-in by preconditioned conjugate gradients (mfx_rec_fold_in_cg_setup)")
    ap.add_argument("--steps", type=int, default=64, help="with --cg: the most steps a row gets")
    ap.add_argument("--max-ws-bytes", type=int, default=8 << 30, help="with --cg: workspace bound that cuts the all-user batch")
    ap.add_argument("--accuracy", type=int, default=0, help="users whose rows are compared with the fp64 dense solve")
    ap.add_argument("--explicit", action="store_true", help="with --block / --cg: the explicit objective")
    ap.add_argument("--reg", type=int, default=0, help="with --explicit: 0 = lambda, 1 = lambda * entries of the row")
    ap.add_argument("--alpha0", type=float, default=None, help="weight of the unobserved pairs (the _reg setups)")
    ap.add_argument("--nu", type=float, default=None, help="exponent of the frequency-scaled regulariser, 0..1")
    a = ap.parse_args()
    if a.explicit and a.block is None and not a.cg:
        ap.error("--explicit needs --block or --cg")
    if a.cg and a.block is not None:
        ap.error("--cg and --block exclude each other")
    if a.accuracy and (a.explicit or not (a.cg or a.block is not None)):
        ap.error("--accuracy compares the implicit objective of --block or --cg")
    reg = {key: v for key, v in (("alpha0", a.alpha0), ("nu", a.nu)) if v is not None}
    if reg and (a.explicit or a.cg):
        ap.error("--alpha0 / --nu apply to the implicit objective of the direct and the block setups")
    import torch
    import mfx
    from mfx import synth_torch
    dev = torch.device("cuda:0")
    d = synth_torch.synth_ratings_device(ROWS, COLS, NNZ, seed=a.seed, device="cuda:0")
    rows, cols = int(d["rows"]), int(d["cols"])
    rp, ci, cv = d["csr_row_ptr"], d["csr_col_idx"], d["csr_val"]
    rp_h = rp.cpu().numpy().astype(np.int64)
    nnz = int(rp_h[-1])
    g = torch.Generator(device=dev)
    g.manual_seed(a.k)
    H = (torch.randn(cols, a.k, generator=g, device=dev) * 0.3).contiguous()
    W = torch.zeros(1, a.k, device=dev)

    def batch(users):
        """Device CSR of the given training rows."""
        lo, hi = rp_h[users], rp_h[users + 1]
        ptr = np.zeros(len(users) + 1, np.int64)
        ptr[1:] = np.cumsum(hi - lo)
        pos = torch.from_numpy(np.concatenate([np.arange(x, y) for x, y in zip(lo, hi)])).to(dev)
        return torch.from_numpy(ptr.astype(np.int32)).to(dev), ci[pos].contiguous(), cv[pos].contiguous()

    batches = {str(n): batch(np.sort(np.random.default_rng(n).choice(rows, n, replace=False))) for n in (1, 64, 1024)}
    batches["all"] = (rp, ci, cv)
    out = {"tool": "foldin_bench", "workload": f"{rows}x{cols} nnz={nnz}", "k": a.k, "n_top": a.n_top, "lambda": a.lam,
           "alpha": a.alpha, "reps": a.reps, "query_arrays": "device", "runs": []}
    by_blocks = a.block is not None
    if by_blocks:
        out.update({"block": a.block, "sweeps": a.sweeps, "tol": a.tol})
    if a.cg:
        out.update({"cg": True, "steps": a.steps, "tol": a.tol})
    if a.explicit:
        out.update({"explicit": True, "reg": a.reg})
    counted = by_blocks or a.cg  # the setups that report a count per row
    unit = "steps" if a.cg else "sweeps"

    def pieces(q):
        """The batch as it is, or (--cg) cut into equal runs of rows whose workspace stays below --max-ws-bytes."""
        users = int(q[0].numel()) - 1
        per = max(1, a.max_ws_bytes // (20 * a.k))
        if not a.cg or users <= per:
            return [q]
        n = -(-users // per)
        per = -(-users // n)
        ptr = q[0].cpu().numpy().astype(np.int64)
        cut = []
        for lo in range(0, users, per):
            hi = min(users, lo + per)
            cut.append(((q[0][lo:hi + 1] - q[0][lo]).contiguous(), q[1][ptr[lo]:ptr[hi]].contiguous(), q[2][ptr[lo]:ptr[hi]].contiguous()))
        print(f"foldin_bench: {users} users cut into {len(cut)} pieces of at most {per} rows "
              f"({20 * a.k * per / 2 ** 30:.2f} GiB of workspace each)", file=sys.stderr, flush=True)
        return cut

    def dense_rows(users):
        """fp64 dense solves of the implicit objective for the given training rows (host)."""
        Hd = H.double().cpu().numpy()
        G = Hd.T @ Hd + float(np.float32(a.lam)) * np.eye(a.k)
        ci_h, cv_h = ci.cpu().numpy(), cv.cpu().numpy()
        Y = np.zeros((len(users), a.k))
        for n, u in enumerate(users):
            j, v = ci_h[rp_h[u]:rp_h[u + 1]].astype(np.int64), cv_h[rp_h[u]:rp_h[u + 1]]
            j, w = j[v > 0], (np.float32(a.alpha) * v[v > 0]).astype(np.float64)
            if j.size:
                Hj = Hd[j]
                Y[n] = np.linalg.solve(G + (Hj * w[:, None]).T @ Hj, Hj.T @ (1.0 + w))
        return Y

    if reg:
        out.update({"alpha0": 1.0 if a.alpha0 is None else a.alpha0, "nu": 0.0 if a.nu is None else a.nu})
    models = (("BLOCK_ALS" if a.explicit else "BLOCK", None),) if by_blocks else (("ALS", mfx.MFX_FOLD_ALS), ("IMPLICIT", mfx.MFX_FOLD_IMPLICIT))
    if a.cg:
        models = ((("CG_CCD", mfx.MFX_FOLD_CCD) if a.reg else ("CG_ALS", mfx.MFX_FOLD_ALS)) if a.explicit else ("CG_IMPLICIT", mfx.MFX_FOLD_IMPLICIT),)
    if reg:
        models = (("BLOCK_REG", None),) if by_blocks else (("IMPLICIT_REG", mfx.MFX_FOLD_IMPLICIT),)
    with mfx.Recommender(W, H, 1) as r:
        for name, model in models:
            t0 = time.perf_counter()
            if a.cg:
                r.fold_in_cg_setup(model, a.lam, a.alpha, steps=a.steps, tol=a.tol)
            elif by_blocks and a.explicit:
                r.fold_in_block_setup_als(a.lam, block=a.block, sweeps=a.sweeps, tol=a.tol, count_reg=bool(a.reg))
            elif by_blocks and reg:
                r.fold_in_block_setup_reg(a.lam, a.alpha, out["alpha0"], out["nu"], block=a.block, sweeps=a.sweeps, tol=a.tol)
            elif by_blocks:
                r.fold_in_block_setup(a.lam, a.alpha, block=a.block, sweeps=a.sweeps, tol=a.tol)
            else:
                r.fold_in_setup(model, a.lam, a.alpha, **reg)
            setup_ms = (time.perf_counter() - t0) * 1e3
            if a.accuracy:
                users = np.sort(np.random.default_rng(a.accuracy).choice(rows, a.accuracy, replace=False))
                got = r.fold_in(batch(users), 0)[2].double().cpu().numpy()
                want = dense_rows(users)
                live = np.linalg.norm(want, axis=1) > 0
                dist = np.linalg.norm(got[live] - want[live], axis=1) / np.linalg.norm(want[live], axis=1)
                out["accuracy"] = {"users": int(live.sum()), "worst_rel": float(dist.max()), "median_rel": float(np.median(dist))}
                print(json.dumps(out["accuracy"]), file=sys.stderr, flush=True)
            for bname, q in batches.items():
                cut = pieces(q)
                for piece in cut:  # warm-up
                    r.fold_in(piece, a.n_top)
                torch.cuda.synchronize()
                ms, split = [], []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    phases = {}
                    for piece in cut:
                        r.fold_in(piece, a.n_top)
                        for key, v in r.fold_in_times().items():
                            phases[key] = phases.get(key, 0.0) + v
                    torch.cuda.synchronize()
                    ms.append((time.perf_counter() - t0) * 1e3)
                    split.append(phases)
                med = int(np.argsort(ms)[len(ms) // 2])
                run = {"model": name, "batch": bname, "users": int(q[0].numel()) - 1, "nnz": int(q[1].numel()),
                       "setup_ms": round(setup_ms, 3), "ms_median": round(float(np.median(ms)), 3),
                       "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}
                run.update({f"{key}_ms": round(v * 1e3, 3) for key, v in split[med].items()})
                if len(cut) > 1:
                    run["pieces"] = len(cut)
                if counted:
                    done = np.concatenate([r.fold_in(piece, 0, return_sweeps=True)[3].cpu().numpy() for piece in cut])
                    live = done[done > 0]
                    longest = int(done.max()) if done.size else 0
                    run.update({f"{unit}_max": longest, f"{unit}_mean": round(float(live.mean()), 3) if live.size else 0.0,
                                f"frozen_row_{unit}_share": round(1.0 - float(live.sum()) / (longest * live.size), 4) if live.size else 0.0})
                out["runs"].append(run)
                print(json.dumps(run), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
