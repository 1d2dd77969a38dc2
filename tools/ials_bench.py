"""Implicit-feedback ALS at the Netflix shape: time per iteration against explicit ALS on the same matrix.

Builds the Netflix-shaped synthetic matrix on the GPU (mfx.synth_torch, as bench.py does; the ratings 1..5 are taken
as interaction strengths) and prints ONE JSON line with, for every k: ms per implicit iteration and per half-sweep,
the two base Gramians (X^T X + lambda I), explicit ALS ms per iteration on the same matrix in the same run, the flop
of an iteration and its fraction of the 157.3 TF fp32 MFMA peak, and the objective (mfx_ials_loss) after each
iteration.

--block k:d,k:d,... adds runs of the block subspace sweeps (mfx_ials_block_create: rank k in blocks of d coordinates,
the only implicit solver above k = 128) after the exact ones, from the same H0 (W = 0) on the same matrix in the same
process: ms per iteration, the loss after every iteration (a different method: read loss against time, not time
alone), the flop and the gathered bytes of an iteration from the shapes.  --again repeats the exact runs at the end
(the spread of the yardstick inside the job).

--explicit-block k:d,k:d,... adds runs of EXPLICIT ALS by block subspace sweeps (mfx_als_block_create, --reg 0 / 1) on
the same matrix, the ratings taken as ratings: ms per iteration and per half-sweep, the test RMSE after every iteration,
flop and gathered bytes from the shapes (no base Gramian, no G y product).

--alpha0 A --nu V (either one; a lone alpha0 means nu = 0, a lone nu means alpha0 = 1) run the implicit solvers, exact and
--block alike, on the objective with an unobserved weight and a frequency-scaled regulariser (mfx_ials_create_reg /
mfx_ials_block_create_reg); the record then carries "alpha0" and "nu".  Explicit runs are not affected.

--cg STEPS:TOL adds runs of the conjugate-gradient trainer (mfx_ials_cg_create) at every rank of --cg-ks (default: --ks)
from the same H0 (W cold): ms per iteration (every iteration listed: warm starts change the steps), the split Gramian /
inverse / solve, mean and most steps per half from mfx_ials_cg_stats and the loss after every iteration; and the time of
the device inverse alone (the trainer's ialscg_inverse on a small matrix) at k = 256 and 1024, next to the whole
mfx_spd_inverse call from host pointers.

    python tools/ials_bench.py [--ks 64,128] [--block 128:64,256:64] [--explicit-block 256:64] [--reg 0] [--again] [--iters 5]
                               [--alpha 1.0] [--lam 0.05] [--alpha0 0.3 --nu 0.5] [--cg 64:1e-4 --cg-ks 256,1024]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-recommender_amd"))

PEAK_TF = 157.3
ROWS, COLS, NNZ = 480189, 17770, 99_072_112


def flop_per_iteration(rows, cols, nnz, k):
    """Flop of one iteration in bench.py's ALS convention (both halves: symmetric Gramian k (k + 1) and rhs 2 k per
    gathered entry) plus the two base Gramians (k (k + 1) per row of each factor)."""
    return 2.0 * (nnz * k * (k + 1) + 2.0 * nnz * k) + (rows + cols) * k * (k + 1)


def block_counts(rows, cols, nnz, k, d):
    """(flop, gathered bytes) of one block-sweep iteration from the shapes: per stored pair and half the symmetric
    block Gramians k (d + 1), the rhs 2 k, the score update 2 k and the scores 2 k; G[block, :] y for every segment
    2 k^2; the two base Gramians.  Gathered: per stored pair and half three passes over a full row (scores, block
    systems, score updates) of k floats."""
    flop = 2.0 * nnz * (k * (d + 1) + 6.0 * k) + (rows + cols) * (2.0 * k * k + k * (k + 1))
    return flop, 2.0 * 3.0 * nnz * k * 4.0


def explicit_block_counts(nnz, k, d):
    """(flop, gathered bytes) of one explicit block-sweep iteration: block_counts without the terms of the base Gramian."""
    return 2.0 * nnz * (k * (d + 1) + 6.0 * k), 2.0 * 3.0 * nnz * k * 4.0


def run_explicit_block(mfx, d_arrays, rows, cols, nnz, k, block, a):
    p = mfx.parameter()
    p.k, p.lambda_, p.log = k, a.lam, 1 if a.verbose else 0
    H0 = mfx.initial_col(cols, k)
    s = mfx.AlsSolver(None, None, p, device_arrays=d_arrays, block=block, count_reg=bool(a.reg))
    s.set_factors(H0)
    rmse = [r.rmse for r in s.iterate(a.iters)]  # the RMSE curve from H0 (these iterations also warm up)
    s.kernel_times()
    s.set_factors(H0)  # the same iterations again, warmed up: the times
    ms = [r.update_time * 1e3 for r in s.iterate(a.iters, with_rmse=False)]
    kt = s.kernel_times()
    s.close()
    per = {name: t * 1e3 / n for name, (t, n) in kt.items()}
    med = float(np.median(ms))
    fl, by = explicit_block_counts(nnz, k, block)
    return {"kind": "explicit_block", "k": k, "block": block, "reg": a.reg, "ms_per_iteration": round(med, 3), "ms_min": round(min(ms), 3),
            "ms_max": round(max(ms), 3), "ms_user_half": round(per["alsb_half_rows(W over H)"], 3),
            "ms_item_half": round(per["alsb_half_cols(H over W)"], 3), "flop_per_iteration": fl,
            "fraction_of_fp32_mfma_peak": round(fl / (med * 1e-3) / (PEAK_TF * 1e12), 4), "gathered_bytes_per_iteration": by,
            "gathered_tb_per_s": round(by / (med * 1e-3) / 1e12, 3), "test_rmse_per_iteration": rmse}


def reg_kwargs(a):
    """alpha0= / nu= of ImplicitAlsSolver as the command line gave them (none: the un-suffixed entry points)."""
    kw = {}
    if a.alpha0 is not None:
        kw["alpha0"] = a.alpha0
    if a.nu is not None:
        kw["nu"] = a.nu
    return kw


def run_block(mfx, d_arrays, rows, cols, nnz, k, block, a):
    p = mfx.parameter()
    p.k, p.lambda_, p.log = k, a.lam, 1 if a.verbose else 0  # (log: the solver reports failed pivots on stdout)
    H0 = mfx.initial_col(cols, k)
    s = mfx.ImplicitAlsSolver(None, p, a.alpha, device_arrays=d_arrays, block=block, **reg_kwargs(a))
    s.set_factors(H0)
    losses = []
    for _ in range(a.iters):  # the loss curve from H0 (these iterations also warm up)
        s.iterate(1)
        losses.append(s.loss())
    s.kernel_times()
    s.set_factors(H0)  # the same five iterations again, warmed up: the times
    ms = [r.update_time * 1e3 for r in s.iterate(a.iters)]
    kt = s.kernel_times()
    s.close()
    per = {name: t * 1e3 / n for name, (t, n) in kt.items()}
    med = float(np.median(ms))
    fl, by = block_counts(rows, cols, nnz, k, block)
    return {"k": k, "block": block, "ms_per_iteration": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
            "ms_user_half": round(per["ialsb_half_rows(W over H)"], 3), "ms_item_half": round(per["ialsb_half_cols(H over W)"], 3),
            "ms_base_gram_H": round(per["ialsb_base_gram(H)"], 3), "ms_base_gram_W": round(per["ialsb_base_gram(W)"], 3),
            "flop_per_iteration": fl, "fraction_of_fp32_mfma_peak": round(fl / (med * 1e-3) / (PEAK_TF * 1e12), 4),
            "gathered_bytes_per_iteration": by, "gathered_tb_per_s": round(by / (med * 1e-3) / 1e12, 3),
            "loss_per_iteration": losses}


def run_cg(mfx, d_arrays, rows, cols, k, steps, tol, a):
    p = mfx.parameter()
    p.k, p.lambda_, p.log = k, a.lam, 1 if a.verbose else 0
    H0 = mfx.initial_col(cols, k)
    s = mfx.ImplicitAlsSolver(None, p, a.alpha, device_arrays=d_arrays, cg=(steps, tol))
    s.set_factors(H0)
    losses, stats = [], []
    for _ in range(a.iters):  # the loss curve and the steps from H0, W cold (these iterations also warm up)
        s.iterate(1)
        losses.append(s.loss())
        st = s.cg_stats()
        stats.append({"mean_steps_user_half": round(st["rows"]["row_steps"] / rows, 3), "max_steps_user_half": st["rows"]["max_steps"],
                      "mean_steps_item_half": round(st["cols"]["row_steps"] / cols, 3), "max_steps_item_half": st["cols"]["max_steps"],
                      "unconverged": st["rows"]["unconverged"] + st["cols"]["unconverged"],
                      "failed": st["rows"]["failed"] + st["cols"]["failed"]})
    s.kernel_times()
    s.set_factors(H0)  # the same iterations again, warmed up: the times
    ms = [r.update_time * 1e3 for r in s.iterate(a.iters)]
    kt = s.kernel_times()
    s.close()
    per = {name: t * 1e3 / n for name, (t, n) in kt.items()}
    return {"kind": "cg", "k": k, "steps": steps, "tol": tol, "ms_per_iteration": round(float(np.median(ms)), 3),
            "ms_of_every_iteration": [round(x, 3) for x in ms],
            "ms_solve_user_half": round(per["ialscg_half_rows(W over H)"], 3), "ms_solve_item_half": round(per["ialscg_half_cols(H over W)"], 3),
            "ms_base_gram_H": round(per["ialscg_base_gram(H)"], 3), "ms_base_gram_W": round(per["ialscg_base_gram(W)"], 3),
            "ms_inverse_H": round(per["ialscg_inverse(H)"], 3), "ms_inverse_W": round(per["ialscg_inverse(W)"], 3),
            "steps_per_iteration": stats, "loss_per_iteration": losses}


def inverse_times(mfx, ks=(256, 1024)):
    """ms of the device inverse alone (the trainer's ialscg_inverse events on a 600 x 500 matrix, after a warm-up iteration)
    and of a whole mfx_spd_inverse call from host pointers (allocation, upload, inverse, download)."""
    import time
    from mfx import dataset as ds
    rng = np.random.default_rng(7)
    mask = rng.random((600, 500)) < 0.05
    r, c = np.nonzero(mask)
    R = ds.from_coo(600, 500, r, c, np.ones(r.size, np.float32))
    out = []
    for k in ks:
        p = mfx.parameter()
        p.k, p.lambda_ = k, 0.05
        s = mfx.ImplicitAlsSolver(R, p, 1.0, cg=(2, 0.0))
        s.set_factors((rng.standard_normal((500, k)) * 0.1).astype(np.float32))
        s.iterate(1)
        s.kernel_times()
        s.iterate(5)
        per = {name: t * 1e3 / n for name, (t, n) in s.kernel_times().items()}
        s.close()
        X = rng.standard_normal((4 * k, k)).astype(np.float32) / np.sqrt(k)
        A = (X.T @ X + 0.1 * np.eye(k, dtype=np.float32)).astype(np.float32)
        mfx.spd_inverse(A)
        t0 = time.perf_counter()
        mfx.spd_inverse(A)
        out.append({"k": k, "ms_device_inverse": round(0.5 * (per["ialscg_inverse(H)"] + per["ialscg_inverse(W)"]), 4),
                    "ms_whole_call_from_host_pointers": round((time.perf_counter() - t0) * 1e3, 3)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="64,128")
    ap.add_argument("--block", default="", help="k:d,k:d,... runs of the block subspace sweeps")
    ap.add_argument("--explicit-block", default="", help="k:d,k:d,... runs of explicit ALS by block subspace sweeps")
    ap.add_argument("--reg", type=int, default=0, help="explicit block runs: 0 = lambda, 1 = lambda * entries of the segment")
    ap.add_argument("--cg", default="", help="STEPS:TOL runs of the conjugate-gradient trainer at every rank of --cg-ks")
    ap.add_argument("--cg-ks", default="", help="ranks of the --cg runs (default: --ks)")
    ap.add_argument("--again", action="store_true", help="repeat the exact runs after the block runs")
    ap.add_argument("--verbose", action="store_true", help="block runs: the solver's own log lines (failed pivots) before the JSON line")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--lam", type=float, default=0.05)
    ap.add_argument("--alpha0", type=float, default=None, help="weight of the unobserved pairs (mfx_ials_create_reg)")
    ap.add_argument("--nu", type=float, default=None, help="exponent of the frequency-scaled regulariser, 0..1")
    ap.add_argument("--seed", type=int, default=1234)
    a = ap.parse_args()
    import torch
    import mfx
    from mfx import synth_torch
    d = synth_torch.synth_ratings_device(ROWS, COLS, NNZ, seed=a.seed, device="cuda:0")
    rows, cols, nnz = int(d["rows"]), int(d["cols"]), int(d["csr_val"].numel())
    out = {"workload": f"{rows}x{cols} nnz={nnz}", "alpha": a.alpha, "lambda": a.lam, "iters": a.iters,
           "library": os.path.relpath(mfx.LIB_PATH, ROOT), "runs": []}
    if reg_kwargs(a):
        out["alpha0"] = 1.0 if a.alpha0 is None else a.alpha0
        out["nu"] = 0.0 if a.nu is None else a.nu
    ks = [int(x) for x in a.ks.split(",") if x]
    blocks = [tuple(int(v) for v in x.split(":")) for x in a.block.split(",") if x]
    eblocks = [tuple(int(v) for v in x.split(":")) for x in a.explicit_block.split(",") if x]
    cg = (int(a.cg.split(":")[0]), float(a.cg.split(":")[1])) if a.cg else None
    cg_ks = [int(x) for x in a.cg_ks.split(",") if x] if a.cg_ks else ks
    plan = ([("exact", k, None) for k in ks] + [("block", k, b) for k, b in blocks] + [("cg", k, None) for k in (cg_ks if cg else [])] +
            [("explicit_block", k, b) for k, b in eblocks] + ([("exact", k, None) for k in ks] if a.again else []))
    if cg:
        out["device_inverse"] = inverse_times(mfx)
    for kind, k, block in plan:
        if kind == "cg":
            out["runs"].append(run_cg(mfx, d, rows, cols, k, cg[0], cg[1], a))
            torch.cuda.synchronize()
            continue
        if kind == "explicit_block":
            out["runs"].append(run_explicit_block(mfx, d, rows, cols, nnz, k, block, a))
            torch.cuda.synchronize()
            continue
        if kind == "block":
            out["runs"].append(run_block(mfx, d, rows, cols, nnz, k, block, a))
            torch.cuda.synchronize()
            continue
        p = mfx.parameter()
        p.k, p.lambda_ = k, a.lam
        H0 = mfx.initial_col(cols, k)
        s = mfx.ImplicitAlsSolver(None, p, a.alpha, device_arrays=d, **reg_kwargs(a))
        s.set_factors(H0)
        s.iterate(1)  # warmup
        s.kernel_times()
        ms, losses = [], []
        for _ in range(a.iters):
            ms.append(s.iterate(1)[0].update_time * 1e3)
            losses.append(s.loss())
        kt = s.kernel_times()
        s.close()
        per = {name: t * 1e3 / n for name, (t, n) in kt.items()}
        e = mfx.AlsSolver(None, None, p, device_arrays=d)
        e.set_factors(H0)
        e.iterate(1, with_rmse=False)
        ems = [r.update_time * 1e3 for r in e.iterate(a.iters, with_rmse=False)]
        e.close()
        med = float(np.median(ms))
        fl = flop_per_iteration(rows, cols, nnz, k)
        out["runs"].append({
            "k": k, "ms_per_iteration": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
            "ms_user_half": round(per["ials_half_rows(W over H)"], 3), "ms_item_half": round(per["ials_half_cols(H over W)"], 3),
            "ms_base_gram_H": round(per["ials_base_gram(H)"], 3), "ms_base_gram_W": round(per["ials_base_gram(W)"], 3),
            "explicit_als_ms_per_iteration": round(float(np.median(ems)), 3),
            "ratio_to_explicit": round(med / float(np.median(ems)), 3),
            "flop_per_iteration": fl, "fraction_of_fp32_mfma_peak": round(fl / (med * 1e-3) / (PEAK_TF * 1e12), 4),
            "loss_per_iteration": losses,
        })
        torch.cuda.synchronize()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
