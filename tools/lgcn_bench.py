"""LightGCN training (mfx_lgcn_*) at the Netflix shape: seconds per step and per epoch by phase, and the gathered bytes per
second of one propagation half-pass.

Builds the Netflix-shaped synthetic matrix on the GPU (mfx.synth_torch, as bench.py does; every stored pair is taken as a
positive interaction) and, for every k of --ks, L of --layers and batch of --batches, trains from 0.1 N(0, 1) base embeddings:
--warm steps, then --steps steps timed by the library's stream events (a step propagates the whole graph 2 L times forward
and 2 L times backward, so an epoch of nnz / batch steps is scaled from the step, not run); then --profile-steps steps on a
handle made with parameters.profile = 1, which synchronises every step and gives the split sample / forward / gradient /
scatter / backward / update.

What the result is held against.  A half-pass gathers nnz rows of k floats: nnz * k * 4 bytes over its time -- the forward
phase holds 2 L of them -- to be read against the rate query_candidates reaches on gathered rows of H (GATHER_TBS; no other
yardstick for this access pattern has been measured here).  The expectation on record: a half-pass reaches at least half of
that rate, and a step costs about 4 L half-passes plus a BPR step (the gradient and scatter phases and BPR's apply, taken
from a BprSolver step at the same k and batch in the same process).  The record carries the heaviest row's and column's
share of a pass.

In the same process a torch baseline runs the same mathematics for --torch-steps steps per point: torch.sparse.mm
propagation with autograd on triples drawn by torch.randint, plain SGD on the base.  Float atomics in arrival order, so it
is NOT reproducible; time only.

With --parent-pkg DIR (the built cuda-recommender_amd directory inside a whole checkout of the parent commit): the unchanged uniform BPR epoch and all-user
query (tools/bpr_bench.py's regression child) and bench.py, each in a fresh process per tree, parent and this tree
alternated --regress-runs times.

    python tools/lgcn_bench.py [--ks 64,128] [--layers 1,2,3] [--batches 65536,1048576] [--parent-pkg DIR] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cuda-recommender_amd")
GATHER_TBS = 4.7  # gathered bytes per second of H rows that query_candidates reaches (README, all users x 1 000)


def matrix(a, torch):
    from mfx import synth_torch
    return synth_torch.synth_ratings_device(a.rows, a.cols, a.nnz, seed=1234, device="cuda:0", sigma_rows=0.5, sigma_cols=1.0)


def torch_steps(torch, d, k, layers, batch, steps, lr, lam):
    """`steps` steps of the same mathematics in torch with autograd; returns seconds per step."""
    dev = torch.device("cuda:0")
    ptr, idx = d["csr_row_ptr"].long(), d["csr_col_idx"].long()
    rows, cols, nnz = int(d["rows"]), int(d["cols"]), idx.numel()
    du = (ptr[1:] - ptr[:-1]).double()
    di = torch.bincount(idx, minlength=cols).double()
    su = torch.where(du > 0, du.rsqrt(), torch.zeros_like(du)).float()
    si = torch.where(di > 0, di.rsqrt(), torch.zeros_like(di)).float()
    row_of = torch.repeat_interleave(torch.arange(rows, device=dev), ptr[1:] - ptr[:-1])
    A = torch.sparse_coo_tensor(torch.stack([row_of, idx]), su[row_of] * si[idx], (rows, cols)).coalesce()
    At = A.t().coalesce()
    key = row_of * cols + idx  # ascending
    W0 = (0.1 * torch.randn(rows, k, device=dev)).requires_grad_()
    H0 = (0.1 * torch.randn(cols, k, device=dev)).requires_grad_()
    g = torch.Generator(device=dev)
    g.manual_seed(1)

    def one():
        p = torch.randint(0, nnz, (batch,), generator=g, device=dev)
        j = torch.randint(0, cols, (batch,), generator=g, device=dev)
        u, i = row_of[p], idx[p]
        want = u * cols + j
        pos = torch.searchsorted(key, want).clamp_(max=nnz - 1)
        keep = key[pos] != want
        u, i, j = u[keep], i[keep], j[keep]
        W, H, eu, ei = W0, H0, W0, H0
        for _ in range(layers):
            eu, ei = torch.sparse.mm(A, ei), torch.sparse.mm(At, eu)
            W, H = W + eu, H + ei
        W, H = W / (layers + 1), H / (layers + 1)
        w, hi, hj = W[u], H[i], H[j]
        x = (w * (hi - hj)).sum(1)
        loss = -torch.nn.functional.logsigmoid(x).sum() + 0.5 * lam * ((w * w).sum() + (hi * hi).sum() + (hj * hj).sum())
        gw, gh = torch.autograd.grad(loss, (W0, H0))
        with torch.no_grad():
            W0.sub_(lr * gw)
            H0.sub_(lr * gh)

    one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        one()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def bpr_step_seconds(mfx, d, a, k, batch):
    """Seconds of one BprSolver step at the same k and batch (the yardstick 'plus a BPR step')."""
    p = mfx.parameter()
    p.k, p.lambda_ = k, a.lam
    s = mfx.BprSolver(None, p, a.lr, batch, seed=1, device_arrays=d, init_seed=k)
    s.steps(a.warm)
    sec = s.steps(a.steps)["seconds"] / a.steps
    s.close()
    return sec


def point(torch, mfx, d, a, k, layers, batch, shares, bpr_sec):
    p = mfx.parameter()
    p.k, p.lambda_ = k, a.lam
    nnz = int(d["csr_val"].numel())
    rec = {"k": k, "layers": layers, "batch": batch, "steps_per_epoch": -(-nnz // batch), "timed_steps": a.steps}
    s = mfx.LightGcnSolver(None, p, a.lr, batch, layers, seed=1, device_arrays=d, init_seed=k)
    s.steps(a.warm)
    e = s.steps(a.steps)
    s.close()
    step = e["seconds"] / a.steps
    rec.update({"seconds_per_step": round(step, 6), "seconds_per_epoch_scaled": round(step * rec["steps_per_epoch"], 3),
                "skipped": e["skipped"], "bad": e["bad"], "auc_of_the_steps": round(e["auc"], 4)})
    p.profile = 1
    s = mfx.LightGcnSolver(None, p, a.lr, batch, layers, seed=1, device_arrays=d, init_seed=k)
    s.steps(min(2, a.profile_steps))
    t0 = s.kernel_times()
    s.steps(a.profile_steps)
    t1 = s.kernel_times()
    s.close()
    split = {name: (t1[name] - t0[name]) / a.profile_steps for name in t1}
    rec["ms_per_step"] = {name: round(v * 1e3, 4) for name, v in split.items()}
    half = split["forward"] / (2 * layers)
    rec["half_pass_ms_forward_mean"] = round(half * 1e3, 4)
    rec["half_pass_gathered_tb_per_s"] = round(nnz * k * 4 / half / 1e12, 4)
    rec["gather_yardstick_tb_per_s"] = GATHER_TBS
    rec["half_pass_reaches_half_the_yardstick"] = bool(nnz * k * 4 / half / 1e12 >= GATHER_TBS / 2)
    rec["bpr_step_ms_same_k_batch"] = round(bpr_sec * 1e3, 4)
    rec["step_over_4L_half_passes_plus_bpr_step"] = round(step / (4 * layers * half + bpr_sec), 3)
    rec.update(shares)
    if a.torch_steps > 0:
        try:
            ts = torch_steps(torch, d, k, layers, batch, a.torch_steps, a.lr, a.lam)
            rec["torch_sparse_mm_autograd"] = {"seconds_per_step": round(ts, 6), "reproducible": False}
            rec["ratio_to_torch"] = round(step / ts, 3)
        except RuntimeError as ex:  # (an allocation torch could not make: the point stands without the baseline)
            rec["torch_sparse_mm_autograd"] = {"failed": str(ex).splitlines()[0][:200]}
        torch.cuda.empty_cache()
    return rec


def regress(a):
    child = os.path.join(ROOT, "tools", "bpr_bench.py")
    shape = ["--rows", str(a.rows), "--cols", str(a.cols), "--nnz", str(a.nnz)]
    lines = []
    for run in range(a.regress_runs):
        for tree, pkg in (("parent", os.path.abspath(a.parent_pkg)), ("this", PKG)):
            t0 = time.perf_counter()
            p = subprocess.run([sys.executable, child, "--regress-child", pkg] + shape, stdout=subprocess.PIPE, text=True, check=True, timeout=600)
            lines.append({"run": run, "tool": "bpr_bench --regress-child", "tree": tree, "seconds": round(time.perf_counter() - t0, 1),
                          "result": json.loads(p.stdout.strip().splitlines()[-1])})
            t0 = time.perf_counter()  # (each tree's own bench.py beside its package: the checkout of the parent commit is whole)
            p = subprocess.run([sys.executable, os.path.join(os.path.dirname(pkg), "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"],
                               stdout=subprocess.PIPE, text=True, check=True, timeout=900)
            lines.append({"run": run, "tool": "bench", "tree": tree, "seconds": round(time.perf_counter() - t0, 1),
                          "result": json.loads(p.stdout.strip().splitlines()[-1])})
            for line in lines[-2:]:
                print(json.dumps(line), file=sys.stderr, flush=True)
    with open(a.ab_out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=480189)
    ap.add_argument("--cols", type=int, default=17770)
    ap.add_argument("--nnz", type=int, default=99_072_112)
    ap.add_argument("--ks", default="64,128")
    ap.add_argument("--layers", default="1,2,3")
    ap.add_argument("--batches", default="65536,1048576")
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--lam", type=float, default=0.01)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--profile-steps", type=int, default=3)
    ap.add_argument("--torch-steps", type=int, default=2)
    ap.add_argument("--parent-pkg", default=None)
    ap.add_argument("--regress-runs", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lgcn_bench.json"))
    ap.add_argument("--ab-out", default=os.path.join(ROOT, "profiles", "lgcn_bench_ab.jsonl"))
    a = ap.parse_args()
    sys.path.insert(0, PKG)
    import torch
    import mfx
    out = {"tool": "lgcn_bench", "rows": a.rows, "cols": a.cols, "nnz": a.nnz, "lr": a.lr, "lambda": a.lam, "points": []}
    ks = [int(x) for x in a.ks.split(",") if x]
    if ks:
        d = matrix(a, torch)
        nnz = int(d["csr_val"].numel())
        du = (d["csr_row_ptr"][1:] - d["csr_row_ptr"][:-1])
        di = (d["csc_col_ptr"][1:] - d["csc_col_ptr"][:-1])
        shares = {"heaviest_row_entries": int(du.max()), "heaviest_column_entries": int(di.max()),
                  "heaviest_row_share_of_a_pass": round(int(du.max()) / nnz, 6), "heaviest_column_share_of_a_pass": round(int(di.max()) / nnz, 6),
                  "work_items_user_side": int(torch.clamp((du + 1023) // 1024, min=1).sum()),
                  "work_items_item_side": int(torch.clamp((di + 1023) // 1024, min=1).sum())}
        for k in ks:
            for batch in (int(x) for x in a.batches.split(",") if x):
                bpr_sec = bpr_step_seconds(mfx, d, a, k, batch)
                for layers in (int(x) for x in a.layers.split(",") if x):
                    out["points"].append(point(torch, mfx, d, a, k, layers, batch, shares, bpr_sec))
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
