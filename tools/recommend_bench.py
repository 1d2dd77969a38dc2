"""Top-N recommendation at the Netflix shape: the fused mfx_rec query against a chunked torch baseline.

Builds the Netflix-shaped synthetic matrix on the GPU (mfx.synth_torch, as bench.py does), random factors, the training
ratings as the exclusion set, and prints ONE JSON line: ms per all-user query (median / min / max over --reps) at
N = 10 and N = 100 for k = 64 and k = 128 (ALS layout), flop and fraction of the 157.3 TF fp32 MFMA peak, the latency of
1 / 64 / 1024-user queries, the torch baseline (chunked torch.mm, -inf scattered over rated items, torch.topk) on the
same inputs, and a contract check on a seeded 2,000-user sample against fp64 scores.

    python tools/recommend_bench.py [--reps 5] [--ks 64,128] [--ns 10,100]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-recommender_amd"))

PEAK_TF = 157.3
PAD = 0xFFFFFFFF


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


def contract_sample(W, H, rp, ci, items, scores, users, n_top):
    """Violations of the query contract on `users` (fp64 reference; the bounds of tests/test_gpu_recommend.py)."""
    k = W.shape[1]
    W64, H64 = W.astype(np.float64), H.astype(np.float64)
    bad = 0
    for u in users:
        s64 = H64 @ W64[u]
        b = 4 * k * 2.0 ** -24 * (np.abs(H64) @ np.abs(W64[u]))
        elig = np.ones(H.shape[0], bool)
        elig[ci[rp[u]:rp[u + 1]]] = False
        it, sc = items[u], scores[u]
        n = int((it != PAD).sum())
        ids = it[:n].astype(np.int64)
        ok = (it[n:] == PAD).all() and elig[ids].all() and len(set(ids.tolist())) == n
        ok = ok and np.all(np.abs(sc[:n] - s64[ids]) <= b[ids])
        if n > 1:
            ok = ok and bool(np.all((sc[:-1] > sc[1:]) | ((sc[:-1] == sc[1:]) & (ids[:-1] < ids[1:]))))
        if n == n_top:
            left = elig.copy()
            left[ids] = False
            ok = ok and bool(np.all(s64[left] - sc[n - 1] - b[left] - b[ids[-1]] <= 0))
        else:
            ok = ok and n == int(elig.sum())
        bad += not ok
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=480189)
    ap.add_argument("--cols", type=int, default=17770)
    ap.add_argument("--nnz", type=int, default=99_072_112)
    ap.add_argument("--ks", default="64,128")
    ap.add_argument("--ns", default="10,100")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-chunk", type=int, default=16384)
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    import torch
    import mfx
    from mfx import synth_torch
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    d = synth_torch.synth_ratings_device(a.rows, a.cols, a.nnz, seed=1234, device="cuda:0", sigma_rows=0.5, sigma_cols=1.0)
    rows, cols = a.rows, a.cols
    rp_t, ci_t = d["csr_row_ptr"].contiguous(), d["csr_col_idx"].contiguous()
    rp, ci = rp_t.cpu().numpy().view(np.uint32), ci_t.cpu().numpy().view(np.uint32)
    nnz = int(ci.shape[0])
    del d
    ex = mfx.dataset.RatingData(rows, cols, rp, ci, np.zeros(0, np.float32), np.zeros(cols + 1, np.uint32),
                                np.zeros(0, np.uint32), np.zeros(0, np.float32))
    # rated (row, col) pairs for the baseline's scatter
    row_of = torch.repeat_interleave(torch.arange(rows, device=dev), (rp_t[1:] - rp_t[:-1]).long())
    out = {"tool": "recommend_bench", "rows": rows, "cols": cols, "nnz": nnz, "peak_tf": PEAK_TF, "cases": []}
    for k in [int(x) for x in a.ks.split(",")]:
        g = torch.Generator(device=dev)
        g.manual_seed(k)
        W = (torch.randn(rows, k, generator=g, device=dev) * 0.3).contiguous()
        H = (torch.randn(cols, k, generator=g, device=dev) * 0.3).contiguous()
        Wn, Hn = W.cpu().numpy(), H.cpu().numpy()
        flop = 2.0 * rows * cols * k
        with mfx.Recommender(W, H, 1, exclude=ex) as r:
            for n_top in [int(x) for x in a.ns.split(",")]:
                case = {"k": k, "n_top": n_top, "flop": flop}
                res = {}

                def q():
                    res["v"] = r.query(n_top, on_device=True)
                case["fused"] = timed(q, a.reps, sync)
                case["fused"]["frac_peak"] = flop / (case["fused"]["median_ms"] * 1e-3) / (PEAK_TF * 1e12)
                items = res["v"][0].cpu().numpy().view(np.uint32)
                scores = res["v"][1].cpu().numpy()
                sample = np.sort(np.random.default_rng(2000).choice(rows, 2000, replace=False))
                case["contract_sample_users"] = 2000
                case["contract_violations"] = contract_sample(Wn, Hn, rp, ci, items, scores, sample, n_top)
                lat = {}
                for nu in (1, 64, 1024):
                    us = torch.from_numpy(np.random.default_rng(nu).choice(rows, nu).astype(np.int32)).to(dev)
                    lat[str(nu)] = timed(lambda: r.query(n_top, users=us), a.reps, sync)["median_ms"]
                case["latency_ms"] = lat
                if not a.no_baseline:
                    bi = torch.empty((rows, n_top), dtype=torch.int64, device=dev)

                    def base():
                        c = a.baseline_chunk
                        for u0 in range(0, rows, c):
                            u1 = min(rows, u0 + c)
                            S = torch.mm(W[u0:u1], H.t())
                            lo, hi = int(rp[u0]), int(rp[u1])
                            S[row_of[lo:hi] - u0, ci_t[lo:hi].long()] = float("-inf")
                            bi[u0:u1] = torch.topk(S, n_top, dim=1).indices
                    case["torch_baseline"] = timed(base, a.reps, sync)
                    case["speedup_vs_torch"] = case["torch_baseline"]["median_ms"] / case["fused"]["median_ms"]
                out["cases"].append(case)
                print(json.dumps(case), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
