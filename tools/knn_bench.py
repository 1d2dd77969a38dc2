"""Item-kNN (mfx_knn_*) at the Netflix shape: build time, recommendation time, and the yardsticks they are held against.

Builds the Netflix-shaped synthetic matrix on the GPU (mfx.synth_torch, as bench.py does), weights it by cosine in torch
(x = r / ||r_.i||, the same fp32 division on both orientations) and measures, for every K of --Ks:
  build      mfx_knn_build on the device arrays: the phases of mfx_knn_times (checks + work order, similarity pass);
  recommend  the training rows of 1 / 64 / 1 024 / all users at n_top = 10: ms per call (median of --reps) and phases;
  floors     sum_u n_u^2 LDS adds (build) and sum_u n_u * K (recommend) over CUs x clock x 5.28 lane-atomics per clock and
             CU -- the "1 x ds_add_u64, random slots" line of profiles/r02_ubench_ldsatomic.txt, one microbenchmark: nobody
             has measured this access pattern -- and the achieved share of each;
  tail       the build of the sub-matrix of the heaviest item's users alone: that item's pass is the same work there and
             the longest by far, so its similarity pass bounds the heaviest item's pass from above;
  torch      the same mathematics as chunked sparse x dense products plus topk, --torch-chunks chunks of --torch-chunk
             items scaled to the catalogue (float sums in library order: NOT bit-reproducible).
Then the ML-1M shape and one 10^5-item catalogue (13 tiles: the cost of the lower-bound searches and of the rescans).

With --parent-pkg DIR (a built cuda-recommender_amd tree of the parent commit): the unchanged all-user query at k = 64, a
fresh process per tree, parent and this tree alternated --regress-runs times.

    python tools/knn_bench.py [--Ks 20,100] [--parent-pkg DIR] [--regress-runs 4] [--out FILE]
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
LANE_ATOMICS_PER_CLK_CU = 5.28  # profiles/r02_ubench_ldsatomic.txt, 1 x ds_add_u64, random slots


def matrix(torch, rows, cols, nnz):
    from mfx import synth_torch
    d = synth_torch.synth_ratings_device(rows, cols, nnz, seed=1234, device="cuda:0", sigma_rows=0.5, sigma_cols=1.0)
    return {k: d[k] for k in ("rows", "cols", "csr_row_ptr", "csr_col_idx", "csr_val", "csc_col_ptr", "csc_row_idx", "csc_val")}


def cosine(torch, d):
    """d with x = r / ||r_.i||_2 on both sides (columns without entries have none to scale)."""
    cnt = (d["csc_col_ptr"][1:] - d["csc_col_ptr"][:-1]).long()
    col = torch.repeat_interleave(torch.arange(d["cols"], device=cnt.device), cnt)
    norm = torch.zeros(d["cols"], device=cnt.device, dtype=torch.float64).index_add_(0, col, d["csc_val"].double() ** 2).sqrt().float()
    out = dict(d)
    out["csc_val"] = (d["csc_val"] / norm[col]).contiguous()
    out["csr_val"] = (d["csr_val"] / norm[d["csr_col_idx"].long()]).contiguous()
    return out


def rows_of_item(torch, d, item):
    """The sub-matrix of the users that hold `item` (rows renumbered in order), both orientations."""
    c0, c1 = int(d["csc_col_ptr"][item]), int(d["csc_col_ptr"][item + 1])
    users = d["csc_row_idx"][c0:c1].long()
    ptr = d["csr_row_ptr"].long()
    lens = ptr[users + 1] - ptr[users]
    new_ptr = torch.zeros(users.numel() + 1, dtype=torch.int64, device=users.device)
    new_ptr[1:] = torch.cumsum(lens, 0)
    pos = torch.repeat_interleave(ptr[users] - new_ptr[:-1], lens) + torch.arange(int(new_ptr[-1]), device=users.device)
    ri = torch.repeat_interleave(torch.arange(users.numel(), device=users.device), lens)
    cj, v = d["csr_col_idx"][pos].long(), d["csr_val"][pos]
    order = torch.sort(cj * users.numel() + ri).indices
    cptr = torch.zeros(d["cols"] + 1, dtype=torch.int64, device=users.device)
    cptr[1:] = torch.cumsum(torch.bincount(cj, minlength=d["cols"]), 0)
    i32 = lambda t: t.to(torch.int32).contiguous()
    return dict(rows=int(users.numel()), cols=d["cols"], csr_row_ptr=i32(new_ptr), csr_col_idx=i32(cj), csr_val=v.contiguous(),
                csc_col_ptr=i32(cptr), csc_row_idx=i32(ri[order]), csc_val=v[order].contiguous())


def torch_baseline(torch, d, K, chunk, chunks):
    """`chunks` chunks of `chunk` items: S = X^T X[:, chunk] by a sparse x dense product, the diagonal masked, topk."""
    rows, cols = d["rows"], d["cols"]
    Xt = torch.sparse_csr_tensor(d["csc_col_ptr"].long(), d["csc_row_idx"].long(), d["csc_val"], size=(cols, rows))
    ptr = d["csr_row_ptr"].long()
    ri = torch.repeat_interleave(torch.arange(rows, device=ptr.device), ptr[1:] - ptr[:-1])
    cj = d["csr_col_idx"].long()

    def one(c0):
        c1 = min(cols, c0 + chunk)
        m = (cj >= c0) & (cj < c1)
        dense = torch.zeros(rows, c1 - c0, device=ptr.device)
        dense[ri[m], cj[m] - c0] = d["csr_val"][m]
        S = torch.sparse.mm(Xt, dense)  # [cols][chunk]
        S[torch.arange(c0, c1, device=ptr.device), torch.arange(c1 - c0, device=ptr.device)] = float("-inf")
        return torch.topk(S.t(), min(K, cols - 1), dim=1)

    one(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for c in range(chunks):
        if c * chunk >= cols:
            break
        one(c * chunk)
        n += min(cols, (c + 1) * chunk) - c * chunk
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    return {"items_done": n, "seconds": round(sec, 4), "seconds_scaled_to_catalogue": round(sec / n * cols, 4), "reproducible": False}


def shape_point(torch, mfx, a, rows, cols, nnz, K, batches, rate, with_tail=False, with_torch=False):
    d = cosine(torch, matrix(torch, rows, cols, nnz))
    ptr = d["csr_row_ptr"].long()
    n_u = (ptr[1:] - ptr[:-1]).double()
    sum_sq = float((n_u * n_u).sum())
    rec = {"rows": rows, "cols": cols, "nnz": nnz, "K": K, "sum_u_nu_squared": sum_sq}
    print(f"sum_u n_u^2 = {sum_sq:.6g}", file=sys.stderr, flush=True)
    m = mfx.ItemKnn(None, K, None, device_arrays=d)
    t = m.times()
    rec["build_seconds"] = {"checks_and_work_order": round(t["build_checks"], 5), "similarity_pass": round(t["build_pass"], 5)}
    rec["build_floor_seconds"] = round(sum_sq / rate, 6)
    rec["build_share_of_floor"] = round(sum_sq / rate / t["build_pass"], 4)
    rec["recommend"] = []
    for n in batches:
        n = min(n, rows)
        z = int(ptr[n])
        q = (d["csr_row_ptr"][:n + 1].contiguous(), d["csr_col_idx"][:z].contiguous(), d["csr_val"][:z].contiguous())
        m.recommend(q, 10)
        wall, passes, checks = [], [], []
        for _ in range(a.reps):
            t0 = m.times()
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            m.recommend(q, 10)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - w0) * 1e3)
            t1 = m.times()
            passes.append((t1["recommend_pass"] - t0["recommend_pass"]) * 1e3)
            checks.append((t1["recommend_checks"] - t0["recommend_checks"]) * 1e3)
        adds = float(z) * K
        rec["recommend"].append({"users": n, "entries": z, "ms_per_call": round(float(np.median(wall)), 4),
                                 "pass_ms": round(float(np.median(passes)), 4), "checks_ms": round(float(np.median(checks)), 4),
                                 "floor_ms": round(adds / rate * 1e3, 5), "share_of_floor": round(adds / rate * 1e3 / float(np.median(passes)), 4),
                                 "bad_rows": m.bad_rows})
    m.close()
    if with_tail:
        cnt = d["csc_col_ptr"][1:] - d["csc_col_ptr"][:-1]
        item = int(torch.argmax(cnt))
        sub = rows_of_item(torch, d, item)
        work = int((sub["csr_row_ptr"][1:] - sub["csr_row_ptr"][:-1]).long().sum())
        with mfx.ItemKnn(None, K, None, device_arrays=sub) as ms:
            ts = ms.times()
        rec["tail"] = {"heaviest_item": item, "its_users": int(cnt[item]), "its_adds": work,
                       "submatrix_similarity_pass_seconds": round(ts["build_pass"], 5),
                       "share_of_the_whole_build_pass": round(ts["build_pass"] / t["build_pass"], 4),
                       "one_cu_floor_seconds": round(work / (rate / a.cus), 6)}
        del sub
    if with_torch:
        try:
            rec["torch_sparse_dense_topk"] = torch_baseline(torch, d, K, a.torch_chunk, a.torch_chunks)
            rec["build_over_torch"] = round(t["build_pass"] / rec["torch_sparse_dense_topk"]["seconds_scaled_to_catalogue"], 4)
        except Exception as e:  # (a torch build without the sparse product: say so, measure the rest)
            rec["torch_sparse_dense_topk"] = {"error": repr(e)[:300]}
    del d
    torch.cuda.empty_cache()
    print(json.dumps(rec), file=sys.stderr, flush=True)
    return rec


def regress_child(a):
    sys.path.insert(0, a.regress_child)
    import torch
    import mfx
    assert os.path.dirname(os.path.dirname(os.path.abspath(mfx.__file__))) == os.path.abspath(a.regress_child)
    from mfx import synth_torch
    d = synth_torch.synth_ratings_device(a.rows, a.cols, a.nnz, seed=1234, device="cuda:0", sigma_rows=0.5, sigma_cols=1.0)
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
        for rep in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r.query(10, on_device=True)
            torch.cuda.synchronize()
            if rep:
                ts.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"query_ms": float(np.median(ts))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=480189)
    ap.add_argument("--cols", type=int, default=17770)
    ap.add_argument("--nnz", type=int, default=99_072_112)
    ap.add_argument("--Ks", default="20,100")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--torch-chunk", type=int, default=256)
    ap.add_argument("--torch-chunks", type=int, default=4)
    ap.add_argument("--skip", default="", help="letters: m = ML-1M shape, b = 10^5-item catalogue, t = torch comparison")
    ap.add_argument("--parent-pkg", default=None)
    ap.add_argument("--regress-runs", type=int, default=4)
    ap.add_argument("--regress-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_bench.json"))
    a = ap.parse_args()
    if a.regress_child:
        return regress_child(a)
    sys.path.insert(0, PKG)
    import torch
    import mfx
    prop = torch.cuda.get_device_properties(0)
    a.cus = int(prop.multi_processor_count)
    clock_hz = float(getattr(prop, "clock_rate", 2_400_000)) * 1e3
    rate = a.cus * clock_hz * LANE_ATOMICS_PER_CLK_CU
    out = {"tool": "knn_bench", "weights": "cosine", "n_top": 10, "cus": a.cus, "clock_ghz": round(clock_hz / 1e9, 3),
           "lane_atomics_per_clk_and_cu": LANE_ATOMICS_PER_CLK_CU, "netflix": [], "ml1m": [], "catalogue_1e5": []}
    Ks = [int(x) for x in a.Ks.split(",") if x]
    for i, K in enumerate(Ks):
        out["netflix"].append(shape_point(torch, mfx, a, a.rows, a.cols, a.nnz, K, (1, 64, 1024, a.rows), rate, with_tail=True,
                                          with_torch="t" not in a.skip and i == 0))
    if "m" not in a.skip:
        for K in Ks:
            out["ml1m"].append(shape_point(torch, mfx, a, 6040, 3706, 1_000_000, K, (1, 64, 1024, 6040), rate))
    if "b" not in a.skip and Ks:
        out["catalogue_1e5"].append(shape_point(torch, mfx, a, 200_000, 100_000, 10_000_000, Ks[0], (1, 64, 1024, 200_000), rate))
    if a.parent_pkg:
        runs = {"parent": [], "this": []}
        for _ in range(a.regress_runs):
            for name, pkg in (("parent", os.path.abspath(a.parent_pkg)), ("this", PKG)):
                cmd = [sys.executable, os.path.abspath(__file__), "--regress-child", pkg, "--rows", str(a.rows), "--cols", str(a.cols),
                       "--nnz", str(a.nnz)]
                p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True, timeout=300)
                runs[name].append(json.loads(p.stdout.strip().splitlines()[-1])["query_ms"])
        pm, tm = float(np.median(runs["parent"])), float(np.median(runs["this"]))
        spread = max(runs["parent"]) - min(runs["parent"])
        out["regression"] = {"workload": "all-user query, k = 64, n_top = 10", "parent_ms": runs["parent"], "this_ms": runs["this"],
                             "parent_median_ms": pm, "this_median_ms": tm, "parent_spread_ms": spread, "no_slower": bool(tm <= pm + spread)}
        print(json.dumps(out["regression"]), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
