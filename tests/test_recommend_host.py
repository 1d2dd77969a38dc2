"""CPU tests of the top-N recommendation surface: the new C ABI symbols, the host-side ranking metrics
(mfx_topn_metrics) against hand-worked and independently computed values, and the failure paths of
mfx.Recommender and `mfx_train -recommend` that must not need a GPU."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden

PAD = 0xFFFFFFFF


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    return m


def test_recommend_symbols_are_exported_and_bound(mfx):
    from mfx import _lib as L
    lib = mfx.lib()
    for name in ("mfx_rec_create", "mfx_rec_query", "mfx_rec_destroy", "mfx_topn_metrics"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert callable(mfx.Recommender) and callable(mfx.recommend) and callable(mfx.topn_metrics)


def _T(rows, cols, r, c, v):
    from mfx.api import TestData
    return TestData(rows, cols, np.array(r, np.uint32), np.array(c, np.uint32), np.array(v, np.float32))


def test_metrics_hand_worked_example(mfx):
    # user 0: R = {1, 4} (4 appears twice in the test set); list [4, 7, 1]    -> hits 2 at ranks 0 and 2
    # user 1: R = {}  after min_rating (its only test rating is 2.0)          -> skipped
    # user 2: R = {0, 3, 5}; list [3, PAD, PAD]                               -> hits 1 at rank 0
    T = _T(3, 8, [0, 0, 0, 1, 2, 2, 2, 2], [1, 4, 4, 6, 0, 3, 5, 7], [4, 5, 4.5, 2, 3, 3.5, 5, 1])
    items = np.array([[4, 7, 1], [6, 2, 0], [3, PAD, PAD]], np.uint32)
    m = mfx.topn_metrics(items, T, min_rating=3.0)
    assert m["users"] == 2
    l2 = lambda j: 1.0 / math.log2(j + 2)
    assert m["hr"] == 1.0
    assert abs(m["precision"] - (2 / 3 + 1 / 3) / 2) < 1e-15
    assert abs(m["recall"] - (2 / 2 + 1 / 3) / 2) < 1e-15
    nd0 = (l2(0) + l2(2)) / (l2(0) + l2(1))
    nd2 = l2(0) / (l2(0) + l2(1) + l2(2))
    assert abs(m["ndcg"] - (nd0 + nd2) / 2) < 1e-15
    # without the threshold user 1 counts (its item 6 is at rank 0) and user 2 also has item 7
    m = mfx.topn_metrics(items, T)
    assert m["users"] == 3
    assert abs(m["precision"] - (2 / 3 + 1 / 3 + 1 / 3) / 3) < 1e-15
    assert abs(m["recall"] - (2 / 2 + 1 / 1 + 1 / 4) / 3) < 1e-15
    # explicit users: the lists belong to users 2, 0, 0
    m = mfx.topn_metrics(items[[2, 0]], T, users=[2, 0], min_rating=3.0)
    assert m["users"] == 2 and m["hr"] == 1.0


def _metrics_numpy(items, users, T, min_rating):
    hr = pr = rc = nd = 0.0
    kept = 0
    n_top = items.shape[1]
    for s, u in enumerate(users):
        sel = (T.test_row == u) & (T.test_val >= min_rating)
        R = set(T.test_col[sel].tolist())
        if not R:
            continue
        kept += 1
        hits, dcg = 0, 0.0
        for j, it in enumerate(items[s].tolist()):
            if it != PAD and it in R:
                hits += 1
                dcg += 1.0 / np.log2(j + 2)
        idcg = sum(1.0 / np.log2(j + 2) for j in range(min(n_top, len(R))))
        hr += hits > 0
        pr += hits / n_top
        rc += hits / len(R)
        nd += dcg / idcg
    return {"hr": hr / kept, "precision": pr / kept, "recall": rc / kept, "ndcg": nd / kept, "users": kept}


def test_metrics_random_against_numpy(mfx):
    rng = np.random.default_rng(0)
    rows, cols, n_top = 200, 50, 7
    nt = 1500
    T = _T(rows, cols, rng.integers(0, rows, nt), rng.integers(0, cols, nt), rng.integers(1, 6, nt))
    users = rng.integers(0, rows, 300)
    items = np.stack([rng.permutation(cols)[:n_top] for _ in users]).astype(np.uint32)
    items[rng.random(items.shape) < 0.1] = PAD
    items = np.sort(np.where(items == PAD, np.iinfo(np.int64).max, items.astype(np.int64)), axis=1)  # padding last
    items = np.where(items > cols, PAD, items).astype(np.uint32)
    for mr in (float("-inf"), 3.0):
        got = mfx.topn_metrics(items, T, users=users, min_rating=mr)
        want = _metrics_numpy(items, users, T, mr)
        assert got["users"] == want["users"]
        for key in ("hr", "precision", "recall", "ndcg"):
            assert abs(got[key] - want[key]) < 1e-12, key


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_recommender_without_gpu_fails_loudly(mfx):
    W = np.ones((5, 3), np.float32)
    H = np.ones((4, 3), np.float32)
    with pytest.raises(mfx.MfxError, match="no usable HIP device"):
        mfx.Recommender(W, H, 1)


def _exe():
    return os.path.join(ROOT, "cuda-recommender_amd", "mfx_train")


def test_cli_recommend_usage(tmp_path):
    for args in ([], ["model"], ["model", "dir", "10"], ["m", "d", "10", "o", "1", "extra"]):
        r = subprocess.run([_exe(), "-recommend"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "usage: mfx_train -recommend" in r.stderr
    r = subprocess.run([_exe(), "-recommend", "m", "d", "0", "o"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "N must be" in r.stderr


def test_cli_recommend_rejects_mismatched_model_before_the_gpu(mfx, tmp_path):
    g, d = load_golden("tiny")
    mfx.dataset.write_dataset_dir(str(tmp_path / "ds"), d)
    k = 4
    with open(tmp_path / "model.bin", "wb") as f:  # W has one row too many
        f.write(struct.pack("<qq", d.rows + 1, k) + np.zeros((d.rows + 1) * k, np.float32).tobytes())
        f.write(struct.pack("<qq", d.cols, k) + np.zeros(d.cols * k, np.float32).tobytes())
    r = subprocess.run([_exe(), "-recommend", str(tmp_path / "model.bin"), str(tmp_path / "ds"), "5",
                        str(tmp_path / "out.txt")], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "rating matrix" in r.stderr and "RECOMMEND FAILED" not in r.stderr
    assert not (tmp_path / "out.txt").exists()
