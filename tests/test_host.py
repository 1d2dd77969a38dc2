"""CPU-only tests: host logic, the dataset format, the flat-stream layout metadata and the C ABI
surface (the library must load and export every symbol include/mfx.h declares; compute entry
points must fail loudly without a GPU instead of falling back)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    return m


def test_library_exports_every_declared_symbol(mfx):
    hdr = open(os.path.join(ROOT, "include", "mfx.h")).read()
    declared = set(re.findall(r"\b(mfx_[a-z0-9_]+)\s*\(", hdr))
    from mfx import _lib as L
    lib = mfx.lib()
    assert declared, "no declarations parsed"
    for name in sorted(declared):
        assert hasattr(lib, name), f"libmfx.so does not export {name}"
    assert declared == set(L.SIGNATURES), declared ^ set(L.SIGNATURES)
    assert lib.mfx_version() == L.MFX_VERSION == 2  # the binding refuses a library of another ABI revision


def test_struct_layouts_match_header(mfx):
    import ctypes as C
    from mfx import _lib as L
    assert C.sizeof(L.mfx_csx) == 72 and C.sizeof(L.mfx_coo) == 32
    assert C.sizeof(L.mfx_params) == 76 and C.sizeof(L.mfx_iter_report) == 32
    p = L.mfx_params()
    mfx.lib().mfx_params_default(C.byref(p))
    # reference defaults, src/pmf.h:26-42
    assert (p.k, p.maxiter, p.maxinneriter, p.nBlocks, p.nThreadsPerBlock) == (10, 5, 1, 32, 256)
    assert abs(p.lambda_ - 0.1) < 1e-7 and p.schedule == 1


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_cpu_fallback_without_gpu(mfx):
    g, d = load_golden("tiny")
    assert mfx.device_count() == 0
    with pytest.raises(mfx.MfxError, match="no usable HIP device"):
        mfx.rank_one_sweep(d.csc_col_ptr, d.csc_row_idx, d.csc_val, g["ccd_T1__W0"][0].copy(), 0.1)
    W = np.array(g["ccd_T1__W0"]); H = np.array(g["ccd_T1__H0"])
    p = mfx.parameter(); p.k = int(g["k"][0])
    mfx.kernel_wrapper_ccdpp_NV(d, mfx.test_data_of(d), W, H, p)  # prints "CCD FAILED", returns
    assert mfx.kernel_wrapper_ccdpp_NV.last_status == -2
    assert np.array_equal(W, g["ccd_T1__W0"])  # untouched on failure


def test_initial_col_is_the_reference_init(mfx):
    for name in ("tiny", "edge"):
        g, d = load_golden(name)
        k = int(g["k"][0])
        assert np.array_equal(mfx.initial_col(k, d.rows), g["ccd_T1__W0"])  # CCD layout
        assert np.array_equal(mfx.initial_col(d.cols, k), g["als__H0"])     # ALS layout


def test_parse_command_line_matches_reference_scanner(mfx):
    p = mfx.parse_command_line(["x", "-CUDA", "-OMP", "-nBlocks", "32", "-nThreadsPerBlock", "512", "-k", "5", "-t", "15",
                                "-T", "3", "-l", "0.05", "-n", "8", "-q", "1", "../DATASETS/netflix/"])
    assert (p.enable_cuda, p.enable_omp, p.nBlocks, p.nThreadsPerBlock) == (True, True, 32, 512)
    assert (p.k, p.maxiter, p.maxinneriter, p.threads, p.verbose) == (5, 15, 3, 8, 1)
    assert abs(p.lambda_ - 0.05) < 1e-12 and p.src_dir == "../DATASETS/netflix/"
    assert mfx.parse_command_line(["x", "-ALS", "d"]).solver_type == mfx.solvertype.ALS
    d = mfx.parse_command_line(["x", "dir"])
    assert (d.k, d.maxiter, d.maxinneriter, d.threads) == (10, 5, 1, 4) and not d.enable_cuda
    assert mfx.parse_command_line(["x", "-p", "1", "dir"]).verbose == 1  # do_predict forces verbose
    for bad in (["x"], ["x", "-k", "3"], ["x", "dir", "-CUDA"][:2] + [], ["x", "-z", "1", "dir"]):
        if bad == ["x", "dir"]:
            continue
        with pytest.raises(mfx.UsageError):
            mfx.parse_command_line(bad)
    # quirk: a valueless flag as the LAST argv pre-consumes past the end -> usage (src/extras.cpp:76-78)
    with pytest.raises(mfx.UsageError):
        mfx.parse_command_line(["x", "-CUDA"])


def test_dataset_directory_roundtrip(mfx, tmp_path):
    g, d = load_golden("edge")
    mfx.dataset.write_dataset_dir(str(tmp_path / "ds"), d)
    back = mfx.dataset.read_dataset_dir(str(tmp_path / "ds"))
    for a in ("csr_row_ptr", "csr_col_idx", "csr_val", "csc_col_ptr", "csc_row_idx", "csc_val", "test_row", "test_col", "test_val"):
        assert np.array_equal(getattr(d, a), getattr(back, a)), a
    assert os.path.getsize(tmp_path / "ds" / "R_train_csr.indptr.bin") == 4 * (d.rows + 1)  # int32 ptr files
    tok = open(tmp_path / "ds" / "meta_modified_all").read().split()
    assert tok[:3] == [str(d.rows), str(d.cols), str(d.nnz)] and len(tok) == 16


def test_text_converter(mfx, tmp_path):
    (tmp_path / "tr.txt").write_text("1 1 5\n1 3 3\n2 2 4\n3 1 1\n3 3 2\n")
    (tmp_path / "te.txt").write_text("2 1 3.5\n")
    d = mfx.dataset.convert_text_ratings(str(tmp_path / "tr.txt"), str(tmp_path / "out"), str(tmp_path / "te.txt"))
    assert (d.rows, d.cols, d.nnz, d.nnz_test) == (3, 3, 5, 1)
    assert list(d.csr_row_ptr) == [0, 2, 3, 5] and list(d.csc_col_ptr) == [0, 2, 3, 5]
    assert list(d.csc_row_idx) == [0, 2, 1, 0, 2] and list(d.csc_val) == [5, 1, 4, 3, 2]
    assert np.array_equal(mfx.dataset.read_dataset_dir(str(tmp_path / "out")).csr_val, d.csr_val)


def test_converter_reads_the_movielens_file_formats(mfx, tmp_path):
    """ML-100K u.data (tabs + timestamp), ML-1M ratings.dat (`::`), ML-20M ratings.csv (header, commas, item ids with
    gaps -> compact_ids): the same five ratings in every dress give the same matrix."""
    trip = [(1, 1, 5.0), (1, 3, 3.0), (2, 2, 4.0), (3, 1, 1.0), (3, 3, 2.5)]
    (tmp_path / "u.data").write_text("".join(f"{i}\t{j}\t{r:g}\t88125{n}\n" for n, (i, j, r) in enumerate(trip)))
    (tmp_path / "ratings.dat").write_text("".join(f"{i}::{j}::{r:g}::97830{n}\n" for n, (i, j, r) in enumerate(trip)))
    gap = {1: 10, 2: 200, 3: 3000}  # item ids with gaps
    (tmp_path / "ratings.csv").write_text("userId,movieId,rating,timestamp\n" +
                                          "".join(f"{i},{gap[j]},{r:g},11{n}\n" for n, (i, j, r) in enumerate(trip)))
    ref = mfx.dataset.convert_text_ratings(str(tmp_path / "u.data"), str(tmp_path / "a"))
    assert (ref.rows, ref.cols, ref.nnz) == (3, 3, 5) and list(ref.csr_val) == [5, 3, 4, 1, 2.5]
    b = mfx.dataset.convert_text_ratings(str(tmp_path / "ratings.dat"), str(tmp_path / "b"))
    c = mfx.dataset.convert_text_ratings(str(tmp_path / "ratings.csv"), str(tmp_path / "c"), compact_ids=True)
    for d in (b, c):
        assert (d.rows, d.cols, d.nnz) == (3, 3, 5)
        assert np.array_equal(d.csr_row_ptr, ref.csr_row_ptr) and np.array_equal(d.csr_col_idx, ref.csr_col_idx)
        assert np.array_equal(d.csc_val, ref.csc_val)
    assert (tmp_path / "c" / "col_ids.txt").read_text().split() == ["10", "200", "3000"]
    h = mfx.dataset.convert_text_ratings(str(tmp_path / "ratings.dat"), str(tmp_path / "h"), test_frac=0.5, seed=1)
    assert h.nnz + h.nnz_test == 5 and 0 < h.nnz_test < 5 and (h.rows, h.cols) == (3, 3)
    assert np.array_equal(mfx.dataset.read_dataset_dir(str(tmp_path / "c")).csc_row_idx, ref.csc_row_idx)


def test_partition_rows_is_nnz_balanced_and_shards_reassemble(mfx):
    d = mfx.dataset.synth_ratings(997, 211, 30000, seed=5, skew=1.0, test_frac=0.02, empty_row_frac=0.05)
    for g in (1, 2, 3, 8):
        b = mfx.partition_rows(d, g)
        assert b[0] == 0 and b[-1] == d.rows and np.all(np.diff(b) >= 0)
        per = np.diff(d.csr_row_ptr.astype(np.int64)[b])
        assert per.sum() == d.nnz
        assert per.max() - per.min() <= 2 * np.diff(d.csr_row_ptr.astype(np.int64)).max()
        col_cnt = np.zeros(d.cols, np.int64); nt = 0
        for r in range(g):
            s = mfx.extract_shard(d, int(b[r]), int(b[r + 1]))
            s.validate()
            assert s.nnz == per[r]
            col_cnt += np.diff(s.csc_col_ptr.astype(np.int64)); nt += s.nnz_test
            # local CSR == the block of the global CSR; local CSC keeps R's per-column order
            lo = int(d.csr_row_ptr[b[r]])
            assert np.array_equal(s.csr_col_idx, d.csr_col_idx[lo:lo + s.nnz])
            for c in (0, d.cols // 2, d.cols - 1):
                gl = slice(int(d.csc_col_ptr[c]), int(d.csc_col_ptr[c + 1]))
                rows_c = d.csc_row_idx[gl].astype(np.int64)
                keep = (rows_c >= b[r]) & (rows_c < b[r + 1])
                ll = slice(int(s.csc_col_ptr[c]), int(s.csc_col_ptr[c + 1]))
                assert np.array_equal(s.csc_row_idx[ll].astype(np.int64), rows_c[keep] - b[r])
                assert np.array_equal(s.csc_val[ll], d.csc_val[gl][keep])
        assert np.array_equal(col_cnt, np.diff(d.csc_col_ptr.astype(np.int64))) and nt == d.nnz_test


def test_golden_compare_and_rmse_helpers(mfx):
    g, d = load_golden("small")
    k = int(g["k"][0])
    W, H = g["ccd_T1__W"], g["ccd_T1__H"]
    assert mfx.golden_compare(W, W, k, d.rows, quiet=True) == 0
    W2 = W.copy(); W2[0, 0] *= 1.2; W2[1, 5] *= 0.5
    assert mfx.golden_compare(W2, W, k, d.rows, quiet=True) == 2
    r = mfx.calculate_rmse_directly(W, H, mfx.test_data_of(d), k, False, quiet=True)
    assert abs(r - float(g["ccd_T1__final_rmse"][0])) < 5.1e-7


def _run_cli(args, cwd=None):
    import subprocess
    exe = os.path.join(ROOT, "cuda-recommender_amd", "mfx_train")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(ROOT, "cuda-recommender_amd"), "cli"], check=True, capture_output=True)
    return subprocess.run([exe] + args, capture_output=True, text=True, cwd=cwd, timeout=300)


def test_cli_usage_and_loader(mfx, tmp_path):
    """mfx_train keeps the reference's flags, help text and load() messages (src/extras.cpp:46-141)."""
    r = _run_cli([])
    assert r.returncode != 0 and "Usage: omp-pmf-train [options] data_dir [model_filename]" in r.stdout
    assert "-ALS: Flag to enable ALS algorithm" in r.stdout
    assert _run_cli(["-CUDA"]).returncode != 0  # valueless flag as last argv -> usage, like the reference
    r = _run_cli([str(tmp_path / "nope")])
    assert r.returncode != 0 and "Can't open meta input file." in r.stdout
    g, d = load_golden("tiny")
    mfx.dataset.write_dataset_dir(str(tmp_path / "ds"), d)
    r = _run_cli(["-k", "8", "-t", "2", str(tmp_path / "ds")])  # neither -CUDA nor -OMP: load, init, validate
    assert r.returncode == 0, r.stderr
    assert "[info] Picked Version: CCD!" in r.stdout and "K = 8 | InnerIter = 1 | OuterIter = 2" in r.stdout
    assert r.stdout.count("Check... PASS!") == 2  # untouched copies compare equal


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_cli_gpu_path_fails_loudly_without_gpu(mfx, tmp_path):
    g, d = load_golden("tiny")
    mfx.dataset.write_dataset_dir(str(tmp_path / "ds"), d)
    r = _run_cli(["-CUDA", "-k", "8", str(tmp_path / "ds")])
    assert "CCD FAILED: no usable HIP device" in r.stderr  # printed, process continues (CCD_CUDA.cu:174-176)
    assert "[info] CUDA Training time:" in r.stdout


@pytest.mark.parametrize("tag", ["ccd_T1", "als"])
def test_reference_model_file_loads_through_predict(tmp_path, tag):
    """(N2, pinned) tests/golden/*.npz hold the bytes the REFERENCE's own save_mat_t (src/tools.cpp:90-118) wrote for its
    final factors -- save_mat_t(W, fp, ifALS); save_mat_t(H, fp, ifALS) as at src/main.cpp:146-147, called by
    oracle/ref_driver.cpp.  Format facts, checked against the factors of the same fixture: two native longs (m, n), then
    m * n floats; with ifALS the matrix itself (rows x k), without it the k x rows CCD++ factor TRANSPOSED -- so both files
    read as rows x k row-major, which is what calculate_rmse_from_file (src/extras.cpp:143-180) loads.  Product code
    under test: mfx_train -predict (load_mat_t + the scoring loop) on the reference's bytes."""
    import struct
    g, d = load_golden("small")
    raw = g[tag + "__model"].tobytes()
    k = int(g["k"][0])
    W, H = g[tag + "__W"], g[tag + "__H"]
    if tag == "ccd_T1":
        W, H = W.T, H.T  # stored k x rows
    m, n = struct.unpack("<qq", raw[:16])
    assert (m, n) == (d.rows, k)
    off = 16 + 4 * m * n
    assert np.array_equal(np.frombuffer(raw[16:off], np.float32).reshape(m, n), W)
    m2, n2 = struct.unpack("<qq", raw[off:off + 16])
    assert (m2, n2) == (d.cols, k) and len(raw) == off + 16 + 4 * m2 * n2
    assert np.array_equal(np.frombuffer(raw[off + 16:], np.float32).reshape(m2, n2), H)
    (tmp_path / "model").write_bytes(raw)
    trip = list(zip(d.test_row.tolist(), d.test_col.tolist(), d.test_val.tolist()))
    (tmp_path / "test.txt").write_text("".join(f"{i + 1} {j + 1} {v!r}\n" for i, j, v in trip))  # 1-based, src/extras.cpp:169
    r = _run_cli(["-predict", str(tmp_path / "model"), str(tmp_path / "test.txt"), str(tmp_path / "out.txt")])
    assert r.returncode == 0, r.stderr
    pred = np.array([float(x) for x in (tmp_path / "out.txt").read_text().split()])
    want = np.array([float(np.dot(W[i].astype(np.float64), H[j].astype(np.float64))) for i, j, _ in trip])
    assert np.allclose(pred, want, atol=1e-5)
    rmse = float(np.sqrt(np.mean((want - np.array([v for *_, v in trip])) ** 2)))
    assert f"[FINAL INFO] Test RMSE = {rmse:f}" in r.stdout


def test_cli_predict_from_model_file(mfx, tmp_path):
    """mfx_train -predict: calculate_rmse_from_file semantics (src/extras.cpp:143-180): row-major model,
    1-based text test file, one prediction per output line."""
    import struct
    rng = np.random.default_rng(1)
    W, H = rng.standard_normal((5, 3)).astype(np.float32), rng.standard_normal((4, 3)).astype(np.float32)
    with open(tmp_path / "model", "wb") as f:
        for M in (W, H):
            f.write(struct.pack("<qq", *M.shape)); f.write(M.tobytes())
    trip = [(1, 1, 3.0), (5, 4, 1.5), (2, 3, 4.0)]
    (tmp_path / "test.txt").write_text("".join(f"{i} {j} {v}\n" for i, j, v in trip))
    r = _run_cli(["-predict", str(tmp_path / "model"), str(tmp_path / "test.txt"), str(tmp_path / "out.txt")])
    assert r.returncode == 0, r.stderr
    pred = np.array([float(x) for x in (tmp_path / "out.txt").read_text().split()])
    want = np.array([float(np.dot(W[i - 1].astype(np.float64), H[j - 1].astype(np.float64))) for i, j, _ in trip])
    assert np.allclose(pred, want, atol=1e-5)
    rmse = float(np.sqrt(np.mean((want - np.array([v for *_, v in trip])) ** 2)))
    assert f"[FINAL INFO] Test RMSE = {rmse:f}" in r.stdout


REF_DROPIN = os.path.join(ROOT, "oracle", "_ref", "ref_dropin")


@pytest.mark.skipif(not os.path.exists(REF_DROPIN), reason="oracle/_ref/ref_dropin not built: build() compiles it only where the reference sources exist")
def test_shim_compiles_against_reference_headers():
    """Drop-in proof: host/reference_api.hpp (both kernel_wrapper_*_NV signatures + the multi-shard
    wrapper) compiles against the REFERENCE's own pmf.h types and links with libmfx.so, with a
    main() that calls them exactly like src/main.cpp:11-17 does.  oracle/Makefile compiles
    oracle/ref_dropin.cpp that way during build(); here the binary must load libmfx.so and run."""
    import subprocess
    r = subprocess.run([REF_DROPIN], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr


def test_one_hip_runtime_whatever_the_import_order():
    """`import mfx` before `import torch` must not leave two libamdhip64 copies in the process (torch
    bundles its own under /opt/rocm's SONAME): mfx/_lib.py maps torch's copy first when torch is installed."""
    import subprocess
    import sys
    pytest.importorskip("torch")
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import mfx; from mfx import _lib; _lib.lib()\n"
            "a = _lib.mapped_hip_runtimes()\n"
            "import torch\n"
            "b = _lib.mapped_hip_runtimes()\n"
            "print(len(a), len(b), a == b)\n") % os.path.join(ROOT, "cuda-recommender_amd")
    env = {k: v for k, v in os.environ.items() if k != "MFX_HIP_RUNTIME"}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["1", "1", "True"], r.stdout
    # the detector itself: with the pin switched off the same sequence maps two runtimes
    env["MFX_HIP_RUNTIME"] = "system"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split()[:2] == ["1", "2"], r.stdout


def test_bench_launches_its_own_workers():
    """`python bench.py --gpus 2` with no launcher around it starts the two ranks itself (RANK / LOCAL_RANK /
    WORLD_SIZE / MASTER_*), they meet (gloo in this GPU-less rehearsal) and rank 0's single JSON line comes
    back through the parent; a bare N = 1 call stays a plain single process."""
    import json
    import subprocess
    import sys
    pytest.importorskip("torch")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    for n, want in ((8, 36.0), (2, 3.0), (1, 1.0)):  # 8: the driver's full-node launch shape
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--dry-run", "--workload", "config5"],
                           capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stderr
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]  # (gloo itself chats on stdout)
        assert len(lines) == 1, r.stdout
        d = json.loads(lines[0])
        assert d == {"dry_run": True, "n_gpus": n, "rank_sum": want, "workload": "config5"}
    # (r4) the DEFAULT workload at N > 1 -- what the driver's scaling run launches -- carries the north star's strong-scaling
    # workload as a second object in the same line: config5_strong, with exactly the keys the real leg fills in
    sys.path.insert(0, ROOT)
    import bench
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--dry-run"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert d["n_gpus"] == 8 and tuple(d["config5_strong"].keys()) == bench.CONFIG5_STRONG_KEYS
    for must in ("ms_per_step", "value", "allreduce_us_per_inner_iter", "host_enqueue_ms_per_step", "rank_nnz_min", "rank_nnz_max", "speedup_vs_n1", "n1_source"):
        assert must in bench.CONFIG5_STRONG_KEYS
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run", "--no-strong"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "config5_strong" not in json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    # a worker that fails makes the launcher fail
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run", "--no-such-flag"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode != 0
    # a rank that dies BEFORE it joins the collective (an OOM kill while the matrix is generated, a failed setup):
    # the launcher supervises every child, reports which rank went, stops the ranks left waiting for it and returns
    # that status -- within seconds, not at the driver's timeout
    import time
    for bad in (3, 0):
        t0 = time.time()
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--dry-run", "--dry-run-fail-rank", str(bad)],
                           capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 3, (r.returncode, r.stderr)
        assert f"rank {bad} exited with status 3" in r.stderr
        assert time.time() - t0 < 120
        assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_bench_dump_outputs_sample(tmp_path):
    """bench.dump_outputs (--dump-outputs): float32 factors, whole when small; a large one keeps the same seeded, sorted sample
    of its entities on every call, listed in <name>_index.npy; two factors of the Netflix-shaped k = 64 run's W size stay
    within 64 MB in all."""
    import sys
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(3)
    W = rng.standard_normal((8, 480189)).astype(np.float32)  # CCD layout: k x rows, entities along axis 1
    H = rng.standard_normal((17770, 8)).astype(np.float32)   # ALS layout: cols x k, entities along axis 0
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"W": (W, 1), "H": (H, 0)})
    assert sorted(os.listdir(tmp_path / "a")) == ["H.npy", "W.npy"]
    assert np.array_equal(np.load(tmp_path / "a" / "W.npy"), W) and np.array_equal(np.load(tmp_path / "a" / "H.npy"), H)
    for shape, axis in (((64, 480189), 1), ((240000, 128), 0)):
        big = np.zeros(shape, np.float32)
        big.flat[::97] = 1.0
        out = tmp_path / ("big%d" % shape[axis])
        bench.dump_outputs(str(out), {"W": (big, axis), "H": (big, axis)})
        assert sorted(os.listdir(out)) == ["H.npy", "H_index.npy", "W.npy", "W_index.npy"]
        assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64 << 20
        idx = np.load(out / "W_index.npy")
        assert idx.dtype == np.float64 and np.all(np.diff(idx) > 0) and idx[-1] < shape[axis]
        assert np.array_equal(idx, np.load(out / "H_index.npy"))
        Ws = np.load(out / "W.npy")
        assert Ws.dtype == np.float32 and np.array_equal(Ws, np.take(big, idx.astype(np.int64), axis=axis))


def test_profile_collector_refuses_foreign_builds(tmp_path):
    """(r4) tools/collect_profiles.py ties every PMC record to the kernel sources it was MEASURED on: the hash comes from the
    bench lines inside the run directory's own logs.  A run measured on another build (a foreign hash), or whose runs
    disagree, is refused -- exit status 2, nothing copied, no traffic entry; a run of this tree is recorded with that hash,
    and collecting the same run again does not touch the entry (no re-stamping)."""
    import json
    import subprocess
    import sys
    sys.path.insert(0, ROOT)
    import bench
    tool = os.path.join(ROOT, "tools", "collect_profiles.py")
    Z, m, n = 1000, 50, 20

    def make_run(root, sha_bench, sha_pmc):
        d = root / "final" / "netflix"
        for sub in ("pmc_fetch_size/x", "pmc_write_size/x"):
            (d / sub).mkdir(parents=True, exist_ok=True)
        line = lambda sha: json.dumps({"metric": "m", "n_gpus": 1, "kernel_src_sha16": sha, "als_src_sha16": "0" * 16,
                                       "config": {"rows_per_gpu": m, "cols": n, "nnz_global": Z}}) + "\n"
        (d / "bench.log").write_text(line(sha_bench))
        (d / "pmc_fetch_size.log").write_text("rocprof chatter\n" + line(sha_pmc))
        (d / "pmc_write_size.log").write_text(line(sha_pmc))
        hdr = "Kernel_Name,Counter_Name,Counter_Value\n"
        (d / "pmc_fetch_size/x/1_counter_collection.csv").write_text(hdr + '"void mfx::k_flat<2, true>(args)",FETCH_SIZE,100\n"void mfx::k_flat<3, true>(args)",FETCH_SIZE,120\n')
        (d / "pmc_write_size/x/1_counter_collection.csv").write_text(hdr + '"void mfx::k_flat<2, true>(args)",WRITE_SIZE,50\n"void mfx::k_flat<3, true>(args)",WRITE_SIZE,60\n')

    def collect(root):
        return subprocess.run([sys.executable, tool, "rXX", "--src", str(root / "final"), "--dst", str(root / "profiles")],
                              capture_output=True, text=True, timeout=120)

    tree = bench.kernel_source_hash()
    foreign = tmp_path / "foreign"
    make_run(foreign, "deadbeefdeadbeef", "deadbeefdeadbeef")
    r = collect(foreign)
    assert r.returncode == 2 and "REFUSED netflix" in r.stderr and "deadbeefdeadbeef" in r.stderr
    assert not (foreign / "profiles" / "rXX_bench_netflix.json").exists()
    assert json.load(open(foreign / "profiles" / "traffic.json")) == {}
    mixed = tmp_path / "mixed"
    make_run(mixed, tree, "deadbeefdeadbeef")  # the bench line is this tree's, the counter passes ran another build
    r = collect(mixed)
    assert r.returncode == 2 and "different builds" in r.stderr
    good = tmp_path / "good"
    make_run(good, tree, tree)
    r = collect(good)
    assert r.returncode == 0, r.stderr
    t1 = json.load(open(good / "profiles" / "traffic.json"))
    ent = t1[f"ccd_fused_csc_pass@{Z}"]
    assert ent["kernel_src_sha16"] == tree and ent["hbm_bytes_per_launch"] == (2 * 100 + 50) * 1024
    t1[f"ccd_fused_csc_pass@{Z}"]["collected"] = "1999-01-01"  # an old entry of the same measurement ...
    json.dump(t1, open(good / "profiles" / "traffic.json", "w"))
    assert collect(good).returncode == 0
    assert json.load(open(good / "profiles" / "traffic.json"))[f"ccd_fused_csc_pass@{Z}"]["collected"] == "1999-01-01"  # ... is not re-stamped
