"""Host-side mirror of the reference's solver interface over libmfx.so's C ABI.

Same names, argument order and error behaviour as the reference's driver-facing API
(reference: cuda_src/CCD_CUDA.h:49, cuda_src/ALS_CUDA.h:40, src/pmf.h:8-43, src/tools.h,
src/extras.h) so that tests read like the reference's own call sites (src/main.cpp:86-141).
Everything numerical happens inside libmfx.so on the GPU; nothing here computes on the CPU
except the reporting helpers the reference also runs on the host (calculate_rmse_directly,
golden_compare).
"""
from __future__ import annotations

import ctypes as C
import sys
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import _lib as L
from .dataset import RatingData


# ---------------------------------------------------------------------------------------------
# parameter / command line (reference: src/pmf.h:8-43, src/extras.cpp:46-141)
# ---------------------------------------------------------------------------------------------
class solvertype:
    CCD = 0
    ALS = 1


class parameter:
    """Field-for-field the reference's `parameter` with its defaults (src/pmf.h:26-42), plus the
    knobs this implementation adds (schedule, kernel_variant, device, profile)."""

    def __init__(self):
        self.solver_type = solvertype.CCD
        self.k = 10
        self.threads = 4
        self.maxiter = 5
        self.maxinneriter = 1
        self.lambda_ = 0.1
        self.eps = 1e-3
        self.do_predict = 0
        self.verbose = 0
        self.do_nmf = 0
        self.enable_cuda = False
        self.enable_omp = False
        self.nBlocks = 32
        self.nThreadsPerBlock = 256
        self.src_dir = "../data/simple"
        # additions
        self.device = 0
        self.schedule = 1
        self.kernel_variant = 1
        self.profile = 0
        self.tiles_per_span = 0
        self.panel_rows = 0
        self.wg_waves = 0
        self.graph = 0
        self.layout_build = 0
        self.log = 0  # print the reference's per-iteration "[-INFO-]" line
        # opt-in: give eps / do_nmf / (verbose and do_predict) their LIBPMF meaning.  The reference parses them and
        # reads none (src/pmf.h:33-36), so by default they are ignored here too.
        self.libpmf_flags = 0

    def to_c(self) -> L.mfx_params:
        p = L.mfx_params()
        L.lib().mfx_params_default(C.byref(p))
        p.k, p.lambda_, p.maxiter, p.maxinneriter = int(self.k), float(self.lambda_), int(self.maxiter), int(self.maxinneriter)
        p.nBlocks, p.nThreadsPerBlock = int(self.nBlocks), int(self.nThreadsPerBlock)
        p.verbose, p.device, p.schedule = int(self.log), int(self.device), int(self.schedule)
        p.kernel_variant, p.profile, p.tiles_per_span = int(self.kernel_variant), int(self.profile), int(self.tiles_per_span)
        p.panel_rows, p.wg_waves, p.graph = int(self.panel_rows), int(self.wg_waves), int(self.graph)
        p.layout_build = int(self.layout_build)
        if self.libpmf_flags:
            p.do_nmf, p.eps = int(self.do_nmf), float(self.eps)
            p.rank_trace = 1 if (self.verbose and self.do_predict) else 0
        return p


HELP = """Usage: omp-pmf-train [options] data_dir [model_filename]
options:
    -k rank : set the rank (default 10)
    -n threads : set the number of threads (default 4)
    -l lambda : set the regularization parameter lambda (default 0.1)
    -t max_iter: set the number of iterations (default 5)
    -T max_inner_iter: set the number of inner iterations used in CCDR1 (default 5)
    -e epsilon : set inner termination criterion epsilon of CCDR1 (default 1e-3)
    -p do_predict: do prediction or not (default 0)
    -q verbose: show information or not (default 0)
    -N do_nmf: do nmf (default 0)
    -CUDA: Flag to enable CUDA
    -nBlocks: Number of blocks on CUDA (default 32)
    -nThreadsPerBlock: Number of threads per block on CUDA (default 256)
    -ALS: Flag to enable ALS algorithm, if not present CCD++ is used
"""


class UsageError(SystemExit):
    """Raised where the reference calls exit_with_help() (prints HELP, exit status 1)."""


def parse_command_line(argv: Sequence[str]) -> parameter:
    """argv[0] is the program name.  Reproduces the reference's scanner including its quirk:
    every token starting with '-' pre-consumes the next argv, valueless flags (-CUDA, -OMP,
    -ALS) hand it back, so a valueless flag as the LAST argv is a usage error
    (src/extras.cpp:72-91)."""
    def usage():
        sys.stdout.write(HELP)
        raise UsageError(1)

    param = parameter()
    argc = len(argv)
    i = 1
    while i < argc:
        if not argv[i].startswith("-"):
            break
        i += 1
        if i >= argc:
            usage()
        flag, val = argv[i - 1], argv[i]
        if flag == "-nBlocks":
            param.nBlocks = _atoi(val)
        elif flag == "-nThreadsPerBlock":
            param.nThreadsPerBlock = _atoi(val)
        elif flag == "-CUDA":
            param.enable_cuda = True; i -= 1
        elif flag == "-OMP":
            param.enable_omp = True; i -= 1
        elif flag == "-ALS":
            param.solver_type = solvertype.ALS; i -= 1
        else:
            c = flag[1:2]
            if c == "k": param.k = _atoi(val)
            elif c == "n": param.threads = _atoi(val)
            elif c == "l": param.lambda_ = _atof(val)
            elif c == "t": param.maxiter = _atoi(val)
            elif c == "T": param.maxinneriter = _atoi(val)
            elif c == "e": param.eps = _atof(val)
            elif c == "p": param.do_predict = _atoi(val)
            elif c == "q": param.verbose = _atoi(val)
            elif c == "N": param.do_nmf = 1 if _atoi(val) == 1 else 0
            else:
                sys.stderr.write(f"unknown option: -{c}\n")
                usage()
        i += 1
    if param.do_predict != 0:
        param.verbose = 1
    if i >= argc:
        usage()
    param.src_dir = argv[i][:1023]
    return param


def _atoi(s: str) -> int:
    import re
    m = re.match(r"\s*[+-]?\d+", s)
    return int(m.group(0)) if m else 0


def _atof(s: str) -> float:
    import re
    m = re.match(r"\s*[+-]?(\d+\.?\d*([eE][+-]?\d+)?|\.\d+([eE][+-]?\d+)?)", s)
    return float(m.group(0)) if m else 0.0


# ---------------------------------------------------------------------------------------------
# data views
# ---------------------------------------------------------------------------------------------
@dataclass
class TestData:
    """reference: TestData (src/pmf_util.h:151-211)."""
    rows: int
    cols: int
    test_row: np.ndarray
    test_col: np.ndarray
    test_val: np.ndarray

    @property
    def nnz(self) -> int:
        return int(self.test_val.shape[0])


def test_data_of(d: RatingData) -> TestData:
    return TestData(d.rows, d.cols, d.test_row, d.test_col, d.test_val)


def _vp(a: Optional[np.ndarray]):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


def _csx(R: RatingData) -> L.mfx_csx:
    R.check_types()
    return L.mfx_csx(R.rows, R.cols, R.nnz, _vp(R.csc_col_ptr), _vp(R.csc_row_idx), _vp(R.csc_val),
                     _vp(R.csr_row_ptr), _vp(R.csr_col_idx), _vp(R.csr_val))


def _coo(T) -> L.mfx_coo:
    if T is None:
        return L.mfx_coo(0, None, None, None)
    for a, dt in ((T.test_row, np.uint32), (T.test_col, np.uint32), (T.test_val, np.float32)):
        assert a.dtype == dt and a.flags["C_CONTIGUOUS"]
    return L.mfx_coo(int(T.test_val.shape[0]), _vp(T.test_row), _vp(T.test_col), _vp(T.test_val))


def _device_csx_coo(d: dict):
    """(mfx_csx, mfx_coo) over the device tensors of a layout dict (mfx.synth_torch); the test triplets are optional."""
    ptr = lambda t: C.c_void_p(int(t.data_ptr())) if t is not None and t.numel() else None
    csx = L.mfx_csx(int(d["rows"]), int(d["cols"]), int(d["csr_val"].numel()), ptr(d["csc_col_ptr"]), ptr(d["csc_row_idx"]),
                    ptr(d["csc_val"]), ptr(d["csr_row_ptr"]), ptr(d["csr_col_idx"]), ptr(d["csr_val"]))
    tv = d.get("test_val")
    coo = L.mfx_coo(int(tv.numel()) if tv is not None else 0, ptr(d.get("test_row")), ptr(d.get("test_col")), ptr(tv))
    return csx, coo


def _f32c(a, shape=None) -> np.ndarray:
    assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags["C_CONTIGUOUS"], "need C-contiguous float32"
    if shape is not None:
        assert a.shape == tuple(shape), (a.shape, shape)
    return a


# ---------------------------------------------------------------------------------------------
# host helpers on the path
# ---------------------------------------------------------------------------------------------
def device_count() -> int:
    return int(L.lib().mfx_device_count())


def initial_col(k: int, n: int) -> np.ndarray:
    """reference: initial_col(X, k, n) (src/tools.cpp:165-173) -> [k][n], glibc rand(), seed 0."""
    X = np.empty((k, n), np.float32)
    L.lib().mfx_initial_col(X.ctypes.data_as(L.f32p), k, n)
    return X


def calculate_rmse_directly(W: np.ndarray, H: np.ndarray, T, rank: int, ifALS: bool, quiet: bool = False) -> float:
    """reference: src/extras.cpp:182-216 (host-side, fp64 accumulation of fp32 products)."""
    import time
    t0 = time.time()
    if T.nnz == 0:
        raise SystemExit(1)  # the reference exits when there are no test instances (:212)
    i, j = T.test_row.astype(np.int64), T.test_col.astype(np.int64)
    acc = np.zeros(T.nnz, np.float64)
    for t in range(rank):
        a = W[i, t] if ifALS else W[t, i]
        b = H[j, t] if ifALS else H[t, j]
        acc += (a * b).astype(np.float64)
    rmse = float(np.sqrt(np.sum((acc - T.test_val.astype(np.float64)) ** 2) / T.nnz))
    if not quiet:
        print("Test RMSE = %f. Calculated in %fs" % (rmse, time.time() - t0))
    return rmse


def golden_compare(W: np.ndarray, W_ref: np.ndarray, k: int, m: int, quiet: bool = False) -> int:
    """reference: src/extras.cpp:218-238: counts entries with |a-b| > 0.1*|b|; returns the count."""
    a, b = W.reshape(k, m).astype(np.float64), W_ref.reshape(k, m).astype(np.float64)
    errors = int(np.count_nonzero(np.abs(a - b) > 0.1 * np.abs(b)))
    if not quiet:
        if errors == 0:
            print("Check... PASS!")
        else:
            print("Check... NO PASS! [%.4f%%] #Error = %u out of %u entries." % (100.0 * errors / (k * m), errors, k * m))
    return errors


# ---------------------------------------------------------------------------------------------
# the two drop-in entry points
# ---------------------------------------------------------------------------------------------
def kernel_wrapper_ccdpp_NV(R: RatingData, T, W: np.ndarray, H: np.ndarray, parameters: parameter) -> List[L.mfx_iter_report]:
    """reference: kernel_wrapper_ccdpp_NV(SparseMatrix&, TestData&, MatData& W, MatData& H,
    parameter&) (cuda_src/CCD_CUDA.cu:164-179).  W [k][rows] initialised by the caller, H [k][cols]
    (content ignored, CCD++ starts from 0); both overwritten in place.  Like the reference it
    does not raise on a device failure: it prints "CCD FAILED: ..." and returns."""
    k = int(parameters.k)
    _f32c(W, (k, R.rows)); _f32c(H, (k, R.cols))
    reports = (L.mfx_iter_report * max(1, int(parameters.maxiter)))()
    csx, coo, p = _csx(R), _coo(T), parameters.to_c()
    rc = L.lib().mfx_ccdpp_run(C.byref(csx), C.byref(coo), _vp(W), _vp(H), C.byref(p), reports)
    kernel_wrapper_ccdpp_NV.last_status = rc
    return list(reports)[: int(parameters.maxiter)]


def kernel_wrapper_als_NV(R: RatingData, T, W: np.ndarray, H: np.ndarray, parameters: parameter) -> List[L.mfx_iter_report]:
    """reference: kernel_wrapper_als_NV (cuda_src/ALS_CUDA.cu:183-198).  W [rows][k], H [cols][k]."""
    k = int(parameters.k)
    _f32c(W, (R.rows, k)); _f32c(H, (R.cols, k))
    reports = (L.mfx_iter_report * max(1, int(parameters.maxiter)))()
    csx, coo, p = _csx(R), _coo(T), parameters.to_c()
    rc = L.lib().mfx_als_run(C.byref(csx), C.byref(coo), _vp(W), _vp(H), C.byref(p), reports)
    kernel_wrapper_als_NV.last_status = rc
    return list(reports)[: int(parameters.maxiter)]


# ---------------------------------------------------------------------------------------------
# resident solvers
# ---------------------------------------------------------------------------------------------
def _kernel_times(fn, handle):
    cap = 32
    names = (C.c_char_p * cap)()
    secs = (C.c_double * cap)()
    cnt = (C.c_int64 * cap)()
    n = fn(handle, cap, names, secs, cnt)
    return {names[i].decode(): (secs[i], cnt[i]) for i in range(n)}


class Comm:
    """RCCL communicator (one process per GPU).  `uid` is the 128-byte id from Comm.unique_id()
    on rank 0, shipped to the other ranks by the caller."""

    def __init__(self, uid: Optional[bytes], rank: int, nranks: int, device: int, local_group: Optional[int] = None):
        self.handle = C.c_void_p()
        if local_group is not None:  # in-process loopback group (threads of one process), see mfx.h
            L.check(L.lib().mfx_comm_create_local(C.byref(self.handle), int(local_group), rank, nranks, device))
        else:
            buf = C.create_string_buffer(bytes(uid), L.MFX_COMM_ID_BYTES)
            L.check(L.lib().mfx_comm_create(C.byref(self.handle), buf, rank, nranks, device))
        self.rank, self.nranks = rank, nranks

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(L.MFX_COMM_ID_BYTES)
        L.check(L.lib().mfx_comm_unique_id(buf))
        return buf.raw

    def agree(self, local_status: int = 0) -> int:
        """Collective: the worst status over all ranks (mfx_comm_agree).  Call it once after every rank's
        setup, failed ranks included, before the first iterate."""
        out = C.c_int(0)
        L.check(L.lib().mfx_comm_agree(self.handle, int(local_status), C.byref(out)))
        return int(out.value)

    def abort(self):
        """Releases the ranks waiting for this one after a local failure (mfx_comm_abort)."""
        if self.handle:
            L.lib().mfx_comm_abort(self.handle)

    def close(self):
        if self.handle:
            L.lib().mfx_comm_destroy(self.handle)
            self.handle = C.c_void_p()


class CcdSolver:
    """Resident CCD++ (mfx_ccd_*).  Arrays may be numpy (host) or anything exposing
    `data_ptr()` (torch CUDA tensors, space=device)."""

    def __init__(self, R, T, parameters: parameter, comm: Optional[Comm] = None,
                 global_col_nnz=None, global_test_nnz: int = 0, device_arrays: Optional[dict] = None):
        self.p = parameters
        self.handle = C.c_void_p()
        self._keep = []
        if device_arrays is not None:
            d = device_arrays
            ptr = lambda t: C.c_void_p(int(t.data_ptr())) if t is not None and t.numel() else None
            self.rows, self.cols, nnz = int(d["rows"]), int(d["cols"]), int(d["csr_val"].numel())
            csx = L.mfx_csx(self.rows, self.cols, nnz, ptr(d["csc_col_ptr"]), ptr(d["csc_row_idx"]), ptr(d["csc_val"]),
                            ptr(d["csr_row_ptr"]), ptr(d["csr_col_idx"]), ptr(d["csr_val"]))
            tv = d.get("test_val")
            coo = L.mfx_coo(int(tv.numel()) if tv is not None else 0, ptr(d.get("test_row")), ptr(d.get("test_col")), ptr(tv))
            space = L.MFX_DEVICE
            gcn = ptr(global_col_nnz) if global_col_nnz is not None else None
        else:
            self.rows, self.cols = R.rows, R.cols
            csx, coo, space = _csx(R), _coo(T), L.MFX_HOST
            gcn = _vp(global_col_nnz) if global_col_nnz is not None else None
        shard = None
        if comm is not None:
            shard = L.mfx_shard(comm.handle, gcn, int(global_test_nnz))
        cp = parameters.to_c()
        L.check(L.lib().mfx_ccd_create(C.byref(self.handle), C.byref(csx), C.byref(coo), C.byref(cp), space,
                                       C.byref(shard) if shard is not None else None))
        self.k = int(parameters.k)

    def set_factors(self, W):
        if hasattr(W, "data_ptr"):
            L.check(L.lib().mfx_ccd_set_factors(self.handle, C.c_void_p(int(W.data_ptr())), None, L.MFX_DEVICE))
        else:
            _f32c(W, (self.k, self.rows))
            L.check(L.lib().mfx_ccd_set_factors(self.handle, _vp(W), None, L.MFX_HOST))

    def iterate(self, n_outer: int, with_rmse: bool = True) -> List[L.mfx_iter_report]:
        reports = (L.mfx_iter_report * max(1, n_outer))()
        L.check(L.lib().mfx_ccd_iterate(self.handle, n_outer, 1 if with_rmse else 0, reports))
        return list(reports)[:n_outer]

    def get_factors(self):
        W = np.empty((self.k, self.rows), np.float32)
        H = np.empty((self.k, self.cols), np.float32)
        L.check(L.lib().mfx_ccd_get_factors(self.handle, _vp(W), _vp(H), L.MFX_HOST))
        return W, H

    def get_residual(self, nnz: int):
        a, b = np.empty(nnz, np.float32), np.empty(nnz, np.float32)
        L.check(L.lib().mfx_ccd_get_residual(self.handle, _vp(a), _vp(b)))
        return a, b

    def rank_trace(self, n_outer: int, k: int):
        """(rmse[n_outer, k], seconds[n_outer, k], ranks_done[n_outer]) of the last iterate() call (parameter.libpmf_flags
        with verbose and do_predict: calrmse_r1 after every rank; NaN where the eps rule skipped a rank)."""
        rm = np.full((n_outer, k), np.nan, np.float64)
        sec = np.zeros((n_outer, k), np.float64)
        done = np.zeros(n_outer, np.int32)
        n = L.lib().mfx_ccd_rank_trace(self.handle, n_outer * k, rm.ctypes.data_as(L.f64p), sec.ctypes.data_as(L.f64p), n_outer,
                                       done.ctypes.data_as(C.POINTER(C.c_int32)))
        L.check(min(n, 0))
        return rm[:n], sec[:n], done[:n]

    def set_profile(self, on: bool):
        L.check(L.lib().mfx_ccd_set_profile(self.handle, 1 if on else 0))

    def layout_info(self):
        """{"csc": {...}, "csr": {...}}: panels, entries per panel, kind ("lds" / "cache" / "plain" / "scatter" / "scatter32": 32-bit segment ids), tiles per span."""
        out = {}
        for side, name in ((0, "csc"), (1, "csr")):
            v = (C.c_int32 * 4)()
            L.check(L.lib().mfx_ccd_layout_info(self.handle, side, v))
            out[name] = {"panels": int(v[0]), "panel_rows": int(v[1]),
                         "kind": "scatter" if v[2] == 2 else "scatter32" if v[2] == 3 else "lds" if v[2] else ("cache" if v[1] else "plain"),
                         "tiles_per_span": int(v[3])}  # kind "tile": panel_rows = slice entries, tiles_per_span = segments per block
        return out

    def kernel_times(self):
        return _kernel_times(L.lib().mfx_ccd_kernel_times, self.handle)

    def close(self):
        if self.handle:
            L.lib().mfx_ccd_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _AlsHandle:
    """What the resident ALS trainers share: an mfx_als_t, the shape (rows, cols, k) and the factor and timing calls."""

    def set_factors(self, H, W=None):
        _f32c(H, (self.cols, self.k))
        if W is not None:
            _f32c(W, (self.rows, self.k))
        L.check(L.lib().mfx_als_set_factors(self.handle, _vp(W) if W is not None else None, _vp(H), L.MFX_HOST))

    def get_factors(self):
        W = np.empty((self.rows, self.k), np.float32)
        H = np.empty((self.cols, self.k), np.float32)
        L.check(L.lib().mfx_als_get_factors(self.handle, _vp(W), _vp(H), L.MFX_HOST))
        return W, H

    def kernel_times(self):
        return _kernel_times(L.lib().mfx_als_kernel_times, self.handle)

    def close(self):
        if self.handle:
            L.lib().mfx_als_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class AlsSolver(_AlsHandle):
    """Resident ALS (mfx_als_*)."""

    def __init__(self, R: RatingData, T, parameters: parameter, comm: Optional[Comm] = None,
                 row_range=None, col_range=None, device_arrays: Optional[dict] = None, block: Optional[int] = None,
                 count_reg: bool = False):
        """With `comm`: rank-local ALS shard of the GLOBAL matrix R -- this rank solves user rows
        row_range for the W-half and item columns col_range for the H-half (mfx_als_create_sharded).
        device_arrays: the matrix as a dict of device tensors (mfx.synth_torch), single GPU only.
        block=None: the exact solver (k <= 128).  block=d (0 = chosen from k): block subspace sweeps over d coordinates
        at a time (mfx_als_block_create, k <= 1024, single GPU) -- a different method above one block; there W, when
        given to set_factors, is the warm start of the first half-sweep.  count_reg (block sweeps only): lambda times
        the entries of the segment on the diagonal (the CCD++ objective) instead of lambda."""
        self.handle = C.c_void_p()
        cp = parameters.to_c()
        if block is None and count_reg:
            raise ValueError("count_reg needs block sweeps (block=...)")
        if block is not None:
            if comm is not None:
                raise ValueError("ALS by block sweeps is single GPU: comm must be None")
            reg = 1 if count_reg else 0
            if device_arrays is not None:
                self.rows, self.cols, self.k = int(device_arrays["rows"]), int(device_arrays["cols"]), int(parameters.k)
                (csx, coo), space = _device_csx_coo(device_arrays), L.MFX_DEVICE
            else:
                self.rows, self.cols, self.k = R.rows, R.cols, int(parameters.k)
                csx, coo, space = _csx(R), _coo(T), L.MFX_HOST
            L.check(L.lib().mfx_als_block_create(C.byref(self.handle), C.byref(csx), C.byref(coo), C.byref(cp), int(block), reg, space))
            return
        if device_arrays is not None:
            assert comm is None, "device-resident inputs: single-GPU ALS only"
            self.rows, self.cols, self.k = int(device_arrays["rows"]), int(device_arrays["cols"]), int(parameters.k)
            csx, coo = _device_csx_coo(device_arrays)
            L.check(L.lib().mfx_als_create(C.byref(self.handle), C.byref(csx), C.byref(coo), C.byref(cp), L.MFX_DEVICE))
            return
        self.rows, self.cols, self.k = R.rows, R.cols, int(parameters.k)
        if comm is None:
            csx, coo = _csx(R), _coo(T)
            L.check(L.lib().mfx_als_create(C.byref(self.handle), C.byref(csx), C.byref(coo), C.byref(cp), L.MFX_HOST))
            return
        (rl, rh), (cl, ch) = row_range, col_range
        a, b = int(R.csr_row_ptr[rl]), int(R.csr_row_ptr[rh])
        c, d = int(R.csc_col_ptr[cl]), int(R.csc_col_ptr[ch])
        keep = [np.ascontiguousarray(x) for x in (
            (R.csr_row_ptr[rl:rh + 1] - np.uint32(a)).astype(np.uint32), R.csr_col_idx[a:b], R.csr_val[a:b],
            (R.csc_col_ptr[cl:ch + 1] - np.uint32(c)).astype(np.uint32), R.csc_row_idx[c:d], R.csc_val[c:d])]
        self._keep = keep
        csx = L.mfx_csx(R.rows, R.cols, 0, _vp(keep[3]), _vp(keep[4]), _vp(keep[5]), _vp(keep[0]), _vp(keep[1]), _vp(keep[2]))
        csx.csc_col_ptr = keep[3].ctypes.data_as(C.c_void_p)  # pointer arrays are never empty
        csx.csr_row_ptr = keep[0].ctypes.data_as(C.c_void_p)
        sel = (R.test_row >= rl) & (R.test_row < rh)
        Tl = TestData(R.rows, R.cols, np.ascontiguousarray(R.test_row[sel]), np.ascontiguousarray(R.test_col[sel]),
                      np.ascontiguousarray(R.test_val[sel]))
        self._keep.append(Tl)
        coo = _coo(Tl)
        shard = L.mfx_als_shard(comm.handle, rl, rh, cl, ch, int(R.test_val.shape[0]))
        L.check(L.lib().mfx_als_create_sharded(C.byref(self.handle), C.byref(csx), C.byref(coo), C.byref(cp), C.byref(shard)))

    def iterate(self, n_iter: int, with_rmse: bool = True):
        reports = (L.mfx_iter_report * max(1, n_iter))()
        L.check(L.lib().mfx_als_iterate(self.handle, n_iter, 1 if with_rmse else 0, reports))
        return list(reports)[:n_iter]


def _reg_pair(alpha0, nu):
    """(alpha0, nu) of the _reg entry points, or None when neither is given (the un-suffixed entry point is called)."""
    if alpha0 is None and nu is None:
        return None
    return (1.0 if alpha0 is None else float(alpha0), 0.0 if nu is None else float(nu))


class ImplicitAlsSolver(_AlsHandle):
    """Resident implicit-feedback ALS (mfx_ials_create): R holds interaction strengths r >= 0, every (user, item)
    pair is in the loss with preference p = (r > 0) and confidence 1 + alpha r.  Factors use the ALS layout,
    W [rows][k] and H [cols][k].  device_arrays: the matrix as a dict of device tensors (mfx.synth_torch).
    block=None: the exact solver (k <= 128).  block=d (0 = chosen from k): block subspace sweeps over d coordinates at
    a time (mfx_ials_block_create, k <= 1024) -- a different method; there W, when given to set_factors, is the warm
    start of the first half-sweep.
    alpha0 / nu (either one given: mfx_ials_create_reg / mfx_ials_block_create_reg): the weight alpha0 > 0 of the unobserved
    pairs and the exponent 0 <= nu <= 1 of the frequency-scaled regulariser lambda (n + alpha0 N)^nu of a row or column
    with n entries over N; a lone alpha0 means nu = 0, a lone nu means alpha0 = 1.
    cg=(steps, tol): preconditioned conjugate gradients (mfx_ials_cg_create, k <= 1024): every half-sweep solves each row's
    system from its current value in at most `steps` steps, a row stopping once its relative residual is <= tol; W, when
    given to set_factors, is the warm start of the first half-sweep (else it starts cold).  Not with block=, alpha0=, nu=."""

    def __init__(self, R: Optional[RatingData], parameters: parameter, alpha: float, device_arrays: Optional[dict] = None,
                 block: Optional[int] = None, alpha0: Optional[float] = None, nu: Optional[float] = None,
                 cg: Optional[tuple] = None):
        self.handle = C.c_void_p()
        if cg is not None and (block is not None or alpha0 is not None or nu is not None):
            raise ValueError("ImplicitAlsSolver: cg= cannot be combined with block=, alpha0= or nu=")
        cp = parameters.to_c()
        if device_arrays is not None:
            self.rows, self.cols, self.k = int(device_arrays["rows"]), int(device_arrays["cols"]), int(parameters.k)
            csx, space = _device_csx_coo(device_arrays)[0], L.MFX_DEVICE
        else:
            self.rows, self.cols, self.k = R.rows, R.cols, int(parameters.k)
            csx, space = _csx(R), L.MFX_HOST
        reg = _reg_pair(alpha0, nu)
        if cg is not None:
            steps, tol = cg
            L.check(L.lib().mfx_ials_cg_create(C.byref(self.handle), C.byref(csx), C.byref(cp), float(alpha), int(steps), float(tol), space))
        elif reg is not None and block is None:
            L.check(L.lib().mfx_ials_create_reg(C.byref(self.handle), C.byref(csx), C.byref(cp), float(alpha), reg[0], reg[1], space))
        elif reg is not None:
            L.check(L.lib().mfx_ials_block_create_reg(C.byref(self.handle), C.byref(csx), C.byref(cp), float(alpha), reg[0], reg[1],
                                                      int(block), space))
        elif block is None:
            L.check(L.lib().mfx_ials_create(C.byref(self.handle), C.byref(csx), C.byref(cp), float(alpha), space))
        else:
            L.check(L.lib().mfx_ials_block_create(C.byref(self.handle), C.byref(csx), C.byref(cp), float(alpha), int(block), space))

    def iterate(self, n_iter: int):
        """n_iter (W-half, H-half) sweeps; the reports carry update_time (rmse stays 0)."""
        reports = (L.mfx_iter_report * max(1, n_iter))()
        L.check(L.lib().mfx_als_iterate(self.handle, n_iter, 0, reports))
        return list(reports)[:n_iter]

    def loss(self) -> float:
        """The implicit objective at the current factors (fp64, include/mfx.h mfx_ials_loss)."""
        out = C.c_double(0.0)
        L.check(L.lib().mfx_ials_loss(self.handle, C.byref(out)))
        return float(out.value)

    def cg_stats(self) -> dict:
        """The last iteration of a cg= solver (mfx_ials_cg_stats): for the W-half ("rows") and the H-half ("cols") the
        row-steps applied, the most steps a row took, the rows that ran out of steps without meeting tol, the failed rows."""
        out = (C.c_int64 * 8)()
        L.check(L.lib().mfx_ials_cg_stats(self.handle, out))
        keys = ("row_steps", "max_steps", "unconverged", "failed")
        return {half: {key: int(out[4 * i + j]) for j, key in enumerate(keys)} for i, half in enumerate(("rows", "cols"))}


_BPR_LOSS = {"bpr": 1, "warp": 2}  # MFX_BPR_NEG_HARDEST, MFX_BPR_NEG_WARP (include/mfx.h)


def _bpr_report(stats, seconds: float) -> dict:
    slots, skipped, bad, correct = (int(x) for x in stats)
    counted = slots - skipped - bad
    return {"slots": slots, "skipped": skipped, "bad": bad, "correct": correct,
            "auc": correct / counted if counted else float("nan"), "seconds": float(seconds)}


class BprSolver:
    """Resident BPR training (mfx_bpr_*, include/mfx.h): every stored entry of R is a positive interaction, a slot pairs
    it with an item drawn by a stateless hash of (seed, slot number), and `batch` slots make one step at frozen factors
    whose sums are exact -- so the factors are fixed bit for bit by (R, seed, parameters, batch).  Reads k, lambda_, device
    and profile of `parameters`.  Factors use the ALS layout, W [rows][k] and H [cols][k]; without set_factors the first
    step draws 0.1 * N(0, 1) factors from numpy.random.default_rng(init_seed).  device_arrays: the matrix as a dict of device
    tensors (mfx.synth_torch); only its CSR pointers and ids are read.

    negatives = M > 1 or loss = "warp" samples the negative by M trials per slot scored at the frozen factors
    (mfx_bpr_create_neg): loss = "bpr" trains against the best-scored trial outside the user's row (hardest of M),
    loss = "warp" against the first trial that violates the margin of 1, with the step scaled by rank_weight [M] of the
    number of trials it took (None: bpr_rank_weights(cols, M), LightFM's log weight).  The defaults are the uniform
    sampler, mfx_bpr_create."""

    def __init__(self, R: Optional[RatingData], parameters: parameter, lr: float, batch: int, seed: int = 0,
                 device_arrays: Optional[dict] = None, init_seed: Optional[int] = None, negatives: int = 1, loss: str = "bpr",
                 rank_weight=None):
        assert loss in _BPR_LOSS, loss
        self.handle = C.c_void_p()
        cp = parameters.to_c()
        if device_arrays is not None:
            self.rows, self.cols, self.k = int(device_arrays["rows"]), int(device_arrays["cols"]), int(parameters.k)
            csx, space = _device_csx_coo(device_arrays)[0], L.MFX_DEVICE
        else:
            self.rows, self.cols, self.k = R.rows, R.cols, int(parameters.k)
            csx, space = _csx(R), L.MFX_HOST
        self._init_seed, self._have_factors = init_seed, False
        if loss == "bpr" and int(negatives) == 1 and rank_weight is None:
            L.check(L.lib().mfx_bpr_create(C.byref(self.handle), C.byref(csx), C.byref(cp), float(lr), int(batch), int(seed), space))
        else:
            rw = None if rank_weight is None else np.ascontiguousarray(rank_weight, np.float32)
            assert rw is None or rw.shape == (int(negatives),), "rank_weight must hold one weight per trial"
            L.check(L.lib().mfx_bpr_create_neg(C.byref(self.handle), C.byref(csx), C.byref(cp), float(lr), int(batch), int(seed),
                                               _BPR_LOSS[loss], int(negatives), _vp(rw), space))

    def trial_stats(self) -> dict:
        """Since create (mfx_bpr_trial_stats): the slots that ended without a chosen trial and the sum of the chosen trial
        numbers -- with WARP the trials scored up to the violator."""
        out = (C.c_int64 * 2)()
        L.check(L.lib().mfx_bpr_trial_stats(self.handle, out))
        return {"none_chosen": int(out[0]), "chosen_trial_sum": int(out[1])}

    def set_factors(self, W, H):
        _f32c(W, (self.rows, self.k))
        _f32c(H, (self.cols, self.k))
        L.check(L.lib().mfx_bpr_set_factors(self.handle, _vp(W), _vp(H), L.MFX_HOST))
        self._have_factors = True

    def _default_factors(self):
        if not self._have_factors:
            rng = np.random.default_rng(self._init_seed)
            W = (0.1 * rng.standard_normal((self.rows, self.k))).astype(np.float32)
            H = (0.1 * rng.standard_normal((self.cols, self.k))).astype(np.float32)
            self.set_factors(W, H)

    def get_factors(self):
        W = np.empty((self.rows, self.k), np.float32)
        H = np.empty((self.cols, self.k), np.float32)
        L.check(L.lib().mfx_bpr_get_factors(self.handle, _vp(W), _vp(H), L.MFX_HOST))
        return W, H

    def steps(self, n: int) -> dict:
        """n steps from the current slot: {"slots", "skipped", "bad", "correct", "auc", "seconds"} of the call."""
        self._default_factors()
        stats, sec = (C.c_int64 * 4)(), C.c_double(0.0)
        L.check(L.lib().mfx_bpr_steps(self.handle, int(n), stats, C.byref(sec)))
        return _bpr_report(stats, sec.value)

    def iterate(self, n_epochs: int) -> List[dict]:
        """n_epochs epochs (the first finishes a started one): one report per epoch."""
        self._default_factors()
        n = int(n_epochs)
        stats, sec = (C.c_int64 * (4 * max(1, n)))(), (C.c_double * max(1, n))()
        L.check(L.lib().mfx_bpr_epochs(self.handle, n, stats, sec))
        return [_bpr_report(stats[4 * e:4 * e + 4], sec[e]) for e in range(n)]

    def position(self) -> int:
        out = C.c_int64(0)
        L.check(L.lib().mfx_bpr_position(self.handle, C.byref(out)))
        return int(out.value)

    def kernel_times(self) -> dict:
        """Stream seconds since create by kernel, collected with parameters.profile = 1 only."""
        out = (C.c_double * 4)()
        L.check(L.lib().mfx_bpr_kernel_times(self.handle, out))
        return dict(zip(("sample", "gradient", "scatter", "apply"), (float(x) for x in out)))

    def close(self):
        if self.handle:
            L.lib().mfx_bpr_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bpr_triples(R: RatingData, seed: int, first: int, count: int):
    """(u, i, j uint32 [count], skipped bool [count]) of the slots first .. first + count - 1 (mfx_bpr_triples: the
    sampler of BprSolver on the host, no GPU)."""
    count = int(count)
    u, i, j = (np.empty(count, np.uint32) for _ in range(3))
    s = np.empty(count, np.uint8)
    csx = _csx(R)
    L.check(L.lib().mfx_bpr_triples(int(seed), int(first), count, C.byref(csx), _u32(u), _u32(i), _u32(j), _vp(s)))
    return u, i, j, s.astype(bool)


def bpr_apply(W, H, u, i, j, lr: float, lam: float, skipped=None, device: int = 0):
    """One BPR step on the given triples at the factors W [rows][k], H [cols][k] (mfx_bpr_apply): returns (W', H', stats);
    a slot is skipped only where `skipped` says so."""
    W, H = np.array(_f32c(W)), np.array(_f32c(H))
    assert W.ndim == 2 and H.ndim == 2 and W.shape[1] == H.shape[1]
    u, i, j = (np.ascontiguousarray(a, np.uint32) for a in (u, i, j))
    assert u.shape == i.shape == j.shape and u.ndim == 1
    s = None if skipped is None else np.ascontiguousarray(skipped, np.uint8)
    assert s is None or s.shape == u.shape
    stats = (C.c_int64 * 4)()
    L.check(L.lib().mfx_bpr_apply(W.shape[0], H.shape[0], W.shape[1], _f32(W), _f32(H), u.shape[0], _u32(u), _u32(i), _u32(j),
                                  _vp(s), float(lr), float(lam), stats, device))
    return W, H, _bpr_report(stats, 0.0)


def bpr_trials(R: RatingData, seed: int, first: int, count: int, negatives: int):
    """(u, i uint32 [count], items uint32 [count][negatives], member bool [count][negatives]) of the slots first .. first +
    count - 1 (mfx_bpr_trials: the trial sampler of BprSolver(negatives=...) on the host, no GPU)."""
    count, m = int(count), int(negatives)
    u, i = (np.empty(count, np.uint32) for _ in range(2))
    items = np.empty((count, max(m, 0)), np.uint32)
    member = np.empty((count, max(m, 0)), np.uint8)
    csx = _csx(R)
    L.check(L.lib().mfx_bpr_trials(int(seed), int(first), count, m, C.byref(csx), _u32(u), _u32(i), _u32(items), _vp(member)))
    return u, i, items, member.astype(bool)


def bpr_rank_weights(cols: int, negatives: int) -> np.ndarray:
    """The default WARP weights (mfx_bpr_rank_weights): out[t - 1] = float32(log(max(1, (cols - 1) // t)))."""
    out = np.empty(max(int(negatives), 0), np.float32)
    L.check(L.lib().mfx_bpr_rank_weights(int(cols), int(negatives), _vp(out)))
    return out


def bpr_apply_neg(W, H, u, i, items, lr: float, lam: float, loss: str = "bpr", member=None, rank_weight=None, device: int = 0):
    """One step on the caller's trials items [n][M] at the factors W [rows][k], H [cols][k] (mfx_bpr_apply_neg): loss "bpr"
    is hardest of M, "warp" is WARP.  Returns (W', H', report, j, t): j [n] the chosen items and t [n] the chosen trials,
    0 where none was chosen.  A trial is a member of the user's row only where `member` says so."""
    W, H = np.array(_f32c(W)), np.array(_f32c(H))
    assert W.ndim == 2 and H.ndim == 2 and W.shape[1] == H.shape[1]
    u, i, items = (np.ascontiguousarray(a, np.uint32) for a in (u, i, items))
    assert u.shape == i.shape and u.ndim == 1 and items.ndim == 2 and items.shape[0] == u.shape[0]
    n, m = items.shape
    mem = None if member is None else np.ascontiguousarray(member, np.uint8)
    assert mem is None or mem.shape == items.shape
    rw = None if rank_weight is None else np.ascontiguousarray(rank_weight, np.float32)
    assert rw is None or rw.shape == (m,)
    stats = (C.c_int64 * 4)()
    j, t = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    L.check(L.lib().mfx_bpr_apply_neg(W.shape[0], H.shape[0], W.shape[1], _f32(W), _f32(H), n, _u32(u), _u32(i), m, _u32(items), _vp(mem),
                                      _BPR_LOSS[loss], _vp(rw), float(lr), float(lam), stats, _vp(j), _vp(t), device))
    return W, H, _bpr_report(stats, 0.0), j, t


# ---------------------------------------------------------------------------------------------
# LightGCN: BPR on graph-propagated embeddings (mfx_lgcn_*)
# ---------------------------------------------------------------------------------------------
class LightGcnSolver:
    """Resident LightGCN training (mfx_lgcn_*, include/mfx.h): BprSolver's deterministic mini-batch steps, with the vectors
    that enter the pairwise loss being the mean of the base embeddings and their `layers` propagated copies under the
    symmetrically normalised interaction graph; layers = 0 is BprSolver bit for bit.  Reads k, lambda_, device and profile of
    `parameters`; both sides of R's pattern are read, values ignored.  The base embeddings use the ALS layout, W0 [rows][k]
    and H0 [cols][k]; without set_base the first step draws BprSolver's defaults, 0.1 * N(0, 1) from
    numpy.random.default_rng(init_seed).  get_factors() returns the final embeddings (W, H), which serve Recommender, query,
    evaluate, IVF and MMR as any factors do.  Every step propagates the whole graph: its cost grows with nnz * k * layers."""

    def __init__(self, R: Optional[RatingData], parameters: parameter, lr: float, batch: int, layers: int, seed: int = 0,
                 device_arrays: Optional[dict] = None, init_seed: Optional[int] = None):
        self.handle = C.c_void_p()
        cp = parameters.to_c()
        if device_arrays is not None:
            self.rows, self.cols, self.k = int(device_arrays["rows"]), int(device_arrays["cols"]), int(parameters.k)
            csx, space = _device_csx_coo(device_arrays)[0], L.MFX_DEVICE
        else:
            self.rows, self.cols, self.k = R.rows, R.cols, int(parameters.k)
            csx, space = _csx(R), L.MFX_HOST
        self.layers = int(layers)
        self._init_seed, self._have_base = init_seed, False
        L.check(L.lib().mfx_lgcn_create(C.byref(self.handle), C.byref(csx), C.byref(cp), float(lr), int(batch), self.layers, int(seed), space))

    def set_base(self, W0, H0):
        _f32c(W0, (self.rows, self.k))
        _f32c(H0, (self.cols, self.k))
        L.check(L.lib().mfx_lgcn_set_base(self.handle, _vp(W0), _vp(H0), L.MFX_HOST))
        self._have_base = True

    def _default_base(self):
        if not self._have_base:
            rng = np.random.default_rng(self._init_seed)
            W0 = (0.1 * rng.standard_normal((self.rows, self.k))).astype(np.float32)
            H0 = (0.1 * rng.standard_normal((self.cols, self.k))).astype(np.float32)
            self.set_base(W0, H0)

    def _pair(self, fn):
        W = np.empty((self.rows, self.k), np.float32)
        H = np.empty((self.cols, self.k), np.float32)
        L.check(fn(self.handle, _vp(W), _vp(H), L.MFX_HOST))
        return W, H

    def get_base(self):
        """The base embeddings (W0, H0): what the steps update."""
        return self._pair(L.lib().mfx_lgcn_get_base)

    def get_factors(self):
        """The final embeddings (W, H) of the current base: lgcn_propagate(R, *get_base(), layers)."""
        return self._pair(L.lib().mfx_lgcn_get_factors)

    def steps(self, n: int) -> dict:
        """n steps from the current slot: {"slots", "skipped", "bad", "correct", "auc", "seconds"} of the call."""
        self._default_base()
        stats, sec = (C.c_int64 * 4)(), C.c_double(0.0)
        L.check(L.lib().mfx_lgcn_steps(self.handle, int(n), stats, C.byref(sec)))
        return _bpr_report(stats, sec.value)

    def iterate(self, n_epochs: int) -> List[dict]:
        """n_epochs epochs (the first finishes a started one): one report per epoch."""
        self._default_base()
        n = int(n_epochs)
        stats, sec = (C.c_int64 * (4 * max(1, n)))(), (C.c_double * max(1, n))()
        L.check(L.lib().mfx_lgcn_epochs(self.handle, n, stats, sec))
        return [_bpr_report(stats[4 * e:4 * e + 4], sec[e]) for e in range(n)]

    def position(self) -> int:
        out = C.c_int64(0)
        L.check(L.lib().mfx_lgcn_position(self.handle, C.byref(out)))
        return int(out.value)

    def kernel_times(self) -> dict:
        """Stream seconds since create by phase, collected with parameters.profile = 1 only."""
        out = (C.c_double * 6)()
        L.check(L.lib().mfx_lgcn_kernel_times(self.handle, out))
        return dict(zip(("sample", "forward", "gradient", "scatter", "backward", "update"), (float(x) for x in out)))

    def close(self):
        if self.handle:
            L.lib().mfx_lgcn_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def lgcn_propagate(R: RatingData, W0, H0, layers: int, device: int = 0):
    """The final embeddings (W, H) of the base embeddings W0 [rows][k], H0 [cols][k] over R's pattern (mfx_lgcn_propagate):
    the mean of the base and its `layers` propagated copies."""
    W0, H0 = _f32c(W0), _f32c(H0)
    assert W0.ndim == 2 and H0.ndim == 2 and W0.shape[1] == H0.shape[1] and W0.shape[0] == R.rows and H0.shape[0] == R.cols
    W, H = np.empty_like(W0), np.empty_like(H0)
    csx = _csx(R)
    L.check(L.lib().mfx_lgcn_propagate(C.byref(csx), _f32(W0), _f32(H0), W0.shape[1], int(layers), _f32(W), _f32(H), device))
    return W, H


def lgcn_apply(R: RatingData, W0, H0, u, i, j, layers: int, lr: float, lam: float, skipped=None, device: int = 0):
    """One LightGCN step on the given triples at the base embeddings W0, H0 (mfx_lgcn_apply): returns (W0', H0', stats); a
    slot is skipped only where `skipped` says so."""
    W0, H0 = np.array(_f32c(W0)), np.array(_f32c(H0))
    assert W0.ndim == 2 and H0.ndim == 2 and W0.shape[1] == H0.shape[1] and W0.shape[0] == R.rows and H0.shape[0] == R.cols
    u, i, j = (np.ascontiguousarray(a, np.uint32) for a in (u, i, j))
    assert u.shape == i.shape == j.shape and u.ndim == 1
    s = None if skipped is None else np.ascontiguousarray(skipped, np.uint8)
    assert s is None or s.shape == u.shape
    stats = (C.c_int64 * 4)()
    csx = _csx(R)
    L.check(L.lib().mfx_lgcn_apply(C.byref(csx), W0.shape[1], _f32(W0), _f32(H0), u.shape[0], _u32(u), _u32(i), _u32(j), _vp(s),
                                   int(layers), float(lr), float(lam), stats, device))
    return W0, H0, _bpr_report(stats, 0.0)


# ---------------------------------------------------------------------------------------------
# hybrid BPR: rows embedded through their features (mfx_hyb_*)
# ---------------------------------------------------------------------------------------------
@dataclass
class HybFeatures:
    """A feature matrix in CSR with values (mfx_features, include/mfx.h "Hybrid BPR"): n rows over nf features, ptr [n + 1]
    uint32, idx [nnz] uint32 strictly ascending inside a row, val [nnz] float32 with |v| <= 1, at most 1024 entries a row."""
    n: int
    nf: int
    ptr: np.ndarray
    idx: np.ndarray
    val: np.ndarray

    def to_c(self) -> L.mfx_features:
        for a, dt in ((self.ptr, np.uint32), (self.idx, np.uint32), (self.val, np.float32)):
            assert isinstance(a, np.ndarray) and a.dtype == dt and a.flags["C_CONTIGUOUS"], "need C-contiguous uint32 / float32 arrays"
        assert self.ptr.shape == (self.n + 1,) and self.idx.shape == self.val.shape and self.idx.ndim == 1
        return L.mfx_features(int(self.n), int(self.nf), _vp(self.ptr), _vp(self.idx), _vp(self.val))


def hyb_features(n: int, tag_rows=None, tag_ids=None, n_tags: int = 0, identity: bool = True, normalize: bool = True) -> HybFeatures:
    """LightFM's default feature matrix [I | tags] of n rows: feature r for row r itself (identity=True), then feature n + t
    (identity=False: t) for every pair (tag_rows[e], tag_ids[e]) = (row, t), a pair named twice counting once.  Every entry
    is 1, or with normalize=True float32(1 / entries of the row), so that a row sums to 1: this keeps |v| <= 1."""
    n, n_tags = int(n), int(n_tags)
    r = np.zeros(0, np.int64) if tag_rows is None else np.asarray(tag_rows, np.int64).ravel()
    t = np.zeros(0, np.int64) if tag_ids is None else np.asarray(tag_ids, np.int64).ravel()
    assert r.shape == t.shape, "tag_rows and tag_ids must pair up"
    assert r.size == 0 or (r.min() >= 0 and r.max() < n and t.min() >= 0 and t.max() < n_tags), "a tag pair is out of range"
    base = n if identity else 0
    nf = base + n_tags
    assert nf >= 1, "no features: identity=False needs n_tags >= 1"
    cells = np.unique(r * nf + base + t)  # row * nf + feature: ascending by row, then by feature
    if identity:
        cells = np.sort(np.concatenate([np.arange(n, dtype=np.int64) * (nf + 1), cells]))
    rows, idx = cells // nf, cells % nf
    counts = np.bincount(rows, minlength=n)
    ptr = np.concatenate([[0], np.cumsum(counts)])
    assert ptr[-1] < 2 ** 32 and (counts.max() if n else 0) <= 1024, "a row may hold at most 1024 features"
    val = np.ones(rows.size, np.float32)
    if normalize:
        val = (1.0 / counts[rows]).astype(np.float32)
    return HybFeatures(n, nf, ptr.astype(np.uint32), idx.astype(np.uint32), val)


def _features_c(F: Optional[HybFeatures], n: int, what: str):
    if F is None:
        return None, n
    assert isinstance(F, HybFeatures), f"{what} must be a HybFeatures (mfx.hyb_features) or None"
    return C.byref(F.to_c()), int(F.nf)


class HybridSolver:
    """Resident hybrid BPR training (mfx_hyb_*, include/mfx.h "Hybrid BPR"): BprSolver's deterministic mini-batch steps on
    rows whose vectors are the weighted sums of the embeddings of their features, so that a row without interactions still
    has a vector.  user_features / item_features are HybFeatures (mfx.hyb_features builds LightFM's [I | tags]); None is the
    identity, and with None on both sides the solver is BprSolver bit for bit.  Reads k, lambda_, device and profile of
    `parameters`; R's CSR pattern is read, values ignored; uniform negatives only.  The tables are Eu [nfu][k] and Ei
    [nfi][k]; without set_embeddings the first step draws 0.1 * N(0, 1) from numpy.random.default_rng(init_seed), Eu then
    Ei -- BprSolver's draw when both sides are identities.  get_factors() returns the embeddings (W, H) of all rows, which
    serve Recommender, query, evaluate, IVF and MMR as any factors do; embed(side, F) gives the rows of any other feature
    matrix over the same features: the cold start."""

    def __init__(self, R: Optional[RatingData], parameters: parameter, lr: float, batch: int, user_features: Optional[HybFeatures] = None,
                 item_features: Optional[HybFeatures] = None, seed: int = 0, device_arrays: Optional[dict] = None,
                 init_seed: Optional[int] = None):
        self.handle = C.c_void_p()
        cp = parameters.to_c()
        self.device = int(parameters.device)
        if device_arrays is not None:
            self.rows, self.cols, self.k = int(device_arrays["rows"]), int(device_arrays["cols"]), int(parameters.k)
            csx, space = _device_csx_coo(device_arrays)[0], L.MFX_DEVICE
        else:
            self.rows, self.cols, self.k = R.rows, R.cols, int(parameters.k)
            csx, space = _csx(R), L.MFX_HOST
        keep = []  # the device copies of the feature arrays live until create returns

        def side(F, n, what):
            if F is None:
                return None, n
            assert isinstance(F, HybFeatures), f"{what} must be a HybFeatures (mfx.hyb_features) or None"
            c = F.to_c()
            if space == L.MFX_DEVICE:
                import torch
                dev = device_arrays["csr_row_ptr"].device
                t = [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev) for a in (F.ptr, F.idx, F.val)]
                keep.extend(t)
                c = L.mfx_features(int(F.n), int(F.nf), *(C.c_void_p(int(x.data_ptr())) if x.numel() else None for x in t))
            keep.append(c)
            return C.byref(c), int(F.nf)

        fu, self.nfu = side(user_features, self.rows, "user_features")
        fi, self.nfi = side(item_features, self.cols, "item_features")
        self._init_seed, self._have_tables = init_seed, False
        L.check(L.lib().mfx_hyb_create(C.byref(self.handle), C.byref(csx), fu, fi, C.byref(cp), float(lr), int(batch), int(seed), space))

    def set_embeddings(self, Eu, Ei):
        _f32c(Eu, (self.nfu, self.k))
        _f32c(Ei, (self.nfi, self.k))
        L.check(L.lib().mfx_hyb_set_embeddings(self.handle, _vp(Eu), _vp(Ei), L.MFX_HOST))
        self._have_tables = True

    def _default_tables(self):
        if not self._have_tables:
            rng = np.random.default_rng(self._init_seed)
            Eu = (0.1 * rng.standard_normal((self.nfu, self.k))).astype(np.float32)
            Ei = (0.1 * rng.standard_normal((self.nfi, self.k))).astype(np.float32)
            self.set_embeddings(Eu, Ei)

    def get_embeddings(self):
        """The embedding tables (Eu, Ei): what the steps update."""
        Eu = np.empty((self.nfu, self.k), np.float32)
        Ei = np.empty((self.nfi, self.k), np.float32)
        L.check(L.lib().mfx_hyb_get_embeddings(self.handle, _vp(Eu), _vp(Ei), L.MFX_HOST))
        return Eu, Ei

    def get_factors(self):
        """The embeddings (W, H) of all rows at the current tables: hyb_embed of either feature matrix."""
        W = np.empty((self.rows, self.k), np.float32)
        H = np.empty((self.cols, self.k), np.float32)
        L.check(L.lib().mfx_hyb_get_factors(self.handle, _vp(W), _vp(H), L.MFX_HOST))
        return W, H

    def embed(self, side: str, F: HybFeatures) -> np.ndarray:
        """The rows of F over the current table of `side` ("user" or "item"): rows that were not in R included."""
        if side not in ("user", "item"):
            raise ValueError('side must be "user" or "item"')
        E = self.get_embeddings()[side == "item"]
        return hyb_embed(F, E, device=self.device)

    def steps(self, n: int) -> dict:
        """n steps from the current slot: {"slots", "skipped", "bad", "correct", "auc", "seconds"} of the call."""
        self._default_tables()
        stats, sec = (C.c_int64 * 4)(), C.c_double(0.0)
        L.check(L.lib().mfx_hyb_steps(self.handle, int(n), stats, C.byref(sec)))
        return _bpr_report(stats, sec.value)

    def iterate(self, n_epochs: int) -> List[dict]:
        """n_epochs epochs (the first finishes a started one): one report per epoch."""
        self._default_tables()
        n = int(n_epochs)
        stats, sec = (C.c_int64 * (4 * max(1, n)))(), (C.c_double * max(1, n))()
        L.check(L.lib().mfx_hyb_epochs(self.handle, n, stats, sec))
        return [_bpr_report(stats[4 * e:4 * e + 4], sec[e]) for e in range(n)]

    def position(self) -> int:
        out = C.c_int64(0)
        L.check(L.lib().mfx_hyb_position(self.handle, C.byref(out)))
        return int(out.value)

    def kernel_times(self) -> dict:
        """Stream seconds since create by phase, collected with parameters.profile = 1 only."""
        out = (C.c_double * 6)()
        L.check(L.lib().mfx_hyb_kernel_times(self.handle, out))
        return dict(zip(("sample", "embed", "gradient", "scatter", "spread", "apply"), (float(x) for x in out)))

    def close(self):
        if self.handle:
            L.lib().mfx_hyb_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def hyb_embed(F: HybFeatures, E, device: int = 0) -> np.ndarray:
    """The embeddings [F.n][k] of the rows of F over the table E [F.nf][k] (mfx_hyb_embed): per coordinate the FMA chain of
    the row's entries in stored order, started from the first product; an empty row gives +0."""
    E = _f32c(E)
    assert isinstance(F, HybFeatures) and E.ndim == 2 and E.shape[0] == F.nf, "E must hold one row per feature of F"
    out = np.empty((F.n, E.shape[1]), np.float32)
    c = F.to_c()
    L.check(L.lib().mfx_hyb_embed(C.byref(c), _vp(E), E.shape[1], _vp(out), device))
    return out


def hyb_apply(rows: int, cols: int, Eu, Ei, u, i, j, lr: float, lam: float, user_features: Optional[HybFeatures] = None,
              item_features: Optional[HybFeatures] = None, skipped=None, device: int = 0):
    """One hybrid step on the given triples at the tables Eu [nfu][k], Ei [nfi][k] (mfx_hyb_apply): returns (Eu', Ei',
    stats); None features are the identity; a slot is skipped only where `skipped` says so."""
    Eu, Ei = np.array(_f32c(Eu)), np.array(_f32c(Ei))
    fu, nfu = _features_c(user_features, int(rows), "user_features")
    fi, nfi = _features_c(item_features, int(cols), "item_features")
    assert Eu.ndim == 2 and Ei.ndim == 2 and Eu.shape[1] == Ei.shape[1] and Eu.shape[0] == nfu and Ei.shape[0] == nfi
    u, i, j = (np.ascontiguousarray(a, np.uint32) for a in (u, i, j))
    assert u.shape == i.shape == j.shape and u.ndim == 1
    s = None if skipped is None else np.ascontiguousarray(skipped, np.uint8)
    assert s is None or s.shape == u.shape
    stats = (C.c_int64 * 4)()
    L.check(L.lib().mfx_hyb_apply(int(rows), int(cols), Eu.shape[1], fu, fi, _vp(Eu), _vp(Ei), u.shape[0], _u32(u), _u32(i), _u32(j), _vp(s),
                                  float(lr), float(lam), stats, device))
    return Eu, Ei, _bpr_report(stats, 0.0)


# ---------------------------------------------------------------------------------------------
# item-kNN: the neighbourhood model on the interaction matrix (mfx_knn_*)
# ---------------------------------------------------------------------------------------------
def knn_weights(R: RatingData, scheme: Optional[str], k1: float = 1.2, b: float = 0.75) -> RatingData:
    """The interaction matrix R with the values of an item-kNN weighting, both orientations filled alike (pure numpy; the
    test triplets are carried over).  Every value is computed in fp64 and rounded to fp32 once.  With N = rows, c_i the
    entries of column i, n_u those of row u and nbar their mean over all rows:
      "cosine": x = r / ||r_.i||_2;
      "tfidf":  y = sqrt(r) * (ln N - ln(1 + c_i)), then column-normalised as for cosine;
      "bm25":   x = r * (k1 + 1) / (k1 * (1 - b + b * n_u / nbar) + r) * (ln N - ln(1 + c_i)), not normalised;
      None:     the values as they are.
    A column whose norm is 0 keeps zeros; empty columns stay empty."""
    if scheme not in ("cosine", "tfidf", "bm25", None):
        raise ValueError('scheme must be "cosine", "tfidf", "bm25" or None')
    R.check_types()
    if scheme is None:
        return R.copy()
    cptr = R.csc_col_ptr.astype(np.int64)
    rptr = R.csr_row_ptr.astype(np.int64)
    cnt = np.diff(cptr)
    col = np.repeat(np.arange(R.cols, dtype=np.int64), cnt)
    row = R.csc_row_idx.astype(np.int64)
    r = R.csc_val.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        idf = np.log(np.float64(R.rows)) - np.log(1.0 + cnt.astype(np.float64))
        if scheme == "bm25":
            n_u = np.diff(rptr).astype(np.float64)
            nbar = n_u.sum() / R.rows
            x = r * (k1 + 1.0) / (k1 * (1.0 - b + b * n_u[row] / nbar) + r) * idf[col]
        else:
            y = r if scheme == "cosine" else np.sqrt(r) * idf[col]
            norm = np.sqrt(np.bincount(col, weights=y * y, minlength=R.cols))
            x = np.where(norm[col] > 0, y / norm[col], 0.0)
    x = x.astype(np.float32)
    to_csr = np.lexsort((col, row))  # the CSC entries in (row, column) order: the CSR side
    if not np.array_equal(col[to_csr], R.csr_col_idx.astype(np.int64)):
        raise ValueError("the CSR and CSC sides of R do not hold the same entries in ascending order")
    out = R.copy()
    out.csc_val = x
    out.csr_val = np.ascontiguousarray(x[to_csr])
    return out


def _rows_recommend(call, handle, device: int, rows, n_top: int, keep_seen: bool, on_device: bool, tile_items: int):
    """The recommendation call shared by ItemKnn, Slim and Ease (mfx_*_recommend: one argument list) ->
    (items, scores, bad_rows)."""
    ptr, idx, val = (rows.csr_row_ptr, rows.csr_col_idx, rows.csr_val) if hasattr(rows, "csr_row_ptr") else rows
    if len(ptr.shape) != 1 or ptr.shape[0] < 1 or tuple(idx.shape) != tuple(val.shape) or len(idx.shape) != 1:
        raise ValueError("rows: ptr [U + 1], idx [nnz], val [nnz]")
    n, nnz, n_top = int(ptr.shape[0]) - 1, int(idx.shape[0]), int(n_top)
    flags = L.MFX_KNN_KEEP_SEEN if keep_seen else 0
    bad = C.c_int64(0)
    if any(_is_dev(a) for a in (ptr, idx, val)) or on_device:
        import torch
        dev = torch.device("cuda", device)

        def put(a, dt):
            if not _is_dev(a):
                a = np.ascontiguousarray(a, dt)
                a = torch.from_numpy(a.view(np.int32) if dt == np.uint32 else a).to(dev)
            assert a.is_contiguous() and a.element_size() == 4, "query tensors: contiguous 32-bit"
            return a
        keep = [put(ptr, np.uint32), put(idx, np.uint32), put(val, np.float32)]
        items = torch.empty((n, n_top), dtype=torch.int32, device=dev)
        scores = torch.empty((n, n_top), dtype=torch.float32, device=dev)
        p = lambda t: C.c_void_p(int(t.data_ptr())) if t.numel() else None
        L.check(call(handle, n, nnz, p(keep[0]), p(keep[1]), p(keep[2]), n_top, flags, int(tile_items), p(items), p(scores), C.byref(bad),
                     L.MFX_DEVICE))
    else:
        ptr, idx = np.ascontiguousarray(ptr, np.uint32), np.ascontiguousarray(idx, np.uint32)
        val = np.ascontiguousarray(val, np.float32)
        items = np.empty((n, n_top), np.uint32)
        scores = np.empty((n, n_top), np.float32)
        L.check(call(handle, n, nnz, _vp(ptr), _vp(idx), _vp(val), n_top, flags, int(tile_items), _vp(items), _vp(scores), C.byref(bad),
                     L.MFX_HOST))
    return items, scores, int(bad.value)


class _ItemModel:
    """What ItemKnn, Slim and Ease share: the handle of a model of `cols` items on `device`, the recommendation for rows of
    interactions (bad_rows: the bad rows of the last call) and the end of the handle.  _destroy: the model's mfx_*_destroy."""
    _destroy = ""

    def _start(self, device: int):
        self.handle = C.c_void_p()
        self.device, self.cols, self.bad_rows = int(device), 0, 0

    def _recommend(self, call, rows, n_top: int, keep_seen: bool, on_device: bool, tile_items: int):
        items, scores, self.bad_rows = _rows_recommend(call, self.handle, self.device, rows, n_top, keep_seen, on_device, tile_items)
        return items, scores

    def close(self):
        if self.handle:
            getattr(L.lib(), self._destroy)(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ItemKnn(_ItemModel):
    """Item-kNN on the interaction matrix (mfx_knn_*, include/mfx.h): the K nearest items of every item by the exact
    fixed-point X^T X of the weighted matrix, and recommendations as sums over the user's own items -- every bit fixed by
    the data.  R: a RatingData; weighting "cosine" / "tfidf" / "bm25" / None as in knn_weights (k1, b: BM25).
    device_arrays: the already weighted matrix as a dict of device tensors (mfx.synth_torch) instead of R; weighting must
    then be None.  tile_items: the test hook of mfx_knn_build."""
    _destroy = "mfx_knn_destroy"

    def __init__(self, R: Optional[RatingData], K: int, weighting: Optional[str] = "cosine", k1: float = 1.2, b: float = 0.75,
                 device: int = 0, device_arrays: Optional[dict] = None, tile_items: int = 0):
        self._start(device)
        self.K = int(K)
        if device_arrays is not None:
            if weighting is not None:
                raise ValueError("device_arrays are taken as they are: pass weighting=None")
            self.cols = int(device_arrays["cols"])
            csx, space = _device_csx_coo(device_arrays)[0], L.MFX_DEVICE
        else:
            X = knn_weights(R, weighting, k1, b)
            self.cols = X.cols
            csx, space = _csx(X), L.MFX_HOST
        L.check(L.lib().mfx_knn_build(C.byref(self.handle), C.byref(csx), self.K, int(tile_items), space, self.device))

    @classmethod
    def from_lists(cls, nbr_idx, nbr_sim, device: int = 0) -> "ItemKnn":
        """A model from given lists nbr_idx [cols][K] (uint32, PAD_ITEM at the tail only) and nbr_sim [cols][K] (float32):
        numpy arrays, or GPU tensors (the ids as int32 bits)."""
        if tuple(nbr_idx.shape) != tuple(nbr_sim.shape) or len(nbr_idx.shape) != 2:
            raise ValueError("nbr_idx and nbr_sim must both be [cols][K]")
        self = cls.__new__(cls)
        self._start(device)
        self.cols, self.K = int(nbr_idx.shape[0]), int(nbr_idx.shape[1])
        if _is_dev(nbr_idx) != _is_dev(nbr_sim):
            raise ValueError("nbr_idx and nbr_sim must both be host arrays or both device tensors")
        if _is_dev(nbr_idx):
            assert nbr_idx.is_contiguous() and nbr_idx.element_size() == 4 and nbr_sim.is_contiguous() and nbr_sim.element_size() == 4
            pi, ps, space = C.c_void_p(int(nbr_idx.data_ptr())), C.c_void_p(int(nbr_sim.data_ptr())), L.MFX_DEVICE
        else:
            nbr_idx = np.ascontiguousarray(nbr_idx, np.uint32)
            nbr_sim = np.ascontiguousarray(nbr_sim, np.float32)
            pi, ps, space = _vp(nbr_idx), _vp(nbr_sim), L.MFX_HOST
        L.check(L.lib().mfx_knn_create_from_lists(C.byref(self.handle), self.cols, self.K, pi, ps, space, self.device))
        return self

    def lists(self):
        """(nbr_idx uint32 [cols][K], nbr_sim float32 [cols][K]): unused slots hold PAD_ITEM and -inf."""
        idx = np.empty((self.cols, self.K), np.uint32)
        sim = np.empty((self.cols, self.K), np.float32)
        L.check(L.lib().mfx_knn_lists(self.handle, _vp(idx), _vp(sim), L.MFX_HOST))
        return idx, sim

    def neighbours(self, n_top: int, items=None, on_device: bool = False):
        """The first n_top <= K stored neighbours of `items` (None: every item in order) -> (ids [Q, n_top], sims
        [Q, n_top]).  An `items` tensor on the GPU or on_device=True: the results are int32 / float32 tensors on it."""
        n_top = int(n_top)
        if _is_dev(items) or on_device:
            import torch
            dev = torch.device("cuda", self.device)
            q = _to_dev32(items, dev) if items is not None else None
            n = int(q.numel()) if q is not None else self.cols
            ids = torch.empty((n, n_top), dtype=torch.int32, device=dev)
            sims = torch.empty((n, n_top), dtype=torch.float32, device=dev)
            p = lambda t: C.c_void_p(int(t.data_ptr())) if t is not None and t.numel() else None
            L.check(L.lib().mfx_knn_neighbours(self.handle, n, p(q), n_top, p(ids), p(sims), L.MFX_DEVICE))
            return ids, sims
        q = _ids_np(items, "items").astype(np.uint32) if items is not None else None
        n = int(q.size) if q is not None else self.cols
        ids = np.empty((n, n_top), np.uint32)
        sims = np.empty((n, n_top), np.float32)
        L.check(L.lib().mfx_knn_neighbours(self.handle, n, _vp(q), n_top, _vp(ids), _vp(sims), L.MFX_HOST))
        return ids, sims

    def recommend(self, rows, n_top: int, keep_seen: bool = False, on_device: bool = False, tile_items: int = 0):
        """Top-n_top items of the users given by their interactions -> (items [U, n_top], scores [U, n_top]); the rows'
        own items are left out unless keep_seen.  rows: a RatingData-like CSR (csr_row_ptr / csr_col_idx / csr_val) or a
        (ptr, idx, val) triple of numpy arrays or GPU tensors, as for Recommender.fold_in.  The number of bad rows (all
        pads: a term that is not finite or of magnitude >= 64) is left in self.bad_rows.  Tensors in, or on_device=True:
        the results are tensors on the device (items as int32 holding the uint32 ids)."""
        return self._recommend(L.lib().mfx_knn_recommend, rows, n_top, keep_seen, on_device, tile_items)

    def times(self) -> dict:
        """Seconds of the build (checks and work order, similarity pass) and of recommend summed over the calls (checks, pass)."""
        out = (C.c_double * 4)()
        L.check(L.lib().mfx_knn_times(self.handle, out))
        return dict(zip(("build_checks", "build_pass", "recommend_checks", "recommend_pass"), (float(x) for x in out)))


# ---------------------------------------------------------------------------------------------
# SLIM: sparse linear item models on given supports (mfx_slim_*)
# ---------------------------------------------------------------------------------------------
def _slim_support(support, cols: int, K: int, on_dev: bool, device: int):
    """The support [cols][K] of a SLIM call as (pointer, keep-alive): an ItemKnn's ids, a numpy array or a GPU tensor, brought
    to the side (host / device) where the matrix of the call lives."""
    if isinstance(support, ItemKnn):
        if (support.cols, support.K) != (cols, K):
            raise ValueError(f"support: an ItemKnn of {support.cols} items and K = {support.K}, need {cols} and {K}")
        if on_dev:
            import torch
            t = torch.empty((cols, K), dtype=torch.int32, device=torch.device("cuda", device))
            L.check(L.lib().mfx_knn_lists(support.handle, C.c_void_p(int(t.data_ptr())), None, L.MFX_DEVICE))
            return C.c_void_p(int(t.data_ptr())), t
        support = support.lists()[0]
    if tuple(support.shape) != (cols, K):
        raise ValueError(f"support must be [cols = {cols}][K = {K}], got {tuple(support.shape)}")
    if on_dev:
        t = _to_dev32(support.reshape(-1), __import__("torch").device("cuda", device))
        return C.c_void_p(int(t.data_ptr())), t
    a = support.cpu().numpy().view(np.uint32) if _is_dev(support) else support
    a = np.ascontiguousarray(a, np.uint32)
    return _vp(a), a


def _slim_matrix(R, weighting, device_arrays):
    """(mfx_csx, memory space, cols, keep-alive) of the matrix of a SLIM call."""
    if device_arrays is not None:
        if weighting is not None:
            raise ValueError("device_arrays are taken as they are: pass weighting=None")
        return _device_csx_coo(device_arrays)[0], L.MFX_DEVICE, int(device_arrays["cols"]), device_arrays
    X = knn_weights(R, weighting)
    return _csx(X), L.MFX_HOST, X.cols, X


def slim_gram(R: Optional[RatingData], K: int, support, weighting: Optional[str] = None, device: int = 0,
              device_arrays: Optional[dict] = None, tile_items: int = 0):
    """The Gram blocks [cols][K + 1][K] of mfx_slim_gram (include/mfx.h): for every item j the fixed-point X^T X over its
    support S_j (rows 0 .. K - 1, d on the diagonal) and against j itself (row K).  A numpy array, or with device_arrays a
    float32 tensor on the device."""
    csx, space, cols, keep = _slim_matrix(R, weighting, device_arrays)
    ps, keep_s = _slim_support(support, cols, int(K), space == L.MFX_DEVICE, device)
    if space == L.MFX_DEVICE:
        import torch
        out = torch.empty((cols, int(K) + 1, int(K)), dtype=torch.float32, device=torch.device("cuda", device))
        po = C.c_void_p(int(out.data_ptr()))
    else:
        out = np.empty((cols, int(K) + 1, int(K)), np.float32)
        po = _vp(out)
    L.check(L.lib().mfx_slim_gram(C.byref(csx), int(K), ps, int(tile_items), po, space, device))
    return out


def slim_solve(blocks, n_real=None, l1: float = 1.0, l2: float = 10.0, sweeps: int = 10, tol: float = 0.0, signed: bool = False,
               device: int = 0):
    """mfx_slim_solve (include/mfx.h) on blocks [n][K + 1][K] (float32 numpy) with n_real [n] real slots each (None: K) ->
    (w float32 [n][K], sweeps_used int32 [n], failed)."""
    blocks = np.ascontiguousarray(blocks, np.float32)
    if blocks.ndim != 3 or blocks.shape[1] != blocks.shape[2] + 1:
        raise ValueError("blocks must be [n][K + 1][K]")
    n, K = int(blocks.shape[0]), int(blocks.shape[2])
    nr = None
    if n_real is not None:
        nr = np.ascontiguousarray(n_real, np.uint32)
        if nr.shape != (n,):
            raise ValueError("n_real must be [n]")
    w = np.empty((n, K), np.float32)
    used = np.empty(n, np.int32)
    failed = C.c_int64(0)
    L.check(L.lib().mfx_slim_solve(n, K, _vp(blocks), _vp(nr), float(l1), float(l2), int(sweeps), float(tol),
                                   L.MFX_SLIM_SIGNED if signed else 0, _vp(w), _vp(used), C.byref(failed), L.MFX_HOST, device))
    return w, used, int(failed.value)


class Slim(_ItemModel):
    """SLIM on given supports (mfx_slim_*, include/mfx.h): for every item the elastic-net regression of its column on the K
    columns of its support, trained on the GPU by coordinate descent on the exact fixed-point Gram matrix, and
    recommendations as sums over the user's own items -- every bit fixed by the data.  R: a RatingData, its values taken
    under `weighting` (knn_weights; None: as they are).  support: [cols][K] ids (PAD_ITEM at the tail only), an ItemKnn, or
    None: the ids of ItemKnn(R, K, "cosine").  l1, l2: the penalties; at most `sweeps` sweeps per item, an item stops after
    the first sweep whose largest change is <= tol; signed: weights of either sign (default: non-negative).
    device_arrays: the matrix as a dict of device tensors (mfx.synth_torch) instead of R; weighting must then be None and a
    support be given.  tile_items: the test hook of mfx_slim_train."""
    _destroy = "mfx_slim_destroy"

    def __init__(self, R: Optional[RatingData], K: int, l1: float = 1.0, l2: float = 10.0, sweeps: int = 10, tol: float = 0.0,
                 signed: bool = False, weighting: Optional[str] = None, support=None, device: int = 0,
                 device_arrays: Optional[dict] = None, tile_items: int = 0):
        self._start(device)
        self.K, self.failed = int(K), 0
        if support is None and device_arrays is not None and weighting is None:
            raise ValueError("device_arrays need a support (an ItemKnn or [cols][K] ids)")
        csx, space, self.cols, keep = _slim_matrix(R, weighting, device_arrays)
        if support is None:
            with ItemKnn(R, self.K, "cosine", device=self.device) as nn:
                support = nn.lists()[0]
        ps, keep_s = _slim_support(support, self.cols, self.K, space == L.MFX_DEVICE, self.device)
        failed = C.c_int64(0)
        L.check(L.lib().mfx_slim_train(C.byref(self.handle), C.byref(csx), self.K, ps, float(l1), float(l2), int(sweeps), float(tol),
                                       L.MFX_SLIM_SIGNED if signed else 0, int(tile_items), C.byref(failed), space, self.device))
        self.failed = int(failed.value)

    @classmethod
    def from_lists(cls, support, w, device: int = 0) -> "Slim":
        """A model from a support [cols][K] (uint32, PAD_ITEM at the tail only) and weights w [cols][K] (float32): numpy
        arrays, or GPU tensors (the ids as int32 bits)."""
        if tuple(support.shape) != tuple(w.shape) or len(support.shape) != 2:
            raise ValueError("support and w must both be [cols][K]")
        if _is_dev(support) != _is_dev(w):
            raise ValueError("support and w must both be host arrays or both device tensors")
        self = cls.__new__(cls)
        self._start(device)
        self.failed = 0
        self.cols, self.K = int(support.shape[0]), int(support.shape[1])
        if _is_dev(support):
            assert support.is_contiguous() and support.element_size() == 4 and w.is_contiguous() and w.element_size() == 4
            ps, pw, space = C.c_void_p(int(support.data_ptr())), C.c_void_p(int(w.data_ptr())), L.MFX_DEVICE
        else:
            support = np.ascontiguousarray(support, np.uint32)
            w = np.ascontiguousarray(w, np.float32)
            ps, pw, space = _vp(support), _vp(w), L.MFX_HOST
        L.check(L.lib().mfx_slim_create_from_lists(C.byref(self.handle), self.cols, self.K, ps, pw, space, self.device))
        return self

    def weights(self):
        """(support uint32 [cols][K], w float32 [cols][K]): unused slots hold PAD_ITEM and 0."""
        sup = np.empty((self.cols, self.K), np.uint32)
        w = np.empty((self.cols, self.K), np.float32)
        L.check(L.lib().mfx_slim_weights(self.handle, _vp(sup), _vp(w), None, L.MFX_HOST))
        return sup, w

    @property
    def sweeps_used(self) -> np.ndarray:
        """int32 [cols]: the sweeps every item ran (0 for a model from lists)."""
        used = np.empty(self.cols, np.int32)
        L.check(L.lib().mfx_slim_weights(self.handle, None, None, _vp(used), L.MFX_HOST))
        return used

    def recommend(self, rows, n_top: int, keep_seen: bool = False, on_device: bool = False, tile_items: int = 0):
        """Top-n_top items of the users given by their interactions, as ItemKnn.recommend: the score of j is the sum of
        x_i * w_ij over the row's items i whose weight for j is stored.  The number of bad rows is left in self.bad_rows."""
        return self._recommend(L.lib().mfx_slim_recommend, rows, n_top, keep_seen, on_device, tile_items)

    def times(self) -> dict:
        """Seconds of the training (checks and inverse lists, Gram pass, solve) and of recommend summed over the calls."""
        out = (C.c_double * 5)()
        L.check(L.lib().mfx_slim_times(self.handle, out))
        return dict(zip(("train_checks", "gram_pass", "solve", "recommend_checks", "recommend_pass"), (float(x) for x in out)))


# ---------------------------------------------------------------------------------------------
# EASE: closed-form dense item-item models (mfx_ease_*)
# ---------------------------------------------------------------------------------------------
def _ease_matrix(R, weighting, k1, b, device_arrays):
    """(mfx_csx, memory space, cols, keep-alive) of the matrix of an EASE call."""
    if device_arrays is not None:
        if weighting is not None:
            raise ValueError("device_arrays are taken as they are: pass weighting=None")
        return _device_csx_coo(device_arrays)[0], L.MFX_DEVICE, int(device_arrays["cols"]), device_arrays
    X = knn_weights(R, weighting, k1, b)
    return _csx(X), L.MFX_HOST, X.cols, X


def _ease_square(a, what: str):
    """A square float32 matrix of an EASE call as (pointer, memory space, n, keep-alive): numpy or a GPU tensor."""
    if len(a.shape) != 2 or a.shape[0] != a.shape[1]:
        raise ValueError(f"{what} must be a square matrix")
    if _is_dev(a):
        import torch
        if a.dtype != torch.float32:
            raise ValueError(f"{what}: a device tensor must be float32")
        a = a.contiguous()
        return C.c_void_p(int(a.data_ptr())), L.MFX_DEVICE, int(a.shape[0]), a
    a = np.ascontiguousarray(a, np.float32)
    return _vp(a), L.MFX_HOST, int(a.shape[0]), a


def _ease_out(like_dev: bool, shape, device: int):
    """An uninitialised float32 result on the side of the input -> (array, pointer)."""
    if like_dev:
        import torch
        out = torch.empty(shape, dtype=torch.float32, device=torch.device("cuda", device))
        return out, C.c_void_p(int(out.data_ptr()))
    out = np.empty(shape, np.float32)
    return out, _vp(out)


def ease_gram(R: Optional[RatingData], lam: float, weighting: Optional[str] = None, k1: float = 1.2, b: float = 0.75, device: int = 0,
              device_arrays: Optional[dict] = None, tile_items: int = 0):
    """G = X^T X + lam I [cols][cols] of mfx_ease_gram (include/mfx.h): the fixed-point item-kNN similarities off the diagonal,
    fp32(d_i + lam) on it.  A numpy array, or with device_arrays a float32 tensor on the device."""
    csx, space, cols, keep = _ease_matrix(R, weighting, k1, b, device_arrays)
    out, po = _ease_out(space == L.MFX_DEVICE, (cols, cols), device)
    L.check(L.lib().mfx_ease_gram(C.byref(csx), float(lam), int(tile_items), po, space, device))
    return out


def ease_inverse(A, simple: bool = False, device: int = 0):
    """The inverse of one symmetric positive definite matrix, n <= 32768, on the device (mfx_ease_inverse): the blocked
    Cholesky inverse of spd_inverse, by grouped LDS-staged kernels or, simple=True, one wavefront per block -- the same
    bits either way.  numpy in, numpy out; a GPU tensor in, a tensor out."""
    pa, space, n, keep = _ease_square(A, "A")
    out, po = _ease_out(space == L.MFX_DEVICE, (n, n), device)
    L.check(L.lib().mfx_ease_inverse(n, pa, po, L.MFX_EASE_INV_SIMPLE if simple else 0, space, device))
    return out


def ease_weights_from_inverse(P, device: int = 0):
    """B_ij = float32(-P_ij / P_jj) with a zero diagonal (mfx_ease_weights_from_inverse).  numpy or a GPU tensor."""
    pp, space, n, keep = _ease_square(P, "P")
    out, po = _ease_out(space == L.MFX_DEVICE, (n, n), device)
    L.check(L.lib().mfx_ease_weights_from_inverse(n, pp, po, space, device))
    return out


class Ease(_ItemModel):
    """EASE (mfx_ease_*, include/mfx.h): the closed-form dense item-item model B = I - P diag(P)^-1 with a zero diagonal,
    P = (X^T X + lam I)^-1, trained on the GPU -- exact fixed-point Gram matrix, blocked Cholesky inverse, one division per
    weight -- and recommendations as fma chains over the user's own items; every bit fixed by the data.  R: a RatingData,
    its values taken under `weighting` (knn_weights; k1, b: BM25; None: as they are).  lam: the ridge penalty, > 0.
    device_arrays: the matrix as a dict of device tensors (mfx.synth_torch) instead of R; weighting must then be None.
    tile_items: the test hook of mfx_ease_train.  simple_inverse: the one-wavefront-per-block schedule of the inverse."""
    _destroy = "mfx_ease_destroy"

    def __init__(self, R: Optional[RatingData], lam: float, weighting: Optional[str] = None, k1: float = 1.2, b: float = 0.75,
                 device: int = 0, device_arrays: Optional[dict] = None, tile_items: int = 0, simple_inverse: bool = False):
        self._start(device)
        csx, space, self.cols, keep = _ease_matrix(R, weighting, k1, b, device_arrays)
        L.check(L.lib().mfx_ease_train(C.byref(self.handle), C.byref(csx), float(lam), L.MFX_EASE_INV_SIMPLE if simple_inverse else 0,
                                       int(tile_items), space, self.device))

    @classmethod
    def from_weights(cls, B, device: int = 0) -> "Ease":
        """A model from given weights B [cols][cols] (float32, finite, zero diagonal): a numpy array or a GPU tensor."""
        pb, space, n, keep = _ease_square(B, "B")
        self = cls.__new__(cls)
        self._start(device)
        self.cols = n
        L.check(L.lib().mfx_ease_create_from_weights(C.byref(self.handle), n, pb, space, self.device))
        return self

    def weights(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """Rows first .. first + count - 1 of B (count None: to the end) as float32 [count][cols]; row i holds the weights
        from source item i to every target."""
        first = int(first)
        count = self.cols - first if count is None else int(count)
        out = np.empty((max(count, 0), self.cols), np.float32)
        L.check(L.lib().mfx_ease_weights(self.handle, first, count, _vp(out), L.MFX_HOST))
        return out

    def recommend(self, rows, n_top: int, keep_seen: bool = False, on_device: bool = False, tile_items: int = 0):
        """Top-n_top items of the users given by their interactions, as ItemKnn.recommend: the score of j is the fma chain of
        x_i * B[i][j] over the row's items i in stored order; every item not in the row is eligible, whatever its score's
        sign.  The number of bad rows (a value that is not finite) is left in self.bad_rows."""
        return self._recommend(L.lib().mfx_ease_recommend, rows, n_top, keep_seen, on_device, tile_items)

    def times(self) -> dict:
        """Seconds of the training (checks, Gram pass, inverse, weights) and of recommend summed over the calls."""
        out = (C.c_double * 6)()
        L.check(L.lib().mfx_ease_times(self.handle, out))
        return dict(zip(("train_checks", "gram_pass", "inverse", "weights", "recommend_checks", "recommend_pass"), (float(x) for x in out)))


# ---------------------------------------------------------------------------------------------
# single operators (one per reference function on the path)
# ---------------------------------------------------------------------------------------------
def _u32(a):
    assert a.dtype == np.uint32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(L.u32p)


def _f32(a):
    assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(L.f32p)


def rank_one_sweep(ptr, idx, val, vec, lam: float, variant: int = 1, device: int = 0) -> np.ndarray:
    nseg = ptr.shape[0] - 1
    out = np.empty(nseg, np.float32)
    L.check(L.lib().mfx_rank_one_sweep(nseg, idx.shape[0], _u32(ptr), _u32(idx), _f32(val), vec.shape[0], _f32(vec),
                                       lam, _f32(out), variant, device))
    return out


def update_rating(ptr, idx, val, gathered, per_seg, add: bool, variant: int = 1, device: int = 0) -> None:
    """In place on `val`."""
    nseg = ptr.shape[0] - 1
    L.check(L.lib().mfx_update_rating(nseg, idx.shape[0], _u32(ptr), _u32(idx), _f32(val), gathered.shape[0],
                                      _f32(gathered), _f32(per_seg), 1 if add else 0, variant, device))


def test_rmse(T, W, H, rows: int, cols: int, k: int, ifALS: bool, device: int = 0) -> float:
    coo = _coo(T)
    out = C.c_double(0.0)
    L.check(L.lib().mfx_test_rmse(C.byref(coo), _f32(W), _f32(H), rows, cols, k, 1 if ifALS else 0, C.byref(out), device))
    return float(out.value)


test_rmse.__test__ = False  # not a pytest test


def als_gramian(idx, X, k: int, device: int = 0) -> np.ndarray:
    A = np.empty((k, k), np.float32)
    L.check(L.lib().mfx_als_gramian(idx.shape[0], _u32(idx), X.shape[0], _f32(X), k, _f32(A), device))
    return A


def als_half(ptr, idx, val, X, k: int, lam: float, device: int = 0, variant: int = 1) -> np.ndarray:
    """variant 1: MFMA Gramian + Cholesky solve (the product path); 0: as written, bit-identical to src/ALS.cpp."""
    nseg = ptr.shape[0] - 1
    Y = np.empty((nseg, k), np.float32)
    L.check(L.lib().mfx_als_half(nseg, idx.shape[0], _u32(ptr), _u32(idx), _f32(val), X.shape[0], _f32(X), _f32(Y),
                                 k, lam, variant, device))
    return Y


def ials_half(ptr, idx, val, X, k: int, lam: float, alpha: float, device: int = 0, alpha0: Optional[float] = None,
              nu: Optional[float] = None) -> np.ndarray:
    """One implicit-feedback half-sweep (mfx_ials_half): Y [nseg][k] over all rows of X [nrows][k].  alpha0 / nu given:
    mfx_ials_half_reg (see ImplicitAlsSolver)."""
    nseg = ptr.shape[0] - 1
    Y = np.empty((nseg, k), np.float32)
    reg = _reg_pair(alpha0, nu)
    if reg is not None:
        L.check(L.lib().mfx_ials_half_reg(nseg, idx.shape[0], _u32(ptr), _u32(idx), _f32(val), X.shape[0], _f32(X), _f32(Y),
                                          k, lam, alpha, reg[0], reg[1], device))
        return Y
    L.check(L.lib().mfx_ials_half(nseg, idx.shape[0], _u32(ptr), _u32(idx), _f32(val), X.shape[0], _f32(X), _f32(Y),
                                  k, lam, alpha, device))
    return Y


def ials_block_half(ptr, idx, val, X, k: int, lam: float, alpha: float, block: int, Y_in=None, device: int = 0,
                    alpha0: Optional[float] = None, nu: Optional[float] = None) -> np.ndarray:
    """One half-sweep of implicit ALS by block subspace sweeps (mfx_ials_block_half) from Y_in [nseg][k] (None = zeros).
    alpha0 / nu given: mfx_ials_block_half_reg (see ImplicitAlsSolver)."""
    nseg = ptr.shape[0] - 1
    Y = np.empty((nseg, k), np.float32)
    if Y_in is not None:
        _f32c(Y_in, (nseg, k))
    reg = _reg_pair(alpha0, nu)
    if reg is not None:
        L.check(L.lib().mfx_ials_block_half_reg(nseg, idx.shape[0], _u32(ptr), _u32(idx), _f32(val), X.shape[0], _f32(X),
                                                _f32(Y_in) if Y_in is not None else None, _f32(Y), k, int(block), lam, alpha,
                                                reg[0], reg[1], device))
        return Y
    L.check(L.lib().mfx_ials_block_half(nseg, idx.shape[0], _u32(ptr), _u32(idx), _f32(val), X.shape[0], _f32(X),
                                        _f32(Y_in) if Y_in is not None else None, _f32(Y), k, int(block), lam, alpha, device))
    return Y


def ials_cg_half(ptr, idx, val, X, k: int, lam: float, alpha: float, steps: int, tol: float, Y_in=None, return_steps: bool = False,
                 device: int = 0):
    """One half-sweep of implicit ALS by conjugate gradients (mfx_ials_cg_half) from Y_in [nseg][k] (None = cold, from
    zero).  return_steps: also the steps applied to every row, int32 [nseg]."""
    nseg = ptr.shape[0] - 1
    Y = np.empty((nseg, k), np.float32)
    if Y_in is not None:
        _f32c(Y_in, (nseg, k))
    counts = np.zeros(nseg, np.int32) if return_steps else None
    L.check(L.lib().mfx_ials_cg_half(nseg, idx.shape[0], _u32(ptr), _u32(idx), _f32(val), X.shape[0], _f32(X),
                                     _f32(Y_in) if Y_in is not None else None, _f32(Y), k, lam, alpha, int(steps), float(tol),
                                     counts.ctypes.data_as(C.POINTER(C.c_int32)) if return_steps else None, device))
    return (Y, counts) if return_steps else Y


def als_block_half(ptr, idx, val, X, k: int, lam: float, block: int, Y_in=None, count_reg: bool = False, device: int = 0) -> np.ndarray:
    """One half-sweep of explicit ALS by block subspace sweeps (mfx_als_block_half) from Y_in [nseg][k] (None = zeros);
    count_reg: lambda times the entries of the segment on the diagonal instead of lambda."""
    nseg = ptr.shape[0] - 1
    Y = np.empty((nseg, k), np.float32)
    if Y_in is not None:
        _f32c(Y_in, (nseg, k))
    L.check(L.lib().mfx_als_block_half(nseg, idx.shape[0], _u32(ptr), _u32(idx), _f32(val), X.shape[0], _f32(X),
                                       _f32(Y_in) if Y_in is not None else None, _f32(Y), k, int(block), lam, 1 if count_reg else 0, device))
    return Y


def als_inverse(A, device: int = 0) -> np.ndarray:
    """inverseMatrix_CholeskyMethod (src/ALS.cpp:41-64) on one matrix, the reference's operation order."""
    A = np.ascontiguousarray(A, np.float32)
    out = np.empty_like(A)
    L.check(L.lib().mfx_als_inverse(A.shape[0], _f32(A), _f32(out), device))
    return out


def spd_inverse(A, device: int = 0) -> np.ndarray:
    """The inverse of one symmetric positive definite matrix, k <= 1024, on the device (mfx_spd_inverse): blocked Cholesky
    on the fp32 matrix cores, exactly symmetric, the same bits on every call."""
    A = np.ascontiguousarray(A, np.float32)
    out = np.empty_like(A)
    L.check(L.lib().mfx_spd_inverse(A.shape[0], _f32(A), _f32(out), device))
    return out


def partition_rows(R: RatingData, nshards: int) -> np.ndarray:
    bounds = np.zeros(nshards + 1, np.int64)
    L.check(L.lib().mfx_partition_rows(R.rows, _u32(R.csr_row_ptr), nshards, bounds.ctypes.data_as(L.i64p)))
    return bounds


def partition_cols(R: RatingData, nshards: int) -> np.ndarray:
    """nnz-balanced contiguous column blocks (the H-half of a sharded ALS)."""
    bounds = np.zeros(nshards + 1, np.int64)
    L.check(L.lib().mfx_partition_rows(R.cols, _u32(R.csc_col_ptr), nshards, bounds.ctypes.data_as(L.i64p)))
    return bounds


def extract_shard(R: RatingData, row_lo: int, row_hi: int) -> RatingData:
    """Local sub-matrix of rows [row_lo, row_hi): local CSR + local CSC over local row ids; the
    test set is filtered to the same rows (row ids rebased)."""
    lnnz = int(R.csr_row_ptr[row_hi]) - int(R.csr_row_ptr[row_lo])
    nr = row_hi - row_lo
    out = RatingData(nr, R.cols, np.zeros(nr + 1, np.uint32), np.zeros(lnnz, np.uint32), np.zeros(lnnz, np.float32),
                     np.zeros(R.cols + 1, np.uint32), np.zeros(lnnz, np.uint32), np.zeros(lnnz, np.float32))
    csx = _csx(R)
    L.check(L.lib().mfx_extract_shard(C.byref(csx), row_lo, row_hi, _u32(out.csr_row_ptr), _u32(out.csr_col_idx),
                                      _f32(out.csr_val), _u32(out.csc_col_ptr), _u32(out.csc_row_idx), _f32(out.csc_val)))
    keep = (R.test_row >= row_lo) & (R.test_row < row_hi)
    out.test_row = np.ascontiguousarray(R.test_row[keep] - np.uint32(row_lo), dtype=np.uint32)
    out.test_col = np.ascontiguousarray(R.test_col[keep])
    out.test_val = np.ascontiguousarray(R.test_val[keep])
    return out


# ---------------------------------------------------------------------------------------------
# top-N recommendation (mfx_rec_*) and ranking metrics (mfx_topn_metrics)
# ---------------------------------------------------------------------------------------------
PAD_ITEM = 0xFFFFFFFF  # item id of the slots a list could not fill (score -inf)
PAD_RANK = 0xFFFFFFFF  # rank of a pair whose item is not eligible for its user (rank_of)


def _is_dev(a) -> bool:
    return hasattr(a, "data_ptr") and not isinstance(a, np.ndarray)


def _ids_np(a, what: str) -> np.ndarray:
    """`a` as a 1-D int64 array of ids in 0 .. 2^32 - 1, or ValueError."""
    a = np.asarray(a)
    if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
        raise ValueError(f"{what} must be a 1-D array of integer ids")
    if a.dtype == np.uint64 and a.size and a.max() >= 2 ** 32:
        raise ValueError(f"{what} must be below 2^32")
    a = a.astype(np.int64)
    if a.size and (a.min() < 0 or a.max() >= 2 ** 32):
        raise ValueError(f"{what} must be non-negative and below 2^32")
    return a


def _ids_torch(t, what: str):
    """`t` as a 1-D int64 tensor of ids in 0 .. 2^32 - 1 (a 32-bit tensor holds the uint32 bits), or ValueError."""
    import torch
    if t.dim() != 1 or t.dtype.is_floating_point or t.dtype == torch.bool or t.element_size() not in (4, 8):
        raise ValueError(f"{what} must be a 1-D tensor of 32- or 64-bit integer ids")
    if t.element_size() == 4:
        return t.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= 2 ** 32):
        raise ValueError(f"{what} must be non-negative and below 2^32")
    return t


def _is_ids32(a) -> bool:
    """A 1-D array of uint32 ids (tensor: any 32-bit integer type, its bits) that can go to the library as it is."""
    if _is_dev(a):
        return a.dim() == 1 and a.element_size() == 4 and not a.dtype.is_floating_point
    return isinstance(a, np.ndarray) and a.ndim == 1 and a.dtype == np.uint32


def _to_dev32(a, d):
    """Ids (0 .. 2^32 - 1) as a contiguous int32 tensor on device d holding their uint32 bits."""
    import torch
    if not _is_dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint32, copy=False).view(np.int32)).to(d)
    if a.element_size() == 8:
        a = a.to(torch.int32)  # (wraps: the low 32 bits)
    return a.contiguous().view(torch.int32).to(d)


def _candidate_lists(c):
    """(ptr, idx) of the three forms Recommender.query_candidates takes."""
    if hasattr(c, "csr_row_ptr") and hasattr(c, "csr_col_idx"):
        return c.csr_row_ptr, c.csr_col_idx
    if isinstance(c, tuple):
        if len(c) != 2:
            raise ValueError("candidates: a (ptr, idx) tuple has two arrays")
        return c
    if _is_dev(c):
        import torch
        if c.dim() != 2:
            raise ValueError("candidates: a tensor of lists must be 2-D [U, C]")
        U, n = int(c.shape[0]), int(c.shape[1])
        return torch.arange(U + 1, dtype=torch.int64, device=c.device) * n, c.reshape(-1)
    a = np.asarray(c)
    if a.ndim != 2:
        raise ValueError("candidates: an array of lists must be 2-D [U, C]")
    return np.arange(a.shape[0] + 1, dtype=np.int64) * a.shape[1], a.reshape(-1)


def _canonical_lists_np(ptr: np.ndarray, idx: np.ndarray):
    """The CSR lists (int64 ptr from 0, non-decreasing; int64 idx) with every row sorted and without repeats and
    PAD_ITEM entries -> (ptr, idx) int64."""
    n = ptr.size - 1
    idx = idx[:ptr[-1]] if n >= 0 else idx
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
    keep = idx != PAD_ITEM
    key = np.unique(rows[keep] << 32 | idx[keep])
    out = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(key >> 32, minlength=n), out=out[1:])
    return out, key & 0xFFFFFFFF


def _canonical_lists_torch(ptr, idx):
    """_canonical_lists_np on int64 tensors, wherever they live."""
    import torch
    n = int(ptr.numel()) - 1
    idx = idx[:int(ptr[-1])]
    rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=ptr.device), ptr[1:] - ptr[:-1])
    keep = idx != PAD_ITEM
    key = torch.unique(rows[keep] << 32 | idx[keep])
    out = torch.zeros(n + 1, dtype=torch.int64, device=ptr.device)
    if n:
        out[1:] = torch.cumsum(torch.bincount(key >> 32, minlength=n), 0)
    return out, key & 0xFFFFFFFF


_KMEANS_CHUNK = 1 << 24  # distances of one assignment step held at a time (items x lists)


def _kmeans_assign_np(H: np.ndarray, Cn: np.ndarray) -> np.ndarray:
    """The nearest centroid of every row by ||c||^2 - 2 <h, c> in fp32 (||h||^2 is common to a row's candidates);
    argmin takes the first minimum: ties go to the lowest list id."""
    cn = np.einsum("ij,ij->i", Cn, Cn)
    out = np.empty(H.shape[0], np.int64)
    step = max(1, _KMEANS_CHUNK // Cn.shape[0])
    for i0 in range(0, H.shape[0], step):
        out[i0:i0 + step] = np.argmin(cn[None, :] - 2.0 * (H[i0:i0 + step] @ Cn.T), axis=1)
    return out


def _kmeans_np(H: np.ndarray, first: np.ndarray, iters: int):
    nlist = first.size
    Cn = H[first].copy()
    for _ in range(iters):
        a = _kmeans_assign_np(H, Cn)
        order = np.argsort(a, kind="stable")
        counts = np.bincount(a, minlength=nlist)
        full = np.nonzero(counts)[0]
        starts = (np.cumsum(counts) - counts)[full]
        sums = np.add.reduceat(H[order], starts, axis=0, dtype=np.float64)
        Cn[full] = (sums / counts[full, None]).astype(np.float32)  # an empty cluster keeps its centroid
    return _kmeans_assign_np(H, Cn).astype(np.uint32), Cn


def _kmeans_torch(H, first: np.ndarray, iters: int):
    import torch
    nlist = first.size
    Cn = H[torch.from_numpy(first).to(H.device)].clone()
    step = max(1, _KMEANS_CHUNK // nlist)

    def assign():
        cn = (Cn * Cn).sum(1)
        return torch.cat([torch.argmin(cn[None, :] - 2.0 * (H[i0:i0 + step] @ Cn.t()), dim=1) for i0 in range(0, H.shape[0], step)])

    for _ in range(iters):
        a = assign()
        counts = torch.bincount(a, minlength=nlist)
        sums = torch.zeros_like(Cn).index_add_(0, a, H)
        full = counts > 0
        Cn[full] = sums[full] / counts[full, None].to(H.dtype)
    return assign().to(torch.int32), Cn


def ivf_kmeans(H, nlist: int, iters: int = 10, seed: int = 0):
    """A clustering of the items for Recommender.ivf_setup -> (assign uint32 [cols], centroids float32 [nlist, k]).

    H [cols, k] float32: numpy (computed with numpy) or a torch tensor (computed on its device; assign is then an int32
    tensor, the bits of the uint32 ids).  Plain Lloyd iterations on the squared L2 distance: the initial centroids are
    nlist distinct rows chosen by np.random.default_rng(seed).choice(cols, nlist, replace=False); a cluster that empties keeps its centroid and stays empty;
    after the last update one more assignment follows, so the returned assignment belongs to the returned centroids;
    ties go to the lowest list id.  nlist <= cols."""
    if len(tuple(H.shape)) != 2:
        raise ValueError("H must be [cols, k]")
    cols = int(H.shape[0])
    if not 1 <= nlist <= cols:
        raise ValueError(f"nlist must be in [1, cols = {cols}] (got {nlist})")
    if iters < 0:
        raise ValueError("iters must be >= 0")
    first = np.random.default_rng(seed).choice(cols, nlist, replace=False).astype(np.int64)
    if _is_dev(H):
        import torch
        if H.dtype != torch.float32:
            raise ValueError("H must be float32")
        return _kmeans_torch(H.contiguous(), first, iters)
    return _kmeans_np(np.ascontiguousarray(H, dtype=np.float32), first, iters)


class Recommender:
    """Resident top-N recommender over trained factors (mfx_rec_*).

    layout 0: CCD++ factors W [k][rows], H [k][cols]; layout 1: ALS factors W [rows][k], H [cols][k].  W and H are
    numpy float32 arrays, or float32 tensors exposing `data_ptr()` on the GPU (both the same kind).  `exclude`: a
    RatingData whose CSR rows name the items each user is never recommended (e.g. the training ratings)."""

    def __init__(self, W, H, layout: int, exclude: Optional[RatingData] = None, device: int = 0):
        self.handle = C.c_void_p()
        self.device = device
        if layout not in (0, 1):
            raise ValueError("layout must be 0 (CCD++: [k][rows]) or 1 (ALS: [rows][k])")
        dev = _is_dev(W)
        if dev != _is_dev(H):
            raise ValueError("W and H must both be host arrays or both device tensors")
        shW, shH = tuple(W.shape), tuple(H.shape)
        if len(shW) != 2 or len(shH) != 2:
            raise ValueError("W and H must be 2-D")
        if layout == 0:
            (k, rows), (k2, cols) = shW, shH
        else:
            (rows, k), (cols, k2) = shW, shH
        if k != k2:
            raise ValueError(f"W and H disagree on k ({k} vs {k2})")
        self.rows, self.cols, self.k, self.layout = int(rows), int(cols), int(k), layout
        self._keep = []
        self._similar = False  # similar_setup() done
        ex = None
        if dev:
            import torch
            for t in (W, H):
                assert t.dtype == torch.float32 and t.is_contiguous(), "need contiguous float32 tensors"
            pw, ph, space = C.c_void_p(int(W.data_ptr())), C.c_void_p(int(H.data_ptr())), L.MFX_DEVICE
            if exclude is not None:
                rp = torch.from_numpy(exclude.csr_row_ptr.view(np.int32)).to(W.device)
                ci = torch.from_numpy(exclude.csr_col_idx.view(np.int32)).to(W.device)
                self._keep += [rp, ci]
                ex = L.mfx_csx(exclude.rows, exclude.cols, int(exclude.csr_col_idx.shape[0]), None, None, None,
                               C.c_void_p(int(rp.data_ptr())), C.c_void_p(int(ci.data_ptr())) if ci.numel() else None, None)
        else:
            _f32c(W); _f32c(H)
            pw, ph, space = _vp(W), _vp(H), L.MFX_HOST
            if exclude is not None:
                exclude.check_types()
                ex = L.mfx_csx(exclude.rows, exclude.cols, int(exclude.csr_col_idx.shape[0]), None, None, None,
                               _vp(exclude.csr_row_ptr), _vp(exclude.csr_col_idx), None)
        L.check(L.lib().mfx_rec_create(C.byref(self.handle), pw, ph, self.rows, self.cols, self.k, layout,
                                       C.byref(ex) if ex is not None else None, space, device))

    def query(self, n_top: int, users=None, item_slices: int = 0, on_device: bool = False):
        """Top-n_top items of `users` (None: all users in order) -> (items uint32 [U, n_top], scores float32
        [U, n_top]).  Padding slots: item PAD_ITEM, score -inf.  A `users` tensor on the GPU (int32 / uint32 bits) or
        on_device=True keeps everything on the device: the results are then int32 / float32 tensors on it (the items'
        bits are the uint32 ids)."""
        if _is_dev(users) or on_device:
            import torch
            dev = torch.device("cuda", self.device)
            if users is not None:
                assert users.is_contiguous() and users.element_size() == 4, "users: contiguous 32-bit tensor"
                n = int(users.numel())
                pu = C.c_void_p(int(users.data_ptr())) if n else None
            else:
                n, pu = self.rows, None
            items = torch.empty((n, n_top), dtype=torch.int32, device=dev)
            scores = torch.empty((n, n_top), dtype=torch.float32, device=dev)
            if n:
                L.check(L.lib().mfx_rec_query(self.handle, n, pu, n_top, C.c_void_p(int(items.data_ptr())),
                                              C.c_void_p(int(scores.data_ptr())), L.MFX_DEVICE, item_slices))
            return items, scores
        if users is None:
            n, pu, keep = self.rows, None, None
        else:
            keep = np.ascontiguousarray(np.asarray(users), dtype=np.int64)
            if keep.ndim != 1 or (keep.size and (keep.min() < 0 or keep.max() >= 2 ** 32)):
                raise ValueError("users must be a 1-D array of non-negative 32-bit ids")
            keep = keep.astype(np.uint32)
            n, pu = int(keep.size), _vp(keep)
        items = np.empty((n, n_top), np.uint32)
        scores = np.empty((n, n_top), np.float32)
        L.check(L.lib().mfx_rec_query(self.handle, n, pu, n_top, _vp(items), _vp(scores), L.MFX_HOST, item_slices))
        return items, scores

    def fold_in_setup(self, model: int, lam: float, alpha: float = 0.0, alpha0: Optional[float] = None, nu: Optional[float] = None):
        """Prepares fold-in (mfx_rec_fold_in_setup): model MFX_FOLD_ALS / MFX_FOLD_ALS_EXACT / MFX_FOLD_CCD /
        MFX_FOLD_IMPLICIT, regularisation lam, confidence scale alpha (implicit model).  k <= 128.  alpha0 / nu given
        (MFX_FOLD_IMPLICIT only): mfx_rec_fold_in_setup_reg, the objective of ImplicitAlsSolver(alpha0=, nu=)."""
        reg = _reg_pair(alpha0, nu)
        if reg is not None:
            if int(model) != L.MFX_FOLD_IMPLICIT:
                raise ValueError("alpha0 / nu apply to MFX_FOLD_IMPLICIT only")
            L.check(L.lib().mfx_rec_fold_in_setup_reg(self.handle, float(lam), float(alpha), reg[0], reg[1]))
            return
        L.check(L.lib().mfx_rec_fold_in_setup(self.handle, int(model), float(lam), float(alpha)))

    def fold_in_block_setup(self, lam: float, alpha: float, block: int = 0, sweeps: int = 8, tol: float = 0.0):
        """Prepares fold-in by block subspace sweeps (mfx_rec_fold_in_block_setup), the method of ImplicitAlsSolver(block=...):
        any k <= 1024.  block 0 = chosen from k, else 1..128; a row gets at most `sweeps` sweeps (1..1024), exactly `sweeps`
        with tol = 0, else it stops once a sweep moves it by at most tol of its largest entry.  A cold start at large alpha
        converges slowly for short rows: choose sweeps / tol for the data, pass W_init to fold_in, or use fold_in_cg_setup
        (a solve with a residual bound).  The objective of ImplicitAlsSolver(block=, alpha0=, nu=): fold_in_block_setup_reg."""
        L.check(L.lib().mfx_rec_fold_in_block_setup(self.handle, float(lam), float(alpha), int(block), int(sweeps), float(tol)))

    def fold_in_block_setup_reg(self, lam: float, alpha: float, alpha0: float = 1.0, nu: float = 0.0, block: int = 0, sweeps: int = 8,
                                tol: float = 0.0):
        """fold_in_block_setup on the objective of ImplicitAlsSolver(block=, alpha0=, nu=) (mfx_rec_fold_in_block_setup_reg):
        the weight alpha0 > 0 of the unobserved pairs and the exponent 0 <= nu <= 1 of the regulariser
        lam (n + alpha0 cols)^nu of a query row with n entries.  block, sweeps, tol and fold_in afterwards as there (its
        parameter list is pinned by tests/test_foldin_block_host.py: hence a method of its own)."""
        L.check(L.lib().mfx_rec_fold_in_block_setup_reg(self.handle, float(lam), float(alpha), float(alpha0), float(nu), int(block),
                                                        int(sweeps), float(tol)))

    def fold_in_block_setup_als(self, lam: float, block: int = 0, sweeps: int = 8, tol: float = 0.0, count_reg: bool = False):
        """Prepares fold-in by block subspace sweeps on the explicit objective (mfx_rec_fold_in_block_setup_als), the method
        of AlsSolver(block=...): any k <= 1024, the objective of MFX_FOLD_ALS, or with count_reg of MFX_FOLD_CCD.  block,
        sweeps and tol as in fold_in_block_setup.  A sweep is not a solve: with more than one block choose sweeps / tol
        for the data, pass W_init to fold_in, or use fold_in_cg_setup (a solve with a residual bound)."""
        L.check(L.lib().mfx_rec_fold_in_block_setup_als(self.handle, float(lam), 1 if count_reg else 0, int(block), int(sweeps), float(tol)))

    def fold_in_cg_setup(self, model: int, lam: float, alpha: float = 0.0, steps: int = 64, tol: float = 1e-5):
        """Prepares fold-in by preconditioned conjugate gradients (mfx_rec_fold_in_cg_setup): model MFX_FOLD_ALS / MFX_FOLD_CCD /
        MFX_FOLD_IMPLICIT at any k <= 1024.  A row gets at most `steps` steps (1..1024) and stops once its residual is at
        most tol of its right-hand side (2-norms; tol = 0: exactly `steps`); a row of n entries needs at most n + 1 steps
        in exact arithmetic.  The implicit model inverts the k x k base Gramian on the host at setup.  fold_in afterwards
        takes W_init and return_sweeps; the counts are steps."""
        L.check(L.lib().mfx_rec_fold_in_cg_setup(self.handle, int(model), float(lam), float(alpha), int(steps), float(tol)))

    def fold_in(self, rows, n_top: int = 0, on_device: bool = False, W_init=None, return_sweeps: bool = False):
        """Solves one factor row per query user against this handle's H and recommends from it (mfx_rec_fold_in).
        rows: a RatingData-like CSR (csr_row_ptr / csr_col_idx / csr_val) or a (ptr, idx, val) triple of numpy arrays
        or GPU tensors (32-bit ids, float32 values).  Returns (items [U, n_top], scores [U, n_top], W [U, k]), the lists
        with each row's own items excluded (None, None when n_top = 0).  Tensors in, or on_device=True: everything
        stays on the device and the results are tensors (items as int32 holding the uint32 ids).
        After fold_in_block_setup / fold_in_block_setup_als / fold_in_cg_setup only (mfx_rec_fold_in_warm): W_init [U, k], numpy or a GPU
        tensor like the rows, is the start row of every user (None: zeros), and return_sweeps=True appends the int32 sweep
        counts [U] to the result (after fold_in_cg_setup: the step counts)."""
        ptr, idx, val = (rows.csr_row_ptr, rows.csr_col_idx, rows.csr_val) if hasattr(rows, "csr_row_ptr") else rows
        if len(ptr.shape) != 1 or ptr.shape[0] < 1 or idx.shape != val.shape:
            raise ValueError("rows: ptr [U + 1], idx [nnz], val [nnz]")
        n, nnz, n_top = int(ptr.shape[0]) - 1, int(idx.shape[0]), int(n_top)
        warm = W_init is not None or return_sweeps
        if W_init is not None and tuple(W_init.shape) != (n, self.k):
            raise ValueError(f"W_init must be [{n}, {self.k}]")
        if any(_is_dev(a) for a in (ptr, idx, val, W_init)) or on_device:
            import torch
            dev = torch.device("cuda", self.device)

            def put(a, dt):
                if not _is_dev(a):
                    a = np.ascontiguousarray(a, dt)
                    a = torch.from_numpy(a.view(np.int32) if dt == np.uint32 else a).to(dev)
                assert a.is_contiguous() and a.element_size() == 4, "query tensors: contiguous 32-bit"
                return a
            keep = [put(ptr, np.uint32), put(idx, np.uint32), put(val, np.float32)]
            w0 = put(W_init, np.float32) if W_init is not None else None
            W = torch.empty((n, self.k), dtype=torch.float32, device=dev)
            items = torch.empty((n, n_top), dtype=torch.int32, device=dev) if n_top else None
            scores = torch.empty((n, n_top), dtype=torch.float32, device=dev) if n_top else None
            done = torch.zeros((n,), dtype=torch.int32, device=dev) if return_sweeps else None
            p = lambda t: C.c_void_p(int(t.data_ptr())) if t is not None and t.numel() else None
            if warm:
                L.check(L.lib().mfx_rec_fold_in_warm(self.handle, n, nnz, p(keep[0]), p(keep[1]), p(keep[2]), p(w0), p(W),
                                                     p(done), n_top, p(items), p(scores), L.MFX_DEVICE))
            else:
                L.check(L.lib().mfx_rec_fold_in(self.handle, n, nnz, p(keep[0]), p(keep[1]), p(keep[2]), p(W), n_top, p(items),
                                                p(scores), L.MFX_DEVICE))
            return (items, scores, W, done) if return_sweeps else (items, scores, W)
        ptr, idx = np.ascontiguousarray(ptr, np.uint32), np.ascontiguousarray(idx, np.uint32)
        val = np.ascontiguousarray(val, np.float32)
        w0 = np.ascontiguousarray(W_init, np.float32) if W_init is not None else None
        W = np.empty((n, self.k), np.float32)
        items = np.empty((n, n_top), np.uint32) if n_top else None
        scores = np.empty((n, n_top), np.float32) if n_top else None
        done = np.zeros(n, np.int32) if return_sweeps else None
        if warm:
            L.check(L.lib().mfx_rec_fold_in_warm(self.handle, n, nnz, _vp(ptr), _vp(idx), _vp(val), _vp(w0), _vp(W), _vp(done),
                                                 n_top, _vp(items), _vp(scores), L.MFX_HOST))
        else:
            L.check(L.lib().mfx_rec_fold_in(self.handle, n, nnz, _vp(ptr), _vp(idx), _vp(val), _vp(W), n_top, _vp(items),
                                            _vp(scores), L.MFX_HOST))
        return (items, scores, W, done) if return_sweeps else (items, scores, W)

    def set_item_filter(self, keep):
        """Only the items with a non-zero keep[i] are returned by every later query, fold_in and similar_items
        (mfx_rec_set_item_filter).  keep: bool / uint8 numpy array or GPU tensor of length cols (copied), or None to
        remove the filter."""
        if keep is None:
            L.check(L.lib().mfx_rec_set_item_filter(self.handle, None, L.MFX_HOST))
            return
        if tuple(keep.shape) != (self.cols,):
            raise ValueError(f"keep must have one entry per item ({self.cols})")
        if _is_dev(keep):
            assert keep.is_contiguous() and keep.element_size() == 1, "keep: contiguous bool / uint8 tensor"
            L.check(L.lib().mfx_rec_set_item_filter(self.handle, C.c_void_p(int(keep.data_ptr())), L.MFX_DEVICE))
            return
        keep = np.asarray(keep)
        if keep.dtype != np.bool_ and keep.dtype != np.uint8:
            raise ValueError("keep must be bool or uint8")
        keep = np.ascontiguousarray(keep).view(np.uint8)
        L.check(L.lib().mfx_rec_set_item_filter(self.handle, _vp(keep), L.MFX_HOST))

    def similar_setup(self):
        """Prepares item-to-item queries (mfx_rec_similar_setup): one more copy of H on the device, and the item norms."""
        L.check(L.lib().mfx_rec_similar_setup(self.handle))
        self._similar = True

    def item_norms(self):
        """(n2, c) float32 [cols]: the squared norm of every row of H as the score chain gives it, and the 1 / sqrt(n2) that
        the cosine of similar_items multiplies with (0 where n2 is 0 or not finite), bit for bit (mfx_rec_item_norms)."""
        n2, c = np.empty(self.cols, np.float32), np.empty(self.cols, np.float32)
        L.check(L.lib().mfx_rec_item_norms(self.handle, _vp(n2), _vp(c), L.MFX_HOST))
        return n2, c

    def similar_items(self, n_top: int, items=None, metric: int = L.MFX_SIM_COSINE, exclude_self: bool = True,
                      item_slices: int = 0, on_device: bool = False):
        """The n_top items most similar to each of `items` (None: all items in order) by MFX_SIM_COSINE or MFX_SIM_DOT ->
        (items uint32 [Q, n_top], scores float32 [Q, n_top]), padded like query (mfx_rec_similar).  exclude_self: an item
        is not its own neighbour.  The item filter applies, the exclude matrix does not.  An `items` tensor on the GPU
        or on_device=True keeps everything on the device, as in query."""
        if not self._similar:
            self.similar_setup()
        if _is_dev(items) or on_device:
            import torch
            dev = torch.device("cuda", self.device)
            if items is not None:
                if not _is_dev(items):
                    items = torch.from_numpy(np.ascontiguousarray(items, np.uint32).view(np.int32)).to(dev)
                assert items.is_contiguous() and items.element_size() == 4, "items: contiguous 32-bit tensor"
                n = int(items.numel())
                pq = C.c_void_p(int(items.data_ptr())) if n else None
            else:
                n, pq = self.cols, None
            out = torch.empty((n, n_top), dtype=torch.int32, device=dev)
            scores = torch.empty((n, n_top), dtype=torch.float32, device=dev)
            if n:
                L.check(L.lib().mfx_rec_similar(self.handle, n, pq, int(metric), int(bool(exclude_self)), n_top,
                                                C.c_void_p(int(out.data_ptr())), C.c_void_p(int(scores.data_ptr())), L.MFX_DEVICE,
                                                item_slices))
            return out, scores
        if items is None:
            n, pq, keep = self.cols, None, None
        else:
            keep = np.ascontiguousarray(np.asarray(items), dtype=np.int64)
            if keep.ndim != 1 or (keep.size and (keep.min() < 0 or keep.max() >= 2 ** 32)):
                raise ValueError("items must be a 1-D array of non-negative 32-bit ids")
            keep = keep.astype(np.uint32)
            n, pq = int(keep.size), _vp(keep)
        out = np.empty((n, n_top), np.uint32)
        scores = np.empty((n, n_top), np.float32)
        L.check(L.lib().mfx_rec_similar(self.handle, n, pq, int(metric), int(bool(exclude_self)), n_top, _vp(out), _vp(scores),
                                        L.MFX_HOST, item_slices))
        return out, scores

    def rank_of(self, users, items, item_slices: int = 0, on_device: bool = False):
        """Exact catalogue rank of each pair (users[p], items[p]) -> (ranks, scores float32, n_eligible), each [P]
        (mfx_rec_rank).  ranks[p] is the position at which query returns the item for the user -- the number of eligible
        items ordered before it -- or PAD_RANK when the item is excluded, filtered out or has a NaN key; scores[p] is the
        score chain of the pair either way; n_eligible[p] counts the items eligible for the user.  numpy in: uint32
        ranks and counts.  GPU tensors in (32-bit ids) or on_device=True: everything stays on the device and they are
        int32 tensors holding the uint32 bits, as in query."""
        if _is_dev(users) or _is_dev(items) or on_device:
            import torch
            dev = torch.device("cuda", self.device)

            def put(a):
                if not _is_dev(a):
                    a = torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(dev)
                assert a.dim() == 1 and a.is_contiguous() and a.element_size() == 4, "pairs: contiguous 1-D 32-bit tensors"
                return a
            tu, ti = put(users), put(items)
            if tu.numel() != ti.numel():
                raise ValueError("users and items must have one entry per pair")
            n = int(tu.numel())
            ranks = torch.empty((n,), dtype=torch.int32, device=dev)
            scores = torch.empty((n,), dtype=torch.float32, device=dev)
            nel = torch.empty((n,), dtype=torch.int32, device=dev)
            if n:
                p = lambda t: C.c_void_p(int(t.data_ptr()))
                L.check(L.lib().mfx_rec_rank(self.handle, n, p(tu), p(ti), p(ranks), p(scores), p(nel), L.MFX_DEVICE, item_slices))
            return ranks, scores, nel
        pu, pi = (np.ascontiguousarray(np.asarray(a), dtype=np.int64) for a in (users, items))
        for a in (pu, pi):
            if a.ndim != 1 or (a.size and (a.min() < 0 or a.max() >= 2 ** 32)):
                raise ValueError("users and items must be 1-D arrays of non-negative 32-bit ids")
        if pu.shape != pi.shape:
            raise ValueError("users and items must have one entry per pair")
        pu, pi = pu.astype(np.uint32), pi.astype(np.uint32)
        n = int(pu.size)
        ranks, scores, nel = np.empty(n, np.uint32), np.empty(n, np.float32), np.empty(n, np.uint32)
        L.check(L.lib().mfx_rec_rank(self.handle, n, _vp(pu), _vp(pi), _vp(ranks), _vp(scores), _vp(nel), L.MFX_HOST, item_slices))
        return ranks, scores, nel

    def rank_times(self) -> dict:
        """Device seconds of the last rank_of / evaluate by phase (mfx_rec_rank_times): {"keys", "count", "exclude"}."""
        out = (C.c_double * 3)()
        L.check(L.lib().mfx_rec_rank_times(self.handle, out))
        return {"keys": out[0], "count": out[1], "exclude": out[2]}

    def query_candidates(self, n_top: int, candidates, users=None, apply_exclude: bool = True, canonical: bool = False,
                         on_device: bool = False, return_counts: bool = False):
        """The n_top best eligible items of each user's own candidate list -> (items [U, n_top], scores [U, n_top][,
        counts [U]]), ordered and padded like query (mfx_rec_query_candidates): the second stage after a retrieval step.
        Slot q is users[q] (None: user q) with the q-th list.  `candidates`: a (ptr, idx) pair of CSR arrays, an object
        with csr_row_ptr / csr_col_idx, or a 2-D [U, C] id array of equal-length lists as an ANN index returns them.
        canonical=False: every list is sorted and loses its repeats and its PAD_ITEM entries first (numpy on the host,
        torch on the device when tensors are given); canonical=True: the lists go to the library as they are, which
        refuses ids that are not strictly ascending within a list.  An item is eligible as in rank_of: not in the user's
        exclusion row (apply_exclude=False: the exclusion plays no part), kept by the item filter, its key not NaN;
        counts is the number of eligible candidates per slot.  numpy in: uint32 items and counts; GPU tensors in or
        on_device=True: int32 tensors holding the uint32 bits, as in query.
        Measured at 480 189 x 17 770, k = 64, N = 10: for all users at once the full-catalogue query (24.6 ms) is
        the faster call from a list length between 300 (9.8 ms) and 1 000 (28.0 ms) on, about 5 % of the catalogue; for a
        batch of 1 024 users this call stays faster up to the whole catalogue as the list (0.98 against 1.36 ms).  The
        choice between the two is the caller's."""
        if not 1 <= int(n_top) <= 1024:
            raise ValueError("n_top must be in 1 .. 1024")
        ptr, idx, users, n = self._candidate_batch(candidates, users, canonical)
        dev = on_device or any(_is_dev(a) for a in (ptr, idx, users))
        flags = 0 if apply_exclude else L.MFX_CAND_NO_EXCLUDE
        fn = L.lib().mfx_rec_query_candidates
        if dev:
            import torch
            d = torch.device("cuda", self.device)
            tp, ti, tu = (None if a is None else _to_dev32(a, d) for a in (ptr, idx, users))
            items = torch.empty((n, n_top), dtype=torch.int32, device=d)
            scores = torch.empty((n, n_top), dtype=torch.float32, device=d)
            counts = torch.empty((n,), dtype=torch.int32, device=d)
            if n:
                p = lambda t: C.c_void_p(int(t.data_ptr())) if t is not None and t.numel() else None
                L.check(fn(self.handle, n, p(tu), p(tp), p(ti), flags, n_top, p(items), p(scores), p(counts), L.MFX_DEVICE))
        else:
            pp, pi = (np.ascontiguousarray(a).astype(np.uint32, copy=False) for a in (ptr, idx))
            pu = None if users is None else np.ascontiguousarray(users).astype(np.uint32, copy=False)
            items, scores, counts = np.empty((n, n_top), np.uint32), np.empty((n, n_top), np.float32), np.empty(n, np.uint32)
            L.check(fn(self.handle, n, _vp(pu), _vp(pp), _vp(pi) if pi.size else None, flags, n_top, _vp(items), _vp(scores),
                       _vp(counts), L.MFX_HOST))
        return (items, scores, counts) if return_counts else (items, scores)

    def _candidate_batch(self, candidates, users, canonical: bool, own_vectors: int = -1):
        """The lists of query_candidates / diversify as the library takes them -> (ptr, idx, users, number of slots):
        int64 (or, canonical, the caller's 32-bit) arrays or tensors, each list sorted and without repeats and PAD_ITEM
        entries unless canonical.  own_vectors >= 0: the slots bring that many query vectors instead of users."""
        ptr, idx = _candidate_lists(candidates)
        if _is_dev(ptr) != _is_dev(idx):
            raise ValueError("the candidate arrays must both be host arrays or both tensors")
        wide = _ids_torch if _is_dev(ptr) else _ids_np
        ptr = wide(ptr, "candidate row pointers")
        if not (canonical and _is_ids32(idx)):  # (canonical 32-bit ids are not copied here)
            idx = wide(idx, "candidate ids")
        n = int(ptr.shape[0]) - 1
        if n < 0:
            raise ValueError("candidate row pointers must have one entry per list and one more")
        if own_vectors >= 0:
            if own_vectors != n:
                raise ValueError(f"{own_vectors} query vectors but {n} candidate lists")
        elif users is None:
            if n > self.rows:
                raise ValueError(f"{n} candidate lists but the model has {self.rows} users: pass `users`")
        else:
            if not _is_ids32(users):
                users = _ids_torch(users, "users") if _is_dev(users) else _ids_np(users, "users")
            if int(users.shape[0]) != n:
                raise ValueError(f"{int(users.shape[0])} users but {n} candidate lists")
        if n and int(ptr[-1]) > int(idx.shape[0]):
            raise ValueError("the candidate row pointers end past the candidate ids")
        if not canonical:
            if n and (int(ptr[0]) != 0 or bool((ptr[1:] < ptr[:-1]).any())):
                raise ValueError("candidate row pointers must start at 0 and be non-decreasing")
            ptr, idx = (_canonical_lists_torch if _is_dev(ptr) else _canonical_lists_np)(ptr, idx)
        return ptr, idx, users, n

    def diversify(self, n_top: int, candidates, users=None, vectors=None, tradeoff: float = 0.5, metric: int = L.MFX_SIM_COSINE,
                  apply_exclude: bool = True, canonical: bool = False, on_device: bool = False, return_values: bool = False,
                  return_counts: bool = False, form: int = 0):
        """Diversity re-ranking of each slot's candidate list by greedy maximal marginal relevance -> (items [U, n_top],
        scores [U, n_top][, values [U, n_top]][, counts [U]]) in pick order (mfx_rec_diversify; the rule, bit for bit, is
        in include/mfx.h).  Step by step the pick is the eligible candidate with the greatest
        tradeoff * score - (1 - tradeoff) * (its greatest similarity to the items picked so far, at least 0); ties go to
        the greater score, then to the smaller id.  tradeoff = 1 is query_candidates; 0 looks at the scores only to break
        ties.  metric: MFX_SIM_COSINE or MFX_SIM_DOT between rows of H, as similar_items computes them.
        `candidates`, `users`, `canonical`, `apply_exclude` and the device forms as in query_candidates; a list holds at
        most 2048 candidates after canonicalisation, n_top is at most 128.  `vectors` float32 [U, k] (numpy or GPU tensor):
        the slots' own query vectors instead of users -- the W of fold_in, a session vector; they have no exclusion rows,
        so apply_exclude must be False with them.  values: what the pick maximised at each step; counts: the eligible
        candidates per slot.  form: 0, or 1 / 2 to force one form of the selection kernel (a test hook, the same bits)."""
        if not 1 <= int(n_top) <= 128:
            raise ValueError("n_top must be in 1 .. 128")
        tradeoff = float(tradeoff)
        if not 0.0 <= tradeoff <= 1.0:  # (NaN fails both)
            raise ValueError("tradeoff must be in 0 .. 1")
        if int(metric) not in (L.MFX_SIM_DOT, L.MFX_SIM_COSINE):
            raise ValueError("metric must be MFX_SIM_DOT or MFX_SIM_COSINE")
        if int(form) not in (0, 1, 2):
            raise ValueError("form must be 0, 1 or 2")
        nvec = -1
        if vectors is not None:
            if users is not None:
                raise ValueError("pass users or vectors, not both")
            if apply_exclude:
                raise ValueError("vectors have no exclusion rows: pass apply_exclude=False")
            if not _is_dev(vectors):
                vectors = np.ascontiguousarray(vectors, np.float32)
            if len(vectors.shape) != 2 or int(vectors.shape[1]) != self.k:
                raise ValueError(f"vectors must be [U, {self.k}]")
            nvec = int(vectors.shape[0])
        ptr, idx, users, n = self._candidate_batch(candidates, users, canonical, nvec)
        dev = on_device or any(_is_dev(a) for a in (ptr, idx, users, vectors))
        flags = 0 if apply_exclude else L.MFX_DIV_NO_EXCLUDE
        fn = L.lib().mfx_rec_diversify
        if dev:
            import torch
            d = torch.device("cuda", self.device)
            tp, ti, tu = (None if a is None else _to_dev32(a, d) for a in (ptr, idx, users))
            tv = None
            if vectors is not None:
                tv = (vectors if _is_dev(vectors) else torch.from_numpy(vectors)).to(d, torch.float32).contiguous()
            items = torch.empty((n, n_top), dtype=torch.int32, device=d)
            scores = torch.empty((n, n_top), dtype=torch.float32, device=d)
            values = torch.empty((n, n_top), dtype=torch.float32, device=d)
            counts = torch.empty((n,), dtype=torch.int32, device=d)
            if n:
                p = lambda t: C.c_void_p(int(t.data_ptr())) if t is not None and t.numel() else None
                L.check(fn(self.handle, n, p(tu), p(tv), p(tp), p(ti), flags, int(metric), tradeoff, n_top, p(items), p(scores),
                           p(values), p(counts), L.MFX_DEVICE, int(form)))
        else:
            pp, pi = (np.ascontiguousarray(a).astype(np.uint32, copy=False) for a in (ptr, idx))
            pu = None if users is None else np.ascontiguousarray(users).astype(np.uint32, copy=False)
            pv = vectors
            items, scores, values = np.empty((n, n_top), np.uint32), np.empty((n, n_top), np.float32), np.empty((n, n_top), np.float32)
            counts = np.empty(n, np.uint32)
            L.check(fn(self.handle, n, _vp(pu), _vp(pv), _vp(pp), _vp(pi) if pi.size else None, flags, int(metric), tradeoff, n_top,
                       _vp(items), _vp(scores), _vp(values), _vp(counts), L.MFX_HOST, int(form)))
        out = (items, scores)
        if return_values:
            out += (values,)
        if return_counts:
            out += (counts,)
        return out

    def diversify_times(self) -> dict:
        """Stream seconds of the last diversify by phase (mfx_rec_diversify_times): {"check": copies in, validity checks,
        similar_setup when it runs; "relevance": the kernel that scores the lists; "select": the kernel of the greedy steps}."""
        out = (C.c_double * 3)()
        L.check(L.lib().mfx_rec_diversify_times(self.handle, out))
        return {"check": out[0], "relevance": out[1], "select": out[2]}

    def query_diverse(self, n_top: int, pool: int, users=None, tradeoff: float = 0.5, metric: int = L.MFX_SIM_COSINE,
                      on_device: bool = False):
        """The one-call form: query(pool) for `users`, then diversify(n_top) over each user's pool -> (items [U, n_top],
        scores [U, n_top]) in pick order.  n_top <= pool <= 1024.  The pool is the exact top-`pool` of the catalogue under the
        exclusion rows and the item filter, so nothing is left for the second step to exclude."""
        if not 1 <= int(n_top) <= 128:
            raise ValueError("n_top must be in 1 .. 128")
        if not int(n_top) <= int(pool) <= 1024:
            raise ValueError("pool must be in n_top .. 1024")
        if on_device and users is not None and not _is_dev(users):
            import torch
            users = _to_dev32(_ids_np(users, "users"), torch.device("cuda", self.device))
        items, _ = self.query(int(pool), users, on_device=on_device)
        if _is_dev(items):
            import torch
            ids = torch.sort(items.to(torch.int64) & 0xFFFFFFFF, dim=1).values  # (the padding sorts last)
            lens = (ids != PAD_ITEM).sum(1)
            ptr = torch.zeros(ids.shape[0] + 1, dtype=torch.int64, device=ids.device)
            ptr[1:] = torch.cumsum(lens, 0)
            idx = ids[ids != PAD_ITEM].to(torch.int32)
        else:
            ids = np.sort(items, axis=1)
            ptr = np.zeros(ids.shape[0] + 1, np.int64)
            np.cumsum((ids != PAD_ITEM).sum(1), out=ptr[1:])
            idx = ids[ids != PAD_ITEM]
        return self.diversify(n_top, (ptr, idx), users=users, tradeoff=tradeoff, metric=metric, canonical=True, on_device=on_device)

    def score(self, users, items, on_device: bool = False):
        """The model's score of each pair (users[p], items[p]) -> float32 [P] (mfx_rec_score): the score chain of
        query, bit for bit, whether the item is eligible for the user or not -- the scores of rank_of without its
        counting pass.  GPU tensors in (32-bit ids) or on_device=True: a float32 tensor on the device."""
        if _is_dev(users) or _is_dev(items) or on_device:
            import torch
            d = torch.device("cuda", self.device)
            tu, ti = (_to_dev32(_ids_torch(a, "pairs") if _is_dev(a) else _ids_np(a, "pairs"), d) for a in (users, items))
            if tu.numel() != ti.numel():
                raise ValueError("users and items must have one entry per pair")
            n = int(tu.numel())
            scores = torch.empty((n,), dtype=torch.float32, device=d)
            if n:
                p = lambda t: C.c_void_p(int(t.data_ptr()))
                L.check(L.lib().mfx_rec_score(self.handle, n, p(tu), p(ti), p(scores), L.MFX_DEVICE))
            return scores
        pu, pi = _ids_np(users, "users"), _ids_np(items, "items")
        if pu.shape != pi.shape:
            raise ValueError("users and items must have one entry per pair")
        pu, pi = pu.astype(np.uint32), pi.astype(np.uint32)
        n = int(pu.size)
        scores = np.empty(n, np.float32)
        L.check(L.lib().mfx_rec_score(self.handle, n, _vp(pu), _vp(pi), _vp(scores), L.MFX_HOST))
        return scores

    def candidates_times(self) -> dict:
        """Stream seconds of the last query_candidates by phase (mfx_rec_candidates_times): {"check": copies in, validity
        checks, the piece table; "score": the kernel that scores and selects within every piece; "select": the merge of
        lists longer than 2048 candidates}.  After score(): {"check": staging, "score": the kernel, "select": 0}."""
        out = (C.c_double * 3)()
        L.check(L.lib().mfx_rec_candidates_times(self.handle, out))
        return {"check": out[0], "score": out[1], "select": out[2]}

    def ivf_setup(self, assign, centroids):
        """Builds the IVF index from a clustering of the items (mfx_rec_ivf_setup): assign [cols] the list of every item
        (uint32 numpy array, or a 32-bit integer GPU tensor holding those bits), centroids float32 [nlist, k], both host
        arrays or both GPU tensors.  Any assignment will do (ivf_kmeans makes one); a second call replaces the index.
        One more copy of H on the device."""
        dev = _is_dev(assign)
        if dev != _is_dev(centroids):
            raise ValueError("assign and centroids must both be host arrays or both device tensors")
        if len(tuple(centroids.shape)) != 2 or int(centroids.shape[1]) != self.k:
            raise ValueError(f"centroids must be [nlist, {self.k}]")
        if tuple(assign.shape) != (self.cols,):
            raise ValueError(f"assign must have one entry per item ({self.cols})")
        nlist = int(centroids.shape[0])
        if dev:
            import torch
            assert centroids.dtype == torch.float32 and centroids.is_contiguous(), "centroids: contiguous float32 tensor"
            assert assign.is_contiguous() and assign.element_size() == 4 and not assign.dtype.is_floating_point, \
                "assign: contiguous 32-bit integer tensor"
            torch.cuda.synchronize(assign.device)  # (the library reads on its own stream: what torch has queued on them comes first)
            L.check(L.lib().mfx_rec_ivf_setup(self.handle, nlist, C.c_void_p(int(assign.data_ptr())),
                                              C.c_void_p(int(centroids.data_ptr())), L.MFX_DEVICE))
        else:
            a = _ids_np(assign, "assign").astype(np.uint32)
            c = np.ascontiguousarray(centroids, dtype=np.float32)
            L.check(L.lib().mfx_rec_ivf_setup(self.handle, nlist, _vp(a), _vp(c), L.MFX_HOST))
        self._nlist = nlist

    def ivf_build(self, H, nlist: int, iters: int = 10, seed: int = 0):
        """ivf_kmeans(H, nlist, iters, seed) followed by ivf_setup -> (assign, centroids).  H as the constructor took it
        ([k, cols] for layout 0, which is transposed here)."""
        if self.layout == 0:
            H = H.t().contiguous() if _is_dev(H) else np.ascontiguousarray(np.asarray(H).T)
        assign, centroids = ivf_kmeans(H, nlist, iters, seed)
        self.ivf_setup(assign, centroids)
        return assign, centroids

    def ivf_lists(self):
        """The lists of the index as built (mfx_rec_ivf_lists) -> (list_ptr uint32 [nlist + 1], list_idx uint32 [cols]):
        list l is list_idx[list_ptr[l]:list_ptr[l + 1]], item ids ascending."""
        ptr = np.empty(getattr(self, "_nlist", 0) + 1, np.uint32)
        idx = np.empty(self.cols, np.uint32)
        L.check(L.lib().mfx_rec_ivf_lists(self.handle, _vp(ptr), _vp(idx), L.MFX_HOST))
        return ptr, idx

    def _ivf_batch(self, width: int, users, on_device: bool, call):
        """(ids [U, width], scores [U, width]) of call(n, users pointer, ids pointer, scores pointer, space), the batch
        taken as query takes it."""
        if _is_dev(users) or on_device:
            import torch
            dev = torch.device("cuda", self.device)
            if users is not None:
                assert users.is_contiguous() and users.element_size() == 4, "users: contiguous 32-bit tensor"
                n = int(users.numel())
                pu = C.c_void_p(int(users.data_ptr())) if n else None
            else:
                n, pu = self.rows, None
            ids = torch.empty((n, width), dtype=torch.int32, device=dev)
            scores = torch.empty((n, width), dtype=torch.float32, device=dev)
            if n:
                L.check(call(n, pu, C.c_void_p(int(ids.data_ptr())), C.c_void_p(int(scores.data_ptr())), L.MFX_DEVICE))
            return ids, scores
        if users is None:
            n, pu, keep = self.rows, None, None
        else:
            keep = _ids_np(users, "users").astype(np.uint32)
            n, pu = int(keep.size), _vp(keep)
        ids = np.empty((n, width), np.uint32)
        scores = np.empty((n, width), np.float32)
        L.check(call(n, pu, _vp(ids), _vp(scores), L.MFX_HOST))
        return ids, scores

    def ivf_probe(self, nprobe: int, users=None, on_device: bool = False):
        """The nprobe lists each of `users` (None: all users in order) probes, best first -> (lists uint32 [U, nprobe],
        scores float32 [U, nprobe]) (mfx_rec_ivf_probe): the score of a list is the score chain against its centroid;
        slots left over (fewer than nprobe lists with a score that is not NaN) hold PAD_ITEM / -inf.  Device in or
        on_device=True: int32 / float32 tensors, as in query."""
        fn = L.lib().mfx_rec_ivf_probe
        return self._ivf_batch(nprobe, users, on_device, lambda n, pu, pi, ps, sp: fn(self.handle, n, pu, nprobe, pi, ps, sp))

    def query_ivf(self, n_top: int, nprobe: int, users=None, on_device: bool = False):
        """Top-n_top items of `users` over the items of the nprobe lists each of them probes -> (items [U, n_top], scores
        [U, n_top]) (mfx_rec_query_ivf): exactly query_candidates on the union of the probed lists, so exclusion rows,
        item filter, order, padding and score bits are query's, and nprobe = nlist is query itself.
        1 <= nprobe <= min(nlist, 1024), nprobe * n_top <= 8192.  Device in or on_device=True as in query."""
        fn = L.lib().mfx_rec_query_ivf
        return self._ivf_batch(n_top, users, on_device, lambda n, pu, pi, ps, sp: fn(self.handle, n, pu, nprobe, n_top, pi, ps, sp))

    def ivf_times(self) -> dict:
        """Stream seconds of the last query_ivf by phase (mfx_rec_ivf_times): {"probe", "build" (the work items), "pass"
        (the list pass), "merge"}."""
        out = (C.c_double * 4)()
        L.check(L.lib().mfx_rec_ivf_times(self.handle, out))
        return {"probe": out[0], "build": out[1], "pass": out[2], "merge": out[3]}

    def evaluate(self, T, cutoffs=(10,), min_rating: float = float("-inf")) -> dict:
        """Ranking metrics of this model on the held-out set T (TestData or RatingData) from exact ranks
        (mfx_rec_evaluate): {"cutoffs", "hr", "precision", "recall", "ndcg" (a list with one value per cutoff each), "mrr",
        "auc", "users", "auc_users"}.  Cutoffs are not limited to 1024.  Only test entries with value >= min_rating count;
        users left with none are skipped, as in topn_metrics."""
        if not isinstance(T, TestData):
            T = test_data_of(T)
        cuts = [int(c) for c in cutoffs]
        if any(c < 1 or c >= 2 ** 31 for c in cuts):
            raise ValueError("cutoffs must be >= 1")
        coo = _coo(T)
        n = len(cuts)
        ca = np.asarray(cuts, np.int32)
        out = (C.c_double * (4 * max(n, 1)))()
        mrr, auc = C.c_double(0), C.c_double(0)
        kept, auc_kept = C.c_int64(0), C.c_int64(0)
        L.check(L.lib().mfx_rec_evaluate(self.handle, C.byref(coo), float(min_rating), n, _vp(ca), out, C.byref(mrr), C.byref(auc),
                                         C.byref(kept), C.byref(auc_kept), L.MFX_HOST))
        col = lambda j: [out[4 * c + j] for c in range(n)]
        return {"cutoffs": cuts, "hr": col(0), "precision": col(1), "recall": col(2), "ndcg": col(3), "mrr": mrr.value,
                "auc": auc.value, "users": int(kept.value), "auc_users": int(auc_kept.value)}

    def explain(self, rows, targets, n_expl: int = 10, on_device: bool = False, return_W: bool = False, return_Z: bool = False,
                max_ws_bytes: int = 1 << 30) -> dict:
        """Why the target items score what they score for fold-in users (mfx_rec_explain): the score of target t for the row
        q splits over the row's own entries, <h_t, w_q> = sum_e b_e <h_e, A_q^-1 h_t>.  After fold_in_setup with MFX_FOLD_ALS,
        MFX_FOLD_CCD or MFX_FOLD_IMPLICIT (alpha0= / nu= included); the explanation is of the fold-in row of the given
        interactions, not of a row of this handle's W.
        rows: as for fold_in.  targets [U, T], 1 <= T <= 64: item ids, 0xFFFFFFFF (or -1 in a signed array or tensor) = padding, so
        the items of fold_in(rows, n_top) can be passed as they are.  Returns {"items" [U, T, n_expl]: the row's entries
        (r > 0 only under the implicit models) by contribution descending, then position in the row, padded with 0xFFFFFFFF;
        "contrib" [U, T, n_expl] float32, padded with -inf; "totals" [U, T]: the score fold_in reports for the target, -inf
        for padding; "W" [U, k] with return_W, "Z" [U, T, k] = A^-1 h_target with return_Z}.  Tensors in, or on_device=True:
        tensors out (items as int32 holding the uint32 ids).  The batch is cut into consecutive pieces whose Z workspace
        (4 k T bytes per user) stays under max_ws_bytes; a row's result does not depend on the cut."""
        return self._explain(False, rows, targets, n_expl, on_device, return_W, return_Z, False, max_ws_bytes)

    def explain_cg(self, rows, targets, n_expl: int = 10, on_device: bool = False, return_W: bool = False, return_Z: bool = False,
                   return_steps: bool = False, max_ws_bytes: int = 1 << 30) -> dict:
        """explain() at any k <= 1024, after fold_in_cg_setup (mfx_rec_explain_cg): the row is fold_in's under that setup and
        Z[q][t] is the conjugate-gradient iterate of A_q z = h_t from zero, with the setup's steps and tol and the stop rule
        |r| <= tol |h_t|, so the contributions sum to the total up to about tol (|b| |z| + |h_t| |w|) (include/mfx.h).
        Arguments and the returned dict are those of explain(); return_steps adds "row_steps" [U] (fold_in's step counts) and
        "target_steps" [U, T] (0 for a padding target, a row without counting entries and a zero target row), int32.
        The batch is cut into consecutive pieces whose device workspace (Z, residual, direction, A p and, under the implicit
        model, the preconditioned residual: up to 20 k T bytes per user, plus the row solve's 16 k) stays under max_ws_bytes;
        a row's result does not depend on the cut."""
        return self._explain(True, rows, targets, n_expl, on_device, return_W, return_Z, return_steps, max_ws_bytes)

    def _explain(self, cg: bool, rows, targets, n_expl, on_device, return_W, return_Z, return_steps, max_ws_bytes) -> dict:
        ptr, idx, val = (rows.csr_row_ptr, rows.csr_col_idx, rows.csr_val) if hasattr(rows, "csr_row_ptr") else rows
        if len(ptr.shape) != 1 or ptr.shape[0] < 1 or idx.shape != val.shape:
            raise ValueError("rows: ptr [U + 1], idx [nnz], val [nnz]")
        n, n_expl = int(ptr.shape[0]) - 1, int(n_expl)
        if len(targets.shape) != 2 or int(targets.shape[0]) != n:
            raise ValueError(f"targets must be [{n}, T]")
        nt, k = int(targets.shape[1]), self.k
        dev_in = any(_is_dev(a) for a in (ptr, idx, val, targets)) or on_device
        per_user = 4 * k * (5 * nt + 4) if cg else 4 * k * nt  # cg: the five arrays per pair, four per row of the row solve
        step = max(1, int(max_ws_bytes) // max(1, per_user))
        if dev_in:
            import torch
            dev = torch.device("cuda", self.device)

            def put(a, dt):
                if not _is_dev(a):
                    a = np.ascontiguousarray(a, dt)
                    a = torch.from_numpy(a.view(np.int32) if dt == np.uint32 else a)
                a = a.to(dev).contiguous()
                assert a.element_size() == 4, "query tensors: 32-bit"
                return a
            ptr, idx, val, targets = put(ptr, np.uint32), put(idx, np.uint32), put(val, np.float32), put(targets, np.uint32)
            new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
            out = {"items": new((n, nt, n_expl), torch.int32), "contrib": new((n, nt, n_expl), torch.float32),
                   "totals": new((n, nt), torch.float32)}
            if return_W:
                out["W"] = new((n, k), torch.float32)
            if return_Z:
                out["Z"] = new((n, nt, k), torch.float32)
            if return_steps:
                out["row_steps"], out["target_steps"] = new((n,), torch.int32), new((n, nt), torch.int32)
            hp = (ptr.cpu().numpy().view(np.uint32).astype(np.int64)) if n > step else None
            p = lambda t: C.c_void_p(int(t.data_ptr())) if t is not None and t.numel() else None
            space = L.MFX_DEVICE
        else:
            ptr, idx = np.ascontiguousarray(ptr, np.uint32), np.ascontiguousarray(idx, np.uint32)
            val, targets = np.ascontiguousarray(val, np.float32), np.asarray(targets)
            if targets.dtype == np.int32:  # (the uint32 bits, as in an int32 tensor: -1 is the padding)
                targets = np.ascontiguousarray(targets).view(np.uint32)
            elif targets.dtype != np.uint32:
                t64 = targets.astype(np.int64)
                if targets.dtype.kind not in "iu" or (t64.size and (t64.min() < -1 or t64.max() > 0xFFFFFFFF)):
                    raise ValueError("targets: integer item ids, 0xFFFFFFFF or -1 for padding")
                targets = (t64 & 0xFFFFFFFF).astype(np.uint32)
            targets = np.ascontiguousarray(targets)
            out = {"items": np.empty((n, nt, n_expl), np.uint32), "contrib": np.empty((n, nt, n_expl), np.float32),
                   "totals": np.empty((n, nt), np.float32)}
            if return_W:
                out["W"] = np.empty((n, k), np.float32)
            if return_Z:
                out["Z"] = np.empty((n, nt, k), np.float32)
            if return_steps:
                out["row_steps"], out["target_steps"] = np.empty(n, np.int32), np.empty((n, nt), np.int32)
            hp = ptr.astype(np.int64)
            p = lambda a: _vp(a) if a is not None and a.size else None
            space = L.MFX_HOST
        for u0 in range(0, max(n, 1), step):
            u1 = min(n, u0 + step)
            if u0 == 0 and u1 == n:
                pp, lo, hi = ptr, 0, int(idx.shape[0])
            else:
                lo, hi = int(hp[u0]), int(hp[u1])
                pp = ptr[u0:u1 + 1] - ptr[u0]
                pp = pp.contiguous() if dev_in else np.ascontiguousarray(pp)
            cut = lambda key: out[key][u0:u1] if key in out else None
            args = (self.handle, u1 - u0, hi - lo, p(pp), p(idx[lo:hi]), p(val[lo:hi]), nt, p(targets[u0:u1]), n_expl,
                    p(cut("items")), p(cut("contrib")), p(cut("totals")), p(cut("W")), p(cut("Z")))
            if cg:
                L.check(L.lib().mfx_rec_explain_cg(*args, p(cut("row_steps")), p(cut("target_steps")), space))
            else:
                L.check(L.lib().mfx_rec_explain(*args, space))
        return out

    def explain_times(self) -> dict:
        """Seconds of the last mfx_rec_explain / mfx_rec_explain_cg call by phase (mfx_rec_explain_times): {"build": host build and checks,
        "solve": the rows and the further right-hand sides, "contrib": totals, contributions and selection}.  After an
        explain() that cut its batch: of the last piece."""
        out = (C.c_double * 3)()
        L.check(L.lib().mfx_rec_explain_times(self.handle, out))
        return {"build": out[0], "solve": out[1], "contrib": out[2]}

    def fold_in_times(self) -> dict:
        """Seconds of the last fold_in call by phase (mfx_rec_fold_in_times): {"build", "solve", "score"}."""
        out = (C.c_double * 3)()
        L.check(L.lib().mfx_rec_fold_in_times(self.handle, out))
        return {"build": out[0], "solve": out[1], "score": out[2]}

    def close(self):
        if self.handle:
            L.lib().mfx_rec_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def recommend(W, H, layout: int, n_top: int, users=None, exclude: Optional[RatingData] = None, device: int = 0,
              item_slices: int = 0):
    """One-shot Recommender(W, H, layout, exclude, device).query(n_top, users, item_slices)."""
    with Recommender(W, H, layout, exclude=exclude, device=device) as r:
        return r.query(n_top, users=users, item_slices=item_slices)


def topn_metrics(items, T, users=None, min_rating: float = float("-inf")) -> dict:
    """Ranking metrics of top-N lists `items` [U, N] (uint32; PAD_ITEM slots never count) against the test set T
    (TestData or RatingData): {"hr", "precision", "recall", "ndcg", "users"}.  users: the user of each list (None:
    list u is user u).  Only test entries with value >= min_rating count; users left with none are skipped."""
    items = np.ascontiguousarray(np.asarray(items), dtype=np.uint32)
    if items.ndim != 2 or items.shape[1] < 1:
        raise ValueError("items must be [users, n_top] with n_top >= 1")
    n, n_top = items.shape
    pu = None
    if users is not None:
        users = np.ascontiguousarray(np.asarray(users), dtype=np.uint32)
        if users.shape != (n,):
            raise ValueError("users must have one entry per list")
        pu = _vp(users)
    if not isinstance(T, TestData):
        T = test_data_of(T)
    coo = _coo(T)
    out = (C.c_double * 4)()
    kept = C.c_int64(0)
    L.check(L.lib().mfx_topn_metrics(n, pu, n_top, _vp(items), C.byref(coo), float(min_rating), out, C.byref(kept)))
    return {"hr": out[0], "precision": out[1], "recall": out[2], "ndcg": out[3], "users": int(kept.value)}
