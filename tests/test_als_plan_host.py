"""The refusals of the fourteen ALS entry points (seven creates, seven single halves) that happen on the host, before any
device is touched: every argument an entry point validates gets one bad value at a time, and two inputs per entry point
carry two bad values, which pins the order of the checks.  The expected (return code, full text of mfx_last_error())
pairs are what the library answered before the entry points were moved onto one AlsSpec and one als_spec_check; they hold
with and without a GPU."""
import ctypes as C
import math

import numpy as np
import pytest

NAN, INF = math.nan, math.inf
BIG = 1 << 32  # a segment count past the 32-bit index range

# name -> the arguments behind (out, R) or behind the segments and X, in the order of include/mfx.h
CREATES = {
    "mfx_als_create": ("T", "p", "space"),
    "mfx_ials_create": ("p", "alpha", "space"),
    "mfx_ials_block_create": ("p", "alpha", "block", "space"),
    "mfx_ials_cg_create": ("p", "alpha", "steps", "tol", "space"),
    "mfx_ials_create_reg": ("p", "alpha", "alpha0", "nu", "space"),
    "mfx_ials_block_create_reg": ("p", "alpha", "alpha0", "nu", "block", "space"),
    "mfx_als_block_create": ("T", "p", "block", "reg", "space"),
}
HALVES = {
    "mfx_als_half": ("Y", "k", "lam", "variant", "device"),
    "mfx_ials_half": ("Y", "k", "lam", "alpha", "device"),
    "mfx_ials_half_reg": ("Y", "k", "lam", "alpha", "alpha0", "nu", "device"),
    "mfx_ials_block_half": ("Y_in", "Y", "k", "block", "lam", "alpha", "device"),
    "mfx_ials_block_half_reg": ("Y_in", "Y", "k", "block", "lam", "alpha", "alpha0", "nu", "device"),
    "mfx_als_block_half": ("Y_in", "Y", "k", "block", "lam", "reg", "device"),
    "mfx_ials_cg_half": ("Y_in", "Y", "k", "lam", "alpha", "steps", "tol", "counts", "device"),
}
GOOD = dict(k=8, lam=0.1, alpha=1.0, alpha0=0.5, nu=0.5, block=0, reg=0, steps=4, tol=1e-4, schedule=1, space=0, variant=1,
            device=0, out=True, R=True, p=True, nseg=1, idx=True)

# the bad values of every entry point: (what is wrong, ...), one or two at a time
_NULLS = [(("out", False),), (("R", False),), (("p", False),)]
_ALPHA = [(("alpha", v),) for v in (-1.0, NAN, INF)]
_REG = [(("alpha0", 0.0),), (("alpha0", NAN),), (("nu", -0.5),), (("nu", 1.5),), (("lam", INF), ("nu", 1.0))]
_BLOCK = [(("block", -1),), (("block", 129),)]
_CG = [(("steps", 0),), (("tol", -1.0),), (("tol", NAN),)]
_SCHED = [(("schedule", 0),)]
_SPACE = [(("space", 7),)]
_ARRAYS = [(("nseg", 0),), (("idx", False),), (("nseg", BIG),)]


def _ranks(*ks):
    return [(("k", k),) for k in ks]


BAD = {
    "mfx_als_create": _NULLS + _ranks(0, 129) + [(("out", False), ("R", False)), (("R", False), ("k", 0))],
    "mfx_ials_create": _NULLS + _ALPHA + _ranks(0, 129) + _SCHED + [(("alpha", -1.0), ("k", 0)), (("k", 129), ("schedule", 0))],
    "mfx_ials_block_create": _NULLS + _ALPHA + _ranks(0, 1025) + _BLOCK + _SCHED
    + [(("alpha", NAN), ("k", 1025)), (("block", 129), ("schedule", 0))],
    "mfx_ials_cg_create": _NULLS + _SPACE + _ALPHA + _ranks(0, 1025) + _CG + _SCHED
    + [(("space", 7), ("alpha", -1.0)), (("tol", NAN), ("schedule", 0)), (("k", 0), ("steps", 0))],
    "mfx_ials_create_reg": _NULLS + _SPACE + _ALPHA + _ranks(0, 129) + _SCHED + _REG
    + [(("schedule", 0), ("alpha0", 0.0)), (("space", 7), ("k", 129))],
    "mfx_ials_block_create_reg": _NULLS + _SPACE + _ALPHA + _ranks(0, 1025) + _BLOCK + _SCHED + _REG
    + [(("block", -1), ("R", False)), (("block", 129), ("schedule", 0)), (("k", 0), ("block", 129))],
    "mfx_als_block_create": _NULLS + _ranks(0, 1025) + _BLOCK + [(("reg", 2),), (("lam", 0.0),), (("lam", NAN),)] + _SCHED
    + [(("reg", 2), ("lam", 0.0)), (("block", 129), ("reg", 2)), (("lam", 0.0), ("schedule", 0))],
    "mfx_als_half": _ARRAYS + _ranks(0, 129) + [(("nseg", BIG), ("k", 129)), (("k", 0), ("idx", False))],
    "mfx_ials_half": _ARRAYS + _ranks(0, 129) + _ALPHA + [(("k", 129), ("alpha", -1.0)), (("alpha", NAN), ("nseg", BIG))],
    "mfx_ials_half_reg": _ARRAYS + _ranks(0, 129) + _ALPHA + _REG
    + [(("nseg", BIG), ("alpha0", 0.0)), (("alpha", INF), ("nu", 1.5)), (("k", 0), ("nseg", BIG))],
    "mfx_ials_block_half": _ARRAYS + _ranks(0, 1025) + _BLOCK + _ALPHA
    + [(("block", 129), ("alpha", -1.0)), (("alpha", -1.0), ("nseg", BIG)), (("k", 1025), ("block", -1))],
    "mfx_ials_block_half_reg": _ARRAYS + _ranks(0, 1025) + _BLOCK + _ALPHA + _REG
    + [(("nseg", BIG), ("nu", -0.5)), (("block", -1), ("alpha", NAN))],
    "mfx_als_block_half": _ARRAYS + _ranks(0, 1025) + _BLOCK + [(("reg", 2),), (("lam", 0.0),), (("lam", NAN),)]
    + [(("reg", 2), ("lam", 0.0)), (("lam", 0.0), ("nseg", BIG)), (("block", 129), ("reg", 2))],
    "mfx_ials_cg_half": _ARRAYS + _ranks(0, 1025) + _CG + _ALPHA
    + [(("tol", -1.0), ("alpha", -1.0)), (("alpha", -1.0), ("nseg", BIG)), (("k", 0), ("steps", 0))],
}


def _id(fn, bad):
    return fn + "[" + ", ".join(f"{n}={v}" for n, v in bad) + "]"


CASES = {_id(fn, bad): (fn, bad) for fn, bads in BAD.items() for bad in bads}


def _matrix():
    from mfx import dataset as ds
    rng = np.random.default_rng(7)
    mask = rng.random((12, 9)) < 0.3
    r, c = np.nonzero(mask)
    return ds.from_coo(12, 9, r, c, rng.integers(1, 5, r.size).astype(np.float32))


def call(mfx, fn, bad):
    """Calls entry point fn with valid arguments except for `bad`; returns (return code, mfx_last_error())."""
    from mfx.api import _csx, _f32, _u32
    lib = mfx.lib()
    a = dict(GOOD)
    a.update(bad)
    keep = []
    if fn in CREATES:
        p = mfx.parameter()
        p.k, p.lambda_ = a["k"], a["lam"]
        cp = p.to_c()
        cp.schedule = a["schedule"]
        csx = _csx(_matrix())
        h = C.c_void_p()
        val = dict(a, T=None, p=C.byref(cp) if a["p"] else None)
        args = [C.byref(h) if a["out"] else None, C.byref(csx) if a["R"] else None] + [val[n] for n in CREATES[fn]]
    else:
        k = max(int(a["k"]), 1)
        ptr, idx, v = np.array([0, 1], np.uint32), np.array([0], np.uint32), np.array([1.0], np.float32)
        X, Y = np.ones((2, k), np.float32), np.zeros((1, k), np.float32)
        keep = [ptr, idx, v, X, Y]
        val = dict(a, Y=_f32(Y), Y_in=None, counts=None)
        args = [a["nseg"], 1, _u32(ptr), _u32(idx) if a["idx"] else None, _f32(v), 2, _f32(X)] + [val[n] for n in HALVES[fn]]
    rc = getattr(lib, fn)(*args)
    msg = lib.mfx_last_error().decode()
    assert rc != 0, (fn, bad, "accepted")
    del keep
    return rc, msg


EXPECTED = {
    'mfx_als_create[out=False]': (-1, 'mfx_als_create: out is NULL'),
    'mfx_als_create[R=False]': (-1, 'mfx_als_create: null argument'),
    'mfx_als_create[p=False]': (-1, 'mfx_als_create: null argument'),
    'mfx_als_create[k=0]': (-1, 'ALS: rank k = 0 not supported (1 <= k <= 128)'),
    'mfx_als_create[k=129]': (-1, 'ALS: rank k = 129 not supported (1 <= k <= 128)'),
    'mfx_als_create[out=False, R=False]': (-1, 'mfx_als_create: out is NULL'),
    'mfx_als_create[R=False, k=0]': (-1, 'mfx_als_create: null argument'),
    'mfx_ials_create[out=False]': (-1, 'mfx_ials_create: out is NULL'),
    'mfx_ials_create[R=False]': (-1, 'mfx_ials_create: null argument'),
    'mfx_ials_create[p=False]': (-1, 'mfx_ials_create: null argument'),
    'mfx_ials_create[alpha=-1.0]': (-1, 'mfx_ials_create: alpha = -1 (finite and >= 0 required)'),
    'mfx_ials_create[alpha=nan]': (-1, 'mfx_ials_create: alpha = nan (finite and >= 0 required)'),
    'mfx_ials_create[alpha=inf]': (-1, 'mfx_ials_create: alpha = inf (finite and >= 0 required)'),
    'mfx_ials_create[k=0]': (-1, 'implicit ALS: rank k = 0 not supported (1 <= k <= 128)'),
    'mfx_ials_create[k=129]': (-1, 'implicit ALS: rank k = 129 not supported (1 <= k <= 128)'),
    'mfx_ials_create[schedule=0]': (-1, 'implicit ALS: schedule must be 1 (there is no as-written mode)'),
    'mfx_ials_create[alpha=-1.0, k=0]': (-1, 'mfx_ials_create: alpha = -1 (finite and >= 0 required)'),
    'mfx_ials_create[k=129, schedule=0]': (-1, 'implicit ALS: rank k = 129 not supported (1 <= k <= 128)'),
    'mfx_ials_block_create[out=False]': (-1, 'mfx_ials_block_create: out is NULL'),
    'mfx_ials_block_create[R=False]': (-1, 'mfx_ials_block_create: null argument'),
    'mfx_ials_block_create[p=False]': (-1, 'mfx_ials_block_create: null argument'),
    'mfx_ials_block_create[alpha=-1.0]': (-1, 'mfx_ials_block_create: alpha = -1 (finite and >= 0 required)'),
    'mfx_ials_block_create[alpha=nan]': (-1, 'mfx_ials_block_create: alpha = nan (finite and >= 0 required)'),
    'mfx_ials_block_create[alpha=inf]': (-1, 'mfx_ials_block_create: alpha = inf (finite and >= 0 required)'),
    'mfx_ials_block_create[k=0]': (-1, 'implicit ALS by block sweeps: rank k = 0 not supported (1 <= k <= 1024)'),
    'mfx_ials_block_create[k=1025]': (-1, 'implicit ALS by block sweeps: rank k = 1025 not supported (1 <= k <= 1024)'),
    'mfx_ials_block_create[block=-1]': (-1, 'implicit ALS by block sweeps: block = -1 (0 = chosen from k, else 1 <= block <= 128)'),
    'mfx_ials_block_create[block=129]': (-1, 'implicit ALS by block sweeps: block = 129 (0 = chosen from k, else 1 <= block <= 128)'),
    'mfx_ials_block_create[schedule=0]': (-1, 'implicit ALS by block sweeps: schedule must be 1 (there is no as-written mode)'),
    'mfx_ials_block_create[alpha=nan, k=1025]': (-1, 'mfx_ials_block_create: alpha = nan (finite and >= 0 required)'),
    'mfx_ials_block_create[block=129, schedule=0]': (-1, 'implicit ALS by block sweeps: block = 129 (0 = chosen from k, else 1 <= block <= 128)'),
    'mfx_ials_cg_create[out=False]': (-1, 'mfx_ials_cg_create: out is NULL'),
    'mfx_ials_cg_create[R=False]': (-1, 'mfx_ials_cg_create: null argument'),
    'mfx_ials_cg_create[p=False]': (-1, 'mfx_ials_cg_create: null argument'),
    'mfx_ials_cg_create[space=7]': (-1, 'mfx_ials_cg_create: bad memory space'),
    'mfx_ials_cg_create[alpha=-1.0]': (-1, 'mfx_ials_cg_create: alpha = -1 (finite and >= 0 required)'),
    'mfx_ials_cg_create[alpha=nan]': (-1, 'mfx_ials_cg_create: alpha = nan (finite and >= 0 required)'),
    'mfx_ials_cg_create[alpha=inf]': (-1, 'mfx_ials_cg_create: alpha = inf (finite and >= 0 required)'),
    'mfx_ials_cg_create[k=0]': (-1, 'implicit ALS by conjugate gradients: rank k = 0 not supported (1 <= k <= 1024)'),
    'mfx_ials_cg_create[k=1025]': (-1, 'implicit ALS by conjugate gradients: rank k = 1025 not supported (1 <= k <= 1024)'),
    'mfx_ials_cg_create[steps=0]': (-1, 'implicit ALS by conjugate gradients: steps = 0 (>= 1 required)'),
    'mfx_ials_cg_create[tol=-1.0]': (-1, 'implicit ALS by conjugate gradients: tol = -1 (finite and >= 0 required)'),
    'mfx_ials_cg_create[tol=nan]': (-1, 'implicit ALS by conjugate gradients: tol = nan (finite and >= 0 required)'),
    'mfx_ials_cg_create[schedule=0]': (-1, 'implicit ALS by conjugate gradients: schedule must be 1 (there is no as-written mode)'),
    'mfx_ials_cg_create[space=7, alpha=-1.0]': (-1, 'mfx_ials_cg_create: bad memory space'),
    'mfx_ials_cg_create[tol=nan, schedule=0]': (-1, 'implicit ALS by conjugate gradients: tol = nan (finite and >= 0 required)'),
    'mfx_ials_cg_create[k=0, steps=0]': (-1, 'implicit ALS by conjugate gradients: rank k = 0 not supported (1 <= k <= 1024)'),
    'mfx_ials_create_reg[out=False]': (-1, 'mfx_ials_create_reg: out is NULL'),
    'mfx_ials_create_reg[R=False]': (-1, 'mfx_ials_create_reg: null argument'),
    'mfx_ials_create_reg[p=False]': (-1, 'mfx_ials_create_reg: null argument'),
    'mfx_ials_create_reg[space=7]': (-1, 'mfx_ials_create_reg: bad memory space'),
    'mfx_ials_create_reg[alpha=-1.0]': (-1, 'mfx_ials_create_reg: alpha = -1 (finite and >= 0 required)'),
    'mfx_ials_create_reg[alpha=nan]': (-1, 'mfx_ials_create_reg: alpha = nan (finite and >= 0 required)'),
    'mfx_ials_create_reg[alpha=inf]': (-1, 'mfx_ials_create_reg: alpha = inf (finite and >= 0 required)'),
    'mfx_ials_create_reg[k=0]': (-1, 'implicit ALS: rank k = 0 not supported (1 <= k <= 128)'),
    'mfx_ials_create_reg[k=129]': (-1, 'implicit ALS: rank k = 129 not supported (1 <= k <= 128)'),
    'mfx_ials_create_reg[schedule=0]': (-1, 'mfx_ials_create_reg: schedule must be 1 (there is no as-written mode)'),
    'mfx_ials_create_reg[alpha0=0.0]': (-1, 'mfx_ials_create_reg: alpha0 = 0 (finite and > 0 required)'),
    'mfx_ials_create_reg[alpha0=nan]': (-1, 'mfx_ials_create_reg: alpha0 = nan (finite and > 0 required)'),
    'mfx_ials_create_reg[nu=-0.5]': (-1, 'mfx_ials_create_reg: nu = -0.5 (0 <= nu <= 1 required)'),
    'mfx_ials_create_reg[nu=1.5]': (-1, 'mfx_ials_create_reg: nu = 1.5 (0 <= nu <= 1 required)'),
    'mfx_ials_create_reg[lam=inf, nu=1.0]': (-1, 'mfx_ials_create_reg: the regulariser lambda ((1 + alpha0) max(rows, cols))^nu = inf is not a finite fp32 number (lambda = inf, alpha0 = 0.5, nu = 1)'),
    'mfx_ials_create_reg[schedule=0, alpha0=0.0]': (-1, 'mfx_ials_create_reg: schedule must be 1 (there is no as-written mode)'),
    'mfx_ials_create_reg[space=7, k=129]': (-1, 'mfx_ials_create_reg: bad memory space'),
    'mfx_ials_block_create_reg[out=False]': (-1, 'mfx_ials_block_create_reg: out is NULL'),
    'mfx_ials_block_create_reg[R=False]': (-1, 'mfx_ials_block_create_reg: null argument'),
    'mfx_ials_block_create_reg[p=False]': (-1, 'mfx_ials_block_create_reg: null argument'),
    'mfx_ials_block_create_reg[space=7]': (-1, 'mfx_ials_block_create_reg: bad memory space'),
    'mfx_ials_block_create_reg[alpha=-1.0]': (-1, 'mfx_ials_block_create_reg: alpha = -1 (finite and >= 0 required)'),
    'mfx_ials_block_create_reg[alpha=nan]': (-1, 'mfx_ials_block_create_reg: alpha = nan (finite and >= 0 required)'),
    'mfx_ials_block_create_reg[alpha=inf]': (-1, 'mfx_ials_block_create_reg: alpha = inf (finite and >= 0 required)'),
    'mfx_ials_block_create_reg[k=0]': (-1, 'implicit ALS by block sweeps: rank k = 0 not supported (1 <= k <= 1024)'),
    'mfx_ials_block_create_reg[k=1025]': (-1, 'implicit ALS by block sweeps: rank k = 1025 not supported (1 <= k <= 1024)'),
    'mfx_ials_block_create_reg[block=-1]': (-1, 'implicit ALS by block sweeps: block = -1 (0 = chosen from k, else 1 <= block <= 128)'),
    'mfx_ials_block_create_reg[block=129]': (-1, 'implicit ALS by block sweeps: block = 129 (0 = chosen from k, else 1 <= block <= 128)'),
    'mfx_ials_block_create_reg[schedule=0]': (-1, 'mfx_ials_block_create_reg: schedule must be 1 (there is no as-written mode)'),
    'mfx_ials_block_create_reg[alpha0=0.0]': (-1, 'mfx_ials_block_create_reg: alpha0 = 0 (finite and > 0 required)'),
    'mfx_ials_block_create_reg[alpha0=nan]': (-1, 'mfx_ials_block_create_reg: alpha0 = nan (finite and > 0 required)'),
    'mfx_ials_block_create_reg[nu=-0.5]': (-1, 'mfx_ials_block_create_reg: nu = -0.5 (0 <= nu <= 1 required)'),
    'mfx_ials_block_create_reg[nu=1.5]': (-1, 'mfx_ials_block_create_reg: nu = 1.5 (0 <= nu <= 1 required)'),
    'mfx_ials_block_create_reg[lam=inf, nu=1.0]': (-1, 'mfx_ials_block_create_reg: the regulariser lambda ((1 + alpha0) max(rows, cols))^nu = inf is not a finite fp32 number (lambda = inf, alpha0 = 0.5, nu = 1)'),
    'mfx_ials_block_create_reg[block=-1, R=False]': (-1, 'implicit ALS by block sweeps: block = -1 (0 = chosen from k, else 1 <= block <= 128)'),
    'mfx_ials_block_create_reg[block=129, schedule=0]': (-1, 'implicit ALS by block sweeps: block = 129 (0 = chosen from k, else 1 <= block <= 128)'),
    'mfx_ials_block_create_reg[k=0, block=129]': (-1, 'implicit ALS by block sweeps: rank k = 0 not supported (1 <= k <= 1024)'),
    'mfx_als_block_create[out=False]': (-1, 'mfx_als_block_create: out is NULL'),
    'mfx_als_block_create[R=False]': (-1, 'mfx_als_block_create: null argument'),
    'mfx_als_block_create[p=False]': (-1, 'mfx_als_block_create: null argument'),
    'mfx_als_block_create[k=0]': (-1, 'explicit ALS by block sweeps: rank k = 0 not supported (1 <= k <= 1024)'),
    'mfx_als_block_create[k=1025]': (-1, 'explicit ALS by block sweeps: rank k = 1025 not supported (1 <= k <= 1024)'),
    'mfx_als_block_create[block=-1]': (-1, 'explicit ALS by block sweeps: block = -1 (0 = chosen from k, else 1 <= block <= 128)'),
    'mfx_als_block_create[block=129]': (-1, 'explicit ALS by block sweeps: block = 129 (0 = chosen from k, else 1 <= block <= 128)'),
    'mfx_als_block_create[reg=2]': (-1, 'explicit ALS by block sweeps: reg = 2 (0 = lambda, 1 = lambda * entries of the segment)'),
    'mfx_als_block_create[lam=0.0]': (-1, 'explicit ALS by block sweeps: lambda = 0 (finite and > 0 required)'),
    'mfx_als_block_create[lam=nan]': (-1, 'explicit ALS by block sweeps: lambda = nan (finite and > 0 required)'),
    'mfx_als_block_create[schedule=0]': (-1, 'explicit ALS by block sweeps: schedule must be 1 (there is no as-written mode)'),
    'mfx_als_block_create[reg=2, lam=0.0]': (-1, 'explicit ALS by block sweeps: reg = 2 (0 = lambda, 1 = lambda * entries of the segment)'),
    'mfx_als_block_create[block=129, reg=2]': (-1, 'explicit ALS by block sweeps: block = 129 (0 = chosen from k, else 1 <= block <= 128)'),
    'mfx_als_block_create[lam=0.0, schedule=0]': (-1, 'explicit ALS by block sweeps: lambda = 0 (finite and > 0 required)'),
    'mfx_als_half[nseg=0]': (-1, 'mfx_als_half: bad argument'),
    'mfx_als_half[idx=False]': (-1, 'mfx_als_half: null idx / val with nnz > 0'),
    'mfx_als_half[nseg=4294967296]': (-1, 'mfx_als_half: sizes exceed the 32-bit index range'),
    'mfx_als_half[k=0]': (-1, 'mfx_als_half: bad argument'),
    'mfx_als_half[k=129]': (-1, 'ALS: rank k = 129 not supported (1 <= k <= 128)'),
    'mfx_als_half[nseg=4294967296, k=129]': (-1, 'mfx_als_half: sizes exceed the 32-bit index range'),
    'mfx_als_half[k=0, idx=False]': (-1, 'mfx_als_half: bad argument'),
    'mfx_ials_half[nseg=0]': (-1, 'mfx_ials_half: bad argument'),
    'mfx_ials_half[idx=False]': (-1, 'mfx_ials_half: null idx / val with nnz > 0'),
    'mfx_ials_half[nseg=4294967296]': (-1, 'mfx_ials_half: sizes exceed the 32-bit index range'),
    'mfx_ials_half[k=0]': (-1, 'implicit ALS: rank k = 0 not supported (1 <= k <= 128)'),
    'mfx_ials_half[k=129]': (-1, 'implicit ALS: rank k = 129 not supported (1 <= k <= 128)'),
    'mfx_ials_half[alpha=-1.0]': (-1, 'mfx_ials_half: alpha = -1 (finite and >= 0 required)'),
    'mfx_ials_half[alpha=nan]': (-1, 'mfx_ials_half: alpha = nan (finite and >= 0 required)'),
    'mfx_ials_half[alpha=inf]': (-1, 'mfx_ials_half: alpha = inf (finite and >= 0 required)'),
    'mfx_ials_half[k=129, alpha=-1.0]': (-1, 'implicit ALS: rank k = 129 not supported (1 <= k <= 128)'),
    'mfx_ials_half[alpha=nan, nseg=4294967296]': (-1, 'mfx_ials_half: alpha = nan (finite and >= 0 required)'),
    'mfx_ials_half_reg[nseg=0]': (-1, 'mfx_ials_half_reg: bad argument'),
    'mfx_ials_half_reg[idx=False]': (-1, 'mfx_ials_half_reg: null idx / val with nnz > 0'),
    'mfx_ials_half_reg[nseg=4294967296]': (-1, 'mfx_ials_half_reg: sizes exceed the 32-bit index range'),
    'mfx_ials_half_reg[k=0]': (-1, 'implicit ALS: rank k = 0 not supported (1 <= k <= 128)'),
    'mfx_ials_half_reg[k=129]': (-1, 'implicit ALS: rank k = 129 not supported (1 <= k <= 128)'),
    'mfx_ials_half_reg[alpha=-1.0]': (-1, 'mfx_ials_half_reg: alpha = -1 (finite and >= 0 required)'),
    'mfx_ials_half_reg[alpha=nan]': (-1, 'mfx_ials_half_reg: alpha = nan (finite and >= 0 required)'),
    'mfx_ials_half_reg[alpha=inf]': (-1, 'mfx_ials_half_reg: alpha = inf (finite and >= 0 required)'),
    'mfx_ials_half_reg[alpha0=0.0]': (-1, 'mfx_ials_half_reg: alpha0 = 0 (finite and > 0 required)'),
    'mfx_ials_half_reg[alpha0=nan]': (-1, 'mfx_ials_half_reg: alpha0 = nan (finite and > 0 required)'),
    'mfx_ials_half_reg[nu=-0.5]': (-1, 'mfx_ials_half_reg: nu = -0.5 (0 <= nu <= 1 required)'),
    'mfx_ials_half_reg[nu=1.5]': (-1, 'mfx_ials_half_reg: nu = 1.5 (0 <= nu <= 1 required)'),
    'mfx_ials_half_reg[lam=inf, nu=1.0]': (-1, 'mfx_ials_half_reg: the regulariser lambda ((1 + alpha0) max(rows, cols))^nu = inf is not a finite fp32 number (lambda = inf, alpha0 = 0.5, nu = 1)'),
    'mfx_ials_half_reg[nseg=4294967296, alpha0=0.0]': (-1, 'mfx_ials_half_reg: sizes exceed the 32-bit index range'),
    'mfx_ials_half_reg[alpha=inf, nu=1.5]': (-1, 'mfx_ials_half_reg: alpha = inf (finite and >= 0 required)'),
    'mfx_ials_half_reg[k=0, nseg=4294967296]': (-1, 'implicit ALS: rank k = 0 not supported (1 <= k <= 128)'),
    'mfx_ials_block_half[nseg=0]': (-1, 'mfx_ials_block_half: bad argument'),
    'mfx_ials_block_half[idx=False]': (-1, 'mfx_ials_block_half: null idx / val with nnz > 0'),
    'mfx_ials_block_half[nseg=4294967296]': (-1, 'mfx_ials_block_half: sizes exceed the 32-bit index range'),
    'mfx_ials_block_half[k=0]': (-1, 'implicit ALS by block sweeps: rank k = 0 not supported (1 <= k <= 1024)'),
    'mfx_ials_block_half[k=1025]': (-1, 'implicit ALS by block sweeps: rank k = 1025 not supported (1 <= k <= 1024)'),
    'mfx_ials_block_half[block=-1]': (-1, 'implicit ALS by block sweeps: block = -1 (0 = chosen from k, else 1 <= block <= 128)'),
    'mfx_ials_block_half[block=129]': (-1, 'implicit ALS by block sweeps: block = 129 (0 = chosen from k, else 1 <= block <= 128)'),
    'mfx_ials_block_half[alpha=-1.0]': (-1, 'mfx_ials_block_half: alpha = -1 (finite and >= 0 required)'),
    'mfx_ials_block_half[alpha=nan]': (-1, 'mfx_ials_block_half: alpha = nan (finite and >= 0 required)'),
    'mfx_ials_block_half[alpha=inf]': (-1, 'mfx_ials_block_half: alpha = inf (finite and >= 0 required)'),
    'mfx_ials_block_half[block=129, alpha=-1.0]': (-1, 'implicit ALS by block sweeps: block = 129 (0 = chosen from k, else 1 <= block <= 128)'),
    'mfx_ials_block_half[alpha=-1.0, nseg=4294967296]': (-1, 'mfx_ials_block_half: alpha = -1 (finite and >= 0 required)'),
    'mfx_ials_block_half[k=1025, block=-1]': (-1, 'implicit ALS by block sweeps: rank k = 1025 not supported (1 <= k <= 1024)'),
    'mfx_ials_block_half_reg[nseg=0]': (-1, 'mfx_ials_block_half_reg: bad argument'),
    'mfx_ials_block_half_reg[idx=False]': (-1, 'mfx_ials_block_half_reg: null idx / val with nnz > 0'),
    'mfx_ials_block_half_reg[nseg=4294967296]': (-1, 'mfx_ials_block_half_reg: sizes exceed the 32-bit index range'),
    'mfx_ials_block_half_reg[k=0]': (-1, 'implicit ALS by block sweeps: rank k = 0 not supported (1 <= k <= 1024)'),
    'mfx_ials_block_half_reg[k=1025]': (-1, 'implicit ALS by block sweeps: rank k = 1025 not supported (1 <= k <= 1024)'),
    'mfx_ials_block_half_reg[block=-1]': (-1, 'implicit ALS by block sweeps: block = -1 (0 = chosen from k, else 1 <= block <= 128)'),
    'mfx_ials_block_half_reg[block=129]': (-1, 'implicit ALS by block sweeps: block = 129 (0 = chosen from k, else 1 <= block <= 128)'),
    'mfx_ials_block_half_reg[alpha=-1.0]': (-1, 'mfx_ials_block_half_reg: alpha = -1 (finite and >= 0 required)'),
    'mfx_ials_block_half_reg[alpha=nan]': (-1, 'mfx_ials_block_half_reg: alpha = nan (finite and >= 0 required)'),
    'mfx_ials_block_half_reg[alpha=inf]': (-1, 'mfx_ials_block_half_reg: alpha = inf (finite and >= 0 required)'),
    'mfx_ials_block_half_reg[alpha0=0.0]': (-1, 'mfx_ials_block_half_reg: alpha0 = 0 (finite and > 0 required)'),
    'mfx_ials_block_half_reg[alpha0=nan]': (-1, 'mfx_ials_block_half_reg: alpha0 = nan (finite and > 0 required)'),
    'mfx_ials_block_half_reg[nu=-0.5]': (-1, 'mfx_ials_block_half_reg: nu = -0.5 (0 <= nu <= 1 required)'),
    'mfx_ials_block_half_reg[nu=1.5]': (-1, 'mfx_ials_block_half_reg: nu = 1.5 (0 <= nu <= 1 required)'),
    'mfx_ials_block_half_reg[lam=inf, nu=1.0]': (-1, 'mfx_ials_block_half_reg: the regulariser lambda ((1 + alpha0) max(rows, cols))^nu = inf is not a finite fp32 number (lambda = inf, alpha0 = 0.5, nu = 1)'),
    'mfx_ials_block_half_reg[nseg=4294967296, nu=-0.5]': (-1, 'mfx_ials_block_half_reg: sizes exceed the 32-bit index range'),
    'mfx_ials_block_half_reg[block=-1, alpha=nan]': (-1, 'implicit ALS by block sweeps: block = -1 (0 = chosen from k, else 1 <= block <= 128)'),
    'mfx_als_block_half[nseg=0]': (-1, 'mfx_als_block_half: bad argument'),
    'mfx_als_block_half[idx=False]': (-1, 'mfx_als_block_half: null idx / val with nnz > 0'),
    'mfx_als_block_half[nseg=4294967296]': (-1, 'mfx_als_block_half: sizes exceed the 32-bit index range'),
    'mfx_als_block_half[k=0]': (-1, 'explicit ALS by block sweeps: rank k = 0 not supported (1 <= k <= 1024)'),
    'mfx_als_block_half[k=1025]': (-1, 'explicit ALS by block sweeps: rank k = 1025 not supported (1 <= k <= 1024)'),
    'mfx_als_block_half[block=-1]': (-1, 'explicit ALS by block sweeps: block = -1 (0 = chosen from k, else 1 <= block <= 128)'),
    'mfx_als_block_half[block=129]': (-1, 'explicit ALS by block sweeps: block = 129 (0 = chosen from k, else 1 <= block <= 128)'),
    'mfx_als_block_half[reg=2]': (-1, 'mfx_als_block_half: reg = 2 (0 = lambda, 1 = lambda * entries of the segment)'),
    'mfx_als_block_half[lam=0.0]': (-1, 'mfx_als_block_half: lambda = 0 (finite and > 0 required)'),
    'mfx_als_block_half[lam=nan]': (-1, 'mfx_als_block_half: lambda = nan (finite and > 0 required)'),
    'mfx_als_block_half[reg=2, lam=0.0]': (-1, 'mfx_als_block_half: reg = 2 (0 = lambda, 1 = lambda * entries of the segment)'),
    'mfx_als_block_half[lam=0.0, nseg=4294967296]': (-1, 'mfx_als_block_half: lambda = 0 (finite and > 0 required)'),
    'mfx_als_block_half[block=129, reg=2]': (-1, 'explicit ALS by block sweeps: block = 129 (0 = chosen from k, else 1 <= block <= 128)'),
    'mfx_ials_cg_half[nseg=0]': (-1, 'mfx_ials_cg_half: bad argument'),
    'mfx_ials_cg_half[idx=False]': (-1, 'mfx_ials_cg_half: null idx / val with nnz > 0'),
    'mfx_ials_cg_half[nseg=4294967296]': (-1, 'mfx_ials_cg_half: sizes exceed the 32-bit index range'),
    'mfx_ials_cg_half[k=0]': (-1, 'implicit ALS by conjugate gradients: rank k = 0 not supported (1 <= k <= 1024)'),
    'mfx_ials_cg_half[k=1025]': (-1, 'implicit ALS by conjugate gradients: rank k = 1025 not supported (1 <= k <= 1024)'),
    'mfx_ials_cg_half[steps=0]': (-1, 'implicit ALS by conjugate gradients: steps = 0 (>= 1 required)'),
    'mfx_ials_cg_half[tol=-1.0]': (-1, 'implicit ALS by conjugate gradients: tol = -1 (finite and >= 0 required)'),
    'mfx_ials_cg_half[tol=nan]': (-1, 'implicit ALS by conjugate gradients: tol = nan (finite and >= 0 required)'),
    'mfx_ials_cg_half[alpha=-1.0]': (-1, 'mfx_ials_cg_half: alpha = -1 (finite and >= 0 required)'),
    'mfx_ials_cg_half[alpha=nan]': (-1, 'mfx_ials_cg_half: alpha = nan (finite and >= 0 required)'),
    'mfx_ials_cg_half[alpha=inf]': (-1, 'mfx_ials_cg_half: alpha = inf (finite and >= 0 required)'),
    'mfx_ials_cg_half[tol=-1.0, alpha=-1.0]': (-1, 'implicit ALS by conjugate gradients: tol = -1 (finite and >= 0 required)'),
    'mfx_ials_cg_half[alpha=-1.0, nseg=4294967296]': (-1, 'mfx_ials_cg_half: alpha = -1 (finite and >= 0 required)'),
    'mfx_ials_cg_half[k=0, steps=0]': (-1, 'implicit ALS by conjugate gradients: rank k = 0 not supported (1 <= k <= 1024)'),
}


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    return m


def test_every_case_has_its_expected_answer():
    assert set(EXPECTED) == set(CASES)
    assert set(BAD) == set(CREATES) | set(HALVES) and len(BAD) == 14


@pytest.mark.parametrize("case", sorted(CASES))
def test_refusal_is_the_same_code_and_text(mfx, case):
    fn, bad = CASES[case]
    assert call(mfx, fn, bad) == EXPECTED[case]


if __name__ == "__main__":  # prints EXPECTED as the loaded library answers (MFX_LIB_PATH selects the build)
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "cuda-recommender_amd"))
    import mfx as m
    print("EXPECTED = {")
    for case in CASES:
        print(f"    {case!r}: {call(m, *CASES[case])!r},")
    print("}")
