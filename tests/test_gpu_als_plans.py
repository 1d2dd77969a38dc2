"""Every ALS trainer the library has (the nine (method, objective) pairs of DESIGN 5.2) on one small matrix that takes every
host path: the resident trainer against chained calls of the pair's single-half operator bit for bit, from host and from
device inputs, the names of kernel_times, and what loss() and cg_stats() answer on the pair.

The matrix: 2100 users x 24 items, item 0 held by every user but one (2099 entries: its column is split into two partial
slots of kAlsChunk = 2048 and reduced), a few hundred other entries, user 7 and item 11 empty, strengths in (0, 4].
Ranks: 40 for the direct solvers (two 32-tiles), 136 with blocks of 64 (three blocks, the last 8 wide) for the block sweeps,
136 with at most 12 steps and tol 1e-5 for conjugate gradients.  Everything compared here is compared bit for bit: both
sides run the same kernels in the same order on the same inputs."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_ials import _device_arrays

pytestmark = pytest.mark.gpu

MFX_ERR_INVALID = -1  # include/mfx.h
LAM, ALPHA, ALPHA0, NU = 0.1, 2.0, 0.5, 0.5
K_DIRECT, K_BLOCKS, BLOCK, CG = 40, 136, 64, (12, 1e-5)


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1, m.lib().mfx_last_error()
    return m


@functools.lru_cache(maxsize=None)
def matrix():
    from mfx import dataset as ds
    rows, cols = 2100, 24
    rng = np.random.default_rng(24)
    mask = rng.random((rows, cols)) < 0.008
    mask[:, 0] = True
    mask[7, :] = False   # an empty user
    mask[:, 11] = False  # an empty item
    r, c = np.nonzero(mask)
    v = (rng.integers(1, 17, r.size) / 4).astype(np.float32)
    R = ds.from_coo(rows, cols, r, c, v)
    assert int(R.csc_col_ptr[1]) == rows - 1 > 2048 and 200 <= R.nnz - (rows - 1) <= 900
    return R


def _names(prefix, gram=True, inverse=False):
    out = [f"{prefix}_half_rows(W over H)", f"{prefix}_half_cols(H over W)"]
    if gram:
        out += [f"{prefix}_base_gram(H)", f"{prefix}_base_gram(W)"]
    if inverse:
        out += [f"{prefix}_inverse(H)", f"{prefix}_inverse(W)"]
    return out


# pair -> (rank, implicit, warm: the operator takes Y_in and W goes to set_factors, the names of kernel_times,
#          the arguments of the solver class, the single-half operator as f(mfx, ptr, idx, val, X, Y_in))
PAIRS = {
    "Direct-Als": (K_DIRECT, False, False, _names("als", gram=False), dict(),
                   lambda m, p, i, v, X, Y: m.als_half(p, i, v, X, K_DIRECT, LAM, variant=1)),
    "DirectExact-Als": (K_DIRECT, False, False, _names("als", gram=False), dict(schedule=0),
                        lambda m, p, i, v, X, Y: m.als_half(p, i, v, X, K_DIRECT, LAM, variant=0)),
    "Direct-Implicit": (K_DIRECT, True, False, _names("ials"), dict(),
                        lambda m, p, i, v, X, Y: m.ials_half(p, i, v, X, K_DIRECT, LAM, ALPHA)),
    "Direct-ImplicitReg": (K_DIRECT, True, False, _names("ials"), dict(alpha0=ALPHA0, nu=NU),
                           lambda m, p, i, v, X, Y: m.ials_half(p, i, v, X, K_DIRECT, LAM, ALPHA, alpha0=ALPHA0, nu=NU)),
    "Blocks-Als": (K_BLOCKS, False, True, _names("alsb", gram=False), dict(block=BLOCK),
                   lambda m, p, i, v, X, Y: m.als_block_half(p, i, v, X, K_BLOCKS, LAM, BLOCK, Y_in=Y)),
    "Blocks-Ccd": (K_BLOCKS, False, True, _names("alsb", gram=False), dict(block=BLOCK, count_reg=True),
                   lambda m, p, i, v, X, Y: m.als_block_half(p, i, v, X, K_BLOCKS, LAM, BLOCK, Y_in=Y, count_reg=True)),
    "Blocks-Implicit": (K_BLOCKS, True, True, _names("ialsb"), dict(block=BLOCK),
                        lambda m, p, i, v, X, Y: m.ials_block_half(p, i, v, X, K_BLOCKS, LAM, ALPHA, BLOCK, Y_in=Y)),
    "Blocks-ImplicitReg": (K_BLOCKS, True, True, _names("ialsb"), dict(block=BLOCK, alpha0=ALPHA0, nu=NU),
                           lambda m, p, i, v, X, Y: m.ials_block_half(p, i, v, X, K_BLOCKS, LAM, ALPHA, BLOCK, Y_in=Y, alpha0=ALPHA0,
                                                                      nu=NU)),
    "Cg-Implicit": (K_BLOCKS, True, True, _names("ialscg", inverse=True), dict(cg=CG),
                    lambda m, p, i, v, X, Y: m.ials_cg_half(p, i, v, X, K_BLOCKS, LAM, ALPHA, *CG, Y_in=Y)),
}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def solver(mfx, pair, device_arrays=None):
    k, implicit, _, _, kw, _ = PAIRS[pair]
    kw = dict(kw)
    p = mfx.parameter()
    p.k, p.lambda_, p.schedule = k, LAM, kw.pop("schedule", 1)
    R = matrix() if device_arrays is None else None
    if implicit:
        return mfx.ImplicitAlsSolver(R, p, ALPHA, device_arrays=device_arrays, **kw)
    return mfx.AlsSolver(R, None, p, device_arrays=device_arrays, **kw)


def start(pair):
    k = PAIRS[pair][0]
    rng = np.random.default_rng(k)
    R = matrix()
    return (rng.standard_normal((R.rows, k)) * 0.1).astype(np.float32), (rng.standard_normal((R.cols, k)) * 0.1).astype(np.float32)


@pytest.mark.parametrize("pair", list(PAIRS))
def test_trainer_is_its_chained_halves_and_answers_as_its_pair(mfx, pair):
    import torch  # noqa: F401  (device-resident inputs)
    R = matrix()
    k, implicit, warm, names, _, half = PAIRS[pair]
    W0, H0 = start(pair)
    # (a) two iterations of the resident trainer = four chained single halves from the same start
    W, H = (W0, H0) if warm else (None, H0)
    for _ in range(2):
        W = half(mfx, R.csr_row_ptr, R.csr_col_idx, R.csr_val, H, W)
        H = half(mfx, R.csc_col_ptr, R.csc_row_idx, R.csc_val, W, H)
    assert np.isfinite(W).all() and np.isfinite(H).all()
    assert not W[7].any() and not H[11].any() and W[8].any() and H[0].any()
    got = []
    for dev in (None, _device_arrays(R)):  # (b) the same from device arrays
        s = solver(mfx, pair, dev)
        s.set_factors(H0, W0 if warm else None)
        s.iterate(2)
        Ws, Hs = s.get_factors()
        assert np.array_equal(bits(Ws), bits(W)) and np.array_equal(bits(Hs), bits(H)), (pair, "device" if dev else "host")
        got.append(s)
    s = got[0]
    # (c) the timed stages of the pair, in the order of mfx_als_kernel_times
    kt = s.kernel_times()
    assert list(kt) == names, (pair, list(kt))
    assert all(sec >= 0 and n == 2 for sec, n in kt.values()) and kt[names[0]][0] > 0 and kt[names[1]][0] > 0, kt
    # (d) loss() and cg_stats()
    lib = mfx.lib()
    out = C.c_double(-1.0)
    if implicit:
        fresh = solver(mfx, pair)
        fresh.set_factors(H, W)
        assert s.loss() == got[1].loss() == fresh.loss() > 0
        fresh.close()
    else:
        assert lib.mfx_ials_loss(s.handle, C.byref(out)) == MFX_ERR_INVALID
        assert lib.mfx_last_error().decode() == "mfx_ials_loss: not an implicit-feedback ALS handle (mfx_ials_create)"
    st = (C.c_int64 * 8)()
    if pair == "Cg-Implicit":
        assert s.cg_stats() == got[1].cg_stats() and s.cg_stats()["rows"]["failed"] == 0 and 1 <= s.cg_stats()["cols"]["max_steps"] <= CG[0]
    else:
        assert lib.mfx_ials_cg_stats(s.handle, st) == MFX_ERR_INVALID
        assert lib.mfx_last_error().decode() == "mfx_ials_cg_stats: not a handle of mfx_ials_cg_create"
    for s in got:
        s.close()


def test_a_refused_create_leaves_the_next_one_working(mfx):
    """(e) after the walk: a create with a bad argument is refused, and the next good create works."""
    p = mfx.parameter()
    p.k, p.lambda_ = K_BLOCKS, LAM
    with pytest.raises(mfx.MfxError, match="block = 129"):
        mfx.ImplicitAlsSolver(matrix(), p, ALPHA, block=129)
    s = solver(mfx, "Blocks-Implicit")
    W0, H0 = start("Blocks-Implicit")
    s.set_factors(H0, W0)
    s.iterate(1)
    W, H = s.get_factors()
    s.close()
    assert np.isfinite(W).all() and np.isfinite(H).all() and H[0].any()
