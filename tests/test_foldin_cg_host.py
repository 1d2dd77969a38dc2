"""Fold-in by preconditioned conjugate gradients without a GPU: the ABI of mfx_rec_fold_in_cg_setup, the Python surface, and
the fp64 reference of tests/foldin_cg_ref.py pinned on the inputs of tests/test_gpu_foldin_cg.py -- every numerical condition
that the GPU tests put on the library must hold for the reference itself on exactly those inputs, so that a bound can never
be met only because the inputs were easy.

What the reference does there (asserted below, the step counts printed as `foldcg-reference` lines): with steps = 64,
tol = 1e-5 every row with a right-hand side stops before the cap from zero and from the warm start at every k in {37, 64, 130,
160, 256, 1024} and alpha in {0, 1, 40} -- after 1 step at alpha = 0 and after at most 11 / 14 / 19 / 22 / 24 / 31 steps at
alpha = 40 -- within 1e-3 of the dense solve and with a backward error below 3e-5; rows of 1 / 3 / 17 entries are solved after
at most 2 / 4 / 18 steps from zero; the same CG without the preconditioner is more than 1e-3 off there at k = 160 and 256,
alpha = 40, for the rows of 1 and 3 entries.  A row of one entry whose value is an explicit zero has no right-hand side under
the implicit model (k = 37 has one): zero after 0 steps."""
import ctypes as C
import inspect

import numpy as np
import pytest

import foldin_cg_ref as ref

MFX_ERR_INVALID = -1  # include/mfx.h
NEW = "mfx_rec_fold_in_cg_setup"


def test_the_symbol_is_exported_and_bound():
    import mfx
    from mfx import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, NEW)
    assert NEW in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[NEW]
    assert res is C.c_int and list(args) == [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int32, C.c_float]
    fn = getattr(mfx.lib(), NEW)
    assert fn.restype is res and list(fn.argtypes) == list(args)
    assert mfx.lib().mfx_version() == 2 == _lib.MFX_VERSION


def test_a_null_handle_is_refused():
    import mfx
    lib = mfx.lib()
    assert lib.mfx_rec_fold_in_cg_setup(None, 3, 0.1, 1.0, 64, 1e-5) == MFX_ERR_INVALID
    assert "null recommender" in lib.mfx_last_error().decode()


def test_the_python_method_and_its_keywords():
    import mfx
    setup = inspect.signature(mfx.Recommender.fold_in_cg_setup).parameters
    assert list(setup) == ["self", "model", "lam", "alpha", "steps", "tol"]
    assert (setup["alpha"].default, setup["steps"].default, setup["tol"].default) == (0.0, 64, 1e-5)
    fold = inspect.signature(mfx.Recommender.fold_in).parameters
    assert list(fold) == ["self", "rows", "n_top", "on_device", "W_init", "return_sweeps"]
    assert (ref.ALS, ref.CCD, ref.IMPLICIT) == (mfx.MFX_FOLD_ALS, mfx.MFX_FOLD_CCD, mfx.MFX_FOLD_IMPLICIT)


def test_the_inputs_are_those_of_the_block_operator_tests():
    import test_gpu_ials
    assert ref.SIZES == test_gpu_ials.SIZES
    ptr, idx, val, H, W0 = ref.inputs(37)
    p2, i2, v2 = test_gpu_ials._segments(137, 6000, test_gpu_ials.SIZES)
    assert np.array_equal(ptr, p2) and np.array_equal(idx, i2) and np.array_equal(val, v2)
    assert H.dtype == np.float32 and H.shape == (6000, 37) and W0.shape == (len(ref.SIZES), 37)


def _converged(model, k, alpha, cols=ref.COLS, sizes=tuple(ref.SIZES)):
    ptr, idx, val, H, W0 = ref.inputs(k, cols, sizes)
    if model != ref.IMPLICIT:
        val = ref.explicit_values(val)
    pair = ref.base(H, ref.LAM) if model == ref.IMPLICIT else None
    most = 0
    for start in (None, W0):
        Y, done = ref.rows(model, ptr, idx, val, H, ref.LAM, alpha, start, 64, 1e-5, base_pair=pair)
        rel, be, cn = ref.errors(model, k, alpha, Y, cols, sizes)
        assert cn <= 1e3, (model, k, alpha, cn)  # the gate may skip no row
        assert rel <= 1e-3 and be <= 3e-5, (model, k, alpha, start is not None, rel, be)
        live = ref.counting(model, k, alpha, cols, sizes)
        assert len(live) >= len([n for n in sizes if n]) - 2  # (a row of one entry may hold an explicit zero)
        for u, n in enumerate(sizes):
            if u not in live:
                assert done[u] == 0 and not Y[u].any()
            else:
                assert 1 <= done[u] < 64, (model, k, alpha, u, done[u])
                if model != ref.IMPLICIT and start is None and n < k:
                    assert done[u] <= n + 1, (model, k, u, n, done[u])
        most = max(most, int(done.max()))
    return most


@pytest.mark.parametrize("alpha", ref.ALPHAS)
@pytest.mark.parametrize("k", ref.KS)
def test_reference_converged_solve(k, alpha):
    most = _converged(ref.IMPLICIT, k, alpha)
    print(f"foldcg-reference k={k} alpha={alpha} most_steps={most}")


def test_reference_on_a_row_of_ten_chunks():
    for alpha in ref.ALPHAS:
        _converged(ref.IMPLICIT, 256, alpha, 30000, (20000, 0, 5))


@pytest.mark.parametrize("k", [160, 256])
@pytest.mark.parametrize("model", [ref.ALS, ref.CCD])
def test_reference_explicit_models(model, k):
    ptr, idx, val, _, _ = ref.inputs(k)
    v = ref.explicit_values(val)
    assert (v == 0).any() and (v < 0).any() and (v > 0).any()
    _converged(model, k, 0.0)


@pytest.mark.parametrize("k", ref.KS)
def test_reference_short_rows_end_after_n_plus_one_steps(k):
    ptr, idx, val, H, _ = ref.inputs(k)
    pair = ref.base(H, ref.LAM)
    for alpha in ref.ALPHAS:
        sol = ref.dense_solutions(ref.IMPLICIT, k, alpha)
        for u, n in ((1, 1), (2, 3), (4, 17)):
            assert ref.SIZES[u] == n
            Y, done = ref.rows(ref.IMPLICIT, ptr, idx, val, H, ref.LAM, alpha, None, n + 1, 0.0, base_pair=pair)
            y = sol[u][2]
            if not sol[u][1].any():  # the row's entries are explicit zeros: no right-hand side
                assert n == 1 and done[u] == 0 and not Y[u].any()
                continue
            assert 1 <= done[u] <= n + 1  # (fewer: the row holds explicit zeros, and gamma reached exactly 0 in fp64)
            assert np.linalg.norm(Y[u] - y) <= 1e-3 * np.linalg.norm(y), (k, alpha, n)
            if k in (160, 256) and n <= 3 and alpha == 40.0:  # what the preconditioner buys: plain CG is not there yet
                P, _ = ref.rows(ref.IMPLICIT, ptr, idx, val, H, ref.LAM, alpha, None, n + 1, 0.0, precondition=False, base_pair=pair)
                assert np.linalg.norm(P[u] - y) > 1e-3 * np.linalg.norm(y), (k, alpha, n)


def test_reference_stop_rule_counts_differ_between_rows():
    k, alpha = 160, 40.0
    ptr, idx, val, H, _ = ref.inputs(k)
    Y, done = ref.rows(ref.IMPLICIT, ptr, idx, val, H, ref.LAM, alpha, None, 64, 1e-4)
    live = ref.counting(ref.IMPLICIT, k, alpha)
    assert 1 <= done[live].min() and done[live].max() < 64 and len(set(done[live].tolist())) >= 3, done.tolist()
    # a start at the converged rows costs no step
    Y2, done2 = ref.rows(ref.IMPLICIT, ptr, idx, val, H, ref.LAM, alpha, Y, 64, 1e-4)
    assert not done2.any() and np.array_equal(Y2, Y)
