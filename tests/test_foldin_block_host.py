"""The ABI of fold-in by block subspace sweeps (mfx_rec_fold_in_block_setup / mfx_rec_fold_in_warm) without a GPU: the
symbols, their bindings, the refusal of a NULL handle and the Python surface."""
import ctypes as C
import inspect

import numpy as np

MFX_ERR_INVALID = -1  # include/mfx.h
NEW = ("mfx_rec_fold_in_block_setup", "mfx_rec_fold_in_warm")


def test_symbols_are_exported_and_bound():
    import mfx
    from mfx import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        res, args = _lib.SIGNATURES[name]
        fn = getattr(mfx.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert len(_lib.SIGNATURES["mfx_rec_fold_in_block_setup"][1]) == 6
    assert len(_lib.SIGNATURES["mfx_rec_fold_in_warm"][1]) == 13


def test_the_abi_revision_is_still_2():
    import mfx
    from mfx import _lib
    assert mfx.lib().mfx_version() == 2 == _lib.MFX_VERSION


def test_a_null_handle_is_refused():
    import mfx
    lib = mfx.lib()
    assert lib.mfx_rec_fold_in_block_setup(None, 0.1, 1.0, 0, 8, 0.0) == MFX_ERR_INVALID
    assert "null recommender" in lib.mfx_last_error().decode()
    ptr = np.zeros(2, np.uint32)
    W = np.zeros((1, 4), np.float32)
    done = np.zeros(1, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.mfx_rec_fold_in_warm(None, 1, 0, vp(ptr), None, None, None, vp(W), vp(done), 0, None, None, 0) == MFX_ERR_INVALID
    assert "null recommender" in lib.mfx_last_error().decode()


def test_the_python_methods_and_keywords_exist():
    import mfx
    setup = inspect.signature(mfx.Recommender.fold_in_block_setup).parameters
    assert list(setup) == ["self", "lam", "alpha", "block", "sweeps", "tol"]
    assert (setup["block"].default, setup["sweeps"].default, setup["tol"].default) == (0, 8, 0.0)
    fold = inspect.signature(mfx.Recommender.fold_in).parameters
    assert list(fold) == ["self", "rows", "n_top", "on_device", "W_init", "return_sweeps"]
    assert fold["W_init"].default is None and fold["return_sweeps"].default is False
