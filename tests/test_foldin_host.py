"""CPU tests of the fold-in surface (mfx_rec_fold_in_setup / mfx_rec_fold_in / mfx_rec_fold_in_times): the symbols are
exported by libmfx.so and bound in mfx._lib, the model constants match include/mfx.h, and a NULL handle is refused
without touching a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

MFX_ERR_INVALID = -1  # include/mfx.h
NAMES = ("mfx_rec_fold_in_setup", "mfx_rec_fold_in", "mfx_rec_fold_in_times")


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    return m


def test_foldin_symbols_are_exported_and_bound(mfx):
    from mfx import _lib as L
    lib = mfx.lib()
    for name in NAMES:
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert lib.mfx_version() == L.MFX_VERSION == 2
    assert callable(mfx.Recommender.fold_in_setup) and callable(mfx.Recommender.fold_in)


def test_fold_models_match_the_header(mfx):
    hdr = open(os.path.join(ROOT, "include", "mfx.h")).read()
    declared = {m: int(v) for m, v in re.findall(r"\b(MFX_FOLD_[A-Z_]+)\s*=\s*(\d+)", hdr)}
    assert declared == {"MFX_FOLD_ALS": 0, "MFX_FOLD_ALS_EXACT": 1, "MFX_FOLD_CCD": 2, "MFX_FOLD_IMPLICIT": 3}
    for name, v in declared.items():
        assert getattr(mfx, name) == v


def test_null_handle_is_invalid(mfx):
    lib = mfx.lib()
    assert lib.mfx_rec_fold_in_setup(None, mfx.MFX_FOLD_ALS, 0.1, 0.0) == MFX_ERR_INVALID
    assert "null recommender" in lib.mfx_last_error().decode()
    ptr = np.array([0, 1], np.uint32)
    idx = np.array([0], np.uint32)
    val = np.array([1.0], np.float32)
    W = np.zeros((1, 4), np.float32)
    items = np.zeros((1, 5), np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.mfx_rec_fold_in(None, 1, 1, vp(ptr), vp(idx), vp(val), vp(W), 5, vp(items), None, 0) == MFX_ERR_INVALID
    assert "null recommender" in lib.mfx_last_error().decode()
    t = (C.c_double * 3)()
    assert lib.mfx_rec_fold_in_times(None, t) == MFX_ERR_INVALID
