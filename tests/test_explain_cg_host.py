"""Explanations by conjugate gradients without a GPU: the ABI of mfx_rec_explain_cg, the Python surface, and the fp64 reference
of tests/explain_cg_ref.py pinned on the inputs of tests/test_gpu_explain_cg.py -- every numerical condition that the GPU tests
put on the library must hold for the reference itself on exactly those inputs.

What the reference does there (asserted below, printed as `explcg-reference` lines): with steps = 64, tol = 1e-5 every live
pair stops before the cap -- implicit k = 37 ... 256 after at most 27 steps and k = 1024 after 34, ALS k = 160 / 256 after
31 / 37, CCD after 6 -- within 2.8e-5 of the dense solve of A_q z = h_t, with a backward error of at most 3.9e-6, and the split
<b, z> = <h_t, w> holds to 1.3e-6 of the bracket of the GPU test; the condition numbers are at most 40.3 up to k = 256 and
144.1 at k = 1024.  Asserted are the bounds of the GPU tests: fewer than 64 steps, relative error <= 1e-3, backward error
<= 3e-5, the split gap <= 3e-5 of its bracket, the condition gate of 1e3 skipping nothing."""
import ctypes as C
import inspect

import numpy as np
import pytest

import explain_cg_ref as xr
import foldin_cg_ref as ref

MFX_ERR_INVALID = -1  # include/mfx.h
NEW = "mfx_rec_explain_cg"


def test_the_symbol_is_exported_and_bound():
    import mfx
    from mfx import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, NEW)
    assert NEW in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[NEW]
    vp = C.c_void_p
    assert res is C.c_int
    assert list(args) == [vp, C.c_int64, C.c_int64, vp, vp, vp, C.c_int32, vp, C.c_int32, vp, vp, vp, vp, vp, vp, vp, C.c_int]
    fn = getattr(mfx.lib(), NEW)
    assert fn.restype is res and list(fn.argtypes) == list(args)
    assert mfx.lib().mfx_version() == 2 == _lib.MFX_VERSION


def test_a_null_handle_is_refused():
    import mfx
    lib = mfx.lib()
    assert lib.mfx_rec_explain_cg(None, 1, 0, None, None, None, 1, None, 0, None, None, None, None, None, None, None, 0) == MFX_ERR_INVALID
    assert "null handle" in lib.mfx_last_error().decode()


def test_the_python_method_and_its_keywords():
    import mfx
    par = inspect.signature(mfx.Recommender.explain_cg).parameters
    assert list(par) == ["self", "rows", "targets", "n_expl", "on_device", "return_W", "return_Z", "return_steps", "max_ws_bytes"]
    assert (par["n_expl"].default, par["on_device"].default, par["return_W"].default, par["return_Z"].default,
            par["return_steps"].default, par["max_ws_bytes"].default) == (10, False, False, False, False, 1 << 30)
    old = inspect.signature(mfx.Recommender.explain).parameters  # unchanged
    assert list(old) == ["self", "rows", "targets", "n_expl", "on_device", "return_W", "return_Z", "max_ws_bytes"]


def test_the_targets():
    for k in ref.KS:
        ptr, idx, _, H, _ = ref.inputs(k)
        tg = xr.targets(k)
        assert tg.shape == (len(ref.SIZES), xr.T) and tg.dtype == np.uint32
        assert (tg[:, 4] == xr.PAD).all() and (tg[:, :4] < ref.COLS).all()
        for u, n in enumerate(ref.SIZES):
            assert n == 0 or tg[u, 0] == idx[ptr[u]]
        Hz, tz = xr.zero_target(k)
        assert not Hz[xr.ZERO_ITEM].any() and H[xr.ZERO_ITEM].any() and tz[xr.ZERO_AT] == xr.ZERO_ITEM
        assert (np.delete(Hz, xr.ZERO_ITEM, 0) == np.delete(H, xr.ZERO_ITEM, 0)).all()
        assert ref.SIZES[xr.ZERO_AT[0]] > 0 and (tz != tg).sum() == 1


def _converged(model, k, alpha):
    ptr, idx, val, H, _ = ref.inputs(k)
    if model != ref.IMPLICIT:
        val = ref.explicit_values(val)
    pair = ref.base(H, ref.LAM) if model == ref.IMPLICIT else None
    tg = xr.targets(k)
    W, _ = ref.rows(model, ptr, idx, val, H, ref.LAM, alpha, None, 64, 1e-5, base_pair=pair)
    Z, done = xr.solve(model, ptr, idx, val, H, ref.LAM, alpha, tg, 64, 1e-5, base_pair=pair)
    live = xr.live_pairs(model, k, alpha, tg)
    assert live.sum() >= 4 * (len([n for n in ref.SIZES if n]) - 2)
    assert (done[live] >= 1).all() and (done[live] < 64).all(), (model, k, alpha, done.tolist())
    assert not done[~live].any() and not Z[~live].any()
    rel, be, gap, cn = xr.errors(model, k, alpha, tg, Z, W, H)
    print(f"explcg-reference model={model} k={k} alpha={alpha} most_steps={int(done.max())} worst_rel={rel:.3e} worst_backward={be:.3e} "
          f"worst_split_gap={gap:.3e} worst_cond={cn:.1f}")
    assert cn <= 1e3, (model, k, alpha, cn)  # the gate may skip no row
    assert rel <= 1e-3 and be <= 3e-5 and gap <= 3e-5, (model, k, alpha, rel, be, gap)
    # the zero target: no system, the other pairs untouched by it
    Hz, tz = xr.zero_target(k)
    Zz, dz = xr.solve(model, ptr, idx, val, Hz, ref.LAM, alpha, tz, 1, 0.0)
    assert dz[xr.ZERO_AT] == 0 and not Zz[xr.ZERO_AT].any() and dz[xr.ZERO_AT[0], 0] == 1


@pytest.mark.parametrize("alpha", ref.ALPHAS)
@pytest.mark.parametrize("k", ref.KS)
def test_reference_converged_targets(k, alpha):
    _converged(ref.IMPLICIT, k, alpha)


@pytest.mark.parametrize("k", [160, 256])
@pytest.mark.parametrize("model", [ref.ALS, ref.CCD])
def test_reference_explicit_models(model, k):
    _converged(model, k, 0.0)


def test_reference_stop_rule_counts_differ_between_pairs():
    k, alpha = 160, 40.0
    ptr, idx, val, H, _ = ref.inputs(k)
    tg = xr.targets(k)
    _, done = xr.solve(ref.IMPLICIT, ptr, idx, val, H, ref.LAM, alpha, tg, 64, 1e-4)
    live = xr.live_pairs(ref.IMPLICIT, k, alpha, tg)
    assert 1 <= done[live].min() and done[live].max() < 64 and len(set(done[live].tolist())) >= 3, done.tolist()
