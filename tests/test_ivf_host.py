"""IVF retrieval (mfx_rec_ivf_*, mfx_rec_query_ivf, mfx.ivf_kmeans) without a GPU: the symbols and their bindings, the
refusal of a NULL handle, the reference of ivf_exact.py against a brute-force loop, and the k-means of the Python layer."""
import ctypes as C
import inspect

import numpy as np
import pytest

from ivf_exact import expected_probe, expected_query, lists_of, union_lists
from rec_exact import PAD, chain_scores

MFX_ERR_INVALID = -1  # include/mfx.h
F32 = np.float32


def test_symbols_are_exported_with_the_declared_argument_types():
    import mfx
    from mfx import _lib
    lib = mfx.lib()
    raw = C.CDLL(_lib.LIB_PATH)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    want = {
        "mfx_rec_ivf_setup": [vp, i32, vp, vp, C.c_int],
        "mfx_rec_ivf_lists": [vp, vp, vp, C.c_int],
        "mfx_rec_ivf_probe": [vp, i64, vp, i32, vp, vp, C.c_int],
        "mfx_rec_query_ivf": [vp, i64, vp, i32, i32, vp, vp, C.c_int],
        "mfx_rec_ivf_times": [vp, C.POINTER(C.c_double)],
    }
    for name, args in want.items():
        assert hasattr(raw, name), name
        res, got = _lib.SIGNATURES[name]
        assert res is C.c_int and list(got) == args, name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert lib.mfx_version() == 2 == _lib.MFX_VERSION


def test_a_null_handle_is_refused():
    import mfx
    lib = mfx.lib()
    u = np.zeros(4, np.uint32)
    f = np.zeros(4, F32)
    t = (C.c_double * 4)()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for rc in (lib.mfx_rec_ivf_setup(None, 1, vp(u), vp(f), 0), lib.mfx_rec_ivf_lists(None, vp(u), vp(u), 0),
               lib.mfx_rec_ivf_probe(None, 1, None, 1, vp(u), vp(f), 0), lib.mfx_rec_query_ivf(None, 1, None, 1, 1, vp(u), vp(f), 0),
               lib.mfx_rec_ivf_times(None, t)):
        assert rc == MFX_ERR_INVALID
        assert "null recommender" in lib.mfx_last_error().decode()


def test_the_python_functions_exist():
    import mfx
    R = mfx.Recommender
    assert list(inspect.signature(mfx.ivf_kmeans).parameters) == ["H", "nlist", "iters", "seed"]
    assert [p.default for p in list(inspect.signature(mfx.ivf_kmeans).parameters.values())[2:]] == [10, 0]
    assert list(inspect.signature(R.ivf_setup).parameters) == ["self", "assign", "centroids"]
    assert list(inspect.signature(R.ivf_build).parameters) == ["self", "H", "nlist", "iters", "seed"]
    assert list(inspect.signature(R.ivf_lists).parameters) == ["self"]
    assert list(inspect.signature(R.ivf_probe).parameters) == ["self", "nprobe", "users", "on_device"]
    assert list(inspect.signature(R.query_ivf).parameters) == ["self", "n_top", "nprobe", "users", "on_device"]
    assert list(inspect.signature(R.ivf_times).parameters) == ["self"]


# ------------------------------------------------------------------------------------------------ the reference
def fma32(a, b, c):
    """One fp32 fma through fp64: exact for the small integers of the brute-force case."""
    return F32(np.float64(a) * np.float64(b) + np.float64(c))


def test_reference_against_a_brute_force_loop():
    rng = np.random.default_rng(3)
    U, cols, k, nlist, nprobe, n_top = 6, 20, 3, 4, 2, 5
    W = rng.integers(-2, 3, (U, k)).astype(F32)           # small integers: many ties, every sum exact
    H = rng.integers(-2, 3, (cols, k)).astype(F32)
    Cn = rng.integers(-2, 3, (nlist, k)).astype(F32)
    Cn[3, 0] = np.nan                                     # a list that is never probed
    assign = rng.integers(0, nlist, cols)
    assign[assign == 2] = 1                               # list 2 is empty
    eligible = rng.random((U, cols)) < 0.8
    users = np.array([4, 0, 5, 5, 2, 1])
    list_ptr, list_idx = lists_of(assign, nlist)
    for l in range(nlist):
        assert list_idx[list_ptr[l]:list_ptr[l + 1]].tolist() == [i for i in range(cols) if assign[i] == l]
    probes, pscores = expected_probe(W, Cn, users, nprobe)
    S = chain_scores(W, H, users)
    items, scores, n_el = expected_query(S, probes, list_ptr, list_idx, eligible, n_top)
    ptr, idx = union_lists(probes, list_ptr, list_idx)
    for s, u in enumerate(users):
        sc = []
        for l in range(nlist):
            acc = F32(0)
            for t in range(k):
                acc = fma32(W[u, t], Cn[l, t], acc)
            if not np.isnan(acc):
                sc.append((-float(acc), l))
        sc.sort()
        want = [l for _, l in sc[:nprobe]] + [PAD] * (nprobe - len(sc[:nprobe]))
        assert probes[s].tolist() == want
        assert 3 not in probes[s]
        cand = sorted(i for i in range(cols) if assign[i] in want)
        assert idx[ptr[s]:ptr[s + 1]].tolist() == cand
        best = []
        for i in cand:
            acc = F32(0)
            for t in range(k):
                acc = fma32(W[u, t], H[i, t], acc)
            if eligible[s, i]:
                best.append((-float(acc) + 0.0, i))
        best.sort()
        assert n_el[s] == len(best)
        got = items[s].tolist()
        assert got == [i for _, i in best[:n_top]] + [PAD] * (n_top - len(best[:n_top]))
        assert [float(x) for x in scores[s][:len(best[:n_top])]] == [-(v) for v, _ in best[:n_top]]
    assert (probes == PAD).sum() == 0 and (pscores > -np.inf).all()
    full, _ = expected_probe(W, Cn, users, nlist)          # the NaN list leaves one padding slot per user
    assert ((full == PAD).sum(1) == 1).all()


# ------------------------------------------------------------------------------------------------ ivf_kmeans on numpy
def test_kmeans_types_shapes_ranges_and_determinism():
    import mfx
    rng = np.random.default_rng(0)
    cols, k, nlist = 700, 9, 13
    H = rng.standard_normal((cols, k)).astype(F32)
    a, c = mfx.ivf_kmeans(H, nlist, iters=4, seed=5)
    assert a.dtype == np.uint32 and a.shape == (cols,) and a.max() < nlist
    assert c.dtype == np.float32 and c.shape == (nlist, k) and np.isfinite(c).all()
    a2, c2 = mfx.ivf_kmeans(H.copy(), nlist, iters=4, seed=5)
    assert a.tobytes() == a2.tobytes() and c.tobytes() == c2.tobytes()
    a3, c3 = mfx.ivf_kmeans(H, nlist, iters=4, seed=6)
    assert c.tobytes() != c3.tobytes()
    a0, c0 = mfx.ivf_kmeans(H, nlist, iters=0, seed=5)    # no update: the centroids are nlist distinct rows of H
    rows = {r.tobytes() for r in H}
    assert all(r.tobytes() in rows for r in c0) and len({r.tobytes() for r in c0}) == nlist
    for bad in (0, cols + 1):
        with pytest.raises(ValueError):
            mfx.ivf_kmeans(H, bad)
    with pytest.raises(ValueError):
        mfx.ivf_kmeans(H[0], 1)


def test_kmeans_empty_clusters_survive():
    import mfx
    rng = np.random.default_rng(1)
    base = rng.standard_normal((10, 4)).astype(F32)
    H = np.repeat(base, 3, axis=0)                         # 30 rows, every row three times
    a, c = mfx.ivf_kmeans(H, 30, iters=3, seed=2)          # nlist = cols: every row starts as a centroid
    counts = np.bincount(a, minlength=30)
    assert (counts == 0).sum() == 20 and sorted(counts[counts > 0].tolist()) == [3] * 10   # ties go to the lowest list id
    assert c.shape == (30, 4) and np.isfinite(c).all()     # the emptied clusters kept their centroids
    assert {r.tobytes() for r in c} == {r.tobytes() for r in base}


@pytest.mark.parametrize("k,nlist", [(1, 3), (16, 8), (130, 40)])
def test_kmeans_assignment_belongs_to_the_returned_centroids(k, nlist):
    import mfx
    rng = np.random.default_rng(k)
    cols = 900
    H = (rng.standard_normal((cols, k)) + 3.0 * rng.standard_normal((7, k))[rng.integers(0, 7, cols)]).astype(F32)
    a, c = mfx.ivf_kmeans(H, nlist, iters=5, seed=0)
    h, cc = H.astype(np.float64), c.astype(np.float64)
    d = ((h[:, None, :] - cc[None, :, :]) ** 2).sum(2)
    # the fp32 rounding of the distance, not a quality margin
    slack = 4 * k * 2.0 ** -24 * (np.sqrt((h * h).sum(1)) + np.sqrt((cc * cc).sum(1)).max()) ** 2
    assert (d[np.arange(cols), a] <= d.min(1) + slack).all()
