"""IVF retrieval (mfx_rec_ivf_*, mfx_rec_query_ivf, mfx.ivf_kmeans) without a GPU: the symbols and their bindings, the
refusal of a NULL handle, the reference of ivf_exact.py against a brute-force loop, its restatement of the library's launch
arithmetic against the kernels' loops written out, the class and the reference property that every case of
tests/test_gpu_ivf_geometry.py is meant to have, and the k-means of the Python layer."""
import ctypes as C
import inspect

import numpy as np
import pytest

import ivf_exact as gx
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


# ------------------------------------------------------------------------------------------------ the launch arithmetic
def test_launch_arithmetic_against_brute_force_loops():
    """pair_counts, work_items and scan_threads against the loops of mfx_ivf_count / _scan / _scatter written out thread by
    thread; tile_class, list_size, slots_per_launch and probe_slices against their defining properties."""
    rng = np.random.default_rng(11)
    for nlist in (1, 9, 255, 256, 257, 300, 511, 512, 513, 1030, 65535, 65536):
        sizes = rng.integers(0, 3, nlist)
        list_ptr = np.concatenate([[0], np.cumsum(sizes)])
        nprobe = min(nlist, 3)
        probes = rng.integers(0, nlist, (500, nprobe)).astype(np.uint32)
        probes[rng.random(probes.shape) < 0.2] = PAD
        probes[:300, 0] = nlist - 1 if sizes[-1] else int(np.argmax(sizes > 0))     # one list with several work items
        cnt = [0] * nlist                                     # mfx_ivf_count
        for row in probes.tolist():
            for l in row:
                if l != PAD and list_ptr[l + 1] > list_ptr[l]:
                    cnt[l] += 1
        counts = gx.pair_counts(probes, list_ptr)
        assert counts.tolist() == cnt and (sum(cnt) == 0 or max(cnt) > 128)
        per = (nlist + 255) // 256                            # mfx_ivf_scan
        rng_of = [(min(nlist, t * per), min(nlist, min(nlist, t * per) + per)) for t in range(256)]
        part = [sum((cnt[l] + 127) // 128 for l in range(l0, l1)) for l0, l1 in rng_of]
        wi_off, nwi = [None] * nlist, None
        for t, (l0, l1) in enumerate(rng_of):
            off = sum(part[:t])
            for l in range(l0, l1):
                wi_off[l] = off
                off += (cnt[l] + 127) // 128
            if t == 255:
                nwi = off
        n, first, total = gx.work_items(counts)
        assert first.tolist() == wi_off and total == nwi and n.tolist() == [(c + 127) // 128 for c in cnt]
        p, full, short, idle = gx.scan_threads(nlist)
        width = [l1 - l0 for l0, l1 in rng_of]
        assert p == per and width[:full] == [per] * full and width.count(0) == idle and sum(width) == nlist
        assert (0 < short < per and width[full] == short) if short else full + idle == 256
        # mfx_ivf_scatter: the r-th pair of list l lands in work item wi_off[l] + r / 128, place r % 128; all places distinct
        places = {(wi_off[l] + r // 128, r % 128) for l in range(nlist) for r in range(cnt[l])}
        assert len(places) == sum(cnt) and all(w < nwi for w, _ in places)
    for k in range(1, 1100):
        kc, nch = gx.tile_class(k)
        assert kc in (1, 2, 4, 8, 16, 32, 64) and 2 * kc * nch >= k > 2 * kc * (nch - 1)
        assert nch == 1 and (kc == 1 or 2 * (kc // 2) < k) if k <= 128 else kc == 64
    for n_top in range(1, 1025):
        L, lds = gx.list_size(n_top)
        assert L in (64, 128, 256, 512, 1024, 2048) and L >= n_top + 32 and (L == 64 or L // 2 < n_top + 32) and lds == (L <= 256)
        for nprobe in (1, 2, 8, 1024):
            q = gx.slots_per_launch(nprobe, n_top)
            assert q % 128 == 0 and q >= 128 and (q == 128 or q * nprobe * L * 8 <= 1 << 30 < (q + 128) * nprobe * L * 8)
            assert (q - 1) << 10 < 1 << 32
    for nlist in (1, 32, 33, 224, 225, 256, 257, 1030, 65536):
        for nusers in (1, 140, 129 * 512):
            for nprobe in (1, 3, 1024):
                for cus in (8, 256, 304):
                    s = gx.probe_slices(nlist, nusers, nprobe, cus)
                    nblkc = (nlist + 31) // 32
                    assert sum(s) == nblkc and len(s) * nprobe <= 8192 and (len(s) == 1 or len(s) <= nblkc // 4)
                    nz = [x for x in s if x]                  # equal slices, a shorter last one, then empty ones
                    assert s[:len(nz)] == nz and all(x == nz[0] for x in nz[:-1]) and nz[-1] <= nz[0]
                    assert len(s) == 1 or (len(s) - 1) * ((nusers + 127) // 128) < 2 * cus


# ------------------------------------------------------------------------------------------------ the cases of the GPU sweep
def test_tile_cases_cover_every_class():
    assert {gx.tile_class(k) for k in gx.TILE_CLASS} == {(kc, 1) for kc in (1, 2, 4, 8, 16, 32, 64)} | {(64, 2), (64, 3), (64, 8)}
    for kc in (1, 2, 4, 8, 16, 32, 64):                       # both edges of every KC
        ks = [k for k in gx.TILE_CLASS if gx.tile_class(k) == (kc, 1)]
        assert min(ks) == (2 if kc == 1 else kc + 1) and max(ks) == 2 * kc
    assert any(k % 2 for k in gx.TILE_CLASS) and {k for k, r in gx.TILE_CASES if r == "huge"} == {4, 16, 128}
    assert len(gx.TILE_CASES) == len(set(gx.TILE_CASES)) == 19


@pytest.mark.parametrize("k,regime", gx.TILE_CASES)
def test_tile_case_lands_in_its_class(k, regime):
    import mfx
    c = gx.tile_case(mfx, k, regime)
    assert np.diff(c.list_ptr.astype(np.int64)).tolist() == gx.SIZES + [600 - sum(gx.SIZES)]
    assert 250 < c.keep.sum() < 350
    if regime == "huge":
        assert np.isnan(c.S).any() and np.isinf(c.S).any()
    full = False
    for nprobe in gx.TILE_NPROBE:
        users, popular = c.batch[nprobe]
        counts = gx.pair_counts(c.probes(nprobe)[0][users], c.list_ptr)
        for n_top in gx.TILE_NTOP:
            g = gx.geometry(k, c.nlist, len(users), nprobe, n_top, counts=counts)
            assert (g.kc, g.nch) == gx.TILE_CLASS[k] and g.L == (64 if n_top == 10 else 256) and g.lds_sort
            assert g.launches == [300] and len(users) == 300 and len(set(users.tolist())) < 300
            assert counts[popular] > 128 and g.wi[popular] >= 2 and g.slices == [1] and g.per == 1 and g.idle == 247
            off, on = c.want("batch", users, nprobe, n_top), c.want("batch", users, nprobe, n_top, c.keep)
            assert (on[2] < n_top).any() and (on[2] == 0).any()           # with the filter: short unions, and empty ones
            full |= bool((on[2] >= n_top).any())
            assert (on[2] <= off[2]).all() and (on[2] < off[2]).any()
            assert not np.array_equal(on[0], off[0])
    assert full                                               # and some that fill n_top


@pytest.mark.parametrize("nprobe", [1, 3])
def test_boundary_batches_hit_the_work_item_edges(nprobe):
    import mfx
    c = gx.boundary_case(mfx)
    batches, l = gx.boundary_batches(c, nprobe)
    assert np.diff(c.list_ptr.astype(np.int64))[l] > 0
    pr = c.probes(nprobe)[0]
    assert (pr[133:] == PAD).all() and (pr[:133] != PAD).all()
    for n in (128, 129, 256, 257):
        users = batches[f"exactly_{n}"]
        counts = gx.pair_counts(pr[users], c.list_ptr)
        g = gx.geometry(8, c.nlist, len(users), nprobe, 10, counts=counts)
        assert counts[l] == n and g.wi[l] == (n + 127) // 128 and len(users) == n + 40 and (g.kc, g.nch) == (4, 1)
    counts = gx.pair_counts(pr[batches["single"]], c.list_ptr)
    assert counts[l] == 200 == counts.sum() and len(batches["single"]) == 200
    users = batches["one_each"]
    counts = gx.pair_counts(pr[users], c.list_ptr)
    assert len(users) == 257 and counts.tolist() == [int(s > 0) for s in np.diff(c.list_ptr.astype(np.int64))]
    assert gx.geometry(8, c.nlist, 257, nprobe, 10, counts=counts).nwi == 7
    if nprobe == 3:                                           # a trio user: two pairs of padding (empty lists), one with work
        assert set(pr[119].tolist()) == {0, 5, gx.NONEMPTY[0]}
        assert (pr[batches["single"]] == 0).any(1).all() and (pr[batches["single"]] == 5).any(1).all()
    want = c.want("one_each", users, nprobe, 10)
    assert ((want[0] == PAD).all(1)).sum() >= 250             # the slots without a pair are all padding


def test_long_case_fills_and_flushes_every_list_size():
    import mfx
    c = gx.long_case(mfx)
    sizes = np.diff(c.list_ptr.astype(np.int64))
    assert sizes.tolist() == gx.SIZES + [1274]
    for n_top, (L, lds) in gx.LONG_NTOP.items():
        assert gx.list_size(n_top) == (L, lds) and (L > 512 or sizes[8] > 2 * L)
    assert {gx.list_size(n)[0] for n in gx.LONG_NTOP} == {64, 128, 256, 512, 1024, 2048}
    for a, b in ((32, 33), (96, 97), (224, 225)):             # the two sides of an edge of L
        assert gx.list_size(a)[0] * 2 == gx.list_size(b)[0]
    assert gx.list_size(224)[1] and not gx.list_size(225)[1]
    for nprobe in gx.LONG_NPROBE:
        pr = c.probes(nprobe)[0]
        assert (pr == 8).any(1).sum() >= 10 and not (pr == 8).any(1).all()
        for n_top in gx.LONG_NTOP:
            assert nprobe * n_top <= 8192
            n_el = c.want("all", np.arange(gx.ROWS), nprobe, n_top)[2]
            assert (n_el < n_top).any() and ((n_el > 2 * gx.list_size(n_top)[0]).any() or n_top > 225)
    # the rising scale keeps admitting: the best of a user that probes list 8 lie late in that list
    u = int(np.nonzero((c.probes(1)[0] == 8).any(1) & (c.want("all", np.arange(gx.ROWS), 1, 32)[2] > 1000))[0][0])
    rest = c.list_idx[c.list_ptr[8]:]
    assert np.isin(c.want("all", np.arange(gx.ROWS), 1, 32)[0][u], rest[len(rest) // 2:]).sum() > 16


@pytest.mark.parametrize("nlist", list(gx.LARGE))
def test_large_case_lands_in_its_class(nlist):
    import mfx
    cols, k, shapes = gx.LARGE[nlist]
    c = gx.large_case(mfx, nlist)
    sizes = np.diff(c.list_ptr.astype(np.int64))
    users = c.users
    assert len(users) == 150 and set(users.tolist()) == set(range(gx.ROWS))
    for nprobe, n_top in shapes:
        pr = c.probes(nprobe)[0]
        counts = gx.pair_counts(pr[users], c.list_ptr)
        g = gx.geometry(k, nlist, len(users), nprobe, n_top, counts=counts)
        assert g.launches == [150] and 2 <= k <= 5
        live = nlist - len(c.dead)
        assert ((pr[:3] != PAD).sum(1) == min(2, nprobe)).all() and (pr[3] == PAD).all()    # two lists, and none
        assert ((pr[4:] != PAD).sum(1) == min(nprobe, live)).all() and not np.isin(pr, c.dead).any()
        if nprobe >= 2:
            assert np.array_equal(np.sort(pr[:3, :2], 1), np.broadcast_to(np.sort(c.hot), (3, 2)))
        want = c.want("users", users, nprobe, n_top)
        assert (want[2] < n_top).any()
        if nlist == 33:
            assert g.slices == [2] and nlist % 32 == 1 and (pr == 32).any()        # one centroid in the second tile, and probed
        if nlist == 257:
            assert (g.per, g.full, g.short, g.idle) == (2, 128, 1, 127) and g.slices == [5, 4]
            assert counts[256] >= 3                                                # the short thread's list has a work item
        if nlist == 1030:
            assert (sizes == 0).sum() > 300 and g.per == 5 and g.short == 0 and g.idle == 50
            assert g.slices == [5, 5, 5, 5, 5, 5, 3, 0] and g.pos_bits == {1: 0, 64: 6, 1024: 10}[nprobe]
            if nprobe == 1024:
                assert n_top == 8 and len(g.slices) * nprobe == 8192 == nprobe * n_top and (pr[:, 1020:] == PAD).all()
                assert (pr[4:, 1019] != PAD).all()                                 # position 1019 = 0b1111111011 holds a list
        if nlist == 65536:
            assert g.per == 256 and g.idle == 0 and g.short == 0 and len(g.slices) == 256 and set(g.slices) == {8}
            assert (sizes == 0).sum() > 4000 and sizes.max() <= 6
            union = want[2]
            assert union.max() <= 12 and (union == 0).any() and (union > 0).sum() > 100    # every row is mostly padding
        if len(g.slices) > 1:                                 # a hot list lies in the probe's second slice
            assert nlist >= 225 and 1 in {int(h) // gx.TILE // g.slices[0] for h in c.hot}
        assert (counts > 128).sum() == 0 or g.nwi > (counts > 0).sum()
    if nlist in (257, 1030):
        assert any(gx.geometry(k, nlist, 150, p, t).slices[1] > 0 for p, t in shapes)


def test_chunk_case_takes_two_launches_and_pads_in_the_second():
    g, c = gx.CHUNK, gx.chunk_case()
    geo = gx.geometry(g.k, g.nlist, g.rows, g.nprobe, g.n_top)
    assert geo.launches == [8192, 108] and geo.L == 2048 and (geo.kc, geo.nch) == (2, 1)
    assert gx.geometry(g.k, g.nlist, g.rows, 2, g.n_top).launches == [8300]
    sizes = np.diff(c.list_ptr.astype(np.int64))
    assert (sizes == 0).tolist() == [l == g.empty for l in range(g.nlist)]
    last = np.arange(8192, g.rows)
    pr, _ = expected_probe(c.W, c.Cn, last, g.nprobe)
    nan = np.array(g.nan_users) - 8192
    assert (nan >= 0).all() and (pr[nan] == PAD).all()        # pairs without a list, in the second launch
    rest = np.setdiff1d(np.arange(108), nan)
    assert (pr[rest] != PAD).all() and (pr[rest] == g.empty).any(1).all()      # and pairs with the empty list
    pr2, _ = expected_probe(c.W, c.Cn, last, 2)
    assert (pr2[rest] == g.empty).any() and not (pr2[rest] == g.empty).any(1).all()


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
