"""IVF retrieval (csrc/rec_ivf.hip, mfx_rec_ivf_probe, mfx_rec_query_ivf) at every tile class, at large list counts and at
the edges of its work items, candidate lists and launches, against the exact reference of tests/ivf_exact.py.  As in
tests/test_gpu_ivf.py every comparison is on the uint32 views of ids and score bits: there are no tolerances.

tests/test_gpu_ivf.py pins the contract (ties, padding, exclusion, filter, batch order, refusals) but in a narrow band of
shapes.  Read beside the kernels that left (BEFORE):

    code                                      run against the reference before    never before
    mfx_ivf_topn<KC, FAC>, 14 variants        KC 1, 32, 64 (nch 2), FAC off       KC 2, 4, 8, 16; every FAC variant (KC 16 only
                                                                                  against the handle's own query); KC 64 at
                                                                                  nch 1, 3, 8
    mfx_ivf_fac, the NaN at list padding      k = 24, GPU against GPU             against the reference, any KC
    mfx_ivf_scan, per = ceil(nlist / 256)     per = 1 (nlist 9; at most 64)       per 2, 5, 256; the ragged last thread; idle ones
    ivf_probe_dev, sliced probe + merge       one slice                           2, 8 and 256 slices, an empty slice
    pair = slot << 10 | probe position        positions 0 .. 8                    positions up to 1023: all ten bits
    nlist, nprobe at their bounds             nlist 64, nprobe 9                  nlist 65536, nprobe 1024
    pairs of a list: ceil(n / 128), r / 128   "more than 128"                     exactly 128, 129, 256, 257; all pairs in one
                                                                                  list; one pair in every list
    L of n_top, and the flush's sort          L 64, 256 (n_top 1, 10, 100)        L 128, 512, 1024, 2048; both sides of every
                                                                                  edge; the sort in global memory (L > 256)
    a second launch, q0 > 0                   with a user array, no padding pair  users = NULL; padding pairs (no list, and an
                                                                                  empty list) written by mfx_ivf_count at q0 > 0

AFTER (this module; the cases and the class each lands in are in tests/ivf_exact.py, and tests/test_ivf_host.py asserts
those classes and the properties of the reference outputs on the CPU):

    test_every_tile_class                     k 2 .. 1024 at both edges of every KC, nch 1, 2, 3, 8, "huge" at k 4, 16, 128;
                                              filter off, on, and off again; nprobe 1, 3; n_top 10, 100; 300 slots
    test_work_item_boundaries                 a list with exactly 128, 129, 256, 257 pairs; 200 pairs and no other; 257 slots
                                              with one pair per list; nprobe 1 and 3 (two of three pairs padding)
    test_candidate_list_sizes                 n_top 32, 33, 96, 97, 224, 225, 512, 1024 on a list of 1274 items with a rising
                                              scale; nprobe 1, 2
    test_large_list_counts                    nlist 33, 257, 1030, 65536; nprobe up to 1024; NaN centroids, users with two
                                              lists and with none; the probe, the lists and the query
    test_second_launch_without_a_user_array   8300 users, users = NULL, an empty list, NaN users among the last 108

What the sweep found: nothing.  All 34 cases pass on the MI355X against the library as it stood, bit for bit, so
rec_ivf.hip, recommend.hip and rec_tiles.hpp are unchanged.  The paths listed under "never before" ran here against a
reference for the first time, among them a probe slice past the last centroid tile (nlist 1030: 33 tiles in 8 slices of
5 leave the eighth empty; it writes padding and the merge drops it).  That the cases would notice was tried on five scratch
builds (never committed) that each only skip work, tests/test_gpu_ivf.py (36 cases) and this module once each per build:
    mfx_ivf_scan handles only the first list of each      test_gpu_ivf.py passes (per = 1 everywhere); here
    thread                                                test_large_list_counts fails at nlist 257, 1030, 65536 (3 of 4)
    the sliced probe admits nothing in slice 1            test_gpu_ivf.py passes (the probe is never sliced); here
                                                          test_large_list_counts fails at 257 and 1030 (65536 passed: nobody
                                                          probed the 256 lists of slice 1; since then one of the two lists
                                                          that users 0 .. 2 probe is list 300, inside it)
    mfx_ivf_topn<4, true> is never launched: KC = 4       test_gpu_ivf.py passes (its filter runs at KC = 16); here
    ignores the item filter                               test_every_tile_class fails at k = 5 and 8 (2 of 19)
    a list of more than 128 pairs gets                    test_gpu_ivf.py fails test_query_against_the_exact_reference (12 of
    floor((pairs + 126) / 128) work items: one too few    12: its batch of 129 slots at nprobe = nlist puts 129 pairs in every
    at 129 and 257                                        list); here test_work_item_boundaries (2 of 2), one tile class and
                                                          the second launch fail
    mfx_ivf_fac writes 1 instead of NaN at a list's       both modules pass, and no case can fail: a padding position lies at
    padding positions                                     or above the list's item count, and the admission compares the
                                                          position with that count before it looks at the key, so the factor
                                                          there is never seen.  The NaN is a second line of defence only.

Wall time on the MI355X (pytest --durations=0; every reference is computed once, in the first case that needs it, and its
time is in that case): the slowest case is test_large_list_counts[65536] at 1.3 s (the reference probe over 65536
centroids), then test_every_tile_class[1024-normal] at 0.4 s (the 1024 fma steps of the reference) and [2-normal] at 0.2 s;
every other case takes 0.15 s or less, the whole module 4 s.  Run alone it pays another 12 s once for the import of torch
and its start on the device, which the suite has paid before this module.
"""
import numpy as np
import pytest

import ivf_exact as gx
from rec_exact import PAD, chain_scores
from test_gpu_ivf import assert_exact, host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1, m.lib().mfx_last_error()
    return m


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------------------------------------ a. every tile class
@pytest.mark.parametrize("k,regime", gx.TILE_CASES)
def test_every_tile_class(mfx, cus, k, regime):
    c = gx.tile_case(mfx, k, regime)
    assert gx.tile_class(k) == gx.TILE_CLASS[k]
    with mfx.Recommender(c.W, c.H, 1, exclude=c.ex) as r:
        r.ivf_setup(c.assign, c.Cn)                                       # the filter is set after the setup
        for keep in (None, c.keep):
            r.set_item_filter(keep)
            for nprobe in gx.TILE_NPROBE:
                users, popular = c.batch[nprobe]
                assert (c.probes(nprobe)[0][users] == popular).sum() > 128   # several work items for one list
                assert gx.geometry(k, c.nlist, len(users), nprobe, 10, cus).slices == [1]
                for n_top in gx.TILE_NTOP:
                    want = c.want("batch", users, nprobe, n_top, keep)
                    if keep is not None:
                        assert (want[2] < n_top).any() and (want[2] == 0).any()
                    assert_exact(r.query_ivf(n_top, nprobe, users), want[:2],
                                 f"k {k} {regime} filter {keep is not None} nprobe {nprobe} n_top {n_top}")
        r.set_item_filter(None)                                           # and taken off again
        users, _ = c.batch[3]
        assert_exact(r.query_ivf(10, 3, users), c.want("batch", users, 3, 10)[:2], f"k {k} {regime} filter removed")


# ------------------------------------------------------------------------------------------------ b. work-item boundaries
@pytest.mark.parametrize("nprobe", [1, 3])
def test_work_item_boundaries(mfx, nprobe):
    c = gx.boundary_case(mfx)
    batches, l = gx.boundary_batches(c, nprobe)
    pr = c.probes(nprobe)[0]
    for n in (128, 129, 256, 257):
        assert gx.pair_counts(pr[batches[f"exactly_{n}"]], c.list_ptr)[l] == n
    with mfx.Recommender(c.W, c.H, 1, exclude=c.ex) as r:
        r.ivf_setup(c.assign, c.Cn)
        for name, users in batches.items():
            assert_exact(r.ivf_probe(nprobe, users), tuple(x[users] for x in c.probes(nprobe)), f"probe, batch {name}, nprobe {nprobe}")
            assert_exact(r.query_ivf(10, nprobe, users), c.want(name, users, nprobe, 10)[:2], f"batch {name}, nprobe {nprobe}")


# ------------------------------------------------------------------------------------------------ c. candidate-list sizes
@pytest.mark.parametrize("n_top", list(gx.LONG_NTOP))
def test_candidate_list_sizes(mfx, n_top):
    c = gx.long_case(mfx)
    assert gx.list_size(n_top) == gx.LONG_NTOP[n_top]
    users = np.arange(gx.ROWS)
    with mfx.Recommender(c.W, c.H, 1, exclude=c.ex) as r:
        r.ivf_setup(c.assign, c.Cn)
        for nprobe in gx.LONG_NPROBE:
            assert (c.probes(nprobe)[0] == 8).any()                       # the long list is probed
            assert_exact(r.query_ivf(n_top, nprobe), c.want("all", users, nprobe, n_top)[:2], f"n_top {n_top} nprobe {nprobe}")


# ------------------------------------------------------------------------------------------------ d. large list counts
@pytest.mark.parametrize("nlist", list(gx.LARGE))
def test_large_list_counts(mfx, cus, nlist):
    cols, k, shapes = gx.LARGE[nlist]
    c = gx.large_case(mfx, nlist)
    users = c.users
    per, full, short, idle = gx.scan_threads(nlist)
    assert (per, full, short, idle) == {33: (1, 33, 0, 223), 257: (2, 128, 1, 127), 1030: (5, 206, 0, 50), 65536: (256, 256, 0, 0)}[nlist]
    with mfx.Recommender(c.W, c.H, 1) as r:
        r.ivf_setup(c.assign, c.Cn)
        ptr, idx = r.ivf_lists()
        assert np.array_equal(ptr, c.list_ptr) and np.array_equal(idx, c.list_idx)
        for nprobe, n_top in shapes:
            g = gx.geometry(k, nlist, len(users), nprobe, n_top, cus)
            if nlist >= 257:                                              # (256 CUs: 2, 8 and 256 slices)
                assert len(g.slices) >= 2 and g.slices[1] > 0, (cus, g.slices)
                assert 1 in {int(h) // gx.TILE // g.slices[0] for h in c.hot}      # a hot list in the second slice
            else:
                assert g.slices == [2]
            want = c.probes(nprobe)
            assert (want[0][:4] == PAD).any()                             # users with fewer lists than nprobe
            assert_exact(r.ivf_probe(nprobe, users), tuple(x[users] for x in want), f"probe nlist {nlist} nprobe {nprobe}")
            assert_exact(r.ivf_probe(nprobe), want, f"probe of every user, nlist {nlist} nprobe {nprobe}")
            assert_exact(r.query_ivf(n_top, nprobe, users), c.want("users", users, nprobe, n_top)[:2],
                         f"nlist {nlist} nprobe {nprobe} n_top {n_top}")


# ------------------------------------------------------------------------------------------------ e. the second launch
def test_second_launch_without_a_user_array(mfx):
    g, c = gx.CHUNK, gx.chunk_case()
    assert gx.geometry(g.k, g.nlist, g.rows, g.nprobe, g.n_top).launches == [8192, 108]
    nan = np.array(g.nan_users)
    last = np.arange(8192, g.rows)
    with mfx.Recommender(c.W, c.H, 1) as r:
        r.ivf_setup(c.assign, c.Cn)
        ptr, idx = r.ivf_lists()
        assert np.array_equal(ptr, c.list_ptr) and ptr[g.empty] == ptr[g.empty + 1]
        qi, qs = r.query(g.n_top)
        assert (qi[nan] == PAD).all() and np.isneginf(qs[nan]).all()       # a NaN user: all padding
        first = r.query_ivf(g.n_top, g.nprobe)                            # users = NULL, two launches
        assert_exact(first, (qi, qs), "two launches, users = NULL")
        # the slots of the second launch against the CPU reference as well (every list probed: the top of all 200 items)
        S = chain_scores(c.W, c.H, last)
        pr = gx.expected_probe(c.W, c.Cn, last, g.nprobe)[0]
        assert (pr == PAD).any() and (pr == g.empty).any()
        want = gx.expected_query(S, pr, c.list_ptr, c.list_idx, True, g.n_top)
        assert_exact((first[0][8192:], first[1][8192:]), want[:2], "the second launch against the reference")
        # one launch, nprobe = 2: query_candidates on the unions
        probes, _ = r.ivf_probe(2)
        assert (probes[nan] == PAD).all() and (probes == g.empty).any()
        cp, ci = gx.union_lists(probes, ptr, idx)
        assert_exact(r.query_ivf(g.n_top, 2), r.query_candidates(g.n_top, (cp, ci), canonical=True)[:2], "one launch, nprobe 2")
        # the rows in reverse as an explicit array: slot s is row 8299 - s
        rev = np.arange(g.rows)[::-1].copy()
        got = r.query_ivf(g.n_top, g.nprobe, rev)
        assert_exact(got, (host(first[0])[::-1], host(first[1])[::-1]), "two launches, reversed user array")
