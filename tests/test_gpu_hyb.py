"""GPU tests of hybrid BPR training (mfx_hyb_*) against the exact reference of tests/hyb_exact.py: every comparison of
tables and embeddings is bit for bit and every count exact, because the contract of include/mfx.h fixes each fp32
operation and its order, and the sums of a step are integer sums at both levels (slots -> rows, rows -> features)."""
import ctypes as C
import functools

import numpy as np
import pytest

import bpr_exact as bx
import hyb_exact as hx

pytestmark = pytest.mark.gpu

MFX_ERR_INVALID = -1  # include/mfx.h
F = np.float32
KEYS = ("slots", "skipped", "bad", "correct")
# the caps of the new kernels (csrc/hybrid.hip), restated for the tests that make each loop take a second turn
MAX_GRID, THREADS, IN_FLIGHT = 4096, 256, 8


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1
    return m


@pytest.fixture(scope="module")
def R():
    return bx.small_matrix()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def counts(rep):
    return [rep[key] for key in KEYS]


def _params(mfx, k, lam):
    p = mfx.parameter()
    p.k, p.lambda_ = k, lam
    return p


def _gs(k):
    gs = 1
    while gs < 64 and gs < k:
        gs *= 2
    return gs


@functools.lru_cache(maxsize=None)
def _small_features():
    """The features of the operator tests on bx.small_matrix() (60 x 40).  Users: identity + up to 3 of 3 tags, normalised.
    Items: 1 .. 3 of 7 shared tags and no identity, so every item feature is shared by several rows and by both item roles."""
    import mfx
    rng = np.random.default_rng(23)
    rows, cols = 60, 40
    tr = np.repeat(np.arange(rows), 3)
    tt = rng.integers(0, 3, tr.size)  # (repeats collapse: 1 .. 3 tags a user)
    Fu = mfx.hyb_features(rows, tr, tt, 3)
    ir = np.repeat(np.arange(cols), 3)
    it = rng.integers(0, 7, ir.size)
    Fi = mfx.hyb_features(cols, ir, it, 7, identity=False)
    assert Fu.nf == 63 and Fi.nf == 7 and np.diff(Fi.ptr.astype(np.int64)).min() >= 1
    assert np.bincount(Fi.idx, minlength=7).min() >= 2
    return Fu, Fi


def _check_apply(mfx, rows, cols, Fu, Fi, Eu, Ei, u, i, j, lr, lam, skipped=None):
    """hyb_apply against the reference: the tables and the four counts; returns the reference's result."""
    ref = hx.step(hx.identity(rows) if Fu is None else Fu, hx.identity(cols) if Fi is None else Fi, Eu, Ei, u, i, j, skipped, lr, lam)
    Gu, Gi, rep = mfx.hyb_apply(rows, cols, Eu, Ei, u, i, j, lr, lam, user_features=Fu, item_features=Fi, skipped=skipped)
    assert counts(rep) == ref[2], (counts(rep), ref[2])
    assert same_bits(Gu, ref[0]), int((bits(Gu) != bits(ref[0])).sum())
    assert same_bits(Gi, ref[1]), int((bits(Gi) != bits(ref[1])).sum())
    return ref


# ------------------------------------------------------------------------------------------------ the embedding
EMBED_LENGTHS = (0, 1, 2, 63, 64, 65, 1023, 1024, 1, 3)


@functools.lru_cache(maxsize=None)
def _embed_matrix():
    """Rows of 0, 1, 2, 63, 64, 65, 1023 and 1024 entries over 1100 features; values in [-1, 1] with -1, 0, 1 and small
    negatives planted; row 8 is the single entry (feature 7, 1) and row 9 starts with a value 0."""
    rng = np.random.default_rng(41)
    nf = 1100
    rows, ids, vals = [], [], []
    for r, n in enumerate(EMBED_LENGTHS):
        f = sorted(rng.choice(nf, n, replace=False).tolist())
        v = (rng.random(n) * 2 - 1).astype(F)
        if n >= 63:
            v[:6] = [-1.0, 0.0, 1.0, -1e-30, -3e-5, -0.0]
        if r == 8:
            f, v = [7], np.ones(1, F)
        if r == 9:
            v[0] = 0.0
        rows += [r] * n
        ids += f
        vals += v.tolist()
    return hx.features(len(EMBED_LENGTHS), nf, rows, ids, vals)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1024])
def test_embed_bit_for_bit(mfx, k):
    """Every lane-group width (k = 1, 2, 3, 4, 31 .. 33, 63, 64), the three coordinate widths of k_hyb_embed (k <= 64, <= 128,
    above) and rows on either side of a group's batch of entries (64 at k >= 33) and of the row limit.  Row 8 names feature 7,
    whose table row is all -0, with the value 1: the chain starts from the first product, so -0 comes through."""
    Fm = _embed_matrix()
    E = np.random.default_rng(k).standard_normal((Fm.nf, k)).astype(F)
    E[7] = F(-0.0)
    E[::5, 0] = F(-0.0)
    want = hx.embed(Fm, E)
    got = mfx.hyb_embed(Fm, E)
    assert same_bits(got, want), int((bits(got) != bits(want)).sum())
    assert np.all(bits(got[0]) == 0)                      # the empty row: +0
    assert np.all(bits(got[8]) == 0x80000000)             # -0 handed through
    assert same_bits(got[8], E[7]) and not same_bits(got[3], got[4])


def test_embed_refuses_a_row_of_1025_entries_with_its_number(mfx):
    nf = 1100
    rows = [0] * 3 + [2] * 1025 + [3] * 1024
    ids = [1, 2, 3] + list(range(1025)) + list(range(1024))
    Fm = hx.features(4, nf, rows, ids, np.full(len(rows), 0.5, F))
    with pytest.raises(mfx.MfxError, match="row 2 of the given features"):
        mfx.hyb_embed(Fm, np.zeros((nf, 3), F))


# ------------------------------------------------------------------------------------------------ the operator
@pytest.mark.parametrize("n", [1, 65, 1000])
@pytest.mark.parametrize("k", [1, 4, 64, 65, 129])
def test_apply_bit_for_bit(mfx, R, k, n):
    Fu, Fi = _small_features()
    rng = np.random.default_rng(1000 * k + n)
    Eu, Ei = hx.initial_tables(Fu.nf, Fi.nf, k, k + n)
    Eu *= F(8.0)  # scores of a few units: the sigmoid away from 1/2
    Ei *= F(8.0)
    lr, lam = 0.05, 0.01

    # a random batch, caller skip flags on a fifth of the slots, item 5 as the positive of some slots and the sampled item
    # of others, an i == j slot and a triple named three times
    u = rng.integers(0, R.rows, n)
    i = rng.integers(0, R.cols - 5, n)
    j = rng.integers(0, R.cols - 5, n)
    i[::3] = 5
    j[1::3] = 5
    skipped = rng.random(n) < 0.2
    if n >= 65:
        j[2], skipped[2] = i[2], False
        for t in (11, 12):
            u[t], i[t], j[t], skipped[t] = u[10], i[10], j[10], False
        skipped[10] = False
    ref = _check_apply(mfx, R.rows, R.cols, Fu, Fi, Eu, Ei, u, i, j, lr, lam, skipped)
    assert ref[2][1] == int(skipped.sum()) and ref[2][2] == 0
    if not skipped.all():
        assert not same_bits(ref[0], Eu) and not same_bits(ref[1], Ei)

    # lr = 0: every bit stays
    z = _check_apply(mfx, R.rows, R.cols, Fu, Fi, Eu, Ei, u, i, j, 0.0, lam, skipped)
    assert same_bits(z[0], Eu) and same_bits(z[1], Ei)

    if n >= 65:
        # a slot with a term >= 64 is counted bad: user 59's own feature is huge, so is g * W[u][0] of its slot (d = 0: g = 1/2)
        Eb = Eu.copy()
        Eb[R.rows - 1, 0] = 1e6
        ub, ib, jb = u.copy(), i.copy(), j.copy()
        ub[0], ib[0], jb[0] = R.rows - 1, R.cols - 1, R.cols - 1
        ref = _check_apply(mfx, R.rows, R.cols, Fu, Fi, Eb, Ei, ub, ib, jb, lr, lam)
        assert ref[2][2] >= 1 and ref[2][1] == 0

        # the order of the slots plays no part
        a = mfx.hyb_apply(R.rows, R.cols, Eu, Ei, u, i, j, lr, lam, user_features=Fu, item_features=Fi, skipped=skipped)
        for seed in (1, 2):
            o = np.random.default_rng(seed).permutation(n)
            b = mfx.hyb_apply(R.rows, R.cols, Eu, Ei, u[o], i[o], j[o], lr, lam, user_features=Fu, item_features=Fi, skipped=skipped[o])
            assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and counts(a[2]) == counts(b[2])


@pytest.mark.parametrize("k", [64, 3])
def test_one_feature_carried_by_every_row(mfx, k):
    """The contention shape: 5 000 items that all carry feature 0 beside their own (values 1/2), 300 users of the identity, one
    step of 2^14 slots.  Every counted slot adds to feature 0's accumulator row twice and to its count twice, from many
    workgroups at once.  m_f is no output of the operator; it enters every element of the updated row through
    fp32(lambda * fp32(m_f)): with lambda = 0.01 and m_0 about 26 000 the factor is about 260, and one counted row more or less
    changes it by 0.01, which moves old * factor by 1e-3 relative to a sum of magnitude below 100 -- thousands of ulps.  The
    reference's own m_f is checked against the slot counts.
    At k = 64 the 3 * 2^14 (slot, role) pairs are 49 152 groups of a wave against 4 096 workgroups of 4: the walk through the
    pairs of k_hyb_embed, k_hyb_spread and k_hyb_apply takes up to three turns."""
    rows, cols, n = 300, 5000, 1 << 14
    rng = np.random.default_rng(k)
    Fi = hx.features(cols, cols + 1, np.repeat(np.arange(cols), 2), np.stack([np.zeros(cols, np.int64), 1 + np.arange(cols)], 1).ravel(),
                     np.full(2 * cols, 0.5, F))
    Eu, Ei = hx.initial_tables(rows, cols + 1, k, 3)
    Eu *= F(4.0)
    u, i, j = rng.integers(0, rows, n), rng.integers(0, cols, n), rng.integers(0, cols, n)
    skipped = rng.random(n) < 0.2
    lr, lam = 1e-4, 0.01
    Ru, Ri, st, mu, mi = hx.step(hx.identity(rows), Fi, Eu, Ei, u, i, j, skipped, lr, lam, counts=True)
    live = int((~skipped).sum())
    assert st[2] == 0 and mi[0] == 2 * live and mu.sum() == live and mi[1:].sum() == 2 * live
    Gu, Gi, rep = mfx.hyb_apply(rows, cols, Eu, Ei, u, i, j, lr, lam, item_features=Fi, skipped=skipped)
    assert counts(rep) == st
    assert same_bits(Gi[0], Ri[0]), (Gi[0][:4], Ri[0][:4])
    assert same_bits(Gu, Ru) and same_bits(Gi, Ri)
    assert not same_bits(Gi[0], Ei[0])
    if k == 64:
        assert 3 * n * _gs(k) > 2 * MAX_GRID * THREADS


def test_step_where_every_loop_takes_more_than_one_turn(mfx, R):
    """The loops of the new kernels that have a cap, each taking at least two turns here or in the test named:
      the walk through the (slot, role) pairs (k_hyb_embed, k_hyb_spread, k_hyb_apply; 4 096 workgroups):
        test_one_feature_carried_by_every_row at k = 64;
      the walk through the rows of a side (k_hyb_embed behind get_factors and mfx_hyb_embed): case C, 70 000 rows at k = 64
        against 4 096 * 4 groups;
      the entries of a row, gs at a time (all three kernels): case A, items of 65 .. 70 features at gs = 64; case B, users of
        up to 4 features at gs = 2;
      the 8 loads in flight of k_hyb_embed: case A, eight turns per 64 entries;
      the coordinates, gs * NC = 256 per turn at k > 128 (k_hyb_embed, k_hyb_spread) and gs = 64 per turn in k_hyb_apply:
        case D, k = 1 024, four and sixteen turns."""
    rng = np.random.default_rng(77)
    lr, lam = 0.05, 0.01
    Fu, Fi = _small_features()

    # A: k = 64, every item carries 65 .. 70 of 90 features
    k, n = 64, 200
    per = rng.integers(65, 71, R.cols)
    ir = np.repeat(np.arange(R.cols), per)
    it = np.concatenate([rng.choice(90, m, replace=False) for m in per])
    Fa = mfx.hyb_features(R.cols, ir, it, 90, identity=False)
    assert np.diff(Fa.ptr.astype(np.int64)).min() > 64 > IN_FLIGHT
    Eu, Ei = hx.initial_tables(Fu.nf, Fa.nf, k, 1)
    Eu *= F(8.0)
    Ei *= F(8.0)
    u, i, j = rng.integers(0, R.rows, n), rng.integers(0, R.cols, n), rng.integers(0, R.cols, n)
    ref = _check_apply(mfx, R.rows, R.cols, Fu, Fa, Eu, Ei, u, i, j, lr, lam)
    assert not same_bits(ref[1], Ei)

    # B: k = 2, groups of two lanes
    k = 2
    assert _gs(k) == 2 and np.diff(Fu.ptr.astype(np.int64)).max() >= 3
    Eu, Ei = hx.initial_tables(Fu.nf, Fi.nf, k, 2)
    _check_apply(mfx, R.rows, R.cols, Fu, Fi, Eu, Ei, u, i, j, lr, lam)

    # C: the embedding of 70 000 rows
    k, rows = 64, 70_000
    assert rows > MAX_GRID * (THREADS // _gs(k))
    Fc = mfx.hyb_features(rows, np.arange(rows), np.arange(rows) % 11, 11)
    E = hx.initial_tables(Fc.nf, 1, k, 4)[0]
    assert same_bits(mfx.hyb_embed(Fc, E), hx.embed(Fc, E))

    # D: k = 1 024
    k, n = 1024, 40
    Eu, Ei = hx.initial_tables(Fu.nf, Fi.nf, k, 5)
    ref = _check_apply(mfx, R.rows, R.cols, Fu, Fi, Eu, Ei, u[:n], i[:n], j[:n], lr, lam)
    assert not same_bits(ref[0][:, -1], Eu[:, -1])


# ------------------------------------------------------------------------------------------------ identity features are BPR
def test_solver_with_identity_features_is_the_bpr_solver(mfx, R):
    """None / None and the identity passed explicitly, against BprSolver: batch 64 over 503 entries is seven full steps and a
    step of 55, two epochs.  W, H, the tables, the per-epoch counts and the position."""
    k, batch, lr, lam, seed = 12, 64, 0.05, 0.01, 9
    W0, H0 = bx.initial_factors(R.rows, R.cols, k, 3)
    H0[4, 1] = F(-0.0)
    b = mfx.BprSolver(R, _params(mfx, k, lam), lr, batch, seed=seed)
    b.set_factors(W0, H0)
    rb = b.iterate(2)
    Wb, Hb = b.get_factors()
    assert b.position() == 2 * R.nnz and bx.epoch_steps(R.nnz, batch, 0)[-1][1] == 55
    assert not same_bits(Wb, W0)
    for fu, fi in ((None, None), (hx.identity(R.rows), hx.identity(R.cols)), (None, hx.identity(R.cols))):
        a = mfx.HybridSolver(R, _params(mfx, k, lam), lr, batch, user_features=fu, item_features=fi, seed=seed)
        a.set_embeddings(W0, H0)
        ra = a.iterate(2)
        assert [counts(r) for r in ra] == [counts(r) for r in rb]
        assert a.position() == b.position()
        for W, H in (a.get_embeddings(), a.get_factors()):
            assert same_bits(W, Wb) and same_bits(H, Hb)
        a.close()
    b.close()
    # the default tables are BprSolver's draw
    a = mfx.HybridSolver(R, _params(mfx, k, lam), lr, batch, seed=seed, init_seed=8)
    b = mfx.BprSolver(R, _params(mfx, k, lam), lr, batch, seed=seed, init_seed=8)
    a.steps(3)
    b.steps(3)
    assert all(same_bits(x, y) for x, y in zip(a.get_factors(), b.get_factors()))
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ the solver
@pytest.mark.parametrize("k,batch", [(8, 100), (65, 64), (8, 1 << 20)])
def test_solver_step_is_the_operator_on_the_sampled_triples(mfx, R, k, batch):
    """Two epochs, one steps(1) at a time, beside hyb_apply on bpr_triples of the same slots: the counts and the tables at every
    step, over the epoch boundary with its short last step; get_factors is the embedding of the current tables."""
    Fu, Fi = _small_features()
    lr, lam, seed = 0.05, 0.01, 21
    nnz = R.nnz
    Eu, Ei = hx.initial_tables(Fu.nf, Fi.nf, k, 4)
    s = mfx.HybridSolver(R, _params(mfx, k, lam), lr, batch, user_features=Fu, item_features=Fi, seed=seed)
    s.set_embeddings(Eu, Ei)
    assert s.position() == 0
    pos = 0
    for epoch in range(2):
        plan = bx.epoch_steps(nnz, batch, pos)
        assert sum(c for _, c in plan) == nnz and plan[-1][1] == (nnz % batch or batch)
        for n_step, (first, cnt) in enumerate(plan):
            u, i, j, sk = mfx.bpr_triples(R, seed, first, cnt)
            Eu, Ei, want = mfx.hyb_apply(R.rows, R.cols, Eu, Ei, u, i, j, lr, lam, user_features=Fu, item_features=Fi, skipped=sk)
            got = s.steps(1)
            assert counts(got) == counts(want) and got["slots"] == cnt
            pos += cnt
            assert s.position() == pos
            Su, Si = s.get_embeddings()
            assert same_bits(Su, Eu) and same_bits(Si, Ei), (epoch, n_step)
    assert pos == 2 * nnz
    W, H = s.get_factors()
    assert same_bits(W, mfx.hyb_embed(Fu, Eu)) and same_bits(H, mfx.hyb_embed(Fi, Ei))
    assert same_bits(W, hx.embed(Fu, Eu)) and same_bits(H, hx.embed(Fi, Ei))
    assert same_bits(s.embed("item", Fi), H) and same_bits(s.embed("user", Fu), W)
    s.close()


def _device_arrays(R):
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a)).to(dev)
    return {"rows": R.rows, "cols": R.cols, "csr_row_ptr": t(R.csr_row_ptr), "csr_col_idx": t(R.csr_col_idx),
            "csr_val": t(R.csr_val), "csc_col_ptr": t(R.csc_col_ptr), "csc_row_idx": t(R.csc_row_idx), "csc_val": t(R.csc_val)}


def test_iterate_matches_the_reference_and_memory_spaces_agree(mfx, R):
    import torch  # noqa: F401  (device-resident inputs)
    Fu, Fi = _small_features()
    k, batch, lr, lam, seed = 8, 100, 0.05, 0.01, 33
    Eu, Ei = hx.initial_tables(Fu.nf, Fi.nf, k, 6)
    p = _params(mfx, k, lam)
    p.profile = 1
    s = mfx.HybridSolver(R, p, lr, batch, user_features=Fu, item_features=Fi, seed=seed, init_seed=6)
    part = s.steps(2)
    assert part["slots"] == 200 and s.position() == 200
    reps = s.iterate(2)
    assert [r["slots"] for r in reps] == [R.nnz - 200, R.nnz] and s.position() == 2 * R.nnz
    assert s.iterate(0) == [] and s.steps(0)["slots"] == 0 and s.position() == 2 * R.nnz
    Ru, Ri, st, pos = hx.train(R, Fu, Fi, Eu, Ei, lr, lam, batch, seed, 2)
    assert pos == 2 * R.nnz
    assert st[0].tolist() == [part[key] + reps[0][key] for key in KEYS] and st[1].tolist() == counts(reps[1])
    Su, Si = s.get_embeddings()
    assert same_bits(Su, Ru) and same_bits(Si, Ri)
    t = s.kernel_times()
    assert list(t) == ["sample", "embed", "gradient", "scatter", "spread", "apply"] and all(v > 0 for v in t.values())
    s.close()
    d = mfx.HybridSolver(None, _params(mfx, k, lam), lr, batch, user_features=Fu, item_features=Fi, seed=seed, device_arrays=_device_arrays(R),
                         init_seed=6)
    d.iterate(2)
    Du, Di = d.get_embeddings()
    d.close()
    assert same_bits(Du, Ru) and same_bits(Di, Ri)
    o = mfx.HybridSolver(R, _params(mfx, k, lam), lr, batch, user_features=Fu, item_features=Fi, seed=seed + 1, init_seed=6)
    o.iterate(2)
    assert not same_bits(o.get_embeddings()[0], Ru)
    o.close()


# ------------------------------------------------------------------------------------------------ refusals
def _broken(Fm, **kw):
    import mfx
    out = mfx.HybFeatures(Fm.n, Fm.nf, Fm.ptr.copy(), Fm.idx.copy(), Fm.val.copy())
    for key, (pos, value) in kw.items():
        getattr(out, key)[pos] = value
    return out


def test_create_refuses_broken_feature_matrices_naming_the_row(mfx, R):
    Fu, Fi = _small_features()
    pu = Fu.ptr.astype(np.int64)
    row = int(np.argmax(np.diff(pu) >= 3))  # a user with the identity and two tags or more
    lo = int(pu[row])
    make = lambda fu, fi=Fi: mfx.HybridSolver(R, _params(mfx, 8, 0.01), 0.05, 64, user_features=fu, item_features=fi)
    for bad in (_broken(Fu, val=(lo + 1, 1.5)), _broken(Fu, val=(lo + 1, -1.0000001)), _broken(Fu, val=(lo, np.nan)),
                _broken(Fu, val=(lo + 2, np.inf)), _broken(Fu, idx=(lo + 1, Fu.idx[lo + 2])), _broken(Fu, idx=(lo + 2, Fu.idx[lo + 1] - 1)),
                _broken(Fu, idx=(lo + 2, Fu.nf)), _broken(Fu, ptr=(row + 1, pu[row + 2] + 1))):
        with pytest.raises(mfx.MfxError, match=f"row {row} of the user features"):
            make(bad)
    with pytest.raises(mfx.MfxError, match="row 39 of the item features"):
        make(Fu, _broken(Fi, val=(len(Fi.val) - 1, 2.0)))
    with pytest.raises(mfx.MfxError, match="row 0 of the item features"):
        make(Fu, _broken(_broken(Fi, val=(0, -7.0)), val=(len(Fi.val) - 1, 2.0)))  # the first of two
    with pytest.raises(mfx.MfxError, match="the item features have 60 rows"):
        make(Fu, Fu)
    with pytest.raises(mfx.MfxError, match=f"row {row} of the user features"):
        E = hx.initial_tables(Fu.nf, Fi.nf, 4, 0)
        z = np.zeros(3, np.uint32)
        mfx.hyb_apply(R.rows, R.cols, E[0], E[1], z, z, z, 0.05, 0.01, user_features=_broken(Fu, val=(lo, -3.0)), item_features=Fi)
    make(_broken(Fu, val=(lo, -1.0))).close()  # |v| = 1 is allowed


def test_stepping_before_the_tables_are_set_is_refused_and_bad_slots_leave_the_tables(mfx, R):
    from mfx import api
    Fu, Fi = _small_features()
    lib = mfx.lib()
    h = C.c_void_p()
    csx, cpar, fu, fi = api._csx(R), _params(mfx, 8, 0.01).to_c(), Fu.to_c(), Fi.to_c()
    assert lib.mfx_hyb_create(C.byref(h), C.byref(csx), C.byref(fu), C.byref(fi), C.byref(cpar), 0.05, 64, 3, 0) == 0
    stats = (C.c_int64 * 4)()
    Eu, Ei = hx.initial_tables(Fu.nf, Fi.nf, 8, 1)
    W, H = np.zeros((R.rows, 8), F), np.zeros((R.cols, 8), F)
    assert lib.mfx_hyb_steps(h, 1, stats, None) == MFX_ERR_INVALID
    assert lib.mfx_hyb_epochs(h, 1, stats, None) == MFX_ERR_INVALID
    assert lib.mfx_hyb_get_embeddings(h, api._vp(Eu), api._vp(Ei), 0) == MFX_ERR_INVALID
    assert lib.mfx_hyb_get_factors(h, api._vp(W), api._vp(H), 0) == MFX_ERR_INVALID
    assert lib.mfx_hyb_steps(h, -1, stats, None) == MFX_ERR_INVALID
    assert lib.mfx_hyb_set_embeddings(h, api._vp(Eu), None, 0) == MFX_ERR_INVALID
    assert lib.mfx_hyb_set_embeddings(h, api._vp(Eu), api._vp(Ei), 0) == 0
    assert lib.mfx_hyb_steps(h, 1, stats, None) == 0 and stats[0] == 64
    u, i, j, sk = mfx.bpr_triples(R, 3, 0, 64)
    Ru, Ri, st = hx.step(Fu, Fi, Eu, Ei, u, i, j, sk, 0.05, 0.01)
    assert list(stats) == st
    assert lib.mfx_hyb_get_embeddings(h, api._vp(Eu), api._vp(Ei), 0) == 0
    assert same_bits(Eu, Ru) and same_bits(Ei, Ri)
    assert lib.mfx_hyb_destroy(h) == 0

    # a slot id out of range: the first such slot is named and the caller's tables are left as they were
    z = np.zeros(70, np.uint32)
    u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    for which, bad in ((0, R.rows), (1, R.cols), (2, R.cols)):
        ids = [z.copy(), z.copy(), z.copy()]
        ids[which][66] = bad
        ids[which][69] = bad + 5
        Eu, Ei = Ru.copy(), Ri.copy()
        rc = lib.mfx_hyb_apply(R.rows, R.cols, 8, C.byref(fu), C.byref(fi), api._vp(Eu), api._vp(Ei), 70, u32(ids[0]), u32(ids[1]), u32(ids[2]),
                               None, 0.05, 0.01, stats, 0)
        assert rc == MFX_ERR_INVALID and b"slot 66" in lib.mfx_last_error()
        assert same_bits(Eu, Ru) and same_bits(Ei, Ri)
    Gu, Gi, rep = mfx.hyb_apply(R.rows, R.cols, Ru, Ri, z[:0], z[:0], z[:0], 0.05, 0.01, user_features=Fu, item_features=Fi)
    assert same_bits(Gu, Ru) and same_bits(Gi, Ri) and counts(rep) == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ end to end
COLD_FLOOR = 0.99


def test_cold_start_end_to_end(mfx):
    """bx.planted_clusters() with three items of every cluster taken out of training (hx.cold_start_split: 48 667 entries left).
    Item features: identity + one tag per cluster, normalised; users: identity.  k = 16, batch 4 096, lr 0.05, lambda 0.001,
    2 epochs, seed 7, init_seed 5.  The cold items' rows come from embed(): half their own untrained vector, half their
    cluster's trained one.  Metric: per user the AUC of its own cluster's 3 cold items among all 60, averaged.
    The GPU run equals hyb_exact bit for bit, so the metric is the reference's: 1.0000 on the CPU (0.9531 after one epoch).
    The floor is that value minus 0.01: the metric's float64 scores come from a matrix product whose order of summation is the
    BLAS library's, so a near-tie may fall either way on another machine; one pair in a hundred is far more than that can move
    and far less than the distance to the control.  The control is the same run with identity item features, where a cold
    item keeps its initial vector: 0.4914 on the CPU; asserted only to be below the hybrid run."""
    R, cold, cluster = hx.cold_start_split()
    assert R.nnz == 48_667 and cold.size == 60
    assert not np.isin(R.csr_col_idx, cold).any()
    k, batch, lr, lam, seed, init = 16, 4096, 0.05, 0.001, 7, 5
    user_cluster = np.arange(R.rows) % 20
    Fu = hx.identity(R.rows)
    Fh = mfx.hyb_features(R.cols, np.arange(R.cols), cluster, 20)
    Fcold = mfx.HybFeatures(cold.size, Fh.nf, (2 * np.arange(cold.size + 1)).astype(np.uint32),
                            np.stack([cold, R.cols + cluster[cold]], 1).ravel().astype(np.uint32), np.full(2 * cold.size, 0.5, F))
    auc = {}
    for name, Fi in (("hybrid", Fh), ("control", None)):
        s = mfx.HybridSolver(R, _params(mfx, k, lam), lr, batch, item_features=Fi, seed=seed, init_seed=init)
        reps = s.iterate(2)
        Eu, Ei = s.get_embeddings()
        W, H = s.get_factors()
        nfi = Fh.nf if Fi is not None else R.cols
        Ru, Ri, st, _ = hx.train(R, Fu, Fi if Fi is not None else hx.identity(R.cols), *hx.initial_tables(R.rows, nfi, k, init), lr, lam,
                                 batch, seed, 2)
        assert [counts(r) for r in reps] == st.tolist() and all(r["bad"] == 0 for r in reps)
        assert same_bits(Eu, Ru) and same_bits(Ei, Ri)
        Hcold = s.embed("item", Fcold) if Fi is not None else H[cold]
        s.close()
        if Fi is not None:
            assert same_bits(Hcold, hx.embed(Fcold, Ri)) and same_bits(Hcold, H[cold])  # the cold rows were rows of Fi all along
        auc[name] = hx.cold_auc(W, Hcold, cluster[cold], user_cluster)
    print("cold-start auc:", auc)
    assert auc["hybrid"] >= COLD_FLOOR, auc
    assert auc["hybrid"] > auc["control"], auc
