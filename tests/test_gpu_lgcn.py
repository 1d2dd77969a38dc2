"""GPU tests of LightGCN training (mfx_lgcn_*) against the exact reference of tests/lgcn_exact.py: every comparison of
embeddings is bit for bit and every count exact, because the contract of include/mfx.h fixes each fp32 operation and its
order, and the sums of a step are integer sums."""
import ctypes as C
import functools

import numpy as np
import pytest

import bpr_exact as bx
import lgcn_exact as lx

pytestmark = pytest.mark.gpu

MFX_ERR_INVALID = -1  # include/mfx.h
F = np.float32
KEYS = ("slots", "skipped", "bad", "correct")


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


def _check_propagate(mfx, M, W0, H0, E, layers):
    Wr, Hr = lx.mean_of(E, layers)
    Wg, Hg = mfx.lgcn_propagate(M, W0, H0, layers)
    assert same_bits(Wg, Wr), (layers, int((bits(Wg) != bits(Wr)).sum()))
    assert same_bits(Hg, Hr), (layers, int((bits(Hg) != bits(Hr)).sum()))
    return Wr, Hr


# ------------------------------------------------------------------------------------------------ the propagation
@pytest.mark.parametrize("k", [1, 3, 4, 63, 64, 65, 128, 129, 200, 1024])
def test_propagate_bit_for_bit(mfx, R, k):
    """L = 0 .. 3 on the small matrix: every lane-group width (k = 1, 3, 4), the three wave-wide kernels (k <= 64, <= 128,
    above) and, at k = 1024, the coordinate loop of k_lgcn_propagate taking four turns of 256 coordinates."""
    assert R.rows == 60 and R.cols == 40 and R.nnz == 503
    W0, H0 = bx.initial_factors(R.rows, R.cols, k, k)
    E = lx.layers_of(R, W0, H0, 3)
    for layers in (0, 1, 2, 3):
        Wr, Hr = _check_propagate(mfx, R, W0, H0, E, layers)
        if layers == 0:
            assert same_bits(Wr, W0) and same_bits(Hr, H0)
        else:
            assert not same_bits(Wr, W0) and not same_bits(Hr, H0)


@functools.lru_cache(maxsize=None)
def _segment_matrix():
    return lx.segment_matrix()


@pytest.mark.parametrize("k", [4, 65])
def test_propagate_segment_boundaries_on_both_sides(mfx, k):
    """Rows and columns of exactly 1023, 1024, 1025, 2048, 2049 and 3000 entries (lgcn_exact.segment_matrix): one chain, a
    chain and a sum of two or three segment sums, through the work items of a segment each and k_lgcn_combine.  At k = 65 a
    group is a wave of 64 entries at a time, so the loop over the 8 loads in flight takes eight turns per 64 entries."""
    S = _segment_matrix()
    W0, H0 = bx.initial_factors(S.rows, S.cols, k, 31 + k)
    E = lx.layers_of(S, W0, H0, 2)
    _check_propagate(mfx, S, W0, H0, E, 2)
    # the heavy rows got their value from more than one segment: a single chain over the whole row gives other bits
    ptr, idx = S.csr_row_ptr.astype(np.int64), S.csr_col_idx.astype(np.int64)
    si = lx.scales(S.csc_col_ptr)
    from rec_exact import fmaf32
    acc = np.zeros(k, F)
    for e in range(ptr[5], ptr[6]):
        acc = fmaf32(si[idx[e]], H0[idx[e]], acc)
    assert not same_bits(lx.scales(S.csr_row_ptr)[5] * acc, E[1][0][5])


@functools.lru_cache(maxsize=None)
def _tall_matrix():
    """70 000 x 50, three entries in most rows, every column about 4 000 entries; rows 0 .. 9 empty."""
    from mfx import dataset as ds
    rng = np.random.default_rng(17)
    rows, cols = 70_000, 50
    r = np.repeat(np.arange(10, rows), 3)
    c = rng.integers(0, cols, r.size)
    cells = np.unique(r * cols + c)
    return ds.from_coo(rows, cols, cells // cols, cells % cols, np.ones(cells.size, F))


def test_propagate_where_every_loop_takes_more_than_one_turn(mfx):
    """The loops of k_lgcn_propagate, each taking at least two turns here or in the tests named:
      the walk through the work order: 70 000 work items at k = 8 -- a group is 8 lanes, a launch is capped at 2 048 workgroups
        of 32 groups = 65 536 groups, so the first 4 000 odd groups take a second item;
      the rows of a workgroup: 32 groups of 8 lanes per workgroup, each with its own row;
      the loop over gs entries at a time: the columns hold about 4 000 entries, 8 at a time, in four segments of 1 024;
      the loop over the 8 loads in flight: at gs = 8 it takes one turn per 8 entries; it takes eight turns per 64 entries in
        test_propagate_segment_boundaries_on_both_sides at k = 65;
      the coordinate loop: k = 1 024 in test_propagate_bit_for_bit (four turns of 256 coordinates).
    The work order is no parameter of the entry points: it is made at create from the row lengths alone."""
    T = _tall_matrix()
    assert T.rows == 70_000 and 190_000 <= T.nnz <= 210_000
    assert T.rows > 2048 * (256 // 8)
    deg = np.diff(T.csc_col_ptr.astype(np.int64))
    assert deg.min() > 3 * 1024
    k = 8
    W0, H0 = bx.initial_factors(T.rows, T.cols, k, 3)
    E = lx.layers_of(T, W0, H0, 2)
    Wr, _ = _check_propagate(mfx, T, W0, H0, E, 2)
    assert same_bits(Wr[:10], W0[:10] * (F(1.0) / F(3.0)))  # the empty rows: the base over L + 1


# ------------------------------------------------------------------------------------------------ the operator
def _check_apply(mfx, R, W0, H0, u, i, j, layers, lr, lam, skipped=None):
    """lgcn_apply against the reference: the base embeddings and the four counts; returns the reference's result."""
    Wr, Hr, st = lx.step(R, W0, H0, u, i, j, skipped, layers, lr, lam)
    Wg, Hg, rep = mfx.lgcn_apply(R, W0, H0, u, i, j, layers, lr, lam, skipped=skipped)
    assert counts(rep) == st, (counts(rep), st)
    assert same_bits(Wg, Wr), int((bits(Wg) != bits(Wr)).sum())
    assert same_bits(Hg, Hr), int((bits(Hg) != bits(Hr)).sum())
    return Wr, Hr, st


@pytest.mark.parametrize("layers", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 64, 65, 1000])
@pytest.mark.parametrize("k", [1, 4, 65, 129])
def test_apply_bit_for_bit(mfx, R, k, n, layers):
    rng = np.random.default_rng(1000 * k + 10 * n + layers)
    W0, H0 = bx.initial_factors(R.rows, R.cols, k, k + n)
    W0 *= F(8.0)  # scores of a few units after the mean: the sigmoid away from 1/2
    lr, lam = 0.05, 0.01

    # a random batch, caller skip flags on a fifth of the slots, item 5 as the positive of some slots and the sampled item
    # of others; i == j happens by chance and is allowed
    u = rng.integers(0, R.rows, n)
    i = rng.integers(0, R.cols - 5, n)
    j = rng.integers(0, R.cols - 5, n)
    i[::3] = 5
    j[1::3] = 5
    skipped = rng.random(n) < 0.2
    if n >= 3:
        j[2], skipped[2] = i[2], False
    Wr, Hr, st = _check_apply(mfx, R, W0, H0, u, i, j, layers, lr, lam, skipped)
    assert st[1] == int(skipped.sum()) and st[2] == 0
    if n in (64, 65):
        # the gradient reaches rows that no slot names
        unnamed = np.setdiff1d(np.arange(R.rows), u[~skipped])
        assert unnamed.size and not same_bits(Wr[unnamed], W0[unnamed])

    # lr = 0: every bit stays
    Wz, Hz, _ = _check_apply(mfx, R, W0, H0, u, i, j, layers, 0.0, lam, skipped)
    assert same_bits(Wz, W0) and same_bits(Hz, H0)

    if n >= 3:
        # a slot with a term >= 64 is counted bad: user 59's first coordinate is huge, so are then g * W[u][0] of its slot
        # and, where the sigmoid does not vanish, the terms of the slots on its neighbours
        Wb, Hb = W0.copy(), H0.copy()
        Wb[R.rows - 1] = 0.0
        Wb[R.rows - 1, 0] = 4000.0
        ub, ib, jb = u.copy(), i.copy(), j.copy()
        ub[0], ib[0], jb[0] = R.rows - 1, R.cols - 1, R.cols - 1  # d = 0: x = 0, g = 1/2
        _, _, st = _check_apply(mfx, R, Wb, Hb, ub, ib, jb, layers, lr, lam)
        assert st[2] >= 1 and st[1] == 0
        # a slot with a NaN factor is counted bad; the NaN spreads with the layers, and the slots it reaches are bad too
        Wb, Hb = W0.copy(), H0.copy()
        Hb[R.cols - 3, k - 1] = np.nan
        ub[n - 1], ib[n - 1], jb[n - 1] = 1, 2, R.cols - 3
        _, _, st = _check_apply(mfx, R, Wb, Hb, ub, ib, jb, layers, lr, lam)
        assert st[2] >= 1

    if n >= 65:  # the order of the slots plays no part
        a = mfx.lgcn_apply(R, W0, H0, u, i, j, layers, lr, lam, skipped=skipped)
        for seed in (1, 2):
            o = np.random.default_rng(seed).permutation(n)
            b = mfx.lgcn_apply(R, W0, H0, u[o], i[o], j[o], layers, lr, lam, skipped=skipped[o])
            assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and counts(a[2]) == counts(b[2])


# ------------------------------------------------------------------------------------------------ layers = 0 is BPR
@pytest.mark.parametrize("n,k", [(1, 1), (65, 4), (1000, 65), (64, 129)])
def test_apply_without_layers_is_bpr_apply(mfx, R, n, k):
    rng = np.random.default_rng(n + k)
    W0, H0 = bx.initial_factors(R.rows, R.cols, k, 5)
    W0 *= F(4.0)
    u, i, j = rng.integers(0, R.rows - 7, n), rng.integers(0, R.cols, n), rng.integers(0, R.cols, n)
    s = rng.random(n) < 0.2
    a = mfx.lgcn_apply(R, W0, H0, u, i, j, 0, 0.05, 0.01, skipped=s)
    b = mfx.bpr_apply(W0, H0, u, i, j, 0.05, 0.01, skipped=s)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and counts(a[2]) == counts(b[2])
    assert same_bits(a[0][R.rows - 7:], W0[R.rows - 7:])
    if not s.all():
        assert not same_bits(a[0], W0)


def test_solver_without_layers_is_the_bpr_solver(mfx, R):
    k, batch, lr, lam, seed = 12, 100, 0.05, 0.01, 9
    W0, H0 = bx.initial_factors(R.rows, R.cols, k, 3)
    a = mfx.LightGcnSolver(R, _params(mfx, k, lam), lr, batch, 0, seed=seed)
    b = mfx.BprSolver(R, _params(mfx, k, lam), lr, batch, seed=seed)
    a.set_base(W0, H0)
    b.set_factors(W0, H0)
    ra, rb = a.iterate(2), b.iterate(2)
    assert [counts(r) for r in ra] == [counts(r) for r in rb]
    assert a.position() == b.position() == 2 * R.nnz
    Wb, Hb = b.get_factors()
    for W, H in (a.get_base(), a.get_factors()):
        assert same_bits(W, Wb) and same_bits(H, Hb)
    assert not same_bits(Wb, W0)
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ the solver
@pytest.mark.parametrize("batch", [64, 100, 1 << 20])
@pytest.mark.parametrize("k", [8, 65])
def test_solver_step_is_the_operator_on_the_sampled_triples(mfx, R, k, batch):
    """Two epochs at L = 2, one steps(1) at a time, beside lgcn_apply on bpr_triples of the same slots: the counts and the base
    embeddings at every step."""
    layers, lr, lam, seed = 2, 0.05, 0.01, 21
    nnz = R.nnz
    W0, H0 = bx.initial_factors(R.rows, R.cols, k, 4)
    s = mfx.LightGcnSolver(R, _params(mfx, k, lam), lr, batch, layers, seed=seed)
    s.set_base(W0, H0)
    assert s.position() == 0
    pos = 0
    for epoch in range(2):
        plan = bx.epoch_steps(nnz, batch, pos)
        assert sum(c for _, c in plan) == nnz and plan[-1][1] == (nnz % batch or batch)
        for n_step, (first, cnt) in enumerate(plan):
            u, i, j, sk = mfx.bpr_triples(R, seed, first, cnt)
            W0, H0, want = mfx.lgcn_apply(R, W0, H0, u, i, j, layers, lr, lam, skipped=sk)
            got = s.steps(1)
            assert counts(got) == counts(want) and got["slots"] == cnt
            pos += cnt
            assert s.position() == pos
            Ws, Hs = s.get_base()
            assert same_bits(Ws, W0) and same_bits(Hs, H0), (epoch, n_step)
    assert pos == 2 * nnz
    Wf, Hf = s.get_factors()
    Wp, Hp = mfx.lgcn_propagate(R, W0, H0, layers)
    assert same_bits(Wf, Wp) and same_bits(Hf, Hp) and not same_bits(Wf, W0)
    s.close()


def test_iterate_finishes_a_started_epoch_and_matches_the_reference(mfx, R):
    k, batch, layers, lr, lam, seed = 8, 100, 2, 0.05, 0.01, 33
    W0, H0 = bx.initial_factors(R.rows, R.cols, k, 6)
    p = _params(mfx, k, lam)
    p.profile = 1
    s = mfx.LightGcnSolver(R, p, lr, batch, layers, seed=seed)
    s.set_base(W0, H0)
    part = s.steps(2)
    assert part["slots"] == 200 and s.position() == 200
    reps = s.iterate(2)
    assert [r["slots"] for r in reps] == [R.nnz - 200, R.nnz] and s.position() == 2 * R.nnz
    assert s.iterate(0) == [] and s.steps(0)["slots"] == 0 and s.position() == 2 * R.nnz
    Wr, Hr, st, pos = lx.train(R, W0, H0, layers, lr, lam, batch, seed, 2)
    assert pos == 2 * R.nnz
    assert st[0].tolist() == [part[key] + reps[0][key] for key in KEYS] and st[1].tolist() == counts(reps[1])
    for r in reps:
        assert r["auc"] == r["correct"] / (r["slots"] - r["skipped"] - r["bad"]) and r["seconds"] > 0
    Ws, Hs = s.get_base()
    assert same_bits(Ws, Wr) and same_bits(Hs, Hr)
    Wf, Hf = s.get_factors()
    Wp, Hp = lx.propagate(R, Wr, Hr, layers)
    assert same_bits(Wf, Wp) and same_bits(Hf, Hp)
    t = s.kernel_times()
    assert list(t) == ["sample", "forward", "gradient", "scatter", "backward", "update"] and all(v > 0 for v in t.values())
    s.close()


def _device_arrays(R):
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a)).to(dev)
    return {"rows": R.rows, "cols": R.cols, "csr_row_ptr": t(R.csr_row_ptr), "csr_col_idx": t(R.csr_col_idx),
            "csr_val": t(R.csr_val), "csc_col_ptr": t(R.csc_col_ptr), "csc_row_idx": t(R.csc_row_idx), "csc_val": t(R.csc_val)}


def test_same_bits_twice_other_seed_differs_memory_spaces_agree(mfx, R):
    import torch  # noqa: F401  (device-resident inputs)
    k, batch, layers = 12, 64, 2

    def run(seed, device_arrays=None, init_seed=8):
        s = mfx.LightGcnSolver(R if device_arrays is None else None, _params(mfx, k, 0.01), 0.05, batch, layers, seed=seed,
                               device_arrays=device_arrays, init_seed=init_seed)
        reps = s.iterate(2)
        W, H = s.get_base()
        s.close()
        return W, H, [counts(r) for r in reps]

    a, b, c = run(5), run(5), run(5, device_arrays=_device_arrays(R))
    for other in (b, c):
        assert same_bits(a[0], other[0]) and same_bits(a[1], other[1]) and a[2] == other[2]
    d = run(6)
    assert not same_bits(a[0], d[0]) and not same_bits(a[1], d[1])
    # the default base is BprSolver's: numpy.random.default_rng(init_seed)
    W0, H0 = bx.initial_factors(R.rows, R.cols, k, 8)
    Wr, Hr, st, _ = lx.train(R, W0, H0, layers, 0.05, 0.01, batch, 5, 2)
    assert same_bits(a[0], Wr) and same_bits(a[1], Hr) and a[2] == st.tolist()


# ------------------------------------------------------------------------------------------------ refusals
def test_create_refuses_ranges_and_a_csc_side_that_is_not_the_transpose(mfx, R):
    from mfx import api
    for kw in (dict(layers=-1), dict(layers=9), dict(k=0), dict(k=1025), dict(batch=0), dict(batch=(1 << 20) + 1), dict(lr=-1.0),
               dict(lr=float("nan")), dict(lam=-0.5), dict(lam=float("inf"))):
        a = {"k": 8, "lam": 0.01, "lr": 0.05, "batch": 64, "layers": 2, **kw}
        with pytest.raises(mfx.MfxError, match="mfx_lgcn_create"):
            mfx.LightGcnSolver(R, _params(mfx, a["k"], a["lam"]), a["lr"], a["batch"], a["layers"])
    cp = R.csc_col_ptr.astype(np.int64)
    member = np.zeros((R.rows, R.cols), bool)
    member[np.repeat(np.arange(R.rows), np.diff(R.csr_row_ptr.astype(np.int64))), R.csr_col_idx] = True
    # one id changed: the last id of a column becomes a greater row that the column does not hold (the column stays in order)
    col = next(c for c in range(R.cols) if cp[c + 1] > cp[c] and R.csc_row_idx[cp[c + 1] - 1] < R.rows - 1
               and not member[R.csc_row_idx[cp[c + 1] - 1] + 1, c])
    B = R.copy()
    B.csc_row_idx[cp[col + 1] - 1] += 1
    with pytest.raises(mfx.MfxError, match=f"column {col} of the CSC side"):
        mfx.LightGcnSolver(B, _params(mfx, 8, 0.01), 0.05, 64, 2)
    with pytest.raises(mfx.MfxError, match=f"column {col} of the CSC side"):
        mfx.lgcn_propagate(B, *bx.initial_factors(R.rows, R.cols, 4, 0), 1)
    # two ids swapped between two columns, each column still in order and without a duplicate
    last = lambda c: int(R.csc_row_idx[cp[c + 1] - 1])
    prev = lambda c: int(R.csc_row_idx[cp[c + 1] - 2])
    ok = lambda a, b: (cp[a + 1] - cp[a] >= 2 and cp[b + 1] - cp[b] >= 2 and last(a) != last(b) and prev(a) < last(b) and prev(b) < last(a)
                       and not member[last(b), a] and not member[last(a), b])
    a, b = next((a, b) for a in range(R.cols) for b in range(a + 1, R.cols) if ok(a, b))
    B = R.copy()
    B.csc_row_idx[cp[a + 1] - 1], B.csc_row_idx[cp[b + 1] - 1] = last(b), last(a)
    with pytest.raises(mfx.MfxError, match=f"column {a} of the CSC side"):
        mfx.LightGcnSolver(B, _params(mfx, 8, 0.01), 0.05, 64, 2)
    # a column out of order is named by the row check
    B = R.copy()
    B.csc_row_idx[cp[a + 1] - 1], B.csc_row_idx[cp[a + 1] - 2] = prev(a), last(a)
    with pytest.raises(mfx.MfxError, match=f"column {a} of the CSC side"):
        mfx.LightGcnSolver(B, _params(mfx, 8, 0.01), 0.05, 64, 2)
    row = int(np.argmax(np.diff(R.csr_row_ptr.astype(np.int64)) >= 3))
    B = R.copy()
    lo = int(R.csr_row_ptr[row])
    B.csr_col_idx[lo], B.csr_col_idx[lo + 1] = R.csr_col_idx[lo + 1], R.csr_col_idx[lo]
    with pytest.raises(mfx.MfxError, match=f"row {row} of the CSR side"):
        mfx.LightGcnSolver(B, _params(mfx, 8, 0.01), 0.05, 64, 2)
    # stepping before the base is set is refused and leaves the handle usable
    h = C.c_void_p()
    csx, cpar = api._csx(R), _params(mfx, 8, 0.01).to_c()
    lib = mfx.lib()
    assert lib.mfx_lgcn_create(C.byref(h), C.byref(csx), C.byref(cpar), 0.05, 64, 2, 3, 0) == 0
    stats = (C.c_int64 * 4)()
    assert lib.mfx_lgcn_steps(h, 1, stats, None) == MFX_ERR_INVALID
    assert lib.mfx_lgcn_epochs(h, 1, stats, None) == MFX_ERR_INVALID
    W, H = bx.initial_factors(R.rows, R.cols, 8, 1)
    assert lib.mfx_lgcn_get_base(h, api._vp(W), api._vp(H), 0) == MFX_ERR_INVALID
    assert lib.mfx_lgcn_get_factors(h, api._vp(W), api._vp(H), 0) == MFX_ERR_INVALID
    assert lib.mfx_lgcn_steps(h, -1, stats, None) == MFX_ERR_INVALID
    assert lib.mfx_lgcn_set_base(h, api._vp(W), None, 0) == MFX_ERR_INVALID
    assert lib.mfx_lgcn_set_base(h, api._vp(W), api._vp(H), 0) == 0
    assert lib.mfx_lgcn_steps(h, 1, stats, None) == 0 and stats[0] == 64
    u, i, j, sk = mfx.bpr_triples(R, 3, 0, 64)
    Wr, Hr, st = lx.step(R, W, H, u, i, j, sk, 2, 0.05, 0.01)
    assert list(stats) == st
    assert lib.mfx_lgcn_get_base(h, api._vp(W), api._vp(H), 0) == 0
    assert same_bits(W, Wr) and same_bits(H, Hr)
    assert lib.mfx_lgcn_destroy(h) == 0


def test_apply_refuses_ids_out_of_range(mfx, R):
    W, H = bx.initial_factors(R.rows, R.cols, 8, 0)
    z = np.zeros(70, np.uint32)
    for which, bad in ((0, R.rows), (1, R.cols), (2, R.cols)):
        ids = [z.copy(), z.copy(), z.copy()]
        ids[which][66] = bad
        ids[which][69] = bad + 5
        with pytest.raises(mfx.MfxError, match="slot 66"):
            mfx.lgcn_apply(R, W, H, *ids, 2, 0.05, 0.01)
    Wg, Hg, rep = mfx.lgcn_apply(R, W, H, z[:0], z[:0], z[:0], 2, 0.05, 0.01)
    assert same_bits(Wg, W) and same_bits(Hg, H) and counts(rep) == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ end to end
def test_planted_clusters_recommend_end_to_end(mfx):
    """The planted clusters of bpr_exact.planted_clusters: k = 32, L = 2, batch 1 024, lr 0.05, lambda 0.01, 10 epochs, seed 7,
    init_seed 5.  No bad slot, the last epoch ranks more of its sampled pairs correctly than the first, and the top-10 lists of
    the final embeddings (training items excluded) find the held-out item for at least 90 % of the users."""
    P = bx.planted_clusters()
    s = mfx.LightGcnSolver(P, _params(mfx, 32, 0.01), 0.05, 1024, 2, seed=7, init_seed=5)
    reps = s.iterate(10)
    W, H = s.get_factors()
    s.close()
    assert all(r["slots"] == P.nnz and r["bad"] == 0 for r in reps)
    print("auc per epoch:", [round(r["auc"], 4) for r in reps])
    assert reps[-1]["auc"] > reps[0]["auc"]
    top, _ = mfx.recommend(W, H, 1, 10, exclude=P)
    m = mfx.topn_metrics(top, mfx.test_data_of(P))
    print("metrics:", m)
    assert m["users"] == P.rows
    assert m["hr"] >= 0.9, m
