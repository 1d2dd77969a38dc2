"""Explanations of fold-in recommendations (mfx_rec_explain, mfx.Recommender.explain) on the GPU.

Shared inputs: H drawn N(0, 0.1^2), lambda = 0.1, values in 1..5, alpha = 1, the reg setup with (alpha0, nu) = (0.3, 0.5);
rows with repeated ids (two entries with the same id are two entries).  Every fp64 system is asserted to have a condition
number <= 1e3.
  1. Z against the fp64 system: normwise backward error <= 3e-5 and relative error <= 1e-3, the bounds that
     tests/test_gpu_ials.py applies to this factorisation.
  2. bitwise links: W_out = fold_in's row, totals = the chain of rec_exact over (W_out, H) = the scores fold_in returns.
  3. the lists bit for bit from Z_out (tests/explain_exact.py), across the Gramian split and the selection pieces.
  4. end to end against fp64: |c_e - c64_e| <= 1.1e-3 |b_e| |h_e| |z64| (Cauchy-Schwarz on the 1e-3 relative bound of 1;
     the chain's own rounding, k 2^-24 <= 8e-6, is inside the 10 % margin), and the sum against the total likewise.
  5. a row's bits do not depend on the batch, its order, the memory space or the cut into pieces.
  6. refusals that leave the handle usable.
Bits are compared as uint32, -0 included."""
import numpy as np
import pytest

import explain_exact as ex
from ials_ref import backward_error
from rec_exact import chain_scores
from test_gpu_foldin import F32, MFX_ERR_INVALID, handle, host, same, select

pytestmark = pytest.mark.gpu

PAD = ex.PAD
LAM, ALPHA, ALPHA0, NU = 0.1, 1.0, 0.3, 0.5
KS = [1, 5, 32, 36, 37, 64, 96, 100, 128]  # 32 x 32 tiles (1, 5, 32, 37), gram16 (36, and the permuted image at 64), blocked (96, 100, 128)


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1, m.lib().mfx_last_error()
    return m


def set_up(mfx, r, setup):
    if setup == "als":
        r.fold_in_setup(mfx.MFX_FOLD_ALS, LAM)
    elif setup == "ccd":
        r.fold_in_setup(mfx.MFX_FOLD_CCD, LAM)
    elif setup == "implicit":
        r.fold_in_setup(mfx.MFX_FOLD_IMPLICIT, LAM, ALPHA)
    else:
        r.fold_in_setup(mfx.MFX_FOLD_IMPLICIT, LAM, ALPHA, alpha0=ALPHA0, nu=NU)


def rows_of(seed, cols, sizes):
    """CSR rows of the given sizes, ids non-decreasing WITH repeats, values 1..5."""
    rng = np.random.default_rng(seed)
    ptr = np.zeros(len(sizes) + 1, np.uint32)
    ptr[1:] = np.cumsum(sizes)
    idx = np.concatenate([np.sort(rng.integers(0, cols, n)) for n in sizes] + [np.zeros(0, np.int64)]).astype(np.uint32)
    val = rng.integers(1, 6, idx.size).astype(F32)
    return ptr, idx, val


def factor_H(seed, cols, k):
    return (0.1 * np.random.default_rng(seed).standard_normal((cols, k))).astype(F32)


def targets_of(seed, ptr, idx, cols):
    """[U, 4]: another item, padding, an item of the row (any item for an empty row), the first again."""
    rng = np.random.default_rng(seed)
    U = len(ptr) - 1
    t = np.empty((U, 4), np.uint32)
    for q in range(U):
        lo, hi = int(ptr[q]), int(ptr[q + 1])
        other = int(rng.integers(0, cols))
        t[q] = [other, PAD, int(idx[rng.integers(lo, hi)]) if hi > lo else int(rng.integers(0, cols)), other]
    return t


def checked_system(setup, ptr, idx, val, q, H):
    A = ex.system(setup, ptr, idx, val, q, H, LAM, ALPHA, ALPHA0, NU)
    cond = float(np.linalg.cond(A))
    assert cond <= 1e3, (setup, q, cond)
    return A, cond


# ------------------------------------------------------------------------------------------------ 1. accuracy of Z
SIZES = [0, 1, 2, 7, 40, 300]


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("setup", ex.SETUPS)
def test_Z_solves_the_fp64_system(mfx, setup, k, layout):
    cols = 300
    ptr, idx, val = rows_of(11, cols, SIZES)
    H = factor_H(100 + k, cols, k)
    targets = targets_of(12, ptr, idx, cols)
    with handle(mfx, np.zeros((3, k), F32), H, layout) as r:
        set_up(mfx, r, setup)
        out = r.explain((ptr, idx, val), targets, n_expl=0, return_Z=True)
    Z, H64 = out["Z"], H.astype(np.float64)
    assert Z.shape == (len(SIZES), 4, k) and Z.dtype == F32
    worst_b = worst_r = worst_c = 0.0
    for q, n in enumerate(SIZES):
        if n == 0:
            assert not Z[q].any(), q                      # an empty row
            continue
        A, cond = checked_system(setup, ptr, idx, val, q, H)
        worst_c = max(worst_c, cond)
        for t in range(4):
            if targets[q, t] == PAD:
                assert same(Z[q, t], np.zeros(k, F32)), (q, t)
                continue
            h = H64[targets[q, t]]
            z64 = np.linalg.solve(A, h)
            be = backward_error(A, Z[q, t], h)
            re = float(np.linalg.norm(Z[q, t] - z64) / np.linalg.norm(z64))
            worst_b, worst_r = max(worst_b, be), max(worst_r, re)
        assert same(Z[q, 0], Z[q, 3]), q                   # a repeated target
    print(f"explain-measured Z setup={setup} k={k} layout={layout} backward={worst_b:.3e} relative={worst_r:.3e} cond={worst_c:.1f}")
    assert worst_b <= 3e-5 and worst_r <= 1e-3, (setup, k, layout, worst_b, worst_r)


# ------------------------------------------------------------------------------------------------ 2. bitwise links
@pytest.mark.parametrize("k", [5, 36, 64, 100])
@pytest.mark.parametrize("setup", ex.SETUPS)
def test_rows_totals_and_scores_are_those_of_fold_in(mfx, setup, k):
    cols = 300
    ptr, idx, val = rows_of(21, cols, SIZES)
    # two more rows that leave fewer than five eligible items: every item, and all but three
    extra = [np.arange(cols), np.arange(3, cols)]
    idx = np.concatenate([idx] + extra).astype(np.uint32)
    val = np.concatenate([val] + [np.random.default_rng(22).integers(1, 6, e.size).astype(F32) for e in extra])
    ptr = np.concatenate([ptr, ptr[-1] + np.cumsum([e.size for e in extra]).astype(np.uint32)]).astype(np.uint32)
    U = len(ptr) - 1
    H = factor_H(200 + k, cols, k)
    targets = targets_of(23, ptr, idx, cols)
    layout = (k + ex.SETUPS.index(setup)) % 2
    with handle(mfx, np.zeros((3, k), F32), H, layout) as r:
        set_up(mfx, r, setup)
        out = r.explain((ptr, idx, val), targets, n_expl=3, return_W=True)
        items5, scores5, Wf = r.fold_in((ptr, idx, val), 5)
        out5 = r.explain((ptr, idx, val), items5, n_expl=3)
    assert same(out["W"], Wf)
    S = chain_scores(Wf, H, np.arange(U))
    want = np.where(targets == PAD, F32(-np.inf), S[np.arange(U)[:, None], np.where(targets == PAD, 0, targets)]).astype(F32)
    assert same(out["totals"], want)
    assert same(out5["totals"], scores5)                   # the scores fold_in reports; -inf at the padded positions
    pad = items5 == PAD
    assert pad[-2].all() and pad[-1, 3:].all() and not pad[-1, :3].any() and not pad[:-2].any()
    assert (out5["items"][pad] == PAD).all() and np.isneginf(out5["contrib"][pad]).all()
    assert (out["items"][targets == PAD] == PAD).all() and np.isneginf(out["contrib"][targets == PAD]).all()


# ------------------------------------------------------------------------------------------------ 3. the lists from Z_out
def check_lists(mfx, setup, k, layout, cols, ptr, idx, val, targets, n_expls):
    H = factor_H(300 + k, cols, k)
    with handle(mfx, np.zeros((3, k), F32), H, layout) as r:
        set_up(mfx, r, setup)
        outs = {n: r.explain((ptr, idx, val), targets, n_expl=n, return_W=True, return_Z=True) for n in n_expls}
        Wf = r.fold_in((ptr, idx, val))[2]
    first = outs[n_expls[0]]
    Z = first["Z"]
    for n, out in outs.items():
        assert same(out["Z"], Z) and same(out["W"], Wf) and same(out["totals"], first["totals"]), n
        assert out["items"].shape == out["contrib"].shape == targets.shape + (n,)
        items, contrib = ex.expected(setup, ptr, idx, val, targets, Z, H, n, ALPHA, ALPHA0)
        bad = np.nonzero((out["items"] != items).any(axis=2) | (out["contrib"].view(np.uint32) != contrib.view(np.uint32)).any(axis=2))
        assert bad[0].size == 0, (setup, k, n, list(zip(*bad))[:5])
    return first


@pytest.mark.parametrize("setup,k", [("als", 5), ("ccd", 37), ("implicit", 96), ("reg", 64), ("als", 128), ("implicit", 32)])
def test_lists_are_bit_for_bit_those_of_the_reference(mfx, setup, k):
    cols = 300
    ptr, idx, val = rows_of(31, cols, SIZES + [7, 64, 65])
    val[ptr[6]:ptr[7]] = 0.0                              # a row of zeros: no entry under the implicit models, seven ties otherwise
    targets = targets_of(32, ptr, idx, cols)
    out = check_lists(mfx, setup, k, k % 2, cols, ptr, idx, val, targets, [64, 1, 10, 0])
    if setup in ("implicit", "reg"):
        assert (out["items"][6] == PAD).all() and not out["W"][6].any()
    else:
        assert (out["items"][6, 0, :7] == idx[ptr[6]:ptr[7]]).all() and (out["items"][6, 0, 7:] == PAD).all()


@pytest.mark.parametrize("setup,k", [("reg", 36), ("als", 64), ("implicit", 128), ("ccd", 100), ("als", 5)])
def test_lists_of_rows_longer_than_a_piece(mfx, setup, k):
    """Rows of 2048, 2049 and 4097 entries over 5000 items: one, two and three chunks of the Gramian (kAlsChunk) and pieces of the
    selection, at row starts that are no multiples of 2048."""
    cols = 5000
    ptr, idx, val = rows_of(41, cols, [3, 2048, 2049, 0, 4097, 40])
    targets = targets_of(42, ptr, idx, cols)
    for q in (1, 2, 4):
        checked_system(setup, ptr, idx, val, q, factor_H(300 + k, cols, k))
    check_lists(mfx, setup, k, (k + 1) % 2, cols, ptr, idx, val, targets, [10, 64, 1])


# ------------------------------------------------------------------------------------------------ 4. end to end against fp64
@pytest.mark.parametrize("k", [5, 64, 128])
@pytest.mark.parametrize("setup", ex.SETUPS)
def test_contributions_against_fp64(mfx, setup, k):
    cols, sizes = 300, [1, 2, 7, 40, 64]
    ptr, idx, val = rows_of(51, cols, sizes)
    H = factor_H(500 + k, cols, k)
    H64 = H.astype(np.float64)
    targets = targets_of(52, ptr, idx, cols)
    with handle(mfx, np.zeros((3, k), F32), H, k % 2) as r:
        set_up(mfx, r, setup)
        out = r.explain((ptr, idx, val), targets, n_expl=64, return_Z=True)
    worst_c = worst_s = 0.0
    for q, n in enumerate(sizes):
        lo, hi = int(ptr[q]), int(ptr[q + 1])
        A, _ = checked_system(setup, ptr, idx, val, q, H)
        b, counts = ex.weights(setup, val[lo:hi], ALPHA, ALPHA0)
        assert counts.all()
        w64 = np.linalg.solve(A, ex.rhs(setup, idx[lo:hi], val[lo:hi], H, ALPHA, ALPHA0))
        Hj = H64[idx[lo:hi]]
        for t in (0, 2):
            h = H64[targets[q, t]]
            z64 = np.linalg.solve(A, h)
            c64 = b.astype(np.float64) * (Hj @ z64)
            # slot e of the list is the entry at position pos[e]: the order the reference derives from the bits of Z_out
            _, _, pos = ex.ranked(idx[lo:hi], ex.contributions(out["Z"][q, t], H, idx[lo:hi], b), counts, 64)
            assert len(pos) == n and (out["items"][q, t, :n] == idx[lo:hi][pos]).all()
            got = out["contrib"][q, t, :n].astype(np.float64)
            bound = 1.1e-3 * np.abs(b[pos].astype(np.float64)) * np.linalg.norm(Hj[pos], axis=1) * np.linalg.norm(z64)
            err = np.abs(got - c64[pos])
            assert (err <= bound).all(), (setup, k, q, t, float((err / bound).max()))
            total = float(out["totals"][q, t])
            sbound = bound.sum() + 1.1e-3 * np.linalg.norm(h) * np.linalg.norm(w64)
            serr = abs(got.sum() - total)
            assert serr <= sbound, (setup, k, q, t, serr, sbound)
            worst_c, worst_s = max(worst_c, float((err / bound).max())), max(worst_s, serr / sbound)
    print(f"explain-measured contributions setup={setup} k={k} worst error / bound: entry {worst_c:.3e}, sum {worst_s:.3e}")


# ------------------------------------------------------------------------------------------------ 5. independence
@pytest.mark.parametrize("setup,k", [("implicit", 64), ("als", 100), ("reg", 37)])
def test_a_row_does_not_depend_on_its_batch(mfx, setup, k):
    import torch
    cols = 3000
    ptr, idx, val = rows_of(61, cols, [5, 0, 2100, 17, 1, 300, 64])
    U = len(ptr) - 1
    H = factor_H(600 + k, cols, k)
    targets = targets_of(62, ptr, idx, cols)
    keys = ("items", "contrib", "totals", "W", "Z")
    with handle(mfx, np.zeros((3, k), F32), H, 1) as r:
        set_up(mfx, r, setup)
        call = lambda rows, tg, **kw: r.explain(rows, tg, n_expl=10, return_W=True, return_Z=True, **kw)
        full = call((ptr, idx, val), targets)
        for q in range(U):                                 # alone
            one = call(select(ptr, idx, val, [q]), targets[q:q + 1])
            assert all(same(one[key][0], full[key][q]) for key in keys), q
        perm = [6, 2, 0, 5, 5, 1, 4, 3, 2]                  # shuffled, with repeats
        sh = call(select(ptr, idx, val, perm), targets[perm])
        assert all(same(sh[key], full[key][perm]) for key in keys)
        signed = call((ptr, idx, val), targets.view(np.int32))  # numpy int32 targets: the uint32 bits, -1 is the padding
        assert all(same(signed[key], full[key]) for key in keys)
        dev = torch.device("cuda", r.device)               # device arrays
        t32 = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)
        on = call((t32(ptr), t32(idx), t32(val)), t32(targets))
        assert all(same(host(on[key]), full[key]) for key in keys)
        cut = call((ptr, idx, val), targets, max_ws_bytes=4 * k * 4 * 3)  # three users per piece: three pieces
        assert all(same(cut[key], full[key]) for key in keys)
        cut = call((t32(ptr), t32(idx), t32(val)), t32(targets), max_ws_bytes=4 * k * 4 * 3)
        assert all(same(host(cut[key]), full[key]) for key in keys)
        t = r.explain_times()
        assert set(t) == {"build", "solve", "contrib"} and all(v > 0 for v in t.values())


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_handle_usable(mfx):
    from mfx.api import _vp
    cols, k = 500, 64
    ptr, idx, val = rows_of(71, cols, [3, 0, 10, 25])
    U = len(ptr) - 1
    H = factor_H(72, cols, k)
    targets = targets_of(73, ptr, idx, cols)
    lib = mfx.lib()

    def raw(r, nt=4, n_expl=5, tg=targets, space=0, null_targets=False):
        it, co = np.empty((U, max(nt, 1), max(n_expl, 1)), np.uint32), np.empty((U, max(nt, 1), max(n_expl, 1)), F32)
        return lib.mfx_rec_explain(r.handle, U, idx.size, _vp(ptr), _vp(idx), _vp(val), nt, None if null_targets else _vp(tg), n_expl,
                                   _vp(it), _vp(co), None, None, None, space)

    with mfx.Recommender(np.zeros((3, k), F32), H, 1) as r:
        assert raw(r) == MFX_ERR_INVALID and "first" in lib.mfx_last_error().decode()          # before any setup
        set_up(mfx, r, "implicit")
        good = r.explain((ptr, idx, val), targets, 5, return_W=True, return_Z=True)
        again = lambda: all(same(a, b) for a, b in zip(r.explain((ptr, idx, val), targets, 5, return_W=True, return_Z=True).values(),
                                                       good.values()))
        assert again()
        wrong = [("MFX_FOLD_ALS", lambda: r.fold_in_setup(mfx.MFX_FOLD_ALS_EXACT, LAM)),
                 ("block", lambda: r.fold_in_block_setup(LAM, ALPHA, block=16, sweeps=2)),
                 ("block", lambda: r.fold_in_block_setup_reg(LAM, ALPHA, ALPHA0, NU, block=16, sweeps=2)),
                 ("block", lambda: r.fold_in_block_setup_als(LAM, block=16, sweeps=2))]
        for word, other in wrong:
            other()
            assert raw(r) == MFX_ERR_INVALID and word in lib.mfx_last_error().decode(), word
            r.fold_in((ptr, idx, val), 3)                  # the handle still folds in under that setup
            set_up(mfx, r, "implicit")
            assert again(), word
        for kw, word in ((dict(nt=0), "n_targets"), (dict(nt=65), "n_targets"), (dict(n_expl=-1), "n_expl"), (dict(n_expl=65), "n_expl"),
                         (dict(null_targets=True), "targets"), (dict(space=7), "memory space")):
            assert raw(r, **kw) == MFX_ERR_INVALID and word in lib.mfx_last_error().decode(), kw
            assert again(), kw
        for badid in (cols, cols + 1, 0x7FFFFFFF, 0xFFFFFFFE):
            tg = targets.copy()
            tg[2, 3] = badid
            assert raw(r, tg=tg) == MFX_ERR_INVALID and "target 3 of slot 2" in lib.mfx_last_error().decode(), badid
            assert again(), badid
        # the checks of the query rows are those of mfx_rec_fold_in
        def rows_call(p, i, v):
            it, co = np.empty((U, 4, 5), np.uint32), np.empty((U, 4, 5), F32)
            return lib.mfx_rec_explain(r.handle, U, i.size, _vp(p), _vp(i), _vp(v), 4, _vp(targets), 5, _vp(it), _vp(co), None, None, None, 0)
        i = idx.copy(); i[20] = cols
        assert rows_call(ptr, i, val) == MFX_ERR_INVALID and again()
        i = idx.copy(); i[[5, 6]] = [i[5] + 1, i[5]]
        assert rows_call(ptr, i, val) == MFX_ERR_INVALID and again()
        v = val.copy(); v[17] = -1.0
        assert rows_call(ptr, idx, v) == MFX_ERR_INVALID and "mfx_rec_explain" in lib.mfx_last_error().decode() and again()
        assert lib.mfx_rec_explain(r.handle, 0, 0, None, None, None, 4, None, 5, None, None, None, None, None, 0) == 0  # nusers = 0
        assert raw(r) == 0
