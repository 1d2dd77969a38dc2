"""The conjugate-gradient kernels at every rank class up to 1024: fold-in (mfx_rec_fold_in_cg_setup), explanations
(mfx_rec_explain_cg) and the training half (mfx_ials_cg_half) against the fp64 references of tests/cg_sweep.py.

The kernels choose their instantiation from the rank k (cg_sweep.dispatch mirrors the dispatchers and is asserted against the
sources).  Coverage of a launch whose result is compared with a reference that is not the kernel, read from the rank lists of
every CG test.  BEFORE this module (ranks 37, 64, 130, 160, 256, 1024 only):

    kernel                    chosen by                               run                                  never run
    k_cg_gather<C, 1, MODE>   C from ceil(k / 64) on 1, 2, 4, 8, 16   C = 1, 4, 16                         C = 2 (65..128), C = 8 (257..512)
    k_cg_gather<C, TG, 1>     the same ladder, TG = 16, 16, 8, 4, 1   <1,16>, <4,8>, <16,1>                <2,16>, <8,4>
    k_foldcg_dense<ND>        k > 128 ? 4 : ceil(k / 32)              ND = 2, 4                            ND = 1 (k <= 32), ND = 3 (65..96)
    load4 of k_foldcg_dense   k % 4, tail k % 8                       k = 37, 130 not vectorised           k = 1, 2, 3, most residues of k % 8
    target groups             T = 5 < TG = 8, 16                      a second, ragged group at C = 16     at every other C
    last column block         k > 128: width k - 128 floor((k-1)/128) widths 2, 32, 128                    a width with mixed mok[t]
    rows per call             11 rows: one wavefront of the dense     -                                    two blocks, a ragged wavefront, a
                              product                                                                      frozen wavefront, seg0 >= nseg
    spd_inverse via the half  nb = ceil(k / 32)                       nb = 2, 5, 8, 32; kp - k = 27, 30, 0 nb = 1, 3, 4; every other kp - k

AFTER (set S: 12 rows of 0 .. 4097 entries; set M: 140 rows; every model on S up to rank 136, implicit alpha 40 and ALS above;
the ranks up to 136 in eight ranges of 17, one case per range and model, a larger rank one case):

    every rank 1 .. 136                 C = 1, 2 and the onset of 4; <1,16>, <2,16>, <4,8>; ND = 1 .. 4 and the second column
                                        block at widths 1 .. 8; every k % 4 and k % 8; nb = 1 .. 5 and every kp - k
    159 160 161 192 193 224 225 255     last widths 31, 32, 33, 64, 65, 96, 97, 127, 128, 1, 4: every count of tiles, whole and
    256 257 260                         ragged; the edge C = 4 / 8
    384 511 512 513 516 767 1000        C = 8 and 16, <8,4> and <16,1>, ranks that are and are not a multiple of 4 in each
    1023 1024
    T = 17 targets                      16 + 1, 8 + 8 + 1, 4 x 4 + 1: a second, ragged group at every TG; seven targets alone
    set M at 3 32 33 96 128 160 257     two blocks of the dense product and of the per-row kernels, a ragged and idle
    513 1024                            wavefronts, a wavefront frozen from the start
    independence at 33 65 96 129 257    a row alone against the row in its batch, layout 0 against layout 1: bits and counts
    513

Checks (cg_sweep.converged / method_check / target_check; tests/test_cg_sweep_host.py shows that the fp64 references pass them at
every one of these ranks, that every condition number is within the gate of 1e3, and that a lost entry of a split row, two
exchanged coordinates, a lost column of Minv, a lost coordinate of G p and a neighbour's target do not):
    1. fold-in converged (steps = 64, tol = 1e-5, from zero and from W0): backward error <= 3e-5 and relative error <= 1e-3
       against the DENSE system on every live row, a count in [1, 64); a row without a right-hand side exactly zero, count 0
    2. the method (tol = 0, steps 1, 2, 4, from zero and from W0): every row within 1e-3 of foldin_cg_ref.rows; from zero a row
       of n entries with n + 1 <= steps within 1e-3 of the dense solve
    3. mfx_ials_cg_half: checks 1 and 2 for the implicit model (the device Gramian and the device inverse)
    4. explanations, T = 17: explain_cg_ref.errors under the bounds of 1, and Z[q][t] for t in 0, 3, 4, 7, 8, 15, 16 bit for bit
       the Z of a call that asks for that target alone
    5. independence bit for bit at the class edges
    6. set M: steps = 3, tol = 0 within 1e-3 of the fp64 method; converged within 1e-3 of the fp64 method at tol = 1e-9; a stopped
       row the bits of the row after exactly its count of steps; rows 32..63 zero with count 0
The bounds are the project's own (tests/test_gpu_ials.py, tests/test_gpu_ialsb.py, tests/test_gpu_foldin_cg.py).

Measured on the MI355X (`cgsweep-measured` / `cgsweep-detail` lines; profiles/r26_cg_sweep_accuracy.txt), maxima over all ranks
at (rank, set, row); row T: the worst (row, target) pair.  The fp64 references themselves (tests/test_cg_sweep_host.py) reach
4.3e-05 (ALS, k = 21) / 4.9e-06 on the same checks, so what is measured is the stop rule at tol = 1e-5, not fp32:
    family                                  backward error             relative error
    fold-in, implicit alpha 1               7.513e-06 (3, S, 2)        1.496e-05 (3, S, 2)
    fold-in, implicit alpha 40              4.665e-06 (6, S, 7)        2.876e-05 (1000, S, 8)
    fold-in, ALS                            4.730e-06 (512, S, 5)      3.634e-05 (4, S, 3)
    fold-in, CCD                            4.923e-06 (90, S, 9)       1.281e-05 (21, S, 6)
    fold-in after 1 / 2 / 4 steps           -                          1.092e-04 (4, S, 4) to the fp64 method (ALS; 1.6e-05 elsewhere)
    training half, implicit alpha 1         7.513e-06 (3, S, 2)        1.496e-05 (3, S, 2)
    training half, implicit alpha 40        4.665e-06 (6, S, 7)        2.912e-05 (1000, S, 8)
    training half after 1 / 2 / 4 steps     -                          2.017e-05 (516, S, 4) to the fp64 method
    explanations, implicit alpha 1          4.942e-06 (3, S, T)        1.092e-05 (81, S, T)
    explanations, implicit alpha 40         4.757e-06 (4, S, T)        3.396e-05 (1024, S, T)
    explanations, ALS                       4.736e-06 (18, S, T)       3.694e-05 (18, S, T)
    explanations, CCD                       4.941e-06 (5, S, T)        1.371e-05 (11, S, T)
    explanations, split gap over bracket    3.140e-06 (4, S, T)        -
    set M, 3 steps                          -                          6.218e-06 (513, M, 126) to the fp64 method
    set M, converged                        -                          2.954e-05 (1024, M, 96) to the fp64 method at tol = 1e-9
    bit for bit: every target alone, every row alone, both layouts, every stopped row of set M against the run of its count.

What the sweep found: no defect.  Every instance that no test had launched (C = 2 and 8, <2,16> and <8,4>, ND = 1 and 3, the
scalar load4 below rank 4, every ragged last column block, the frozen wavefront, two blocks, nb = 1, 3, 4) meets the bounds
with the margin of the six ranks tested before, and no figure grows towards a class edge.  That the checks would have seen one
was tried once with two deliberate defects in a build that was not kept: the last column of k_foldcg_dense<3> not stored at
k % 8 = 5 (refused by checks 1 to 4 under the implicit model at k = 69, 77 and 85, at no other rank of 69..85), and the last
target of a ragged group of k_cg_gather<8, 4, 1> not gathered (refused by check 4 at k = 257, the first rank of that class; the
run was stopped there).
"""
import numpy as np
import pytest

import cg_sweep as cs
from test_gpu_foldin import F32, handle, same, select

pytestmark = pytest.mark.gpu

LAM = cs.LAM


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1, m.lib().mfx_last_error()
    return m


def rec(mfx, H, layout=1):
    """A recommender over H and a one-row dummy W."""
    return handle(mfx, np.zeros((1, H.shape[1]), F32), H, layout)


def fold(r, rows, start=None):
    _, _, Y, cnt = r.fold_in(rows, W_init=start, return_sweeps=True)
    return Y, cnt


def explain(r, rows, tg):
    return r.explain_cg(rows, tg, n_expl=1, return_W=True, return_Z=True, return_steps=True)


def bad_rows(a, b):
    a, b = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
    return np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0].tolist()


# ------------------------------------------------------------------------------------------------ checks 1 to 4, per rank
def sweep_rank(mfx, k, worst, misses, only=None):
    """Checks 1 to 4 at rank k for the models of cs.models(k), or for `only` of them."""
    models = [m for m in cs.models(k) if only is None or m == only]
    ptr, idx, _, H, W0 = cs.data(k)
    tg = cs.targets(k)
    starts = (("zero", None), ("W0", W0))
    with rec(mfx, H, k % 2) as r:
        for model, alpha in models:
            name = cs.NAMES[(model, alpha)]
            rows = (ptr, idx, cs.values(model, k))
            # 1. converged, and 4. the targets under the same setup
            r.fold_in_cg_setup(model, LAM, alpha, steps=cs.STEPS, tol=cs.TOL)
            for label, start in starts:
                Y, cnt = fold(r, rows, start)
                errs, m = cs.converged(model, k, alpha, Y, cnt, ("fold_in", label))
                worst["fold-in"].add(k, "S", errs, name)
                misses += m
                if start is None:
                    cold = Y
            out = explain(r, rows, tg)
            if not same(out["W"], cold):
                misses.append(("explain_cg", name, k, "W is not fold_in's row", bad_rows(out["W"], cold)))
            values, m = cs.target_check(model, k, alpha, out["Z"], out["W"], out["target_steps"], ("explain_cg",))
            misses += m
            if values is not None:
                worst["explain"].add(k, "S", [("T", values[1], values[0])], name)
                worst["explain split gap"].add(k, "S", [("T", values[2], None)], name)
            for t in cs.ALONE:
                one = explain(r, rows, tg[:, [t]])
                if not (same(one["Z"][:, 0], out["Z"][:, t]) and np.array_equal(one["target_steps"][:, 0], out["target_steps"][:, t])):
                    misses.append(("explain_cg", name, k, "target %d alone has other bits" % t, bad_rows(one["Z"][:, 0], out["Z"][:, t])))
            # 2. the method itself
            for steps in cs.SHORT_STEPS:
                r.fold_in_cg_setup(model, LAM, alpha, steps=steps, tol=0.0)
                for label, start in starts:
                    Y, cnt = fold(r, rows, start)
                    errs, m = cs.method_check(model, k, alpha, start is not None, steps, Y, cnt, ("fold_in",))
                    worst["fold-in method"].add(k, "S", errs, name)
                    misses += m
    # 3. the training half: the device Gramian and the device inverse
    for model, alpha in models:
        if model != cs.IMPLICIT:
            continue
        name = cs.NAMES[(model, alpha)]
        val = cs.values(model, k)
        for label, start in starts:
            Y, cnt = mfx.ials_cg_half(ptr, idx, val, H, k, LAM, alpha, cs.STEPS, cs.TOL, Y_in=start, return_steps=True)
            errs, m = cs.converged(model, k, alpha, Y, cnt, ("ials_cg_half", label))
            worst["training half"].add(k, "S", errs, name)
            misses += m
            for steps in cs.SHORT_STEPS:
                Y, cnt = mfx.ials_cg_half(ptr, idx, val, H, k, LAM, alpha, steps, 0.0, Y_in=start, return_steps=True)
                errs, m = cs.method_check(model, k, alpha, start is not None, steps, Y, cnt, ("ials_cg_half",))
                worst["training half method"].add(k, "S", errs, name)
                misses += m
    cs.release(k)


FAMILIES = ("fold-in", "fold-in method", "training half", "training half method", "explain", "explain split gap")


def sweep(mfx, ranks, only=None):
    worst, misses = {f: cs.Worst() for f in FAMILIES}, []
    try:
        for k in ranks:
            sweep_rank(mfx, k, worst, misses, only)
    finally:
        for f in FAMILIES:
            if worst[f].parts:
                print(worst[f].line(f, ranks[0], ranks[-1]))
    assert not misses, "\n".join(map(str, misses))


@pytest.mark.parametrize("model", list(cs.NAMES), ids=lambda m: cs.NAMES[m].replace(" ", "-"))
@pytest.mark.parametrize("ranks", cs.RANGES, ids=lambda r: "%d-%d" % r)
def test_cg_sweep(mfx, ranks, model):
    """every rank of the range under one model (the training half under the implicit ones)"""
    sweep(mfx, list(range(ranks[0], ranks[1] + 1)), model)


@pytest.mark.parametrize("k", cs.LARGE)
def test_cg_sweep_large(mfx, k):
    sweep(mfx, [k])


# ------------------------------------------------------------------------------------------------ 5. independence
@pytest.mark.parametrize("k", cs.EDGE_RANKS)
def test_a_row_depends_on_neither_its_batch_nor_the_layout(mfx, k):
    ptr, idx, _, H, W0 = cs.data(k)
    tg = cs.targets(k)
    U = len(cs.S)
    with rec(mfx, H, 1) as r, rec(mfx, H, 0) as r2:
        for model, alpha in ((cs.IMPLICIT, 40.0), (cs.ALS, 0.0)):
            val = cs.values(model, k)
            rows = (ptr, idx, val)
            for steps, tol, start in ((cs.STEPS, cs.TOL, None), (cs.STEPS, 1e-4, W0), (4, 0.0, W0)):
                for h in (r, r2):
                    h.fold_in_cg_setup(model, LAM, alpha, steps=steps, tol=tol)
                Y, cnt = fold(r, rows, start)
                Y2, cnt2 = fold(r2, rows, start)
                assert bad_rows(Y2, Y) == [] and np.array_equal(cnt2, cnt), (k, model, steps, tol, "layout")
                for u in range(1, U):
                    Ya, ca = fold(r, select(ptr, idx, val, [u]), None if start is None else np.ascontiguousarray(start[[u]]))
                    assert same(Ya[0], Y[u]) and ca[0] == cnt[u], (k, model, steps, tol, u, "fold_in alone")
                out, out2 = explain(r, rows, tg), explain(r2, rows, tg)
                for key in ("Z", "W", "target_steps", "row_steps", "totals"):
                    assert same(out2[key], out[key]), (k, model, steps, tol, key, "layout")
                for u in (1, 5, 7, 9, 10):
                    one = explain(r, select(ptr, idx, val, [u]), tg[[u]])
                    for key in ("Z", "W", "target_steps", "row_steps", "totals"):
                        assert same(one[key][0], out[key][u]), (k, model, steps, tol, u, key, "explain_cg alone")
                if model == cs.IMPLICIT:  # the training half: a permuted subset with a row twice
                    sel = np.array([10, 3, 9, 0, 7, 9, 1])
                    Yh, ch = mfx.ials_cg_half(ptr, idx, val, H, k, LAM, alpha, steps, tol, Y_in=start, return_steps=True)
                    sp, si, sv = select(ptr, idx, val, sel)
                    Ys, cs_ = mfx.ials_cg_half(sp, si, sv, H, k, LAM, alpha, steps, tol, Y_in=None if start is None else np.ascontiguousarray(start[sel]),
                                               return_steps=True)
                    assert bad_rows(Ys, Yh[sel]) == [] and np.array_equal(cs_, ch[sel]), (k, steps, tol, "ials_cg_half subset")
    cs.release(k)


# ------------------------------------------------------------------------------------------------ 6. many rows
def many_rows(k, label, call, w):
    """steps = 3 at tol = 0 and the converged setup on set M through call(steps, tol, start) -> (Y, counts); returns the
    converged cold (Y, counts)."""
    alpha = 40.0
    ptr, idx, val, H, W0 = cs.data(k, cs.M)
    U = len(cs.M)
    live = np.array([bool((val[ptr[u]:ptr[u + 1]] > 0).any()) for u in range(U)])
    assert live.sum() >= 100 and not live[32:64].any()
    kept = None
    for steps, tol, rtol in ((3, 0.0, 0.0), (cs.STEPS, cs.TOL, 1e-9)):
        for warm in (False, True):
            Y, cnt = call(steps, tol, W0 if warm else None)
            want, _ = cs.method_m(k, alpha, warm, steps, rtol)
            assert np.isfinite(Y).all(), (label, k, steps, warm)
            assert not Y[~live].any() and not cnt[~live].any(), (label, k, steps, warm, "a row without a right-hand side")
            rel = np.array([cs.rel_error(Y[u], want[u]) for u in np.nonzero(live)[0]])
            at = int(np.nonzero(live)[0][rel.argmax()])
            w.add(k, "M", [(at, None, float(rel.max()))], "%s %s" % (label, "steps 3" if tol == 0.0 else "converged"))
            assert rel.max() <= cs.MAX_REL, (label, k, steps, warm, at, float(rel.max()))
            if tol == 0.0:
                assert (cnt[live] >= 1).all() and (cnt[live] <= steps).all(), (label, k, warm, cnt.tolist())
            else:
                assert (cnt[live] >= 1).all() and (cnt[live] < steps).all(), (label, k, warm, cnt.tolist())
                if not warm:
                    kept = (Y, cnt, live)
    return kept


@pytest.mark.parametrize("k", cs.M_RANKS)
def test_many_rows(mfx, k):
    alpha = 40.0
    ptr, idx, val, H, _ = cs.data(k, cs.M)
    w = cs.Worst()
    try:
        with rec(mfx, H, k % 2) as r:
            def call(steps, tol, start):
                r.fold_in_cg_setup(cs.IMPLICIT, LAM, alpha, steps=steps, tol=tol)
                return fold(r, (ptr, idx, val), start)
            Y, cnt, live = many_rows(k, "fold-in", call, w)
            # a stopped row is the row after exactly its count of steps: across wavefronts and blocks
            counts = sorted(set(cnt[live].tolist()))
            assert len(counts) >= 2, counts
            for c in counts:
                fixed, fc = call(c, 0.0, None)
                at = np.nonzero(cnt == c)[0]
                assert bad_rows(fixed[at], Y[at]) == [] and (fc[at] == c).all(), (k, c, at.tolist())
        many_rows(k, "training half", lambda steps, tol, start: mfx.ials_cg_half(ptr, idx, val, H, k, LAM, alpha, steps, tol, Y_in=start,
                                                                                  return_steps=True), w)
    finally:
        print(w.line("many rows", k, k))
    cs.release(k)
