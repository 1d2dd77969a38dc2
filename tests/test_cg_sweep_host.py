"""Host checks of the per-rank sweep of the conjugate-gradient kernels (tests/cg_sweep.py), for every rank 1..136 and the
larger ranks of cg_sweep.LARGE: what tests/test_gpu_cg_sweep.py asserts on the GPU is (1) aimed at every template instance the
dispatchers can pick, (2) met by the fp64 references on every row and pair, with every condition number within the gate of 1e3
(so none is left out) and 64 steps enough, and (3) out of reach for five wrong answers:
    a row split over chunks that loses one entry from its sums               refused by check 1 on that row
    the last two coordinates exchanged                                        refused by check 1
    Minv with its last row and column zeroed (a lost column of k_foldcg_dense or of the device inverse)
                                                                              refused by check 1 (and by the n + 1 rule of check 2)
    G p with its last coordinate lost                                         refused by check 1
    one target answered with its neighbour's h_t                              refused by check 4
The checks are cg_sweep.converged / method_check / target_check, the very functions the GPU test calls.

Measured here over all these ranks (printed as `cgsweep-host` lines): the fp64 references' worst relative error 4.3e-05 (ALS,
k = 21, the row of 17 entries), backward error 4.9e-06 (a target at k = 3), condition number 234.3 (k = 1023, implicit alpha 40),
at most 36 steps (a target under ALS at k = 115); a row of n <= 3 entries after n + 1 steps (4 at the most) within 3.5e-10 of the
dense solve."""
import numpy as np
import pytest

import cg_sweep as cs
import foldin_cg_ref as ref
import ials_cg_ref
import ials_ref

RANK_SETS = [list(range(lo, hi + 1)) for lo, hi in cs.RANGES] + [[k] for k in cs.LARGE]


def _id(ranks):
    return "%d-%d" % (ranks[0], ranks[-1]) if len(ranks) > 1 else str(ranks[0])


# ------------------------------------------------------------------------------------------------ 0. inputs and mirror
def test_size_sets_and_dispatch_constants():
    d = cs.dispatch_constants()
    assert d == {"fold": (1, 2, 4, 8, 16), "explain": ((1, 16), (2, 16), (4, 8), (8, 4), (16, 1)), "dense": (128, 4, 128), "spd": 32,
                 "chunk": 2048, "rows": 4}
    assert [cs.chunks(n) for n in cs.S] == [1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 3, 1] and [cs.S[u] for u in cs.SPLIT_ROWS] == [2049, 4097]
    assert 0 in cs.S and {n % d["rows"] for n in cs.S if 0 < n <= 5} == set(range(d["rows"]))  # every tail of the rows in flight
    # M: two blocks of k_foldcg_dense (128 rows each), the second with one ragged wavefront; wavefront 1 frozen from the start
    assert len(cs.M) == 140 and -(-len(cs.M) // 128) == 2 and 0 < len(cs.M) - 128 < 32 and set(cs.M) == set(range(41))
    assert not any(cs.M[32:64]) and all(any(cs.M[w:w + 32]) for w in (0, 64, 96, 128))
    # T = 17: a second, ragged group of targets for every TG but 1
    assert all(cs.T > tg and cs.T % tg == 1 for _, tg in d["explain"] if tg > 1)
    ptr, idx, val, H, W0 = cs.data(37)
    assert H.shape == (cs.COLS, 37) and W0.shape == (12, 37) and list(np.diff(ptr.astype(np.int64))) == list(cs.S)
    assert np.array_equal(H, ref.inputs(37, cs.COLS, cs.S)[3]) and np.array_equal(H[:9], ref.inputs(37, cs.COLS, cs.M)[3][:9])  # one H for both sets
    tg = cs.targets(37)
    assert tg.shape == (12, cs.T) and (tg[:, cs.PAD_AT] == 0xFFFFFFFF).all() and (np.delete(tg, cs.PAD_AT, 1) < cs.COLS).all()
    assert all(tg[u, 0] == idx[ptr[u]] for u in range(12) if cs.S[u]) and cs.PAD_AT not in cs.ALONE and max(cs.ALONE) == cs.T - 1


def test_the_rank_lists_reach_every_instance():
    d = cs.dispatch_constants()
    assert cs.ALL_RANKS == sorted(set(cs.ALL_RANKS)) and cs.ALL_RANKS[:136] == list(range(1, 137)) and cs.RANGES[0] == (1, 17) and cs.RANGES[-1] == (120, 136)
    disp = {k: cs.dispatch(k) for k in cs.ALL_RANKS}
    # k_cg_gather<C, 1, MODE>: every rank runs MODE 2 (cold start), MODE 3 (warm start) and MODE 1 (a step), so every C is enough
    assert {v[0] for v in disp.values()} == set(d["fold"])
    assert {(v[0], v[1]) for v in disp.values()} == set(d["explain"])                      # k_cg_gather<C, TG, 1>
    assert {v[2] for v in disp.values()} == {1, 2, 3, 4}                                   # k_foldcg_dense<ND>
    for C in d["fold"]:                                                                    # both settings of vec in every class
        assert {cs.vec(k) for k, v in disp.items() if v[0] == C} == {True, False}, C
    for ND in (1, 2, 3, 4):
        assert {k % 8 for k, v in disp.items() if v[2] == ND} == set(range(8)), ND         # every tail of the k loop of 8
    assert {k for k in range(1, 4)} <= set(disp)                                           # load4 below one vector
    # the last column block above rank 128: every count of tiles, whole and ragged, and the widths the issue names
    above = [k for k in cs.ALL_RANKS if k > 128]
    assert {cs.width_class(k) for k in above} == {(t, r) for t in (1, 2, 3, 4) for r in (False, True)}
    assert {disp[k][3] for k in above} >= set(range(1, 9)) | {31, 32, 33, 64, 65, 96, 97, 127, 128, 4}
    assert {v[4] for k, v in disp.items() if k <= 136} == {1, 2, 3, 4, 5} and {k % 32 for k in range(1, 137)} == set(range(32))  # nb and kp - k
    assert {disp[k][4] for k in cs.LARGE} >= {5, 8, 16, 17, 32}
    # the class edges
    assert [disp[k][0] for k in (64, 65, 128, 129, 256, 257, 512, 513, 1024)] == [1, 2, 2, 4, 4, 8, 8, 16, 16]
    assert [disp[k][2] for k in (32, 33, 64, 65, 96, 97, 128, 129)] == [1, 2, 2, 3, 3, 4, 4, 4]
    # one rank per class on set M, and the class edges of the independence checks
    assert {cs.dispatch(k)[0] for k in cs.M_RANKS} == set(d["fold"]) and {cs.dispatch(k)[2] for k in cs.M_RANKS} == {1, 2, 3, 4}
    assert {cs.dispatch(k)[:2] for k in cs.EDGE_RANKS} == set(d["explain"]) and {cs.dispatch(k)[2] for k in cs.EDGE_RANKS} == {2, 3, 4}
    assert set(cs.M_RANKS) <= set(cs.ALL_RANKS) and set(cs.EDGE_RANKS) <= set(cs.ALL_RANKS)


# ------------------------------------------------------------------------------------------------ 1. the helpers' own pins
@pytest.mark.parametrize("k", [3, 32, 33])
def test_the_batched_method_is_the_method_row_by_row(k):
    ptr, idx, val, H, W0 = cs.data(k, cs.M)
    pair = cs.base_pair(k)
    live = 0
    for warm, steps, tol in ((False, 3, 0.0), (True, 3, 0.0), (False, 64, 1e-5), (True, 64, 1e-9)):
        want, wc = ref.rows(ref.IMPLICIT, ptr, idx, val, H, cs.LAM, 40.0, W0 if warm else None, steps, tol, base_pair=pair)
        got, gc = cs.rows_batched(ptr, idx, val, H, cs.LAM, 40.0, W0 if warm else None, steps, tol, pair)
        assert np.array_equal(gc, wc), (k, warm, steps, tol, gc.tolist(), wc.tolist())
        assert np.abs(got - want).max() <= 1e-11 * np.abs(want).max(), (k, warm, steps, tol)
        assert not got[32:64].any() and not gc[32:64].any()
        live = int(np.count_nonzero(wc))
    assert live >= 100


@pytest.mark.parametrize("k", [5, 65])
def test_the_training_reference_is_the_method(k):
    """ials_cg_ref.half is foldin_cg_ref.rows on the implicit model: cg_sweep.method, to the bit"""
    ptr, idx, val, H, W0 = cs.data(k)
    for warm, steps, tol in ((False, cs.STEPS, cs.TOL), (True, 2, 0.0)):
        Y, cnt = ials_cg_ref.half(ptr, idx, val, H, cs.LAM, 40.0, W0 if warm else None, steps, tol)
        want, wc = cs.method(ref.IMPLICIT, k, 40.0, warm, steps, tol)
        assert np.array_equal(Y, want) and np.array_equal(cnt, wc)


@pytest.mark.parametrize("k", [2, 37])
def test_row_errors_are_the_projects_errors(k):
    for model, alpha in cs.models(k):
        Y, _ = cs.method(model, k, alpha, True, 2, 0.0)  # two steps from W0: errors worth measuring
        errs = cs.row_errors(model, k, alpha, Y)
        rel, be, _ = ref.errors(model, k, alpha, Y, cs.COLS, cs.S)
        assert [e[0] for e in errs] == cs.live_rows(model, k, alpha) and max(e[1] for e in errs) == be and max(e[2] for e in errs) == rel
        sol = ref.dense_solutions(model, k, alpha, cs.COLS, cs.S)
        for u, b_, _ in errs:
            assert abs(b_ - ials_ref.backward_error(sol[u][0], Y[u], sol[u][1])) <= 1e-9 * b_, (model, k, u)


# ------------------------------------------------------------------------------------------------ 2. references and controls
@pytest.mark.parametrize("ranks", RANK_SETS, ids=_id)
def test_references_meet_the_bounds_and_controls_do_not(ranks):
    worst = {"rel": (0.0, None), "backward": (0.0, None), "cond": (0.0, None), "steps": (0, None), "short": (0.0, None)}

    def note(key, value, where):
        if value >= worst[key][0]:
            worst[key] = (value, where)

    for k in ranks:
        tg = cs.targets(k)
        for model, alpha in cs.models(k):
            name = cs.NAMES[(model, alpha)]
            live = cs.live_rows(model, k, alpha)
            assert set(live) >= {6, 7, 8, 9, 10} and 0 not in live, (name, k, live)
            for u, s in ref.dense_solutions(model, k, alpha, cs.COLS, cs.S).items():
                assert s[3] <= cs.MAX_COND, (name, k, u, s[3])  # the gate skips no row
                note("cond", s[3], (name, k, u))
            # ---- the references pass checks 1, 2 (3: the same references) and 4
            for warm in (False, True):
                Y, cnt = cs.method(model, k, alpha, warm, cs.STEPS, cs.TOL)
                errs, misses = cs.converged(model, k, alpha, Y, cnt, ("fp64",))
                assert not misses, misses
                for u, b_, r_ in errs:
                    note("backward", b_, (name, k, u))
                    note("rel", r_, (name, k, u))
                note("steps", int(cnt.max()), (name, k, int(cnt.argmax())))
                for steps in cs.SHORT_STEPS:
                    Ys, cs_ = cs.method(model, k, alpha, warm, steps, 0.0)
                    errs, misses = cs.method_check(model, k, alpha, warm, steps, Ys, cs_, ("fp64",))
                    assert not misses, misses
                    if not warm:
                        sol = ref.dense_solutions(model, k, alpha, cs.COLS, cs.S)
                        for u in live:
                            if cs.S[u] + 1 <= steps:
                                note("short", cs.rel_error(Ys[u], sol[u][2]), (name, k, u, steps))
            Y, cnt = cs.method(model, k, alpha, False, cs.STEPS, cs.TOL)
            Z, zc = cs.target_solves(model, k, alpha)
            values, misses = cs.target_check(model, k, alpha, Z, Y, zc, ("fp64",))
            assert not misses, misses
            note("rel", values[0], (name, k, "targets"))
            note("backward", values[1], (name, k, "targets"))
            note("steps", int(zc.max()), (name, k, "targets"))
            # ---- the controls
            for u in cs.SPLIT_ROWS:  # one entry lost from a split row's sums: that row misses check 1
                bad = np.array(Y)
                bad[u] = cs.lost_entry(model, k, alpha, u)
                _, misses = cs.converged(model, k, alpha, bad, cnt, ("lost entry",))
                assert misses and all(m[3] == u for m in misses), (name, k, u, misses)
            if k >= 2:  # the last two coordinates exchanged
                _, misses = cs.converged(model, k, alpha, cs.swap_last_two(Y), cnt, ("exchanged",))
                assert misses, (name, k)
            if model == ref.IMPLICIT:
                for what, pair in (("lost column of Minv", cs.lost_column_of_minv(k)), ("lost coordinate of G p", cs.lost_coordinate_of_gp(k))):
                    for warm in (False, True):
                        with np.errstate(all="ignore"):  # (a wrong operator may well divide by zero)
                            Yb, cb = cs.method_with(pair, model, k, alpha, warm, cs.STEPS, cs.TOL)
                        _, misses = cs.converged(model, k, alpha, Yb, cb, (what,))
                        assert misses, (what, name, k, warm)
                Yb, cb = cs.method_with(cs.lost_column_of_minv(k), model, k, alpha, False, 4, 0.0)
                _, misses = cs.method_check(model, k, alpha, False, 4, Yb, cb, ("lost column of Minv",))
                assert any("n + 1 steps" in str(m[-2]) for m in misses), (name, k, misses)  # the rule that sees a wrong preconditioner
            _, misses = cs.target_check(model, k, alpha, cs.neighbours_target(Z), Y, zc, ("neighbour's target",))
            assert misses, (name, k)
        cs.release(k)
    print(f"cgsweep-host ranks {_id(ranks)} " + " ".join(f"{key}={v:.3e} {w}" if isinstance(v, float) else f"{key}={v} {w}" for key, (v, w) in worst.items()))
    assert worst["steps"][0] < cs.STEPS
