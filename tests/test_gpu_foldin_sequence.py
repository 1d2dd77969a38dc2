"""Every fold-in setup one after the other on one handle.  A setup is a method (direct solve, block sweeps, conjugate
gradients) on an objective (implicit, implicit with alpha0 / nu, ALS, CCD); the setups share their start (the device, the
unpacked H, the "not set up" mark), and each must leave nothing behind that the next one sees.  The chain is ordered so that
every kind of buffer a setup keeps (the direct base Gramian, the block pack, the cg Gramian and its inverse) is followed by a
setup that must not see it.  After each setup the solved rows pass the check that the setup's own test applies to a fresh
handle -- the bits of the single operator (tests/test_gpu_foldin.py, tests/test_gpu_foldin_reg.py) or of the chained block
halves (tests/test_gpu_foldin_block.py, tests/test_gpu_foldin_alsb.py), which the conjugate gradients do not have -- and
rows, lists, scores, sweep or step counts and what mfx_rec_explain / mfx_rec_explain_cg return or refuse equal those of a
fresh handle given that setup alone.  A refused setup call leaves what was set up as it was, whatever the method.

40 x 70 factors at k = 12 (one MFMA chunk, three item tiles, blocks of 5 + 5 + 2), 33 query rows of 1 to 5 entries: one
slot more than the 32 of a wave."""
import numpy as np
import pytest

from test_gpu_foldin import MFX_ERR_INVALID, factors, same, segments
from test_gpu_foldin_block import LAM

pytestmark = pytest.mark.gpu

ROWS, COLS, K, N_TOP, ALPHA, ALPHA0, NU, D, SWEEPS, STEPS, TOL = 40, 70, 12, 5, 2.0, 0.3, 0.5, 5, 2, 8, 1e-5
REG = dict(alpha0=ALPHA0, nu=NU)


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1, m.lib().mfx_last_error()
    return m


def setups(mfx):
    """name -> (method, objective, setup(r))"""
    I, A, C, X = mfx.MFX_FOLD_IMPLICIT, mfx.MFX_FOLD_ALS, mfx.MFX_FOLD_CCD, mfx.MFX_FOLD_ALS_EXACT
    blk = dict(block=D, sweeps=SWEEPS)
    return {
        "direct implicit": ("direct", "implicit", lambda r: r.fold_in_setup(I, LAM, ALPHA)),
        "direct reg": ("direct", "reg", lambda r: r.fold_in_setup(I, LAM, ALPHA, **REG)),
        "direct ccd": ("direct", "ccd", lambda r: r.fold_in_setup(C, LAM)),
        "direct als": ("direct", "als", lambda r: r.fold_in_setup(A, LAM)),
        "direct exact": ("exact", "als", lambda r: r.fold_in_setup(X, LAM)),
        "blocks implicit": ("blocks", "implicit", lambda r: r.fold_in_block_setup(LAM, ALPHA, **blk)),
        "blocks reg": ("blocks", "reg", lambda r: r.fold_in_block_setup_reg(LAM, ALPHA, ALPHA0, NU, **blk)),
        "blocks als": ("blocks", "als", lambda r: r.fold_in_block_setup_als(LAM, **blk)),
        "blocks ccd": ("blocks", "ccd", lambda r: r.fold_in_block_setup_als(LAM, count_reg=True, **blk)),
        "cg implicit": ("cg", "implicit", lambda r: r.fold_in_cg_setup(I, LAM, ALPHA, steps=STEPS, tol=TOL)),
        "cg als": ("cg", "als", lambda r: r.fold_in_cg_setup(A, LAM, steps=STEPS, tol=TOL)),
        "cg ccd": ("cg", "ccd", lambda r: r.fold_in_cg_setup(C, LAM, steps=STEPS, tol=TOL)),
    }


CHAIN = ["direct implicit", "direct reg", "blocks implicit", "blocks reg", "blocks als", "blocks ccd", "cg implicit", "cg als", "cg ccd",
         "direct ccd", "direct als", "direct implicit"]


def refusal(mfx, call):
    with pytest.raises(mfx.MfxError) as e:
        call()
    return str(e.value)


def observe(mfx, r, method, rows, targets):
    """Everything a handle gives under its setup: fold_in (with the counts where the method has them) and the two
    explanations, each as its result or as the text of its refusal."""
    out = {"fold": r.fold_in(rows, N_TOP, return_sweeps=method in ("blocks", "cg"))}
    kw = dict(n_expl=3, return_W=True, return_Z=True)
    if method == "direct":
        out["explain"] = r.explain(rows, targets, **kw)
    else:
        out["explain"] = refusal(mfx, lambda: r.explain(rows, targets, **kw))
        word = {"exact": "MFX_FOLD_ALS_EXACT", "cg": "not after mfx_rec_fold_in_cg_setup", "blocks": "not after a block setup"}[method]
        assert word in out["explain"], (method, out["explain"])
    if method == "cg":
        out["explain_cg"] = r.explain_cg(rows, targets, return_steps=True, **kw)
    else:
        out["explain_cg"] = refusal(mfx, lambda: r.explain_cg(rows, targets, return_steps=True, **kw))
        assert "call mfx_rec_fold_in_cg_setup first" in out["explain_cg"], (method, out["explain_cg"])
    return out


def equal(a, b):
    if isinstance(a, str) or isinstance(b, str):
        return isinstance(a, str) and isinstance(b, str) and a == b
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(equal(a[key], b[key]) for key in a)
    if isinstance(a, tuple):
        return len(a) == len(b) and all(equal(x, y) for x, y in zip(a, b))
    return same(a, b)


@pytest.fixture(scope="module")
def case(mfx):
    """The data, and what a fresh handle gives under each setup alone."""
    sizes = np.random.default_rng(15).integers(1, 6, 33).tolist()
    assert min(sizes) >= 1 and max(sizes) <= 5
    rows = segments(15, COLS, sizes)
    W, H = factors(15, COLS, K, rows=ROWS)
    targets = np.random.default_rng(16).integers(0, COLS, (33, 2)).astype(np.uint32)
    alone = {}
    for name, (method, _, setup) in setups(mfx).items():
        with mfx.Recommender(W, H, 1) as fresh:
            setup(fresh)
            alone[name] = observe(mfx, fresh, method, rows, targets)
    return rows, W, H, targets, alone


def test_the_setups_in_sequence_equal_each_alone(mfx, case):
    rows, W, H, targets, alone = case
    ptr, idx, val = rows
    table = setups(mfx)

    def chained(half):
        Y = None
        for _ in range(SWEEPS):
            Y = half(Y)
        return Y

    single = {  # the single operators (the conjugate gradients have none: they rest on the fresh handle and its step counts)
        "direct implicit": mfx.ials_half(ptr, idx, val, H, K, LAM, ALPHA),
        "direct reg": mfx.ials_half(ptr, idx, val, H, K, LAM, ALPHA, **REG),
        "direct als": mfx.als_half(ptr, idx, val, H, K, LAM, variant=1),
        "blocks implicit": chained(lambda Y: mfx.ials_block_half(ptr, idx, val, H, K, LAM, ALPHA, D, Y_in=Y)),
        "blocks reg": chained(lambda Y: mfx.ials_block_half(ptr, idx, val, H, K, LAM, ALPHA, D, Y_in=Y, **REG)),
        "blocks als": chained(lambda Y: mfx.als_block_half(ptr, idx, val, H, K, LAM, D, Y_in=Y)),
        "blocks ccd": chained(lambda Y: mfx.als_block_half(ptr, idx, val, H, K, LAM, D, Y_in=Y, count_reg=True)),
    }
    # the setups do solve different rows: the four methods-on-objectives this file began with, and under every method each
    # pair of objectives (another regulariser on the diagonal, another Gramian or none: another system for every row but
    # at most the rows of one entry under ALS against CCD)
    solved = {name: alone[name]["fold"][2].tobytes() for name in CHAIN}
    assert len({solved[name] for name in ("direct implicit", "blocks implicit", "blocks als", "direct als")}) == 4
    for method in ("direct", "blocks", "cg"):
        names = [name for name in solved if table[name][0] == method]
        assert len(names) >= 3 and len({solved[name] for name in names}) == len(names), method

    with mfx.Recommender(W, H, 1) as r:
        for step, name in enumerate(CHAIN):
            method, _, setup = table[name]
            setup(r)
            got = observe(mfx, r, method, rows, targets)
            if name in single:
                assert same(got["fold"][2], single[name]), (step, name)
            assert got["fold"][0].shape == (33, N_TOP), (step, name)
            for what in got:
                assert equal(got[what], alone[name][what]), (step, name, what)


def test_a_refused_setup_leaves_every_method_usable(mfx, case):
    rows, W, H, _, alone = case
    lib = mfx.lib()
    bad = {  # one refused call per entry point
        "mfx_rec_fold_in_setup": (7, LAM, ALPHA),                                   # unknown model
        "mfx_rec_fold_in_setup_reg": (LAM, ALPHA, 0.0, NU),                         # alpha0
        "mfx_rec_fold_in_block_setup": (LAM, ALPHA, 129, SWEEPS, 0.0),              # block
        "mfx_rec_fold_in_block_setup_reg": (LAM, -1.0, ALPHA0, NU, D, SWEEPS, 0.0),  # alpha
        "mfx_rec_fold_in_block_setup_als": (LAM, 2, D, SWEEPS, 0.0),                # reg
        "mfx_rec_fold_in_cg_setup": (mfx.MFX_FOLD_ALS_EXACT, LAM, ALPHA, STEPS, TOL),  # not an objective
    }

    def refused(r, fn):
        assert getattr(lib, fn)(r.handle, *bad[fn]) == MFX_ERR_INVALID, fn
        return lib.mfx_last_error().decode()

    with mfx.Recommender(W, H, 1) as fresh:
        text = {fn: refused(fresh, fn) for fn in bad}
    assert all(fn in text[fn] for fn in bad), text
    table = setups(mfx)
    with mfx.Recommender(W, H, 1) as r:
        for name in ("direct reg", "direct exact", "blocks reg", "cg implicit"):  # one step of each method
            method, _, setup = table[name]
            setup(r)
            for fn in bad:
                assert refused(r, fn) == text[fn], (name, fn)
                got = r.fold_in(rows, N_TOP, return_sweeps=method in ("blocks", "cg"))
                assert equal(got, alone[name]["fold"]), (name, fn)
